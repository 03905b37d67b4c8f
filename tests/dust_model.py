"""DBdust's method (db/DBdust.c, Myers' incremental SDUST with integer counts) stated plainly, as a second opinion on
host/dust.c: nothing incremental, every quantity recomputed from the window each step.

Step j takes triplet j into a window of the last w - 2 triplets.  The suffix (lb, j] is the longest suffix of the window
in which no triplet occurs more than ceil(2 t) times -- kept as the reference keeps it: it never starts before the window,
and when triplet j is one too many it starts behind the first of its like.  A candidate whose start has left the window
is retired.  If the window's score exceeds t times the suffix's, every start c from lb down to the window's first is
tried: the score of [c, j] must reach t (j - c) and (j - c) times the best score of the candidates that start at or after
c; it is then the candidate of start c, with score / (j - c).  At the read's end every candidate is retired.  The mask
joins retired candidates (start, last triplet + 2) that touch or overlap and keeps those of at least minlen bases."""
from math import ceil


def pairs(codes):
    """sum over the triplets of count * (count - 1) / 2"""
    seen, s = {}, 0
    for c in codes:
        s += seen.get(c, 0)
        seen[c] = seen.get(c, 0) + 1
    return s


def candidates(seq, w=64, t=2.0, start=0, own=None, stop=None):
    """The retired candidates (start, last triplet) in the order they retire; with start/own/stop one piece of the read."""
    tri = [(seq[k] << 4) | (seq[k + 1] << 2) | seq[k + 2] for k in range(len(seq) - 2)]
    n = len(tri)
    stop = n if stop is None else min(stop, n)
    own = (0, n) if own is None else own
    most = int(ceil(2. * t))
    cand = {}                                   # start -> [last, score]
    out, longest = [], 0
    lb = start - 1
    for j in range(start, stop):
        wb = j - (w - 2) if j - start > w - 3 else start - 1
        lb = max(lb, wb)
        if tri[lb + 1:j].count(tri[j]) >= most:
            lb = lb + 1 + tri[lb + 1:j].index(tri[j])
        if wb in cand:
            if own[0] <= wb < own[1]:
                out.append((wb, cand[wb][0]))
            del cand[wb]
        if pairs(tri[wb + 1:j + 1]) <= pairs(tri[lb + 1:j + 1]) * t:
            continue
        best = 0.
        old = sorted(cand.items(), reverse=True)        # each looked at once, as it stood when the walk began
        for c in range(lb, wb, -1):
            score = pairs(tri[c:j + 1])
            if score >= t * (j - c):
                while old and old[0][0] >= c:
                    best = max(best, old.pop(0)[1][1])
                if score >= best * (j - c):
                    best = (1. * score) / (j - c)
                    cand[c] = [j, best]
                    longest = max(longest, len(cand))
    if stop == n:
        for b in sorted(cand):
            if own[0] <= b < own[1]:
                out.append((b, cand[b][0]))
    return out, longest


def join(cands, minlen=10):
    """retired candidates in order of their starts -> [beg, end) pairs"""
    mask = []
    for b, e in cands:
        e += 2
        if mask and mask[-1][1] + 1 >= b:
            mask[-1][1] = max(mask[-1][1], e)
        else:
            mask.append([b, e])
    return [(b, e + 1) for b, e in mask if e - b >= minlen - 1]


def dust(seq, w=64, t=2.0, minlen=10):
    return join(candidates(seq, w, t)[0], minlen)
