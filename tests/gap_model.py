"""A plain model of LAgap's per-pile routine (scrub/LAgap.c drop_containments, the OVL_TEMP marks and the bins of
handle_gaps_and_breaks, drop_break, stitchable), in integers, written the slow way: every loop runs over the whole pile, the
bins are a list counted up bin by bin, the first interval and the first longest record are found in file order.  It shares no
mechanism with kernels/pile_gaps.hip (no runs, no difference array, no chunks of 64), so it can be held against it.

run(piles, read_len, stitch, exclude) takes what api.pile_gaps takes and returns a Result: flags (OVL_TEMP included), the
events of every pile as (first bin, bin after the run, kind, v0, v1, records dropped), and per pile what damar_pile_gaps
needs to decide who does it: the number of events, the number of bins, whether the B reads descend.

MUTANTS names the model with one of the kernel's borders got wrong: what the shapes of gap_shapes.py must tell from it."""
import numpy as np

COMP, DISCARD, STITCH, TEMP, CONT, GAP, TRIM = 0x1, 0x2, 0x80, 0x800, 0x8000, 0x10000, 0x20000      # lib/oflags.h
MASKED, STITCHABLE, DROP_L, DROP_R, DROP_NONE, TRAILING = 0, 1, 2, 3, 4, 0x100                       # include/damar_hip.h
BIN, MIN_LR = 100, 450                                                                               # LAgap.c:33-34
WAVE = 64

MUTANTS = ("run_at_64",            # a record at index 64 always begins a run
           "carry_lost",           # the coverage carry is lost at every 64th bin
           "beg_forgotten",        # the open thin run is forgotten at every 64th bin counted from b0
           "tie_highest",          # a length tie goes to the highest index
           "tie_lane",             # a length tie goes to the lowest index % 64
           "ex_first64",           # only the first 64 exclude intervals are looked at
           "ex_lane",              # the reported interval is the containing one with the lowest index % 64
           "stitch_first64",       # stitch pairs are counted for i < 64 only
           "ev_limit_low",         # the event limit is off by one: a pile of exactly the limit goes to the host
           "ev_limit_high",        # ... the other way: a pile of one more stays
           "e_unclamped")          # e is not held to nb


def cdiv(a, b):
    """C's a / b: truncated toward zero"""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b > 0) else -q


def contained(ab, ae, bb, be):
    if ab >= bb and ae <= be:
        return 1
    if bb >= ab and be <= ae:
        return 2
    return 0


class Result:
    def __init__(self):
        self.flags, self.events, self.info = [], [], []

    def flags_array(self):
        return np.array(self.flags, dtype=np.int32)

    def on_host(self, limits, mutant=None):
        """per pile: whether damar_pile_gaps must leave it to the host routine under limits = (bins, events)"""
        evlim = limits[1] + {"ev_limit_low": -1, "ev_limit_high": 1}.get(mutant, 0)
        return [i["descends"] or i["nbins"] > limits[0] or i["nev"] > evlim for i in self.info]

    def host_piles(self, limits, mutant=None):
        return sum(self.on_host(limits, mutant))


def one_pile(aread, ab, ae, bb, be, br, flags, read_len, stitch=0, intervals=None, mutant=None):
    """-> (flags, events, info) of one pile; intervals: the (begin, end) pairs of the A read's exclude track, None: no track"""
    n = len(ab)
    fl = [int(f) for f in flags]
    other_run = (lambda i, k: k // WAVE > i // WAVE) if mutant == "run_at_64" else (lambda i, k: False)

    gone = 0
    if n >= 2:                                                          # drop_containments
        for i in range(n):
            if (fl[i] & DISCARD) or br[i] == aread:
                continue
            blen = int(read_len[br[i]])
            b1 = (blen - be[i], blen - bb[i]) if fl[i] & COMP else (bb[i], be[i])
            for k in range(i + 1, n):
                if fl[k] & DISCARD:
                    continue
                if br[k] != br[i] or other_run(i, k):
                    break
                b2 = (blen - be[k], blen - bb[k]) if fl[k] & COMP else (bb[k], be[k])
                cont = contained(ab[i], ae[i], ab[k], ae[k])
                if cont and contained(b1[0], b1[1], b2[0], b2[1]):
                    gone += 1
                    if cont == 1:
                        fl[i] |= DISCARD | CONT
                        break
                    fl[k] |= DISCARD | CONT

    nb = cdiv(int(read_len[aread]) + BIN, BIN)
    hold = (lambda e: e) if mutant == "e_unclamped" else (lambda e: min(e, nb))
    bins = [0] * (nb + 1)
    spans = []
    tb, te = None, 0
    for i in range(n):                                                  # OVL_TEMP and the bins
        if (fl[i] & DISCARD) or br[i] == aread:
            continue
        for j in range(i + 1, n):
            if br[j] != br[i] or other_run(i, j):
                break
            if max(ab[i], ab[j]) < min(ae[i], ae[j]):
                if ae[i] - ab[i] < ae[j] - ab[j]:
                    fl[i] |= TEMP
                else:
                    fl[j] |= TEMP
        if fl[i] & TEMP:
            continue
        tb = ab[i] if tb is None else min(tb, ab[i])
        te = max(te, ae[i])
        b, e = max(cdiv(ab[i] + MIN_LR, BIN), 0), hold(cdiv(ae[i] - MIN_LR, BIN))
        if e > len(bins):
            bins += [0] * (e - len(bins))
        for x in range(b, e):
            bins[x] += 1
        spans.append((b, e))
    if mutant == "carry_lost":
        for x in range(len(bins)):
            c0 = x - x % WAVE
            bins[x] = sum(1 for b, e in spans if b < e and c0 <= b <= x) - sum(1 for b, e in spans if b < e and c0 <= e <= x)

    events = []
    info = dict(nev=0, nbins=nb, gone=gone, descends=any(br[i] < br[i - 1] for i in range(1, n)))
    if tb is None or tb >= te:
        return fl, events, info

    def drop_break(p1, p2):
        best, left = 0, False
        for i in range(n):
            if fl[i] & DISCARD:
                continue
            ln = ae[i] - ab[i]
            if ln > best or (mutant == "tie_highest" and ln == best and ln > 0):
                best, left = ln, ab[i] < p1
        if mutant == "tie_lane" and best > 0:
            i = min((i for i in range(n) if not (fl[i] & DISCARD) and ae[i] - ab[i] == best), key=lambda i: (i % WAVE, i))
            left = ab[i] < p1
        if best == 0:
            return DROP_NONE, 0
        d = 0
        for i in range(n):
            if (ab[i] < p1) if not left else (not (fl[i] & DISCARD) and ae[i] > p2):
                d += 0 if fl[i] & DISCARD else 1
                fl[i] |= DISCARD | GAP
        return (DROP_R if left else DROP_L), d

    def stitchable(p1, p2):
        ignore, t = TEMP | CONT | TRIM | STITCH, 0
        if n < 2:
            return 0
        for i in range(n if mutant != "stitch_first64" else min(n, WAVE)):
            if fl[i] & ignore:
                continue
            for k in range(i + 1, n):
                if br[k] != br[i]:
                    break
                if (fl[k] & ignore) or (fl[i] & COMP) != (fl[k] & COMP):
                    continue
                if abs(ae[i] - ab[k]) < stitch and abs(be[i] - bb[k]) < stitch and ab[i] < p1 - MIN_LR and ae[k] > p2 + MIN_LR:
                    t += 1
        return t

    b0, e0 = cdiv(tb + MIN_LR, BIN), hold(cdiv(te - MIN_LR, BIN))
    if e0 > len(bins):
        bins += [0] * (e0 - len(bins))
    beg = -1
    for b in range(b0, e0):
        if mutant == "beg_forgotten" and b > b0 and (b - b0) % WAVE == 0:
            beg = -1
        if bins[b] <= 1:
            if beg == -1:
                beg = b
            continue
        if beg == -1:
            continue
        p1, p2 = (beg - 1) * BIN, (b + 1) * BIN
        ev = None
        if intervals is not None:
            look = list(enumerate(intervals))
            if mutant == "ex_first64":
                look = look[:WAVE]
            inside = [(j, iv) for j, iv in look if p1 > iv[0] and p2 < iv[1]]
            if mutant == "ex_lane":
                inside.sort(key=lambda x: (x[0] % WAVE, x[0]))
            if inside:
                ev = (beg, b, MASKED, int(inside[0][1][0]), int(inside[0][1][1]), 0)
        if ev is None and stitch > 0:
            t = stitchable(p1, p2)
            if t:
                ev = (beg, b, STITCHABLE, t, 0, 0)
        if ev is None:
            kind, d = drop_break(p1, p2)
            ev = (beg, b, kind, 0, 0, d)
        events.append(ev)
        beg = -1
    if beg != -1:
        kind, d = drop_break((beg - 1) * BIN, (e0 + 1) * BIN)
        events.append((beg, e0, kind | TRAILING, 0, 0, d))
    info["nev"] = len(events)
    return fl, events, info


def run(piles, read_len, stitch=0, exclude=None, mutant=None):
    off = [int(x) for x in piles["pile_off"]]
    col = {k: [int(x) for x in piles[k]] for k in ("abpos", "aepos", "bbpos", "bepos", "bread", "flags")}
    res = Result()
    for p in range(len(off) - 1):
        a, lo, hi = int(piles["pile_aread"][p]), off[p], off[p + 1]
        iv = None
        if exclude is not None:
            d = [int(x) for x in exclude[1][int(exclude[0][a]) // 4:int(exclude[0][a + 1]) // 4]]
            iv = list(zip(d[0::2], d[1::2]))
        fl, ev, info = one_pile(a, col["abpos"][lo:hi], col["aepos"][lo:hi], col["bbpos"][lo:hi], col["bepos"][lo:hi],
                                col["bread"][lo:hi], col["flags"][lo:hi], read_len, stitch, iv, mutant)
        res.flags += fl
        res.events.append(ev)
        res.info.append(info)
    return res


def lines(aread, events):
    """what the reference prints of a pile's events (LAgap.c:1693-1751, :198, :217)"""
    out = []
    for beg, b, kind, v0, v1, _ in events:
        k = kind & 0xff
        if not kind & TRAILING:
            out.append("READ %7d BREAK %3d..%3d " % (aread, beg, b) +
                       (" MASKED %5d..%5d" % (v0, v1) if k == MASKED else " STITCHABLE using %d" % v0 if k == STITCHABLE else ""))
        if k in (DROP_L, DROP_R):
            out.append("DROP %s @ %5d..%5d" % ("L" if k == DROP_L else "R", (beg - 1) * BIN, (b + 1) * BIN))
    return out


def counts(res):
    """(containments, records dropped at breaks, breaks): the two closing lines of the reference"""
    return sum(i["gone"] for i in res.info), sum(e[5] for ev in res.events for e in ev), sum(1 for ev in res.events for e in ev if (e[2] & 0xff) >= DROP_L)
