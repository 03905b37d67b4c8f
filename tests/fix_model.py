"""A small model of what damar_pile_patches computes (LAfix's breaks and weak segments of one pile, steps 4 to 6 of the
issue), written from the description of the method and independent of host/fix.c: numpy over the pile's records, the trace
as a running sum per record.  patches() takes what api.pile_patches takes and returns the same lists of dicts.  `seen`
counts what the two rules for out-of-range reads would decide: q values asked for beyond the track's data, and scans for
the first or last scored segment that ran to the read's border."""
import numpy as np

KEYS = ("ab", "ae", "bb", "be", "diff", "b", "support", "comp")


def cdiv(a, b):
    """C's integer division"""
    return int(a / b) if a * b < 0 and a % b else a // b


class Model:
    def __init__(self, batch, rl, q, repeats=None, low_q=28, max_gap=500, low_coverage=False):
        self.b, self.rl, self.tw = batch, np.asarray(rl), int(batch["tspace"])
        self.qa, self.qd = np.asarray(q[0], dtype=np.int64) // 4, np.asarray(q[1])
        self.rep = None if repeats is None else (np.asarray(repeats[0], dtype=np.int64) // 4, np.asarray(repeats[1]))
        self.low_q, self.max_gap = low_q, max_gap
        self.maxspanners, self.minsupport = (3, 2) if low_coverage else (7, 4)
        self.seen = dict(q_beyond_data=0, scan_hit_border=0)
        dt = np.uint8 if batch["tbytes"] == 1 else "<u2"
        self.trace = np.frombuffer(np.ascontiguousarray(batch["trace"]).tobytes(), dtype=dt)
        self.tb = int(batch["tbytes"])

    def q(self, read, k):
        at = int(self.qa[read]) + k
        if at < 0 or at >= len(self.qd):
            self.seen["q_beyond_data"] += 1
            return 0
        return int(self.qd[at])

    def blens(self, r):
        """the B lengths of record r's trace intervals"""
        o, n = int(self.b["trace_off"][r]) // self.tb, int(self.b["tlen"][r])
        return self.trace[o:o + n][1::2].astype(np.int64)

    def min_span(self, aread, pt):
        if self.rep is None:
            return 400
        anno, data = self.rep
        iv = data[anno[aread]:anno[aread + 1]].reshape(-1, 2)
        return 800 if np.any((iv[:, 0] <= pt) & (iv[:, 1] > pt)) else 400

    def pile(self, p, trim_ab, trim_ae):
        b, tw = self.b, self.tw
        lo, hi = int(b["pile_off"][p]), int(b["pile_off"][p + 1])
        aread = int(b["pile_aread"][p])
        if trim_ab >= trim_ae:
            return []
        ab, ae, bb, be = (b[k][lo:hi].astype(np.int64) for k in ("abpos", "aepos", "bbpos", "bepos"))
        br, comp = b["bread"][lo:hi], b["flags"][lo:hi] & 1
        nsegs = (int(self.rl[aread]) + tw - 1) // tw
        qa = lambda k: self.q(aread, k)
        bad = lambda v: v == 0 or v >= self.low_q

        def many_across(pt):
            m = self.min_span(aread, pt)
            return int(np.sum((ab < pt - m) & (ae > pt + m))) > self.maxspanners

        # step 4: a hole between two neighbouring records of one B read in one orientation
        cand = []
        for i in range(1, hi - lo):
            if br[i - 1] != br[i] or comp[i - 1] != comp[i] or not ae[i - 1] < ab[i]:
                continue
            sa, se = cdiv(int(ae[i - 1]) - 1, tw), int(ab[i]) // tw + 1
            gb, ge = int(be[i - 1]) - int(self.blens(lo + i - 1)[-1]), int(bb[i]) + int(self.blens(lo + i)[0])
            if gb >= ge:
                continue
            if comp[i]:
                gb, ge = int(self.rl[br[i]]) - ge, int(self.rl[br[i]]) - gb
            qs = [self.q(int(br[i]), k) for k in range(cdiv(gb, tw), cdiv(ge, tw) + 1)]
            if 0 in qs:
                continue
            if many_across(sa * tw) and many_across(se * tw):
                continue
            if sum(1 for k in range(sa + 1, se - 1) if qa(k) != 0) > 1:
                continue
            if (se - sa) * tw * 10 < ge - gb:
                continue
            cand.append(dict(ab=sa * tw, ae=se * tw, bb=gb, be=ge, diff=int(tw * 1.0 * sum(qs) / (ge - gb)), b=int(br[i]), support=1,
                             comp=int(comp[i])))
        # step 5: Python's sort is stable, as the reference's is
        key = lambda g: (g["ab"], g["ae"], g["diff"])
        cand.sort(key=key)
        n = len(cand)
        for i, g in enumerate(cand):
            if g["support"] == -1:
                continue
            if self.max_gap != -1 and (g["ae"] - g["ab"] >= self.max_gap or abs(g["be"] - g["bb"]) >= self.max_gap):
                g["support"] = -1
                continue
            for h in cand[i + 1:]:
                if (h["ab"], h["ae"]) != (g["ab"], g["ae"]):
                    break
                if h["support"] != -1 and abs((h["be"] - h["bb"]) - (g["be"] - g["bb"])) < 50:
                    g["support"] += 1
                    h["support"] = -1
        for i, g in enumerate(cand):
            if g["support"] == -1:
                continue
            for h in cand[i + 1:]:
                if not (g["ae"] > h["ab"] and g["ab"] < h["ae"]):
                    break
                if h["support"] == -1:
                    continue
                if g["support"] > h["support"]:
                    g["support"] += h["support"]
                    h["support"] = -1
                else:
                    h["support"] += g["support"]
                    g["support"] = -1
                    break
        kept = [g for g in cand if g["support"] >= self.minsupport and any(bad(qa(k)) for k in range(g["ab"] // tw, g["ae"] // tw))]
        assert n == len(cand)
        # step 6
        first, last = trim_ab // tw, trim_ae // tw
        while first < nsegs and qa(first) == 0:
            first += 1
        while last > 0 and qa(last - 1) == 0:
            last -= 1
        if first >= nsegs or last <= 0:
            self.seen["scan_hit_border"] += 1
        out = list(kept)
        for s in range(first, last):
            if not bad(qa(s)):
                continue
            wa, we = s * tw, (s + 1) * tw
            if any(g["ab"] <= wa and g["ae"] >= we for g in out):
                continue
            support = int(np.sum(((ab >= wa) & (ab <= we)) | ((ae >= wa) & (ae <= we))))
            best = None
            for j in np.flatnonzero((ab + tw <= wa) & (ae - tw >= we)):
                run = np.concatenate([[0], np.cumsum(self.blens(lo + j))]) + int(bb[j])
                m = min(s - int(ab[j]) // tw + 1, len(run) - 1)        # the interval of the trace that holds the segment
                gb, ge = int(run[m - 1]), int(run[m])
                if comp[j]:
                    gb, ge = int(self.rl[br[j]]) - ge, int(self.rl[br[j]]) - gb
                beg, end = cdiv(gb, tw), cdiv(ge, tw)
                qs = []
                for k in range(beg, end):
                    qs.append(self.q(int(br[j]), k))
                    if qs[-1] == 0:
                        break
                if not qs or 0 in qs:
                    continue
                mean = np.float32(1.0 * sum(qs) / (end - beg))
                if best is None or mean < best[0]:
                    best = (mean, int(j), gb, ge)
            if best is not None:
                out.append(dict(ab=wa, ae=we, bb=best[2], be=best[3], diff=int(best[0]), b=int(br[best[1]]), support=support,
                                comp=int(comp[best[1]])))
        out.sort(key=key)
        return out


def patches(batch, rl, trims, q, **kw):
    m = Model(batch, rl, q, **kw)
    return [m.pile(p, int(trims[p][0]), int(trims[p][1])) for p in range(len(batch["pile_aread"]))], m.seen
