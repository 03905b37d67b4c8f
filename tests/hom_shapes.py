"""Planted shapes for TKhomogenize: small records on tiny2's reads, spacing 100, and the interval and trim tracks they meet,
as arrays (for api.pile_homogenize) and as one synthetic .las (tests/golden/homogenize/synth.las, which the generator also
runs through the reference, so tests/hom_model.py is itself pinned).  Each record is there for one thing that can go wrong;
PLANTED lists what the model's walk must have met (hom_model.add / read_out count it in `seen`).

min(j1 * res, rlen) cannot bite: a run that does not reach the last bit ends at j1 <= alen - 2, and (alen - 2) * res < rlen
for alen = ceil(rlen / res).  The model counts it all the same and the tests hold the count to 0."""
import struct

import numpy as np

import q_common

TW = 100
PLANTED = ("identity", "short", "stop_before_more", "touching", "zero_under_iab", "zero_under_iae", "iab_on_segment_end",
           "iab_in_partial_first", "same_segment", "clipped_at_abpos", "clipped_at_aepos", "comp", "discarded_marks", "no_trace",
           "spare_bit", "reaches_last", "ends_before_last")


class Plan:
    def __init__(self, read_len, tw=TW):
        self.rl, self.tw = np.asarray(read_len, dtype=np.int32), tw
        self.tb = 1 if tw <= 125 else 2
        self.ivs, self.recs, self.trim = {}, [], {}

    def iv(self, a, *pairs):
        assert a not in self.ivs and all(0 <= b and e <= self.rl[a] for b, e in pairs)
        self.ivs[a] = list(pairs)

    def rec(self, a, b, ab, ae, bb, blens=None, flags=0, be=None, bl=None):
        """blens: the B length of every segment (bl: the same for all); be: bepos, the sum's end unless given"""
        nseg = (ae + self.tw - 1) // self.tw - ab // self.tw
        if bl is not None:
            blens = [bl] * nseg
        tr = b""
        if blens is not None:
            assert len(blens) == nseg, (len(blens), nseg)
            fmt = "<2B" if self.tb == 1 else "<2H"
            tr = b"".join(struct.pack(fmt, 3, x) for x in blens)
        be = bb + sum(blens or [ae - ab]) if be is None else be
        assert 0 <= ab <= ae <= self.rl[a] and 0 <= bb <= be <= self.rl[b], (a, b, ab, ae, bb, be)
        self.recs.append((a, len(self.recs), (2 * len(blens) if blens is not None else 0, 0, ab, bb, ae, be, flags, a, b, 0), tr))

    def piles(self):
        return sorted(set(r[0] for r in self.recs))

    def batch(self, piles=None):
        """the records of `piles` (all by default) as one batch of the read_trace_piles form"""
        recs = sorted((r for r in self.recs if piles is None or r[0] in piles), key=lambda r: (r[0], r[1]))
        cols = np.array([r[2] for r in recs], dtype=np.int32).reshape(len(recs), 10)
        aread = cols[:, 7]
        off = np.concatenate([[0], np.flatnonzero(np.diff(aread)) + 1, [len(recs)]]).astype(np.int64) if len(recs) else np.zeros(1, dtype=np.int64)
        lens = np.array([len(r[3]) for r in recs], dtype=np.int64)
        return dict(pile_off=off, pile_aread=aread[off[:-1]].copy(), abpos=cols[:, 2].copy(), aepos=cols[:, 4].copy(),
                    bbpos=cols[:, 3].copy(), bepos=cols[:, 5].copy(), bread=cols[:, 8].copy(), flags=cols[:, 6].copy(),
                    tlen=cols[:, 0].copy(), trace=np.frombuffer(b"".join(r[3] for r in recs), dtype=np.uint8),
                    trace_off=(np.cumsum(lens) - lens).astype(np.int64), tbytes=self.tb, tspace=self.tw)

    def las(self, piles=None):
        recs = sorted((r for r in self.recs if piles is None or r[0] in piles), key=lambda r: (r[0], r[1]))
        return struct.pack("<qi", len(recs), self.tw) + b"".join(struct.pack("<10i", *r[2]) + r[3] for r in recs)

    def track(self):
        anno, data = [0], []
        for r in range(len(self.rl)):
            for b, e in self.ivs.get(r, []):
                data += [b, e]
            anno.append(4 * len(data))
        return np.array(anno, dtype=np.uint64), np.array(data, dtype=np.int32)

    def trim_track(self):
        """every read whole, but what self.trim says (None: no entry)"""
        anno, data = [0], []
        for r in range(len(self.rl)):
            t = self.trim.get(r, (0, int(self.rl[r])))
            if t is not None:
                data += list(t)
            anno.append(4 * len(data))
        return np.array(anno, dtype=np.uint64), np.array(data, dtype=np.int32)


def synth():
    """the plan behind synth.las -> (plan, roles: the read numbers by what they are there for)"""
    rl = q_common.db_read_len("tiny2")
    by_len = [int(r) for r in np.argsort(-rl.astype(np.int64), kind="stable")]
    assert rl[by_len[3]] >= 13500 and rl[by_len[40]] >= 8700
    p = Plan(rl)
    A3, B14 = by_len[0], by_len[1]                       # 129 segments need 13 000 bases on both sides
    A = by_len[4:14]                                     # A reads, at least 8 700 bases each
    B = iter(by_len[14:])                                # every shape its own B read
    nb = lambda: next(B)
    rng = np.random.default_rng(20261020)
    wob = lambda n: [int(x) for x in rng.integers(80, 121, n)]
    role = {}

    a1 = A[0]
    p.iv(a1, (1000, 1600), (2000, 2499), (3000, 3500), (5000, 5600))
    role["both"] = b1 = nb()
    p.rec(a1, b1, 1250, 1450, 2000, [45, 105, 48])       # clipped at abpos and at aepos, iab in the partial first segment
    role["no_entry"] = b2 = nb()
    p.rec(a1, b2, 1600, 1900, 2000, wob(3))              # touches (1000, 1600): iab == iae
    p.rec(a1, nb(), 1900, 3600, 2000, wob(17))           # over a 499 interval (skipped) and a 500 one
    p.rec(a1, b2, 2900, 3300, 2100, wob(4))              # aoff + tw == iab exactly, in the first segment
    p.rec(a1, nb(), 3450, 3700, 2000, wob(3))            # iab and iae in one segment
    p.rec(a1, nb(), 900, 1700, 2000, [0] + wob(5) + [0, 97])          # B length 0 under iab (segment 0) and under iae (segment 6)
    p.rec(a1, nb(), 1000, 1600, 2000, wob(6), flags=1)   # complement
    p.rec(a1, a1, 1000, 1600, 1000, wob(6))              # identity: skipped
    p.rec(a1, nb(), 1000, 1600, 2000, wob(6), flags=2)   # discarded: marks all the same
    p.rec(a1, nb(), 1000, 1600, 2000, None)              # no trace: nothing
    a2 = A[1]
    p.iv(a2, (6000, 6600), (1000, 1600))                 # the walk stops at the first and never sees the second
    p.rec(a2, nb(), 900, 2000, 2000, wob(11))
    p.iv(A3, (100, 12990))
    for ab, ae in ((200, 300), (200, 6600), (200, 6700)):              # 1, 64 and 65 segments
        p.rec(A3, nb(), ab, ae, 50, wob((ae + 99) // 100 - ab // 100))
    role["wide"] = B14
    p.rec(A3, B14, 100, 13000, 5, bl=100)                # 129 segments, and a range of 400 words
    for a, n, step, every, at in ((A[2], 64, 50, 8, 0), (A[3], 65, 50, 8, 0), (A[4], 200, 40, 16, 3)):
        p.iv(a, *[(k * step, k * step + (600 if k % every == at else 70)) for k in range(n)])
        p.rec(a, nb(), 500, 7000, 1000, wob(65))         # 64, 65 and 200 intervals; the 200's walk stops in its third chunk
    p.rec(A[5], nb(), 1000, 1600, 2000, wob(6))          # an A read without intervals
    a8, a9 = A[6], A[7]
    p.iv(a8, (1000, 1600))
    p.iv(a9, (1000, 1600))
    role["words"] = []
    for x, y in ((31, 31), (31, 32), (32, 63), (0, 95), (33, 70)):     # word borders, against an all-zero mask
        b = nb()
        role["words"].append((b, x, y))
        p.rec(a8, b, 1000, 1600, x, bl=100, be=y)
    b_in, b_over = role["words"][3][0], role["words"][4][0]
    p.rec(a9, b_in, 1000, 1600, 33, bl=100, be=70)       # against a part-set mask: inside what is set, and over its end
    p.rec(a9, b_over, 1000, 1600, 0, bl=100, be=95)
    role["adjacent"], role["overlap"] = nb(), nb()
    p.rec(a8, role["adjacent"], 1000, 1600, 100, bl=100, be=200)       # two piles, one B read: exactly adjacent ...
    p.rec(a9, role["adjacent"], 1000, 1600, 201, bl=100, be=300)
    p.rec(a8, role["overlap"], 1000, 1600, 100, bl=100, be=200)        # ... and overlapping
    p.rec(a9, role["overlap"], 1000, 1600, 150, bl=100, be=400)
    role["last"], role["before_last"] = nb(), nb()
    p.rec(a8, role["last"], 1000, 1600, int(rl[role["last"]]) - 300, bl=100, be=int(rl[role["last"]]))      # the spare bit, and a run to the last bit
    p.rec(a8, role["before_last"], 1000, 1600, int(rl[role["before_last"]]) - 300, bl=100, be=int(rl[role["before_last"]]) - 2)
    p.trim[b1] = (1800, 2400)                            # -e 1500: both rules fire for the range at 2000
    p.trim[b2] = None                                    # no entry counts as (0, 0): the right rule alone
    role["a_pair"] = (a8, a9)
    return p, role


def two_byte():
    """spacing 200: two-byte trace values, some above 255"""
    rl = q_common.db_read_len("tiny2")
    p = Plan(rl, tw=200)
    p.iv(3, (1000, 2600), (3000, 3700))
    p.iv(5, (0, 900))
    p.rec(3, 7, 900, 3900, 1000, [150, 260, 300, 190, 0, 210, 256, 199, 201, 180, 220, 200, 240, 170, 230, 195])
    p.rec(3, 8, 1100, 3500, 500, [90] + [205] * 11 + [100], flags=1)
    p.rec(5, 7, 0, 850, 3000, [200, 190, 310, 180, 50])
    return p


def write_synth(path):
    p, _ = synth()
    open(path, "wb").write(p.las())
