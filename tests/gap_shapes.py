"""Deterministic piles at the borders of kernels/pile_gaps.hip (runs found 64 records at a time, the coverage summed 64 bins a
step, thin runs found in chunks of 64 bins from b0 on, drop_break / exclude intervals / stitch pairs with the lanes over
records with stride 64, the event slot), one pile each on an A read of its own, and seeded random piles.  api.pile_gaps takes
read_len as an argument, so the shapes need no database: READ_LEN is theirs.

A bin is 100 bases; a record covers the bins [(ab + 450) / 100, (ae - 450) / 100); a read of `len` bases has
nb = (len + 100) / 100 bins (kernels/pile_gaps.hip PG_BIN, PG_MINLR).  shapes() -> the list of Shape; arrays(shapes) -> the
piles as api.pile_gaps takes them, and the exclude track."""
import hashlib

import numpy as np

import gap_model as gm
from gap_model import COMP, DISCARD, STITCH, TEMP, CONT, TRIM

BIN, MIN_LR, WAVE = 100, 450, 64
NREADS, NA = 400, 110                    # reads 0 .. NA-1 are the shapes' A reads, the others the pool of B reads
BLEN = 40000
B0 = 7                                   # the first scanned bin of the break-scan shapes: no multiple of 64


class Shape:
    def __init__(self, tag, border, alen, recs, ex=(), api_only=False, refused=False, want=None):
        self.tag, self.border, self.alen, self.ex, self.api_only, self.refused = tag, border, alen, list(ex), api_only, refused
        self.want = want or {}           # what the generator holds the shape to, computed with the model
        self.aread = None
        self.recs = [tuple(r) + (None,) * (6 - len(r)) for r in recs]     # (b, ab, ae, bb, be, flags), in file order


def cover(x, y):
    """(ab, ae) of a record that covers the bins [x, y)"""
    assert 5 <= x < y
    return BIN * x - MIN_LR, BIN * y + MIN_LR


def thick(segs, b=NA):
    """records, two of different B reads per segment (x, y), or `c` of them for (x, y, c): coverage c on the bins [x, y)"""
    recs = []
    for s in segs:
        for _ in range(s[2] if len(s) > 2 else 2):
            recs.append((b,) + cover(s[0], s[1]))
            b += 1
    return recs


def shapes():
    S = []
    add = lambda *a, **k: S.append(Shape(*a, **k))
    short = lambda b: (b, 0, 800)                                      # covers no bin

    # ---- run borders: 131 records, single short records but for the runs named ---------------------------------------
    def runs(feature):
        recs = [short(NA + i) for i in range(131)]
        for lo, hi in ((125, 127), (128, 130)):                        # a run that ends at 127, the next begins at 128
            for i in range(lo, hi + 1):
                recs[i] = (NA + lo, 0, 800)
        recs[126] = (NA + 125, 100, 700)                               # inside 125: dropped
        recs[129] = (NA + 128, 100, 700)                               # inside 128: dropped
        recs[127] = (NA + 125, 0, 400)
        recs[130] = (NA + 128, 400, 800)
        for i, r in feature.items():
            recs[i] = r
        return recs
    b = NA + 62
    add("run_62_66", "a run of one B read over the records 62..66: 63 is dropped only as the partner of 65", 3000,
        runs({62: (b, 100, 700), 63: (b, 0, 800), 64: (b, 50, 750), 65: (b, 0, 800), 66: (b, 10, 790)}),
        want=dict(run=(62, 66), flag={63: CONT, 65: 0}))
    add("run_begins_64", "a run that ends at 63 and one that begins exactly at 64", 3000,
        runs({61: (b, 0, 800), 62: (b, 100, 700), 63: (b, 200, 600), 64: (b + 2, 0, 800), 65: (b + 2, 100, 700), 66: (b + 2, 0, 800)}),
        want=dict(run=(64, 66), flag={62: CONT, 63: CONT, 64: CONT, 65: CONT, 66: 0}))
    b = NA + 63
    add("cont1_63_64", "the containment pair (63, 64), the earlier record inside the later (cont == 1)", 3000,
        runs({63: (b, 100, 700), 64: (b, 0, 800)}), want=dict(run=(63, 64), flag={63: CONT, 64: 0}))
    add("cont2_63_64", "the containment pair (63, 64), the later record inside the earlier (cont == 2)", 3000,
        runs({63: (b, 0, 800), 64: (b, 100, 700)}), want=dict(run=(63, 64), flag={63: 0, 64: CONT}))
    add("temp_63_64_later", "an OVL_TEMP pair (63, 64), the later record the shorter", 3000,
        runs({63: (b, 0, 2000), 64: (b, 1000, 2500, 1200)}), want=dict(run=(63, 64), flag={63: 0, 64: TEMP}))
    add("temp_63_64_earlier", "an OVL_TEMP pair (63, 64), the earlier record the shorter", 3000,
        runs({63: (b, 0, 1500), 64: (b, 1000, 3000, 1200)}), want=dict(run=(63, 64), flag={63: TEMP, 64: 0}))
    recs = [(NA, 60 * i, 60 * i + 50) for i in range(200)]
    recs[100] = (NA, 290, 350)                                         # holds 5: 5 is dropped at (5, 100) and paired no more
    recs[150] = (NA, 295, 345)                                         # holds 5 as well, lies inside 100: dropped by 100
    recs[160] = (NA, 302, 338)                                         # inside 5, 100 and 150
    add("run_200", "one run of 200 records walked by a single lane, with a chain of containments", 13000, recs,
        want=dict(run=(0, 199), flag={5: CONT, 100: 0, 150: CONT, 160: CONT}))
    b = NA + 61
    add("run_discarded_mid", "a record discarded in the input inside a run over 61..66: 62 and 64 pair across it", 3000,
        runs({61: (b, 900, 1000), 62: (b, 0, 800), 63: (b, 50, 750, None, None, DISCARD), 64: (b, 100, 700), 65: (b, 1000, 1100),
              66: (b, 1200, 1300)}), want=dict(run=(61, 66), flag={62: 0, 64: CONT}))

    # ---- bins and the prefix sum ---------------------------------------------------------------------------------------
    for nb in (63, 64, 65, 127, 128, 129):
        ln = BIN * nb - 50
        add("nb_%d" % nb, "a read of %d bins, a record reaching its last base: e as large as it gets" % nb, ln,
            [(NA, 0, ln), (NA + 1, 0, ln - 1000), (NA + 2, 0, ln - 1000)], want=dict(nb=nb, events=[(nb - 15, nb - 5)]))
    add("b_63_64", "a record whose first bin is 63 and one whose first bin is 64", 9000,
        [(NA, 0, 9000), (NA + 1, 5850, 9000), (NA + 2, 5950, 9000)], want=dict(events=[(4, 63)]))
    add("carry_only", "coverage made by the carry alone: records that begin in chunk 0 and end in chunk 2", 15000,
        [(NA,) + cover(5, 140), (NA + 1,) + cover(10, 135), (NA + 2,) + cover(20, 130)], want=dict(events=[(5, 10), (135, 140)]))
    add("lds_atomics", "101 records adding to the same two bins", 6000,
        [(NA,) + cover(5, 40)] + [(NA + 1 + i,) + cover(10, 30) for i in range(100)], want=dict(events=[(5, 10), (30, 40)]))

    # ---- the break scan: chunk c holds the bins B0 + 64 c .. B0 + 64 c + 63 ---------------------------------------------
    L = lambda c, lane: B0 + WAVE * c + lane
    scan = [
        ("thin_l63_l0", "a thin run that begins in lane 63, its break in the next chunk's lane 0",
         [(B0, L(0, 63)), (L(1, 0), L(1, 10))], [(L(0, 63), L(1, 0))]),
        ("break_l63", "a thin run whose break bin is lane 63", [(B0, 60), (L(0, 63), 85)], [(60, L(0, 63))]),
        ("first_l0", "a thin run whose first bin is lane 0 of the second chunk", [(B0, L(1, 0)), (80, 90)], [(L(1, 0), 80)]),
        ("whole_chunk", "a thin run over a whole chunk and more: begins in chunk 0, breaks in chunk 2",
         [(B0, 20), (L(2, 5), L(2, 15)), (B0, L(2, 15), 1)], [(20, L(2, 5))]),
        ("two_breaks_open", "two breaks in one chunk, a third run left open into the next",
         [(B0, 10), (15, 20), (25, 60), (L(1, 10), L(1, 20))], [(10, 15), (20, 25), (60, L(1, 10))]),
        ("trailing_l63", "a trailing run that opens in lane 63 of the last full chunk", [(B0, L(0, 63)), (L(0, 63), L(1, 4), 1)],
         [(L(0, 63), L(1, 4))]),
    ]
    for k in (63, 64, 65):
        scan.append(("trailing_%d" % k, "a trailing run in a pile with e0 - b0 = %d" % k, [(B0, B0 + k - 3), (B0 + k - 3, B0 + k, 1)],
                     [(B0 + k - 3, B0 + k)]))
    for tag, border, segs, evs in scan:
        add(tag, border, 20000, thick(segs), want=dict(b0=B0, events=evs))
    add("tb_not_first", "tb set by a record that is not first in file order", 20000,
        [(NA,) + cover(20, 40), (NA + 1,) + cover(B0, 40), (NA + 2,) + cover(B0 + 1, 40)] + thick([(45, 60)], NA + 3),
        want=dict(b0=B0, events=[(B0, B0 + 1), (40, 45)]))

    # ---- drop_break with the lanes over the records: a break (19, 30), p1 = 1800, p2 = 3100 ----------------------------
    LEFT, RIGHT, LLONG, RLONG = (50, 2440), (2560, 4950), (50, 2460), (2540, 4950)        # 2390 bases, and 2410
    def sides(n, special, flags=None):
        recs = [(NA + i,) + (LEFT if i % 2 == 0 else RIGHT) for i in range(n)]
        for i, r in special.items():
            recs[i] = (NA + i,) + r + (None, None, (flags or {}).get(i, 0))
        return recs
    for n in (64, 65, 129):
        add("longest_last_%d" % n, "the longest record at index n - 1, the others tied", 8000, sides(n, {n - 1: RLONG}),
            want=dict(kinds=[gm.DROP_L], longest=[n - 1]))
        add("longest_discarded_%d" % n, "the longest record discarded in the input: ignored", 8000,
            sides(n, {n - 1: (2500, 5000), 2: LLONG}, {n - 1: DISCARD}), want=dict(kinds=[gm.DROP_R], longest=[2]))
        # the first drop removes the pile's longest record (0), the second break's longest sits in the last stride
        recs = [(NA, 50, 4960)] + [(NA + i,) + (LEFT, RIGHT, cover(56, 70))[(n - 1 - i) % 3] for i in range(1, n)]
        last = n - 1
        recs[last] = (NA + last,) + LLONG
        add("two_drops_%d" % n, "two breaks: the first drop removes the longest record, the second's longest sits in another stride",
            8000, recs, want=dict(kinds=[gm.DROP_R, gm.DROP_R], longest=[0, last]))
        add("none_left_%d" % n, "a break with no live record left: DROP_NONE", 8000,
            [(NA, 0, 3000)] + [(NA + i, 200, 2800) for i in range(1, n)], want=dict(kinds=[gm.DROP_R, gm.DROP_NONE | gm.TRAILING]))
        if n > 64:
            add("tie_1_64_%d" % n, "a tie in length between 1 and 64 on different sides of the break: 1 decides", 8000,
                sides(n, {1: LLONG, 64: RLONG}), want=dict(kinds=[gm.DROP_R], longest=[1, 64]))
            add("tie_0_64_%d" % n, "a tie in length between 0 and 64, both lane 0: 0 decides", 8000,
                sides(n, {0: LLONG, 64: RLONG}), want=dict(kinds=[gm.DROP_R], longest=[0, 64]))

    # ---- exclude intervals: the break (15, 27), p1 = 1400, p2 = 2800 -------------------------------------------------------
    base = lambda: [(NA, 0, 2000), (NA + 1, 0, 2000), (NA + 2, 2300, 4500), (NA + 3, 2300, 4500)]
    IN1, IN2, OUT = (1350, 2850), (1300, 2900), (100, 200)
    def ivs(n, inside):
        return [inside.get(j, OUT) for j in range(n)]
    for tag, border, ex, ev in (
            ("ex_0", "a read without intervals: the break of ex_1, not masked", [], None),
            ("ex_1", "one interval, containing", ivs(1, {0: IN1}), IN1),
            ("ex_64", "64 intervals, the only containing one the last", ivs(64, {63: IN1}), IN1),
            ("ex_65_only64", "65 intervals, the only containing one at index 64", ivs(65, {64: IN1}), IN1),
            ("ex_1_and_64", "containing intervals at 1 and 64: 1 is reported", ivs(65, {1: IN2, 64: IN1}), IN2),
            ("ex_70_and_130", "131 intervals, containing ones at 70 and 130: 70 is reported", ivs(131, {70: IN2, 130: IN1}), IN2),
            ("ex_130", "130 intervals, the only containing one the last", ivs(130, {129: IN1}), IN1),
            ("ex_edge", "an interval that shares an edge with the break and does not mask it", [(1400, 2900), (1300, 2800)], None)):
        add(tag, border, 6000, base(), ex=ex, want=dict(masked=ev))

    # ---- stitch: the same break; a pair (i, i + 1) of one B read, 250 apart on A and on B -------------------------------------
    def pairs(n, at, delta=250, fi=0, fk=0):
        recs = [(NA + i,) + ((0, 2000) if i % 2 == 0 else (2300, 4500)) for i in range(n)]
        for i in at:
            recs[i] = (NA + i, 0, 2000, 100, 2100, fi)
            recs[i + 1] = (NA + i, 2000 + delta, 4500, 2100 + delta, 4600, fk)
        return recs
    add("stitch_three", "stitchable pairs (2, 3), (64, 65) and (129, 130): 3 under -s 300", 6000, pairs(131, (2, 64, 129)), want=dict(s300=3))
    add("stitch_63_64", "a stitchable pair (63, 64)", 6000, pairs(130, (63,)), want=dict(s300=1))
    add("stitch_equal", "a delta exactly equal to -s 100: not under it", 6000, pairs(6, (4,), delta=100), want=dict(s100=0, s300=1))
    add("stitch_comp", "one record of the pair complemented", 6000, pairs(6, (4,), fk=COMP), want=dict(s300=0))
    for nm, f in (("temp", TEMP), ("cont", CONT), ("trim", TRIM), ("stitch", STITCH)):
        add("stitch_flag_" + nm, "one record of the pair carrying OVL_%s" % nm.upper(), 6000, pairs(6, (4,), fi=f), want=dict(s300=0))

    # ---- the event slot: the recipe of synth.las's many_events ------------------------------------------------------------------
    many = lambda k: [r for j in range(k) for r in ((NA + 2 * j, 300 * j, 300 * j + 1000), (NA + 2 * j + 1, 300 * j, 300 * j + 1000))]
    add("events_16", "a pile of exactly DAMAR_GAP_MAXEVENTS events: stays on the device", 7000, many(17), want=dict(nev=16))
    add("events_17", "a pile of one event more: goes to the host", 7000, many(18), want=dict(nev=17))

    # ---- degenerate shapes ----------------------------------------------------------------------------------------------------
    deg = lambda *a, **k: add(*a, api_only=True, **k)
    deg("empty", "a pile of no records", 3000, [])
    deg("all_discarded", "records that all arrive discarded", 6000, [r + (None, None, DISCARD) for r in base()])
    deg("self_only", "self overlaps only", 6000, [(-1, 0, 3000, 0), (-1, 1000, 6000, 1000)])
    deg("all_short", "records all under 900 bases", 6000, [(NA, 0, 899), (NA + 1, 100, 950), (NA + 1, 120, 940)])
    deg("te_under_450", "te < 450: (te - 450) / 100 truncates to 0 from below", 6000, [(NA, 0, 440), (NA + 1, 10, 300)])
    deg("discarded_outside", "a record discarded in the input whose A coordinates lie outside the read: drop_break reads them",
        4600, thick([(5, 19), (30, 41)]) + [(NA + 9, -300, 5200, 100, 5600, DISCARD), (NA + 10,) + cover(30, 41)])
    deg("descending", "B reads that descend: the host's", 6000, [(NA + 5, 0, 2000), (NA + 5, 100, 1900), (NA + 1, 0, 2000), (NA + 1, 2300, 4500)])
    # outside what damar_gap_inputs_valid admits: the only input at which an e that is not held to nb shows
    S.append(Shape("live_past_end", "a live record that ends past its read: refused by the call, e held to nb by the model", 6000,
                   [(NA, 0, 9000), (NA + 1, 0, 8000)], api_only=True, refused=True))

    assert len(S) <= NA and len({s.tag for s in S}) == len(S)
    for a, s in enumerate(S):
        s.aread = a
        recs = []
        for b, ab, ae, bb, be, fl in s.recs:
            b = a if b == -1 else b
            bb = 100 + max(ab, 0) if bb is None else bb
            be = bb + (ae - ab) if be is None else be
            assert NA <= b < NREADS or b == a, s.tag
            assert 0 <= bb <= be <= BLEN, s.tag
            assert (fl or 0) & DISCARD or s.refused or 0 <= ab <= ae <= s.alen, s.tag
            recs.append((b, ab, ae, bb, be, fl or 0))
        s.recs = recs
        assert s.tag == "descending" or all(x[0] <= y[0] for x, y in zip(recs, recs[1:])), s.tag
    return S


def read_len(S):
    rl = np.full(NREADS, BLEN, dtype=np.int32)
    for s in S:
        rl[s.aread] = s.alen
    return rl


def arrays(S, rl=None):
    """the shapes S, in that order, as api.pile_gaps takes them -> (piles, read_len, (exclude anno, exclude data))"""
    rl = read_len(shapes()) if rl is None else rl
    cols = np.array([r for s in S for r in s.recs], dtype=np.int64).reshape(-1, 6)
    off = np.concatenate([[0], np.cumsum([len(s.recs) for s in S])]).astype(np.int64)
    piles = dict(pile_off=off, pile_aread=np.array([s.aread for s in S], dtype=np.int32), bread=cols[:, 0].astype(np.int32),
                 abpos=cols[:, 1].astype(np.int32), aepos=cols[:, 2].astype(np.int32), bbpos=cols[:, 3].astype(np.int32),
                 bepos=cols[:, 4].astype(np.int32), flags=cols[:, 5].astype(np.int32))
    ex = {s.aread: s.ex for s in S}
    anno, data = [0], []
    for r in range(len(rl)):
        for b, e in ex.get(r, []):
            data += [b, e]
        anno.append(4 * len(data))
    return piles, rl, (np.array(anno, dtype=np.uint64), np.array(data, dtype=np.int32))


def digest(piles, rl):
    """sha256 over the columns and read_len: what ties tests/golden/gap/shapes.json to this file"""
    h = hashlib.sha256()
    for k in ("pile_off", "pile_aread", "abpos", "aepos", "bbpos", "bepos", "bread", "flags"):
        h.update(np.ascontiguousarray(piles[k], dtype=np.int64).tobytes())
    h.update(np.ascontiguousarray(rl, dtype=np.int64).tobytes())
    return h.hexdigest()


def random_piles(seed=20261021):
    """about 150 seeded piles of 1 to 300 records on read lengths of 500 to 30 000: runs of 1 to 6 records of one B read,
    ascending, coverage thin enough for a few breaks per pile, every input flag, 0 to 5 exclude intervals per read
    -> (piles, read_len, (exclude anno, exclude data))"""
    rng = np.random.default_rng(seed)
    rl = rng.integers(500, 30001, size=NREADS).astype(np.int32)
    rows, off, areads = [], [0], []
    for a in np.sort(rng.choice(NREADS, size=150, replace=False)):
        alen = int(rl[a])
        n = 1 + int(300 * rng.random() ** 2.2)
        typ = max(300, min(alen, int(rng.uniform(1.5, 4.0) * alen / max(n, 1)) + 900))
        b, left = -1, n
        while left > 0:
            b = int(a) if rng.integers(15) == 0 and b < a else min(b + 1 + int(rng.integers(0, max(1, 2 * NREADS // max(n, 1)))), NREADS - 1)
            run = min(left, int(rng.integers(1, 7)))
            left -= run
            blen, prev = int(rl[b]), None
            for _ in range(run):
                if prev is not None and rng.integers(3) == 0:              # a contained, an equal or a stitchable record
                    kind, (ab, ae, bb, be) = int(rng.integers(3)), prev
                    if kind == 0:
                        q = (ae - ab) // 5
                        ab, ae, bb, be = ab + q, ae - q, bb + q, be - q
                    elif kind == 2:
                        d = int(rng.integers(0, 320))
                        ab, bb = min(ae + d, alen), min(be + d, blen)
                        ae, be = min(ab + typ, alen), min(bb + typ, blen)
                else:
                    ln = int(min(alen, max(50, typ * rng.uniform(0.3, 1.7))))
                    ab = 0 if rng.integers(5) == 0 else int(rng.integers(0, alen - ln + 1))
                    ae = alen if rng.integers(6) == 0 else ab + ln
                    span = min(ae - ab, blen)
                    bb = int(rng.integers(0, blen - span + 1))
                    be = bb + span
                fl = 0
                for bit, one_in in ((COMP, 3), (DISCARD, 12), (STITCH, 25), (TEMP, 25), (CONT, 25), (gm.GAP, 25), (TRIM, 25)):
                    fl |= bit if rng.integers(one_in) == 0 else 0
                prev = (ab, ae, bb, be)
                rows.append((b, ab, ae, bb, be, fl))
        areads.append(int(a))
        off.append(len(rows))
    cols = np.array(rows, dtype=np.int64)
    piles = dict(pile_off=np.array(off, dtype=np.int64), pile_aread=np.array(areads, dtype=np.int32), bread=cols[:, 0].astype(np.int32),
                 abpos=cols[:, 1].astype(np.int32), aepos=cols[:, 2].astype(np.int32), bbpos=cols[:, 3].astype(np.int32),
                 bepos=cols[:, 4].astype(np.int32), flags=cols[:, 5].astype(np.int32))
    anno, data = [0], []
    for r in range(NREADS):
        for _ in range(int(rng.integers(0, 6))):
            x = int(rng.integers(0, rl[r]))
            data += [x, int(rng.integers(x, rl[r] + 1))]
        anno.append(4 * len(data))
    return piles, rl, (np.array(anno, dtype=np.uint64), np.array(data, dtype=np.int32))


OPTION_SETS = (("def", dict()), ("s100", dict(stitch=100)), ("s300", dict(stitch=300)), ("e", dict(exclude=True)),
               ("es", dict(exclude=True, stitch=300)))


def model_runs(S, rl=None):
    """the model on the shapes S under every option set -> {name: Result}"""
    piles, rl, ex = arrays(S, rl)
    return {nm: gm.run(piles, rl, stitch=kw.get("stitch", 0), exclude=ex if kw.get("exclude") else None) for nm, kw in OPTION_SETS}


def hold_to_borders(S, runs):
    """every shape of S (none of them refused) sits on the border it names, by the model's results `runs`: a shape that
    drifts off fails here"""
    piles, rl, _ = arrays(S)
    off = piles["pile_off"]
    for p, s in enumerate(S):
        w, lo, n = s.want, int(off[p]), len(s.recs)
        res = runs["def"]
        fl, ev, info = res.flags[lo:lo + n], res.events[p], res.info[p]
        br = [r[0] for r in s.recs]
        if "run" in w:
            i, k = w["run"]
            assert len(set(br[i:k + 1])) == 1 and (i == 0 or br[i - 1] != br[i]) and (k == n - 1 or br[k + 1] != br[k]), s.tag
            assert n >= 130 and (i > 0 or n == 200), s.tag
            if n == 131:
                assert br[127] != br[128] and br[125] == br[127] and br[128] == br[130] and br[124] != br[125], s.tag
        for i, f in w.get("flag", {}).items():
            assert bool(fl[i] & CONT) == bool(f & CONT) and (fl[i] & DISCARD or not f & CONT), (s.tag, i, hex(fl[i]))
            assert f & CONT or bool(fl[i] & TEMP) == bool(f & TEMP), (s.tag, i, hex(fl[i]))
        if "nb" in w:
            assert info["nbins"] == w["nb"] and max(r[2] for r in s.recs) == s.alen, s.tag
        if "b0" in w:
            tb = min(r[1] for r, f in zip(s.recs, fl) if not f & (TEMP | CONT))
            assert gm.cdiv(tb + MIN_LR, BIN) == w["b0"] and w["b0"] % WAVE != 0, s.tag
        if "events" in w:
            assert [e[:2] for e in ev] == [tuple(x) for x in w["events"]], (s.tag, ev)
        if "kinds" in w:
            assert [e[2] for e in ev] == w["kinds"], (s.tag, ev)
            assert n in (64, 65, 129), s.tag
        if "longest" in w:
            top = max(r[2] - r[1] for r in s.recs if not r[5] & DISCARD)
            if len(w["kinds"]) == 1:                    # the records named are the longest live ones, tied among themselves
                assert [i for i, r in enumerate(s.recs) if r[2] - r[1] == top and not r[5] & DISCARD] == w["longest"], s.tag
                if len(w["longest"]) == 2:
                    p1 = (ev[0][0] - 1) * BIN
                    assert (s.recs[w["longest"][0]][1] < p1) != (s.recs[w["longest"][1]][1] < p1), s.tag
            else:                                       # the first is the longest and goes at the first break; then the second
                i0, i1 = w["longest"]
                assert s.recs[i0][2] - s.recs[i0][1] == top and fl[i0] & gm.GAP and i1 == n - 1, s.tag
                left = [r[2] - r[1] for r, f in zip(s.recs, runs["def"].flags[lo:lo + n]) if not f & DISCARD]
                assert left.count(max(left)) == 1 and s.recs[i1][2] - s.recs[i1][1] == max(left), s.tag
        if "masked" in w:
            e = runs["e"].events[p]
            assert len(e) == 1 and len(ev) == 1 and ev[0][2] == gm.DROP_L, (s.tag, e)
            assert e[0][2:5] == ((gm.MASKED,) + tuple(w["masked"]) if w["masked"] else (gm.DROP_L, 0, 0)), (s.tag, e)
        for key in ("s100", "s300"):
            if key in w:
                e = runs[key].events[p]
                assert len(e) == 1 and e[0][2:4] == ((gm.STITCHABLE, w[key]) if w[key] else (gm.DROP_L, 0)), (s.tag, key, e)
        if "nev" in w:
            assert all(r.info[p]["nev"] == w["nev"] for r in runs.values()), s.tag
        assert info["descends"] == (s.tag == "descending"), s.tag
