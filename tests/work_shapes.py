"""Planted seed lists for test_gpu_work_list.py: runs of seeds whose bucket sums are chosen, placed where the work-list
kernels (kernels/seed_merge.hip pair_work_mark / pair_heads_mark / pair_screen) change their code path.  What a list's work
items ARE is never decided here: that is tests/work_model.py, the reference's rule.  A planted run only carries a tag and
whether its maker meant it to fire, so that a test can tell that both kinds are present (and that maker and model agree).

The constants are those of kernels/seed_merge.hip (SCREEN_MAX 48, SCREEN_PANEL 50000, PW_HALO 64, PW_SMALL 8, PW_SHORT 4,
OR_MAX 2048) and kernels/kernels.h (DAMAR_SCAN_TILE 4096)."""
import copy

import numpy as np

import work_model as M

TILE = 4096               # DAMAR_SCAN_TILE (kernels/kernels.h): seeds per workgroup of pair_work_mark
HALO = 64                 # PW_HALO: seeds behind the tile that pair_work_mark holds in LDS
SCREEN_MAX = 48           # the longest run that is screened
SCREEN_PANEL = 50000      # the largest A position of a screened run
OR_MAX = 2048             # the longest run the ordering step takes

LADDER_PARAMS = [(14, 35, 6), (12, 35, 5), (14, 15, 6), (32, 35, 6)]
LADDER_LENGTHS = list(range(1, 10)) + [47, 48, 49, 64, 65, 66, 100]
MINHIT_EDGES = [1, 2, 3, 48, 49, 65, 66]          # with kmer 14: hitmin = 14 * minhit


def contribs(n, total, first, kmer):
    """what n seeds of one bucket add to its score: the first `first`, the others 0 .. kmer spread evenly, `total` in all"""
    rest = total - first
    assert n >= 1 and 0 <= rest <= (n - 1) * kmer, (n, total, first, kmer)
    out = [first]
    for left in range(n - 1, 0, -1):
        c = min(kmer, -(-rest // left))
        out.append(c)
        rest -= c
    assert rest == 0
    return out


def seeds_of(cs, diags, kmer, a0):
    """(apos, diag) of seeds that add cs[i] to their bucket: the first lies at a0 and adds min(kmer, a0); a seed that adds
    kmer lies kmer or more behind the one before it, one that adds 0 at the same A position"""
    assert cs[0] == min(kmer, a0) and a0 >= kmer - 1
    ap, out = a0, [(a0, diags[0])]
    for i, c in enumerate(cs[1:], 1):
        assert 0 <= c <= kmer
        ap += c if c < kmer else kmer + 3 * (i % 4)
        out.append((ap, diags[i]))
    return out


def bucket(n, total, d, kmer, binshift, a0=None, diags=None):
    """n seeds of diagonal bucket d whose score is exactly total (diags: their diagonals, all of one bucket)"""
    if a0 is None:
        a0 = kmer + 5 if total >= kmer else kmer - 1
    if diags is None:
        diags = [(d << binshift) + (5 * i) % (1 << binshift) for i in range(n)]
    else:
        diags = [diags[i % len(diags)] for i in range(n)]
    assert len({x >> binshift for x in diags}) == 1
    return seeds_of(contribs(n, total, min(kmer, a0), kmer), diags, kmer, a0)


def split_totals(n, kmer, hitmin):
    """(n1, t1, a0_1, n2, t2, a0_2): two buckets that reach hitmin only together"""
    n1 = n // 2
    n2 = n - n1
    assert n1 >= 1
    if 2 * kmer <= hitmin:
        t1 = max(kmer, hitmin - n2 * kmer)
        return n1, t1, None, n2, hitmin - t1, None
    assert 2 * (kmer - 1) >= hitmin > kmer - 1             # a seed at apos kmer - 1 adds kmer - 1: two of them are enough
    return n1, kmer - 1, kmer - 1, n2, kmer - 1, kmer - 1


def planted_run(kind, n, kmer, hitmin, binshift, d=-6):
    """-> (seeds, fires).  one_eq: one bucket, sum hitmin; one_lt: one bucket, hitmin - 1; adj: buckets d and d + 1 that
    reach hitmin only together; gap: the same sums in d and d + 2."""
    if kind == "one_eq":
        return bucket(n, hitmin, d, kmer, binshift), True
    if kind == "one_lt":
        return bucket(n, hitmin - 1, d, kmer, binshift), False
    n1, t1, a1, n2, t2, a2 = split_totals(n, kmer, hitmin)
    assert t1 < hitmin and t2 < hitmin and t1 + t2 >= hitmin
    d2 = d + 1 if kind == "adj" else d + 2
    return bucket(n1, t1, d, kmer, binshift, a1) + bucket(n2, t2, d2, kmer, binshift, a2), kind == "adj"


class Case:
    """A whole sorted seed list, unpacked, with the parameters it is meant for and its planted runs (start, length, tag, fires)"""

    def arrays(self):
        return self.bread, self.aread, self.apos, self.diag

    def truncated(self, n):
        c = copy.copy(self)
        c.bread, c.aread, c.apos, c.diag = (x[:n] for x in self.arrays())
        c.planted = [p for p in self.planted if p[0] + p[1] <= n]
        return c

    def run_starts(self):
        """start of every read pair's run, and len(list) behind them"""
        pair = (self.bread << 32) | self.aread
        return np.concatenate(([0], np.flatnonzero(pair[1:] != pair[:-1]) + 1, [len(pair)]))

    def order(self, how, rng):
        """A permutation of the list that moves seeds inside their runs only.  random; reversed; ties: random, but seeds of
        equal A position stay in the order they have; top_first / top_middle / top_last: the run's largest A position goes
        there, the others stay in order."""
        o = np.arange(len(self.bread))
        st = self.run_starts()
        for s, e in zip(st[:-1].tolist(), st[1:].tolist()):
            if e - s < 2:
                continue
            if how == "reversed":
                o[s:e] = o[s:e][::-1]
            elif how in ("random", "ties"):
                p = s + rng.permutation(e - s)
                if how == "ties":
                    a = self.apos[p]
                    for v in np.unique(a):
                        at = np.flatnonzero(a == v)
                        p[at] = np.sort(p[at])
                o[s:e] = p
            else:
                rest = list(range(s, e - 1))
                at = {"top_first": 0, "top_middle": len(rest) // 2, "top_last": len(rest)}[how]
                o[s:e] = rest[:at] + [e - 1] + rest[at:]
        return o


class Builder:
    def __init__(self, kmer, hitmin, binshift, seed, ppos=17, dbits=17, abits=10):
        self.kmer, self.hitmin, self.binshift = kmer, hitmin, binshift
        self.minhit = M.minhit_of(kmer, hitmin)
        self.ppos, self.dbits, self.abits = ppos, dbits, abits
        self.rng = np.random.default_rng(seed)
        self.b, self.a, self.n = 0, -1, 0
        self.cols = ([], [], [], [])
        self.planted = []
        self.fresh = False                                 # the next run starts a new B read

    def add(self, seeds, tag=None, fires=None):
        """one read pair's run: the seeds in key order (A position, then B position)"""
        seeds = sorted(seeds, key=lambda s: (s[0], s[0] - s[1]))
        if self.fresh or self.a + 1 >= (1 << self.abits):
            self.b, self.a, self.fresh = self.b + 1, 0, False
        else:
            self.a += 1
        for ap, dg in seeds:
            for col, x in zip(self.cols, (self.b, self.a, ap, dg)):
                col.append(x)
        if tag is not None:
            self.planted.append((self.n, len(seeds), tag, fires))
        self.n += len(seeds)
        return self.n - len(seeds)

    def plant(self, kind, n, tag=None, d=-6):
        seeds, fires = planted_run(kind, n, self.kmer, self.hitmin, self.binshift, d)
        return self.add(seeds, tag or "%s/%d" % (kind, n), fires)

    def plant_fire(self, fire, n, tag):
        """a run of n seeds that fires, or one that does not, of either make"""
        kinds = ("one_eq", "adj") if fire else ("one_lt", "gap")
        kind = kinds[int(self.rng.integers(0, 2))] if n >= 2 else kinds[0]
        return self.plant(kind, n, "%s:%s/%d" % (tag, kind, n))

    def filler(self, n=None, tag=None):
        """a read pair with too few seeds to be entered: 1 .. minhit - 1 of them (none where minhit is 1)"""
        if n is None:
            n = int(self.rng.integers(1, self.minhit)) if self.minhit > 1 else 0
        if n == 0:
            return
        assert n < self.minhit
        ap = np.cumsum(self.rng.integers(1, 40, n)) + self.kmer
        dg = -self.rng.integers(0, 600, n)
        self.add(list(zip(ap.tolist(), dg.tolist())), tag, None if tag is None else False)

    def pad_to(self, index):
        """filler pairs up to seed `index` exactly"""
        assert index >= self.n and (self.minhit > 1 or index == self.n), (index, self.n)
        while self.n < index:
            self.filler(min(index - self.n, int(self.rng.integers(1, self.minhit))))

    def case(self, name):
        c = Case()
        c.name, c.kmer, c.hitmin, c.binshift, c.minhit = name, self.kmer, self.hitmin, self.binshift, self.minhit
        c.ppos, c.dbits, c.abits = self.ppos, self.dbits, self.abits
        c.bread, c.aread, c.apos, c.diag = (np.array(x, dtype=np.int64) for x in self.cols)
        c.planted = list(self.planted)
        assert len(c.bread) <= 10 * TILE + 2 * HALO
        return c


def _extras(b):
    """the planted shapes beside the ladder: three buckets, the buckets around diagonal 0 and at multiples of 1 << binshift,
    a first seed at kmer - 1, equal A positions"""
    K, H, S = b.kmer, b.hitmin, b.binshift
    W = 1 << S
    far = 4 * W + K                                        # an A position at which every diagonal used here has bpos >= 0
    if 2 * K - 1 < H:                                      # three buckets: only one pair of neighbours reaches hitmin
        ta, na = H - K, -(-(H - K) // K)
        for name, lo, hi, fires in (("three_low", ta, K - 1, True), ("three_high", K - 1, ta, True),
                                    ("three_low_lt", ta - 1, K - 1, False), ("three_high_lt", K - 1, ta - 1, False)):
            b.filler()
            seeds = bucket(na if lo >= K else 1, lo, -7, K, S) + bucket(1, K, -6, K, S) + bucket(na if hi >= K else 1, hi, -5, K, S)
            b.add(seeds, name, fires)
    n = max(2, b.minhit)
    n1, t1, a1, n2, t2, a2 = split_totals(n, K, H)
    a1, a2 = (far, far) if a1 is None else (a1, a2)
    for name, da, db, fires in (("diag_-1_0", -1, 0, True), ("diag_-W_0", -W, 0, True), ("diag_-W-1_0", -W - 1, 0, False),
                                ("diag_-1_W", -1, W, False), ("diag_W-1_2W", W - 1, 2 * W, False), ("diag_W-1_W", W - 1, W, True),
                                ("diag_-2W-1_-1", -2 * W - 1, -1, False)):
        if a1 < far and (da > 0 or db > 0):
            continue                                       # (a seed at apos kmer - 1 has no positive diagonal that wide)
        b.filler()
        b.add(bucket(n1, t1, 0, K, S, a1, [da]) + bucket(n2, t2, 0, K, S, a2, [db]), name, fires)
    for name, dd, tot in (("same_W_2W-1", [W, 2 * W - 1], H), ("same_W_2W-1_lt", [W, 2 * W - 1], H - 1),
                          ("same_-W_-1", [-W, -1], H), ("same_-W_-1_lt", [-W, -1], H - 1),
                          ("same_-2W_-W-1", [-2 * W, -W - 1], H), ("same_-2W_-W-1_lt", [-2 * W, -W - 1], H - 1)):
        b.filler()
        b.add(bucket(n, tot, 0, K, S, far, dd), name, tot >= H)
    m = b.minhit
    b.filler()                                             # the first seed at kmer - 1 adds kmer - 1 ...
    b.add(bucket(m, H - 1, -6, K, S, K - 1), "first_at_k-1", False)
    b.filler()                                             # ... and at kmer, kmer
    b.add(bucket(m, H, -6, K, S, K), "first_at_k", True)
    if H - 1 - K >= 0:                                     # the second of two seeds at one A position adds 0
        cs = [K, 0] + (contribs(m, H - 1, K, K)[1:] if m > 1 else [])
        if sum(cs) == H - 1:
            b.filler()
            b.add(seeds_of(cs, [(-6 << S) + 3 * i for i in range(len(cs))], K, K + 2), "tie_adds_0", False)


def ladder(kmer, hitmin, binshift):
    """Every length of LADDER_LENGTHS that is at least minhit, four ways, with fillers between; the extras; then the ladder
    again across the border of the first two tiles."""
    b = Builder(kmer, hitmin, binshift, seed=kmer * 100 + hitmin)
    for rep in range(2):
        for n in LADDER_LENGTHS:
            if n < b.minhit:
                continue
            for kind in ("one_eq", "one_lt", "adj", "gap"):
                if n < 2 and kind in ("adj", "gap"):
                    continue
                b.filler()
                b.plant(kind, n)
        if rep == 0:
            _extras(b)
            b.pad_to(max(b.n, TILE - 700))
    b.filler()
    return b.case("ladder_%d_%d_%d" % (kmer, hitmin, binshift))


def minhit_edge(minhit):
    """kmer 14 and hitmin 14 * minhit.  1 and 2: more than a tile in which every seed, or every second one, is a head.  3 and
    48: the ladder's four makes at the lengths around them.  49, 65, 66 (never screened; 65 the last minhit read from LDS, 66
    the first read from keys): runs of minhit - 1 and of minhit seeds that end with a tile, that start on a tile's last seed,
    and a last run of minhit + 1 seeds that ends the list (truncated(n - 1), truncated(n - 2): of minhit, of minhit - 1)."""
    K, S = 14, 6
    H = K * minhit
    b = Builder(K, H, S, seed=minhit)
    kinds = ("one_eq", "one_lt", "adj", "gap")
    if minhit == 1:
        for i in range(TILE + 300):
            if b.rng.integers(0, 2):
                b.add([(K - 1, -int(b.rng.integers(0, 500)))], "single_at_k-1", False)
            else:
                b.add([(K + int(b.rng.integers(0, 900)), -int(b.rng.integers(0, 500)))], "single", True)
    elif minhit == 2:
        for i in range(TILE // 2 + 150):
            b.plant(kinds[int(b.rng.integers(0, 4))], 2)
    elif minhit in (3, 48):
        for rep in range(2):
            for n in ([3, 4, 5, 6, 7, 8, 9] if minhit == 3 else [48, 49]):
                for kind in kinds:
                    b.filler()
                    b.plant(kind, n)
            b.filler(minhit - 1)
            if rep == 0 and minhit == 48:
                b.pad_to(TILE - 60)
    else:
        m = minhit
        for t, (start, n) in enumerate([(TILE - m, m), (2 * TILE - (m - 1), m - 1), (3 * TILE - 1, m), (4 * TILE - 1, m - 1)]):
            b.pad_to(start)
            if n < m:
                b.filler(n, "t%d/%d" % (t, n))
            else:
                b.plant("one_eq", n, "t%d/%d" % (t, n))
        b.pad_to(5 * TILE + 100)
        b.plant("one_eq", m + 1, "last")
    return b.case("minhit_%d" % minhit)


def tile_geometry(variant):
    """(14, 35, 6): heads at tile offsets 0, 1, 4095 - 48, 4095 - 8 and 4095; a run of 48 from offset 4095 (screened in the
    halo), runs of 49 and 65 from there; a run whose successor's head is the next tile's first seed; offset 0 after another
    pair and inside the previous tile's last run; a tile with no head between two that have some; a last run that ends the
    list.  Some planted runs fire and some do not; variant 1 swaps the two."""
    b = Builder(14, 35, 6, seed=50 + variant)
    T = TILE

    def run(n, tag, fire):
        return b.plant_fire(fire != bool(variant), n, tag)

    run(3, "list_start", True)
    b.pad_to(T - 1 - 48)
    run(48, "off_4095-48", False)
    assert b.n == T - 1
    run(48, "halo_48", True)
    b.pad_to(2 * T - 1 - 8)
    run(8, "off_4095-8", False)
    assert b.n == 2 * T - 1
    run(49, "halo_49", False)
    b.pad_to(3 * T - 1)
    run(65, "halo_65", True)
    b.pad_to(4 * T - 5)
    run(5, "ends_with_tile", True)
    assert b.n == 4 * T
    run(4, "off_0_after_another_pair", False)
    b.pad_to(5 * T - 2)
    run(6, "over_the_border", True)                        # (the next tile's first seed is no head)
    run(3, "behind_it", False)
    b.pad_to(6 * T - 1)
    run(48, "halo_48_again", False)
    b.pad_to(7 * T)
    b.filler(1)
    run(3, "off_1", True)
    b.pad_to(8 * T - 1 - 8)
    run(8, "off_4095-8_again", True)
    b.filler(1)
    b.pad_to(9 * T)                                        # tile 8: no head at all
    run(3, "off_0_behind_an_empty_tile", False)
    run(7, "next", True)
    b.pad_to(9 * T + 500)
    run(4, "list_end", False)
    return b.case("tiles_%d" % variant)


def list_of_length(nhits, last):
    """(14, 35, 6): nhits seeds whose last run, of `last` seeds and firing, ends the list"""
    b = Builder(14, 35, 6, seed=nhits * 7 + last)
    if nhits <= last:
        if nhits >= 3:
            b.plant("one_eq", nhits, "whole")
        else:
            b.add(bucket(nhits, 14 * nhits, -6, 14, 6), "whole", False)
    else:
        if nhits > 1000:
            b.plant("one_eq", 5, "first")
        b.pad_to(nhits - last)
        b.plant("adj", last, "last")
    assert b.n == nhits
    return b.case("nhits_%d_%d" % (nhits, last))


def mixed(kmer, hitmin, long_share, seed):
    """Three tiles of runs of 1 .. 8 seeds at random, of the four makes at random -- more than 600 heads a tile, so that every
    register variant of the one-lane screen runs with shorter runs beside it; long_share of the runs have 9 .. 48 seeds."""
    b = Builder(kmer, hitmin, 6, seed=seed)
    kinds = ("one_eq", "one_lt", "adj", "gap")
    while b.n < 3 * TILE:
        n = int(b.rng.integers(9, 49)) if b.rng.random() < long_share else int(b.rng.integers(1, 9))
        if n < b.minhit:
            b.filler(n)
        else:
            b.plant(kinds[int(b.rng.integers(0, 4))] if n >= 2 else kinds[int(b.rng.integers(0, 2))], n)
    return b.case("mixed_%d_%d_%d" % (kmer, hitmin, int(100 * long_share)))


def panel():
    """(14, 35, 6), ppos 17: runs that do not fire whose largest A position is 50000 (one panel: dropped) or 50001 (not
    screened: kept), and one that fires at 50000; at lengths of every screen (3, 4: short; 5, 8: small; 9, 48: a wavefront),
    in the middle of a tile and from a tile's last seed."""
    K, H, S = 14, 35, 6
    b = Builder(K, H, S, seed=9)

    def run(n, top, tag):
        cs = [K] + contribs(n - 1, H - 1 - 2 * K, 0, K)[1:] + [K]      # (the last seed, moved to `top`, adds kmer)
        assert len(cs) == n and sum(cs) == H - 1
        seeds = seeds_of(cs, [(-6 << S) + (3 * i) % (1 << S) for i in range(n)], K, K + 1)
        seeds[-1] = (top, seeds[-1][1])
        b.add(seeds, tag, False)

    for n in (3, 4, 5, 8, 9, 48):
        for top in (SCREEN_PANEL, SCREEN_PANEL + 1):
            b.filler()
            run(n, top, "top_%d/%d" % (top, n))
    b.filler()
    seeds, _ = planted_run("one_eq", 5, K, H, S)
    b.add(seeds[:-1] + [(SCREEN_PANEL, seeds[-1][1])], "fires_at_50000", True)
    for t, (n, top) in enumerate([(5, SCREEN_PANEL + 1), (5, SCREEN_PANEL), (12, SCREEN_PANEL + 1), (12, SCREEN_PANEL)], 1):
        b.pad_to(t * TILE - 1)
        run(n, top, "halo_top_%d/%d" % (top, n))
    b.filler()
    return b.case("panel")


SLICE_UNIT = 160          # seeds per slice of the list below at nshift 6


def sliced():
    """(14, 35, 6): 64 * 160 seeds, a B read per stretch of 160, so that with nshift 6 a slice ends every 160 seeds (25 ends a
    tile) and with nshift 2 every 2560.  Every second end e has a firing head at e - minhit - 1 (entered), the others at
    e - minhit (not entered); where t % 4 == 2 the B read goes on for 7 seeds behind the nominal end, and the end with it.
    A firing or non-firing run starts every stretch.  -> (case, ends)"""
    b = Builder(14, 35, 6, seed=77)
    U, m = SLICE_UNIT, 3
    ends = []
    for t in range(1, 65):
        e = t * U + (7 if t % 4 == 2 else 0)
        n = m + 1 if t % 2 else m
        b.fresh = True
        b.plant_fire(bool(b.rng.integers(0, 2)), int(b.rng.integers(3, 7)), "stretch_%d" % t)
        b.pad_to(e - n)
        b.plant("one_eq" if t % 3 else "adj", n, "end_%d-%d" % (t, n))
        assert b.n == e
        ends.append(e)
    return b.case("sliced"), ends


def too_long(n, seed):
    """(14, 35, 6): a run of n seeds (2048: the longest that is ordered) on a B read of its own between short runs"""
    K, S = 14, 6
    b = Builder(K, 35, S, seed=seed)
    b.filler()
    b.plant("one_eq", 5)
    b.filler()
    b.plant("one_lt", 4)
    b.fresh = True
    b.add([(K + 14 * i, (-6 << S) + i % 50) for i in range(n)], "long_%d" % n, True)
    c_long = b.b
    b.fresh = True
    b.filler()
    b.plant("adj", 6)
    b.filler()
    b.plant("gap", 6)
    b.filler()
    c = b.case("too_long_%d" % n)
    c.long_bread = c_long
    return c
