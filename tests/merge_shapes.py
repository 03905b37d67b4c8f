"""Planted k-mer indexes for the merge of two sorted indexes into seed pairs (kernels/seed_merge.hip: merge_tiles, merge_fast,
merge_sweep / merge_sweep_tile, merge_emit, merge_range, merge_bread_hist), for tests/test_merge_shapes_host.py (the oracle
on the planted shapes, no GPU) and tests/test_gpu_merge_shapes.py (the kernels against the oracle).

The handle is a read of exactly k bases: it holds one k-mer, so a block of such reads has an index that is a chosen multiset of
codes, one read per entry.  A Plan lists the runs of one block's index in ascending code order and knows the index at which
each run starts; a Case is one comparison: two Plans (one for a self comparison), a few "rich" reads (homopolymers: one code
many times in one read; one random read of 1500 bases: several codes per read and a realistic pbits), the table of what was
planted (tag, code, A-run length, B-run length, kept or capped as its maker expects) and the checks of the geometry the case
is named for, which run on the ORACLE's index arrays.  A pair of one-k-mer reads never reaches minhit = 3 seeds, so the report
stage behind damar_match gets (next to) nothing and the comparison is about the merge.

The order of the reads inside a block is shuffled with a fixed seed: read id is not monotone in code.  Everything is made from
fixed seeds: CASES is the same table in every process.

The constants below are those of kernels/seed_merge.hip and shim.hip; a change there must be made here on purpose."""
import ctypes as C
import zlib

import numpy as np

MT_PER = 4
MT_A = 1024                 # A entries per tile
MT_BCAP = 3072              # B codes staged in LDS per tile
MT_HITS = 4                 # seed pairs a thread has in flight in merge_emit: rounds of 256 * MT_HITS
MT_NBK = 2048               # buckets over a tile's code range
MT_SMP = 8192               # samples of B in merge_tiles (half as many for 64-bit codes)
WINDOW = 64                 # entries in which the ends of a border run are looked for first
MAXGRAM = 10000             # the cap on mutual matches, filter.c:71

K32, K64 = 14, 17           # 32-bit codes (four per 16-byte vector) and 64-bit codes (two)


def NS(k):
    return MT_SMP if k <= 16 else MT_SMP // 2


def VPK(k):
    return 4 if k <= 16 else 2


def bases_of(codes, k):
    """the mapping from a code to its bases, fixed once: base i of the k-mer is bits 2 (k - 1 - i) of the code"""
    c = np.asarray(codes, dtype=np.uint64)
    sh = (2 * (k - 1 - np.arange(k))).astype(np.uint64)
    return ((c[:, None] >> sh[None, :]) & np.uint64(3)).astype(np.uint8)


def revcomp(code, k):
    r = 0
    for _ in range(k):
        r = (r << 2) | (3 - (code & 3))
        code >>= 2
    return r


class Plan:
    """The one-k-mer reads of a block as runs (tag, code, count), codes ascending, and the index each run starts at.  Codes
    given by run() are multiples of 4, those of fill() are 1 mod 4 (their reverse complements begin with T and G: above every
    planted code, wherever a complemented block is compared).  loose() takes codes above all of these, in any order, and
    extern() makes room for the entries a rich read puts in front."""

    def __init__(self, k):
        self.k, self.runs, self.extra, self.rich = k, [], [], []
        self.at, self.next, self.shift = 0, 4, 0

    def extern(self, n):
        assert not self.runs
        self.at += n
        self.shift += n

    def add(self, tag, code, n):
        code = int(code)
        assert n > 0 and (not self.runs or code > self.runs[-1][1]), (tag, code)
        self.runs.append((tag, code, n))
        start = self.at
        self.at += n
        self.next = (code // 4 + 1) * 4
        return code, start

    def run(self, tag, n):
        return self.add(tag, self.next, n)

    def fill(self, n, other=None, every=7):
        """n single entries; every `every`th code gets one entry in `other` too"""
        for i in range(n):
            c, _ = self.add(None, self.next + 1, 1)
            if other is not None and i % every == 0:
                other.add(None, c, 1)

    def fill_to(self, index, other=None):
        assert index >= self.at, (index, self.at)
        self.fill(index - self.at, other)

    def loose(self, tag, code, n):
        self.extra.append((tag, int(code), n))

    def codes(self):
        """the planted one-k-mer codes, sorted (without the rich reads' k-mers)"""
        top = self.runs[-1][1] if self.runs else 0
        assert all(c > top for _, c, _ in self.extra)
        rr = self.runs + self.extra
        return np.sort(np.repeat(np.array([r[1] for r in rr], dtype=np.uint64), [r[2] for r in rr]))


class Case:
    def __init__(self, cid, group, k, self_=0, comp=0, identity=0):
        self.id, self.group, self.k, self.self_, self.comp, self.identity = cid, group, k, self_, comp, identity
        self.a = Plan(k)
        self.b = self.a if self_ else Plan(k)
        self.table = []                 # (tag, code, A-run length, B-run length, "kept" | "capped")
        self.checks = []                # callables over the oracle's context: the geometry the case is named for
        self.flagged = None             # tiles left to the general kernel: None (not asserted), ">0" or the exact number
        self.lowmem = False             # run under a squeezed MEM_LIMIT
        self.caps = None                # slab cases: callables (seed pairs per B read) -> DAMAR_TEST_SEED_CAP

    def plant(self, tag, code, na, nb, expect=None):
        if expect is None:
            expect = "kept" if na * nb < MAXGRAM else "capped"
        self.table.append((tag, int(code), na, nb, expect))

    def reads(self, plan):
        rr = plan.runs + plan.extra
        codes = np.repeat(np.array([r[1] for r in rr], dtype=np.uint64), [r[2] for r in rr])
        assert codes.max() < 4 ** self.k
        rows = list(bases_of(codes, self.k)) + [np.asarray(b, dtype=np.uint8) for _, b in plan.rich]
        rng = np.random.RandomState(zlib.crc32(self.id.encode()) & 0x7fffffff)
        return [rows[i] for i in rng.permutation(len(rows))]

    def dbs(self):
        """(A block, B block) as HITS_DBs, the B block complemented where the case says so (in place, by `comp_fn`)"""
        import la_shapes
        adb = la_shapes.make_db(self.reads(self.a))
        bdb = la_shapes.make_db(self.reads(self.b))
        return adb, bdb


def _rand1500(k):
    """a random read of C, G and T only: every k-mer is above 4^(k-1), beyond the planted codes"""
    return ("rand1500", np.random.RandomState(1500 + k).randint(1, 4, 1500).astype(np.uint8))


def _homo(base, n):
    return np.full(n, base, dtype=np.uint8)


# ---- what a check sees: the oracle's indexes and seeds of a case -------------------------------------------------------

class Ctx:
    pass


_ctx = {}


def squeeze_memory(full, na, nb, one_index, dbb, seeds_under):
    """MEM_LIMIT squeezed as in test_gpu_memory_limit_lowers_the_cap_like_the_oracle: step down through fractions of the
    uncapped seeds until the oracle's LAST_LIMIT lies between 2 and 5000.  -> (mem, seeds, limit)"""
    import oracle_api as O
    for frac in (.9, .8, .7, .6):
        avail = int(full * frac / .98) + 8
        words = (2 * avail + na) if one_index else (avail + na + nb)           # undo filter.c:2646-2650
        if not one_index and words > na + 2 * nb:
            words = 2 * avail + na
        mem = 16 * words + dbb
        w = seeds_under(mem)
        if 2 < O.LAST_LIMIT < 5000 and 0 < len(w) < full:
            return mem, w, O.LAST_LIMIT
    raise AssertionError("no memory limit found that lowers the cap")


def db_bytes(db):
    from damar_amd import api
    return C.sizeof(api.HITS_DB) + C.sizeof(api.HITS_READ) * (db.nreads + 2) + db.totlen + db.nreads + 4


def context(case):
    """the oracle's view of a case, computed once per process: A and B index (KMER_DT), the seeds (SEED_DT), the cap"""
    if case.id in _ctx:
        return _ctx[case.id]
    import oracle_api as O
    x = Ctx()
    x.case = case
    adb, bdb = case.dbs()
    if case.comp:
        O.lib().damar_complement_block(C.byref(bdb), 1)
    prm = O.params(k=case.k, identity=case.identity)
    pa, na, x.A = O.sort_kmers(adb, prm)
    one = case.self_ and not case.comp
    if one:
        pb, nb, x.B = pa, na, x.A
    else:
        pb, nb, x.B = O.sort_kmers(bdb, prm)
    x.nrb = bdb.nreads

    def seeds_under(mem):
        prm.mem_limit = mem
        return O.seed_pairs(adb, bdb, pa, na, pb, nb, case.self_, case.comp, prm)

    x.mem = None
    x.want = seeds_under(64 << 30)
    x.limit = O.LAST_LIMIT
    x.full = len(x.want)
    if case.lowmem:
        x.mem, x.want, x.limit = squeeze_memory(x.full, na, nb, one, db_bytes(adb) + db_bytes(bdb), seeds_under)
    x.acode, x.bcode = x.A["code"], x.B["code"]
    # the A entry of every seed: (read, position) names an entry
    key = (x.A["read"].astype(np.int64) << 32) | x.A["rpos"].astype(np.int64)
    order = np.argsort(key, kind="stable")
    skey = (x.want["aread"].astype(np.int64) << 32) | x.want["apos"].astype(np.int64)
    x.order, x.key_sorted = order, key[order]
    x.entry = order[np.searchsorted(key[order], skey)] if len(skey) else np.zeros(0, dtype=np.int64)
    x.per_entry = np.bincount(x.entry, minlength=len(x.A))
    x.ntiles = (len(x.A) + MT_A - 1) // MT_A
    x.tile_hits = np.add.reduceat(x.per_entry, np.arange(0, len(x.A), MT_A)) if len(x.A) else np.zeros(0, int)
    x.keep = (adb, bdb)
    _ctx[case.id] = x
    return x


def entry_of(x, aread, apos):
    """index in the A index of the entry a seed record names"""
    k = (int(aread) << 32) | int(apos)
    i = np.searchsorted(x.key_sorted, k)
    return int(x.order[i]) if i < len(x.order) and x.key_sorted[i] == k else -1


def run_of(codes, code):
    """[start, end) of a code's run in a sorted code array"""
    return int(np.searchsorted(codes, np.uint64(code), "left")), int(np.searchsorted(codes, np.uint64(code), "right"))


def piece(x, tile):
    """[b0, b1): the B entries whose codes lie between the first and the last code of an A tile (merge_tiles)"""
    a0, a1 = tile * MT_A, min(len(x.acode), (tile + 1) * MT_A)
    return int(np.searchsorted(x.bcode, x.acode[a0], "left")), int(np.searchsorted(x.bcode, x.acode[a1 - 1], "right"))


def run_hits(x, code):
    s, e = run_of(x.acode, code)
    return int(x.per_entry[s:e].sum())


def flagged_tiles(x):
    """The tiles merge_fast hands to the general kernel, by its rule restated on the oracle's indexes: the B piece exceeds
    MT_BCAP, or some A code of the tile has a B run longer than pad[1] = (limit - 1) / (longest possible A run of the tile:
    from the start of the run of its first entry to the end of the run of its last).  (Not the modes in which merge_fast
    does not run at all.)"""
    cb, nb = np.unique(x.bcode, return_counts=True)
    out = set()
    for t in range(x.ntiles):
        a0, a1 = t * MT_A, min(len(x.acode), (t + 1) * MT_A)
        b0, b1 = piece(x, t)
        if b1 - b0 > MT_BCAP:
            out.add(t)
            continue
        arun = run_of(x.acode, x.acode[a1 - 1])[1] - run_of(x.acode, x.acode[a0])[0]
        codes = np.unique(x.acode[a0:a1])
        i = np.minimum(np.searchsorted(cb, codes), len(cb) - 1)
        ok = cb[i] == codes
        if ok.any() and int(nb[i[ok]].max()) > (x.limit - 1) // arun:
            out.add(t)
    return out


def cross_closed_form(x, limit):
    """sum over codes of na * nb where na * nb < limit (filter.c:1334-1335)"""
    ca, na = np.unique(x.acode, return_counts=True)
    cb, nb = np.unique(x.bcode, return_counts=True)
    _, ia, ib = np.intersect1d(ca, cb, return_indices=True)
    prod = na[ia].astype(np.int64) * nb[ib].astype(np.int64)
    return int(prod[prod < limit].sum())


def describe(case, x, rec):
    """where a seed record belongs: its A entry, tile, code and the planted run of that code"""
    i = entry_of(x, rec["aread"], rec["apos"])
    if i < 0:
        return "a record whose (aread, apos) names no A entry"
    code = int(x.acode[i])
    s, e = run_of(x.acode, code)
    tags = [t[0] for t in case.table if t[1] == code]
    return "A entry %d (tile %d, entry %d of it), code %#x, A run [%d, %d), B run of %d, planted as %s" % (
        i, i // MT_A, i % MT_A, code, s, e, run_of(x.bcode, code)[1] - run_of(x.bcode, code)[0], tags or "filler")


# ---- checks shared by the groups ------------------------------------------------------------------------------------

def _chk_codes(case):
    """the mapping from code to bases, asserted against the oracle's index: its codes are the intended ones"""
    def chk(x):
        if not any(p.rich for p in (case.a, case.b)):
            assert np.array_equal(x.acode, case.a.codes())
            if not case.comp:
                assert np.array_equal(x.bcode, case.b.codes())
        else:                           # (with rich reads: the planted codes are a sub-multiset, in place below 4^(k-1))
            top = 4 ** (case.k - 1)
            for plan, got in ((case.a, x.acode),) + (() if case.comp else ((case.b, x.bcode),)):
                want = plan.codes()
                want = want[want < top]
                have = got[got < np.uint64(top)]
                assert len(have) == len(want) + plan.shift and np.array_equal(have[plan.shift:], want)
    return chk


def _chk_table(case):
    """every planted run has the lengths and the fate its maker says"""
    def chk(x):
        for tag, code, na, nb, expect in case.table:
            s, e = run_of(x.acode, code)
            assert e - s == na, (tag, e - s, na)
            if nb is not None:
                bs, be = run_of(x.bcode, code)
                assert be - bs == nb, (tag, be - bs, nb)
            hits = run_hits(x, code)
            if expect == "capped":
                assert hits == 0, (tag, hits)
            elif expect == "kept":
                assert hits > 0, tag
                if not case.self_:
                    assert hits == na * nb, (tag, hits)
            else:                       # a self run of N identical reads: the exact count
                assert hits == expect, (tag, hits, expect)
    return chk


def _chk_cross_total(case):
    def chk(x):
        assert len(x.want) == cross_closed_form(x, x.limit)
    return chk


def _chk_start(tag, code, start):
    def chk(x):
        assert run_of(x.acode, code)[0] == start, (tag, run_of(x.acode, code), start)
    return chk


def _finish(case):
    case.checks = [_chk_codes(case), _chk_table(case)] + ([] if case.self_ else [_chk_cross_total(case)]) + case.checks
    for plan in (case.a, case.b):
        if plan.runs:
            assert plan.runs[-1][1] < 4 ** (case.k - 1)
    return case


# ---- A: the B sample table and the piece search ----------------------------------------------------------------------

def _pick(rng, lo, hi, n, forced):
    """n distinct codes of [lo, hi], the forced ones among them, sorted"""
    forced = sorted(set(c for c in forced if lo <= c <= hi))
    pool = np.setdiff1d(np.arange(lo, hi + 1), forced)
    assert len(pool) + len(forced) >= n
    return np.sort(np.concatenate([rng.choice(pool, n - len(forced), replace=False), forced]).astype(np.int64))


def _a_blen(k, name, n):
    c = Case("A_blen_%s-k%d" % (name, k), "A", k)
    rng = np.random.RandomState(n)
    B0, G = 8000, 4
    bc = B0 + G * np.arange(n)
    for code in bc:
        c.b.add(None, code, 1)
    j = n // 2
    lo, hi = int(bc[0]), int(bc[-1])
    for code in _pick(rng, B0 - 2000, int(bc[j]) - 3, MT_A, [B0 - 2000, B0 - 1] + ([lo] if j > 0 else [])):
        c.a.add(None, code, 1)                                              # tile 0: from below B to its middle
    for d, cnt in ((2, 341), (1, 341), (0, 342)):                           # tile 1: inside one stretch of B
        c.a.add("same_stretch" if d == 0 else None, int(bc[j]) - d, cnt)
    c.plant("same_stretch", int(bc[j]), 342, 1)
    for code in _pick(rng, int(bc[j]) + 1, hi + 2000, MT_A, [hi + 1, hi + 2000] + ([hi] if j < n - 1 else [])):
        c.a.add(None, code, 1)                                              # tile 2: from the middle to above B
    for d in range(7):                                                      # tile 3: all above B's last code
        c.a.add(None, hi + 2001 + d, 1)

    def chk(x):
        ns = NS(k)
        assert len(x.bcode) == n and len(x.acode) == 3 * MT_A + 7
        stride = (n + ns - 1) // ns
        smp = x.bcode[np.minimum((np.arange(ns) + 1) * stride - 1, n - 1)]
        st = lambda code: int(np.searchsorted(smp, code, "left"))
        assert (x.acode < x.bcode[0]).any() and (x.acode > x.bcode[-1]).any()
        assert (x.acode == x.bcode[0]).any() and (x.acode == x.bcode[-1]).any()
        assert st(x.acode[MT_A]) == st(x.acode[2 * MT_A - 1]) < ns          # tile 1: one stretch
        if n > 2:
            assert st(x.acode[MT_A - 1]) - st(x.acode[0]) >= (n // 2) // stride // 2 > 100      # tile 0: far apart
        assert st(x.acode[3 * MT_A]) == ns                                  # tile 3: beyond every stretch
        if n > ns:                                                          # stretches that start beyond the end repeat the last code
            assert ((np.arange(ns) * stride) >= n).sum() > 1000 and smp[-1] == smp[(n - 1) // stride]
        assert piece(x, 3) == (n, n)
        assert x.tile_hits[3] == 0 and x.tile_hits[1] == 342
    c.checks.append(chk)
    return _finish(c)


def _a_disjoint(k):
    c = Case("A_disjoint-k%d" % k, "A", k)
    for i in range(2 * MT_A + 5):
        c.a.add(None, 1001 + 2 * i, 1)
    for i in range(3000):
        c.b.add(None, 1000 + 2 * i, 1)

    def chk(x):
        assert len(np.intersect1d(x.acode, x.bcode)) == 0 and len(x.want) == 0
        assert piece(x, 0)[1] - piece(x, 0)[0] == MT_A - 1                  # (pieces are not empty: no partner all the same)
    c.checks.append(chk)
    return _finish(c)


# ---- B: runs over tile borders -----------------------------------------------------------------------------------------

def _b_len(la, keep):
    return (MAXGRAM - 1) // la if keep else -(-MAXGRAM // la)


def _b_borders(k):
    c = Case("B_cross_borders-k%d" % k, "B", k)
    c.a.rich.append(_rand1500(k))
    c.b.rich.append(_rand1500(k))
    for keep in (1, 0):
        for before in (1, 63, 64, 65):
            for after in (1, 63, 64, 65):
                tag = "cross_%d_before_%d_after_%s" % (before, after, "keep" if keep else "drop")
                border = ((c.a.at + before) // MT_A + 1) * MT_A
                c.a.fill_to(border - before, c.b)
                code, start = c.a.run(tag, before + after)
                nb = _b_len(before + after, keep)
                c.b.add(tag, code, nb)
                c.plant(tag, code, before + after, nb)
                c.checks.append(_chk_start(tag, code, border - before))
    c.a.fill(300, c.b)
    c.flagged = ">0"
    return _finish(c)


def _b_span0(k):
    c = Case("B_span0-k%d" % k, "B", k)
    c.a.rich.append(_rand1500(k))
    c.b.rich.append(_rand1500(k))
    n = MT_A + 2 * 70
    for keep in (1, 0):
        tag = "span0_%s" % ("keep" if keep else "drop")
        border = ((c.a.at + 70) // MT_A + 1) * MT_A
        c.a.fill_to(border - 70, c.b)
        code, _ = c.a.run(tag, n)
        c.b.add(tag, code, _b_len(n, keep))
        c.plant(tag, code, n, _b_len(n, keep))
        c.checks.append(_chk_start(tag, code, border - 70))

        def chk(x, t=border // MT_A, code=code):
            assert x.acode[t * MT_A] == x.acode[(t + 1) * MT_A - 1] == code            # the middle tile: span 0
            assert x.acode[t * MT_A - 71] != code and x.acode[(t + 1) * MT_A + 70] != code
        c.checks.append(chk)
    c.a.fill(100, c.b)
    c.flagged = ">0"
    return _finish(c)


def _b_alen(k, alen, keep):
    c = Case("B_alen_%d_%s-k%d" % (alen, "keep" if keep else "drop", k), "B", k)
    code, _ = c.a.run("first", 5)
    c.b.add("first", code, _b_len(5, keep))
    c.plant("first", code, 5, _b_len(5, keep))
    c.a.fill_to(alen - 66, c.b)
    code, _ = c.a.run("last", 66)
    c.b.add("last", code, _b_len(66, keep))
    c.plant("last", code, 66, _b_len(66, keep))

    def chk(x):
        assert len(x.acode) == alen and (alen - 1) % MT_A + 1 == {3071: 1023, 3072: 1024, 3073: 1}[alen]
        assert run_of(x.acode, c.table[0][1]) == (0, 5) and run_of(x.acode, c.table[1][1]) == (alen - 66, alen)
    c.checks.append(chk)
    return _finish(c)


# ---- C: bucket table and staged piece ----------------------------------------------------------------------------------

def _c_span(k):
    c = Case("C_span_0_2047_2048-k%d" % k, "C", k)
    rng = np.random.RandomState(7)
    code, _ = c.a.add("span0", 100, MT_A)
    c.b.add("span0", code, 3)
    c.plant("span0", code, MT_A, 3)
    firsts = {}
    for t, span in ((1, MT_NBK - 1), (2, MT_NBK)):
        f = 10000 * t
        firsts[t] = (f, span)
        acodes = _pick(rng, f, f + span, MT_A, [f, f + span])
        for i, code in enumerate(acodes):
            c.a.add(None, code, 1)
        with_b = set(int(code) for i, code in enumerate(acodes) if i % 3 == 0) | {f + span}
        others = np.setdiff1d(np.arange(f, f + span + 1), acodes)[::2]
        for code in sorted(with_b | set(int(o) for o in others)):
            c.b.add(None, code, 1)

    def chk(x):
        assert len(x.acode) == 3 * MT_A
        for t, want_sh in ((0, 0), (1, 0), (2, 1)):
            c0, c1 = int(x.acode[t * MT_A]), int(x.acode[(t + 1) * MT_A - 1])
            span = c1 - c0
            assert span == (0 if t == 0 else firsts[t][1])
            sh = 0
            while (span >> sh) >= MT_NBK:
                sh += 1
            assert sh == want_sh
            assert (x.bcode == np.uint64(c1)).any()                          # a B entry equal to the tile's last code
            if t:
                tc = x.acode[t * MT_A:(t + 1) * MT_A].astype(np.int64)
                bk_b = np.unique((x.bcode[piece(x, t)[0]:piece(x, t)[1]].astype(np.int64) - c0) >> sh)
                empty = ~np.isin((tc - c0) >> sh, bk_b)
                hit = x.per_entry[t * MT_A:(t + 1) * MT_A] > 0
                e = np.flatnonzero(empty)
                assert len(e) > 50 and hit[:e[0]].any() and hit[e[-1]:].any()              # empty buckets between full ones
                assert not hit[empty].any()
    c.checks.append(chk)
    c.flagged = 0
    return _finish(c)


def _c_span_all(k):
    c = Case("C_span_all-k%d" % k, "C", k)
    rng = np.random.RandomState(8)
    top = 4 ** k - 1
    acodes = np.unique(np.concatenate([[0, top], rng.randint(1, 1 << 62, 998).astype(np.int64) % top]))
    for code in acodes:
        c.a.runs.append((None, int(code), 1))
    bcodes = np.unique(np.concatenate([acodes[::3], [0, top], rng.randint(1, 1 << 62, 2000).astype(np.int64) % top]))
    for code in bcodes:
        c.b.runs.append((None, int(code), 1))

    def chk(x):
        assert len(x.acode) <= MT_A and x.acode[0] == 0 and int(x.acode[-1]) == top
        assert x.bcode[0] == 0 and int(x.bcode[-1]) == top
        sh = 0
        while (top >> sh) >= MT_NBK:
            sh += 1
        assert sh == 2 * k - 11
        assert len(x.want) == len(np.intersect1d(acodes, bcodes)) > 300
    c.checks.append(chk)
    c.flagged = 0
    c.checks = [_chk_codes(c), _chk_cross_total(c)] + c.checks
    return c                                    # (not _finish: the codes span the whole space on purpose)


def _c_piece(k, size):
    c = Case("C_piece_%d-k%d" % (size, k), "C", k)
    vpk = VPK(k)
    code = 1000
    for t in range(4):
        while c.b.at % vpk != t % vpk or (t and c.b.runs[-1][0] != "pad"):  # B-only entries below the tile's codes
            c.b.add("pad", code, 1)
            code += 1
        code += 1
        for i in range(MT_A):
            c.a.add(None, code, 1)
            c.b.add(None, code, 2 if (size == MT_BCAP - 1 and i == 500) else 3)
            code += 1
            if size == MT_BCAP + 1 and i == 500:
                c.b.add(None, code, 1)                                       # a B-only code inside the range
            code += 1

    def chk(x):
        assert len(x.acode) == 4 * MT_A
        for t in range(4):
            b0, b1 = piece(x, t)
            assert b1 - b0 == size and b0 % vpk == t % vpk, (t, b0, b1)
            assert x.tile_hits[t] == size - (size == MT_BCAP + 1)
        if size == MT_BCAP:                     # the last piece ends exactly at blen, inside a vector
            assert piece(x, 3)[1] == len(x.bcode) and len(x.bcode) % vpk != 0
    c.checks.append(chk)
    c.flagged = 4 if size > MT_BCAP else 0
    return _finish(c)


def _c_neighbours(k):
    c = Case("C_neighbours-k%d" % k, "C", k)
    # B entries per A code, tile by tile: fast (1024 hits) | flagged (piece of 3073) | no hits | 1 hit | 1025 hits | fast
    per = [lambda i: 1, lambda i: 3, lambda i: 0, lambda i: int(i == 700), lambda i: 1 + (i == 9), lambda i: 1]
    code = 1000
    for t, f in enumerate(per):
        for i in range(MT_A):
            c.a.add(None, code, 1)
            if f(i):
                c.b.add(None, code, f(i))
            if t == 1 and i == 500:
                c.b.add(None, code + 1, 1)
            code += 2

    def chk(x):
        assert list(x.tile_hits) == [MT_A, MT_BCAP, 0, 1, MT_A + 1, MT_A]
        assert [piece(x, t)[1] - piece(x, t)[0] for t in range(6)] == [MT_A, MT_BCAP + 1, 0, 1, MT_A + 1, MT_A]
    c.checks.append(chk)
    c.flagged = 1
    return _finish(c)


# ---- D: the caps -----------------------------------------------------------------------------------------------------

def _d_cross(k):
    c = Case("D_cross_caps-k%d" % k, "D", k)
    c.a.rich.append(_rand1500(k))
    c.b.rich.append(_rand1500(k))

    def put(tag, na, nb, start):
        c.a.fill_to(start, c.b)
        code, _ = c.a.run(tag, na)
        c.b.add(tag, code, nb)
        c.plant(tag, code, na, nb)
        c.checks.append(_chk_start(tag, code, start))

    t = 0
    for na, nb in ((99, 101), (101, 99), (100, 100), (73, 137)):            # in the middle of a tile
        put("mid_%dx%d" % (na, nb), na, nb, t * MT_A + 400)
        t += 1
    for na, nb, before in ((99, 101, 40), (101, 99, 40), (100, 100, 40), (73, 137, 30)):        # neither part reaches the cap
        t += 1
        put("split_%d+%dx%d" % (before, na - before, nb), na, nb, t * MT_A - before)
    for nb in (49, 50):                                                     # each part beyond the 64-entry window
        t += 2
        put("split_100+100x%d" % nb, 200, nb, t * MT_A - 100)
    # a B run longer than pad[1] in a tile where nothing is capped after all
    t += 2
    put("deep_border_200x1", 200, 1, t * MT_A - 100)
    put("deep_1x60", 1, 60, t * MT_A + 500)
    c.a.fill(700, c.b)

    def chk(x, t=t):
        a0, a1 = t * MT_A, (t + 1) * MT_A
        ja, ia = run_of(x.acode, x.acode[a0])[0], run_of(x.acode, x.acode[a1 - 1])[1]
        assert ia - ja == 100 + MT_A                                        # the tile's longest possible A run
        b0, b1 = piece(x, t)
        assert b1 - b0 <= MT_BCAP
        _, nb = np.unique(x.bcode[b0:b1], return_counts=True)
        assert nb.max() == 60 > (MAXGRAM - 1) // (ia - ja)
        assert t in flagged_tiles(x)                                        # flagged for pad[1] alone: the piece fits
        for code in np.unique(x.acode[a0:a1]):                              # ... and nothing is capped
            na = run_of(x.acode, code)[1] - run_of(x.acode, code)[0]
            assert run_hits(x, code) == na * (run_of(x.bcode, code)[1] - run_of(x.bcode, code)[0])
    c.checks.append(chk)
    c.flagged = ">0"
    return _finish(c)


def _d_self(k, comp, identity):
    c = Case("D_self%s%s-k%d" % ("C" if comp else "N", "_I" if identity else "", k), "D", k, self_=1, comp=comp, identity=identity)
    a = c.a
    # poly-A of 150 bases and two one-k-mer reads of its code in front; poly-C of 160 bases above every planted code
    a.rich.append(("polyA150", _homo(0, 150)))
    a.rich.append(("polyC160", _homo(1, 160)))
    a.extern(150 - k + 1)
    a.add("polyA", 0, 2)
    if comp:
        a.rich.append(("polyT150", _homo(3, 150)))
    tri = lambda n: n * (n - 1) // 2
    slots = []
    for tag, n, start in (("self141_mid", 141, MT_A + 400), ("self142_mid", 142, 2 * MT_A + 400),
                          ("self141_split", 141, 4 * MT_A - 70), ("self142_split", 142, 6 * MT_A - 71)):
        a.fill_to(start)
        code, _ = a.run(tag, n)
        c.checks.append(_chk_start(tag, code, start))
        if not comp:
            c.plant(tag, code, n, n, tri(n) if tri(n) < MAXGRAM else "capped")
        else:
            slots.append((tag, code, n, start - a.shift))
    a.fill_to(8 * MT_A + 300)                  # (two tiles of single entries: nothing for a cap there)
    if comp and k % 2 == 0:                     # a code that is its own reverse complement: N reads meet themselves
        for n in (140, 141, 142):
            x0 = (0b0011 << (k - 4)) | n        # the first half: A, T, ...
            pal = (x0 << k) | revcomp(x0, k // 2)
            assert revcomp(pal, k) == pal
            cnt = n * (n + 1) // 2 if identity else tri(n)
            a.loose("pal%d" % n, pal, n)
            c.plant("pal%d" % n, pal, n, n, cnt if cnt < MAXGRAM else "capped")
    if comp:
        # Against the complemented block the partners of a code are the reads of its reverse complement, and a run of n reads
        # against m such reads has as many seeds as pairs with bread < aread: a matter of the shuffled read ids.  Each run
        # gets a slot of SLOT reads behind everything else, m of the reverse complement and SLOT - m of codes nothing pairs
        # with, so that the shuffle (fixed by the case id and the number of reads) does not depend on m; m is then the
        # largest whose count stays below the cap (runs of 141) or one more (runs of 142): the border in m, exactly.
        SLOT = 200
        rows = sum(r[2] for r in a.runs) + sum(r[2] for r in a.extra)
        total = rows + SLOT * len(slots) + len(a.rich)
        perm = np.random.RandomState(zlib.crc32(c.id.encode()) & 0x7fffffff).permutation(total)
        rid = np.empty(total, dtype=np.int64)
        rid[perm] = np.arange(total)            # the read id of a row (Case.reads)
        spare = 2 * 4 ** (k - 1)
        for j, (tag, code, n, off) in enumerate(slots):
            ida, idb = rid[off:off + n], rid[rows + SLOT * j:rows + SLOT * (j + 1)]
            cum = np.cumsum([(ida > b).sum() for b in idb])
            assert cum[-1] >= MAXGRAM
            m = int(np.searchsorted(cum, MAXGRAM, "left")) + (n == 142)         # cum[m - 1] < MAXGRAM <= cum[m]
            cnt = int(cum[m - 1])
            assert (MAXGRAM - n <= cnt < MAXGRAM) if n == 141 else (MAXGRAM <= cnt < MAXGRAM + n), (tag, m, cnt)
            a.loose("rc_" + tag, revcomp(code, k), m)
            for _ in range(SLOT - m):
                a.loose("spare", spare, 1)
                spare += 4
            c.plant(tag, code, n, m, cnt if cnt < MAXGRAM else "capped")
        assert sum(r[2] for r in a.runs) + sum(r[2] for r in a.extra) + len(a.rich) == total

    def chk(x):
        pa = run_of(x.acode, 0)
        assert pa == (0, 150 - k + 1 + 2)
        pc = run_of(x.acode, (4 ** k - 1) // 3)
        assert pc[1] - pc[0] == 160 - k + 1
        if not comp:
            # the bound cuts inside the run of one read: without -I a read never meets itself, with -I poly-A's run
            # stays below the cap and poly-C's 147 (144) entries meet themselves tri(147) = 10731 (10296) times
            n = 150 - k + 1
            if identity:
                assert tri(n) <= run_hits(x, 0) < MAXGRAM and run_hits(x, (4 ** k - 1) // 3) == 0
                assert tri(160 - k + 1) >= MAXGRAM
            else:
                assert 0 < run_hits(x, 0) <= 2 * n + 1 and run_hits(x, (4 ** k - 1) // 3) == 0
        else:
            fate = {t[0]: t[4] for t in c.table if t[0].startswith("self")}     # (_chk_table holds the oracle to these)
            assert all((fate[t] == "capped") == t.startswith("self142") for t in fate) and len(fate) == 4
    c.checks.append(chk)
    c.flagged = ">0"
    return _finish(c)


def _d_lowmem(k, self_):
    c = Case("D_lowmem_%s-k%d" % ("self" if self_ else "cross", k), "D", k, self_=self_)
    c.lowmem = True
    other = None if self_ else c.b
    if self_:
        for i in range(200):                    # the bulk: runs of three identical reads, three hits each
            c.a.run(None, 3)
        for n in range(20, 101, 10):            # tri(n) = 190 ... 4950, every run over a tile border
            border = ((c.a.at + n // 2) // MT_A + 1) * MT_A
            c.a.fill_to(border - n // 2)
            code, _ = c.a.run("low_%d" % n, n)
            c.plant("low_%d" % n, code, n, n, None)
    else:
        for i in range(300):
            code, _ = c.a.run(None, 2)
            c.b.add(None, code, 2)
        for nb in range(10, 121, 10):           # 40 x nb = 400 ... 4800
            border = ((c.a.at + 20) // MT_A + 1) * MT_A
            c.a.fill_to(border - 20, other)
            code, _ = c.a.run("low_40x%d" % nb, 40)
            c.b.add("low_40x%d" % nb, code, nb)
            c.plant("low_40x%d" % nb, code, 40, nb, None)
    c.a.fill(100, other)
    c.table = [t[:4] + (None,) for t in c.table]

    def chk(x):
        assert 2 < x.limit < 5000 and 0 < len(x.want) < x.full
        decided = [t for t in c.table if (t[2] * (t[2] - 1) // 2 if self_ else t[2] * t[3]) == x.limit]
        assert len(decided) == 1                # the run whose mutual count is the new limit ...
        s, e = run_of(x.acode, decided[0][1])
        assert s // MT_A != (e - 1) // MT_A     # ... crosses a tile border
        for tag, code, na, nb, _ in c.table:
            ct = na * (na - 1) // 2 if self_ else na * nb
            assert run_hits(x, code) == (ct if ct < x.limit else 0), tag
    c.checks = [_chk_codes(c)] + ([] if self_ else [_chk_cross_total(c)]) + [chk]
    return c


# ---- E: slabs --------------------------------------------------------------------------------------------------------

def _e_slabs(k, self_):
    c = Case("E_slabs_%s-k%d" % ("self" if self_ else "cross", k), "E", k, self_=self_)
    rng = np.random.RandomState(31)
    for i, n in enumerate(rng.randint(60, 121, 30)):
        c.a.fill(90, None if self_ else c.b)
        if self_:
            code, _ = c.a.run("run_%d" % i, int(n))
            c.plant("run_%d" % i, code, int(n), int(n), int(n) * (int(n) - 1) // 2)
        else:
            code, _ = c.a.run("run_%d" % i, 5)
            c.b.add("run_%d" % i, code, int(n))
            c.plant("run_%d" % i, code, 5, int(n))
    # two rich B reads that hold one code 40 and 100 times: stretches of equal bread shorter and longer than a wavefront
    g, cc = 2 * (4 ** k - 1) // 3, (4 ** k - 1) // 3
    c.b.rich.append(("polyG_40", _homo(2, 40 + k - 1)))
    c.b.rich.append(("polyC_100", _homo(1, 100 + k - 1)))
    c.a.loose("polyC_x30", cc, 30)
    c.a.loose("polyG_x30", g, 30)
    if not self_:
        c.a.rich.append(_rand1500(k))
        c.b.rich.append(_rand1500(k))
    c.caps = [lambda h: int(h.max()), lambda h: max(int(h.max()), int(h.sum()) // 5)]

    def chk(x):
        h = np.bincount(x.want["bread"], minlength=x.nrb)
        assert run_hits(x, g) > 0 and run_hits(x, cc) > 0 and h.max() >= 30 * 100 * (not self_)
        for f in c.caps:
            lo, acc = [0], 0                    # the greedy cut of include/damar_hip.h
            for r, v in enumerate(h):
                if r > lo[-1] and acc + v > f(h):
                    lo.append(r)
                    acc = 0
                acc += int(v)
            assert len(lo) >= 3
            spans = [x.B["read"][slice(*run_of(x.bcode, t[1]))] for t in c.table]
            for b in lo[1:]:                    # every slab border falls inside several planted B runs
                assert sum(1 for rd in spans if rd.min() < b <= rd.max()) >= 3, b
    c.checks.append(chk)
    return _finish(c)


def _make():
    out = []
    for k in (K32, K64):
        ns = NS(k)
        for name, n in (("1", 1), ("2", 2), ("NS-1", ns - 1), ("NS", ns), ("NS+1", ns + 1), ("2NS+1", 2 * ns + 1)):
            out.append(_a_blen(k, name, n))
        out.append(_a_disjoint(k))
        out += [_b_borders(k), _b_span0(k)]
        out += [_b_alen(k, alen, keep) for alen in (3 * MT_A - 1, 3 * MT_A, 3 * MT_A + 1) for keep in (1, 0)]
        out += [_c_span(k), _c_span_all(k)] + [_c_piece(k, s) for s in (MT_BCAP - 1, MT_BCAP, MT_BCAP + 1)] + [_c_neighbours(k)]
        out.append(_d_cross(k))
        out += [_d_self(k, comp, ident) for comp in (0, 1) for ident in (0, 1)]
        out += [_d_lowmem(k, 1), _d_lowmem(k, 0)]
    out += [_e_slabs(K32, 0), _e_slabs(K32, 1)]
    return out


CASES = _make()
BY_ID = {c.id: c for c in CASES}
IDS = [c.id for c in CASES]
assert len(BY_ID) == len(CASES)
