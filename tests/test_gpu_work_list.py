"""The work list of a comparison -- which read pairs are aligned at all -- alone, through the test hook damar_pair_work_test
(kernels/seed_merge.hip pair_work_mark<UNS>, slice_ends, pair_heads_expand, order_probe; and the older two steps
pair_heads_mark, pair_screen, scan, compact_u32), on planted seed lists (tests/work_shapes.py), against the reference's rule
(tests/work_model.py, pinned to the reference in test_work_model_host.py).  Every list is checked in mode 0 (one pass, sorted
seeds), mode 2 (two steps) and mode 1 (one pass, the seeds of a run in no order: random, reversed, ties kept in input order);
the packed lists again with dbits == 0 (the diagonals beside the keys) in modes 0 and 2.  The device list must EQUAL the
model's `may`; `must <= got <= heads` is asserted first so that a failure says whether a pair was lost or one too many kept.
Everything here needs a real MI355X."""
import functools

import numpy as np
import pytest

import work_model as M
import work_shapes as S

pytestmark = pytest.mark.gpu

# kernels/seed_merge.hip and kernels/kernels.h, copied: a change there must be made here on purpose
SCREEN_MAX = 48           # SCREEN_MAX: the longest run that is screened
SCREEN_PANEL = 50000      # SCREEN_PANEL = PANEL_SIZE (filter.c:73)
HALO = 64                 # PW_HALO
TILE = 4096               # DAMAR_SCAN_TILE
OR_MAX = 2048             # OR_MAX
assert (SCREEN_MAX, SCREEN_PANEL, HALO, TILE, OR_MAX) == (S.SCREEN_MAX, S.SCREEN_PANEL, S.HALO, S.TILE, S.OR_MAX)
assert (SCREEN_MAX, SCREEN_PANEL, OR_MAX) == (M.SCREEN_MAX, M.SCREEN_PANEL, M.OR_MAX)

PERMS = ("random", "reversed", "ties")


@pytest.fixture(scope="module")
def gpu(built):
    from damar_amd import api
    L = api.lib()
    assert L.damar_hip_init(0) >= 1
    return L


@functools.lru_cache(maxsize=None)
def ladder(p):
    return S.ladder(*p)


@functools.lru_cache(maxsize=None)
def sliced():
    return S.sliced()


def compare(got, m, what, flag=None):
    got = np.asarray(got, dtype=np.int64)
    assert (np.diff(got) > 0).all(), "%s: the list is not ascending" % what
    g, must, may, heads = set(got.tolist()), set(m["must"].tolist()), set(m["may"].tolist()), set(m["heads"].tolist())
    lost, not_heads = sorted(must - g), sorted(g - heads)
    assert lost == [], "%s: %d pairs the reference aligns are not in the list, first at seed %d" % (what, len(lost), lost[0])
    assert not_heads == [], "%s: %d items are no run the reference enters, first at seed %d" % (what, len(not_heads), not_heads[0])
    diff = sorted(g ^ may)
    assert np.array_equal(got, m["may"]), "%s: %d items differ from the model's (%d too many), first at seed %d" % (
        what, len(diff), len(g - may), diff[0])
    if flag is not None:
        assert int(flag[0]) == m["flag"], "%s: flag %d, expected %d" % (what, int(flag[0]), m["flag"])


def check(case, nshift, b_lo=0, b_hi=0xffffffff, off=0, nhits=None, perms=PERMS, seed=1):
    """all modes and layouts of one list (or of its stretch [off, off + nhits)) against the model; -> the model's answer"""
    from damar_amd import api
    n = len(case.bread)
    nhits = n - off if nhits is None else nhits
    par = (case.kmer, case.hitmin, case.binshift, nshift, b_lo, b_hi)
    dev = (case.minhit, nshift, case.binshift, case.kmer, case.hitmin, b_lo, b_hi)
    want = M.work_list(*case.arrays(), *par, off=off, nhits=nhits)
    for dbits in (case.dbits, 0):
        keys, vals = M.pack(*case.arrays(), case.ppos, dbits, case.abits)
        assert all(np.array_equal(a, b) for a, b in zip(M.unpack(keys, vals, case.ppos, dbits, case.abits), case.arrays()))
        assert (np.diff(keys.astype(np.int64)) >= 0).all()             # sorted, as the device takes them
        v = None if vals is None else vals[off:off + nhits]
        for mode in (0, 2):
            work, flag = api.pair_work(keys[off:off + nhits], v, off, n, case.ppos, dbits, case.abits, *dev, mode)
            compare(work, want, "%s nshift %d dbits %d mode %d" % (case.name, nshift, dbits, mode))
            assert int(flag[0]) == 0                                   # (only mode 1 looks for runs too long to order)
    rng = np.random.default_rng(seed)
    for how in perms:
        o = case.order(how, rng)
        arr = [x[o] for x in case.arrays()]
        m1 = M.work_list(*arr, *par, unsorted=True, off=off, nhits=nhits)
        keys, _ = M.pack(*arr, case.ppos, case.dbits, case.abits)
        work, flag = api.pair_work(keys[off:off + nhits], None, off, n, case.ppos, case.dbits, case.abits, *dev, 1)
        compare(work, m1, "%s nshift %d mode 1 %s" % (case.name, nshift, how), flag)
    return want


def both_kinds(case, want):
    """The planted runs: some are in the model's list and some are not (an all-kept or all-dropped answer cannot pass)."""
    may = set(want["may"].tolist())
    kept = [p for p in case.planted if p[0] in may]
    dropped = [p for p in case.planted if p[0] not in may]
    assert len(kept) > 0 and len(dropped) > 0, (case.name, len(kept), len(dropped))
    return kept, dropped


def agrees_with_its_maker(case, want):
    """where a planted run is screened and no slice end is near, the model says what its maker meant"""
    may = set(want["may"].tolist())
    for start, n, tag, fires in case.planted:
        if case.minhit <= n <= SCREEN_MAX and case.minhit <= SCREEN_MAX and case.apos[start:start + n].max() <= SCREEN_PANEL:
            assert (start in may) == fires, (case.name, tag)


@pytest.mark.parametrize("p", S.LADDER_PARAMS, ids=["k%d-h%d-w%d" % p for p in S.LADDER_PARAMS])
def test_gpu_work_list_threshold_ladder(gpu, p):
    """Every run length of 1 .. 9, 47, 48, 49, 64, 65, 66, 100 that is at least minhit: one bucket with sum hitmin, one with
    hitmin - 1, buckets d and d + 1 that reach it only together, d and d + 2 (never); three buckets of which one pair of
    neighbours reaches it; diagonals -1 and 0, and at multiples of 1 << binshift on both sides of 0; a first seed at kmer - 1;
    equal A positions.  Fillers of 1 .. minhit - 1 seeds between; the ladder a second time across the first tile border."""
    case = ladder(p)
    assert len(case.bread) > TILE
    want = check(case, -1)
    kept, dropped = both_kinds(case, want)
    agrees_with_its_maker(case, want)
    tags = {t[2] for t in case.planted}
    assert {"first_at_k-1", "first_at_k", "diag_-1_0", "same_-W_-1_lt"} <= tags
    for kind in ("one_eq", "one_lt", "adj", "gap"):                    # each of the four makes at a screened length, both answers
        assert any(t[2].startswith(kind) and t[1] <= SCREEN_MAX for t in (kept if kind in ("one_eq", "adj") else dropped)), kind
    assert any(t[2].startswith("one_lt") and t[1] > SCREEN_MAX for t in kept)          # (too long to screen: kept)
    check(case, 0, perms=("random",))                                  # one slice: only the end of the list


@pytest.mark.parametrize("minhit", S.MINHIT_EDGES)
def test_gpu_work_list_minhit_edges(gpu, minhit):
    """kmer 14, hitmin 14 * minhit: minhit 1 and 2 (a tile of 4096 and of 2048 heads), 3, 48 (the last that is screened), 49
    (never screened), 65 (the last read from LDS), 66 (the first read from keys).  From 49 on: runs of minhit - 1 and of
    minhit seeds that end with a tile and that start on a tile's last seed, and a last run of minhit + 1, minhit and
    minhit - 1 seeds that ends the list, with one slice (nshift 0) and with none (nshift -1)."""
    case = S.minhit_edge(minhit)
    assert case.minhit == minhit
    n = len(case.bread)
    if minhit <= 2:
        want = check(case, -1)
        assert np.bincount(want["heads"] // TILE)[0] == TILE // minhit
        both_kinds(case, want)
        agrees_with_its_maker(case, want)
    elif minhit <= SCREEN_MAX:
        want = check(case, -1)
        both_kinds(case, want)
        agrees_with_its_maker(case, want)
        check(case, 0, perms=("reversed",))
    else:
        seen = set()
        for cut in (0, 1, 2):
            c = case.truncated(n - cut)
            for nshift in (0, -1):
                want = check(c, nshift, perms=("random",))
                heads = set(want["heads"].tolist())
                assert set(want["may"].tolist()) == heads              # (never screened)
                for start, ln, tag, _ in case.planted:
                    if tag.startswith("t"):
                        assert (start in heads) == (ln == minhit), tag
                seen.add((cut, nshift, (n - cut - (minhit + 1 - cut)) in heads))
        # the last run: minhit + 1 seeds are entered; minhit only without a slice end behind them; minhit - 1 never
        assert seen == {(0, 0, True), (0, -1, True), (1, 0, False), (1, -1, True), (2, 0, False), (2, -1, False)}


@pytest.mark.parametrize("variant", [0, 1])
def test_gpu_work_list_tile_geometry(gpu, variant):
    """Heads at tile offsets 0, 1, 4095 - 48, 4095 - 8, 4095; runs of 48 (screened in the halo), 49 and 65 from offset 4095; a
    run whose successor's head is the next tile's first seed; offset 0 inside the previous tile's last run; a tile with no
    head between two with heads; a last run that ends the list.  Variant 1 swaps firing and non-firing runs."""
    case = S.tile_geometry(variant)
    at = {t[2].split(":")[0]: t[0] for t in case.planted}
    assert at["list_start"] == 0 and at["off_4095-48"] % TILE == TILE - 1 - 48 and at["off_4095-8"] % TILE == TILE - 1 - 8
    assert at["off_1"] % TILE == 1 and at["off_0_after_another_pair"] % TILE == 0 and at["off_0_behind_an_empty_tile"] % TILE == 0
    for t in ("halo_48", "halo_49", "halo_65", "halo_48_again"):
        assert at[t] % TILE == TILE - 1
    assert at["over_the_border"] % TILE == TILE - 2 and case.aread[at["over_the_border"]] == case.aread[at["over_the_border"] + 2]
    want = check(case, 0)
    both_kinds(case, want)
    agrees_with_its_maker(case, want)
    per_tile = np.bincount(want["heads"] // TILE, minlength=10)
    assert per_tile[8] == 0 and per_tile[7] > 0 and per_tile[9] > 0
    halo = {t[2].split(":")[0]: (t[0] in set(want["may"].tolist())) for t in case.planted}
    assert halo["halo_48"] != halo["halo_48_again"] and halo["halo_49"] and halo["halo_65"]


def test_gpu_work_list_lengths_of_the_list(gpu):
    """nhits of 1, minhit - 1, minhit, 4096, 4097, 4096 + 63 and 4096 + 64, the last run (firing, of minhit or minhit + 1
    seeds) ending the list: with one slice a run of exactly minhit seeds at the end is not entered, without slices it is."""
    kept = dropped = 0
    for nhits in (1, 2, 3, TILE, TILE + 1, TILE + HALO - 1, TILE + HALO):
        for last in (3, 4):
            case = S.list_of_length(nhits, last)
            assert len(case.bread) == nhits
            for nshift in (0, -1):
                want = check(case, nshift, perms=("random",), seed=nhits)
                ln = min(nhits, last)                                  # the last run, from seed nhits - ln on; it fires
                entered = (nhits - ln) in set(want["may"].tolist())
                assert entered == (ln >= case.minhit and (ln > case.minhit or nshift < 0)), (nhits, last, nshift)
                kept += entered
                dropped += not entered
    assert kept > 0 and dropped > 0


@pytest.mark.parametrize("kmer,hitmin,share", [(14, 35, 0.), (14, 35, .1), (14, 14, 0.)])
def test_gpu_work_list_mixed_wavefronts(gpu, kmer, hitmin, share):
    """Three tiles of runs of 1 .. 8 seeds drawn at random, four makes at random: every register variant of the one-lane
    screen runs with shorter runs beside it, the lists span several rounds (more than 600 heads a tile); with a tenth of the
    runs at 9 .. 48 seeds (the list of the wavefront-per-run screen fills); and with minhit 1 (runs of 1 and 2 seeds)."""
    case = S.mixed(kmer, hitmin, share, seed=int(kmer + hitmin + 100 * share))
    want = check(case, -1)
    both_kinds(case, want)
    agrees_with_its_maker(case, want)
    per_tile = np.bincount(want["heads"] // TILE, minlength=3)[:3]
    if share == 0:
        assert per_tile.min() > 600
    else:
        assert sum(1 for t in case.planted if t[1] > 8) > 3 * 30
    lengths = {t[1] for t in case.planted}
    assert set(range(max(case.minhit, 1), 9)) <= lengths


def test_gpu_work_list_panel(gpu):
    """A run that does not fire is dropped with its largest A position at 50000 and kept (not screened) at 50001, at the
    lengths of every screen, in a tile's middle and from its last seed; in mode 1 with that seed first, in the middle and
    last in the run."""
    case = S.panel()
    assert case.ppos >= 16
    want = check(case, -1, perms=("top_first", "top_middle", "top_last", "random"))
    may = set(want["may"].tolist())
    for start, n, tag, fires in case.planted:
        top = int(case.apos[start:start + n].max())
        assert top in (SCREEN_PANEL, SCREEN_PANEL + 1)
        assert (start in may) == (fires or top > SCREEN_PANEL), tag
    both_kinds(case, want)


@pytest.mark.parametrize("nshift", [0, 2, 6, -1])
def test_gpu_work_list_slice_ends(gpu, nshift):
    """64 stretches of 160 seeds, a B read each: before every slice end e a firing head at e - minhit - 1 (entered) or at
    e - minhit (not entered); every fourth nominal end lies 7 seeds inside a B read and moves to its end; 25 slice ends a
    tile at nshift 6."""
    case, ends = sliced()
    want = check(case, nshift, perms=("random",))
    may = set(want["may"].tolist())
    sl = M.slices(case.bread, nshift) if nshift >= 0 else []
    real_ends = {e for _, e in sl}
    if nshift == 6:
        assert real_ends == set(ends) and len([e for e in ends if e < TILE]) >= 3
        assert any(e % S.SLICE_UNIT == 7 for e in ends)
    n_in = n_out = 0
    for start, n, tag, fires in case.planted:
        if tag.startswith("end_"):
            e = start + n
            assert fires and (start in may) == (e not in real_ends or n == case.minhit + 1), tag
            n_in += start in may
            n_out += start not in may
    assert n_in > 0 and (n_out > 0 or nshift < 0)
    both_kinds(case, want)


@pytest.mark.parametrize("nshift", [0, 2, 6])
def test_gpu_work_list_middle_stretch_has_the_whole_lists_answer(gpu, nshift):
    """The same list handed over as a stretch [off, off + nhits) of gtotal seeds, both cuts where bread changes (one of them
    a moved slice end): the slices are those of the whole list, the answer is the whole list's on that stretch."""
    case, ends = sliced()
    off, stop = ends[5], ends[40]
    assert off % S.SLICE_UNIT == 7 and case.bread[off] != case.bread[off - 1] and case.bread[stop] != case.bread[stop - 1]
    whole = M.work_list(*case.arrays(), case.kmer, case.hitmin, case.binshift, nshift)
    part = check(case, nshift, off=off, nhits=stop - off, perms=("random",))
    inside = whole["may"][(whole["may"] >= off) & (whole["may"] < stop)] - off
    assert np.array_equal(part["may"], inside) and 0 < len(inside) < len(whole["may"])
    assert len(part["may"]) < len(part["heads"])


@pytest.mark.parametrize("nshift", [-1, 6])
def test_gpu_work_list_b_read_range(gpu, nshift):
    """b_lo and b_hi cut the list in the middle: heads outside are dropped, a firing one whose bread is exactly b_hi too."""
    case, _ = sliced()
    b_lo, b_hi = 21, 41                                    # (odd stretches end with a head that is entered at every nshift)
    free = M.work_list(*case.arrays(), case.kmer, case.hitmin, case.binshift, nshift)
    want = check(case, nshift, b_lo=b_lo, b_hi=b_hi, perms=("random",))
    assert any(case.bread[i] == b_hi for i in free["must"]) and any(case.bread[i] == b_lo for i in want["must"])
    assert any(case.bread[i] < b_lo for i in free["must"])
    b = case.bread[want["may"]]
    assert len(b) > 0 and b.min() == b_lo and b.max() < b_hi
    inside = free["may"][(case.bread[free["may"]] >= b_lo) & (case.bread[free["may"]] < b_hi)]
    assert np.array_equal(want["may"], inside) and len(want["may"]) < len(want["heads"])


@pytest.mark.parametrize("n,ranged,flag", [(OR_MAX, False, 0), (OR_MAX + 1, False, 1), (OR_MAX + 1, True, 0)])
def test_gpu_work_list_too_long_flag(gpu, n, ranged, flag):
    """Mode 1 says whether a kept run is too long for the ordering step: 2048 seeds are not, 2049 are, and 2049 on a B read
    outside [b_lo, b_hi) are not (the run is not kept)."""
    case = S.too_long(n, seed=n)
    b_hi = case.long_bread if ranged else 0xffffffff
    want = check(case, -1, b_hi=b_hi)
    m1 = M.work_list(*case.arrays(), case.kmer, case.hitmin, case.binshift, -1, 0, b_hi, unsorted=True)
    assert m1["flag"] == flag
    long_head = [t[0] for t in case.planted if t[2].startswith("long")][0]
    assert (long_head in set(want["may"].tolist())) == (not ranged)
    if not ranged:
        both_kinds(case, want)


def test_gpu_work_list_hook_refuses_what_it_cannot_run(gpu):
    """mode 1 with dbits == 0 (SeedStage never takes that path), a mode that does not exist, vals without dbits == 0; and an
    empty list has no work items."""
    from damar_amd import api
    case = ladder(S.LADDER_PARAMS[0])
    keys, vals = M.pack(*case.arrays(), case.ppos, 0, case.abits)
    args = (0, len(keys), case.ppos, 0, case.abits, case.minhit, -1, case.binshift, case.kmer, case.hitmin, 0, 0xffffffff)
    with pytest.raises(ValueError):
        api.pair_work(keys, vals, *args, 1)
    with pytest.raises(ValueError):
        api.pair_work(keys, vals, *args, 3)
    with pytest.raises(ValueError):
        api.pair_work(keys, None, *args, 0)
    work, flag = api.pair_work(keys[:0], vals[:0], 0, 0, case.ppos, 0, case.abits, case.minhit, -1, case.binshift, case.kmer,
                               case.hitmin, 0, 0xffffffff, 0)
    assert len(work) == 0 and int(flag[0]) == 0
