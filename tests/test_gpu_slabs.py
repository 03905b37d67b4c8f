"""A comparison with more seed pairs than one seed stage holds -- the 32-bit seed index, or what the seed arrays can be
grown to -- runs in slabs: consecutive ranges of B reads, cut greedily from the seed pairs per B read, each slab a seed
stage of its own.  Nothing here can make 2^32 seed pairs: the production figure is exercised only through the test hook
DAMAR_TEST_SEED_CAP, which replaces it.  Everything here needs a real MI355X."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, GOLDEN, read_case, link_db, compare_las, opts_to_plan_kwargs

pytestmark = pytest.mark.gpu

HOOK = "DAMAR_TEST_SEED_CAP"


@pytest.fixture(scope="module")
def gpu(built):
    from damar_amd import api
    L = api.lib()
    assert L.damar_hip_init(0) >= 1
    return L


@pytest.fixture(autouse=True)
def no_hook_left_behind():
    yield
    os.environ.pop(HOOK, None)


def greedy(h, cap):
    """The rule of include/damar_hip.h: a slab takes B reads while its seed pairs stay <= cap, and at least one."""
    lo, sums, acc = [0], [], 0
    for r, x in enumerate(h):
        if r > lo[-1] and acc + x > cap:
            sums.append(acc)
            lo.append(r)
            acc = 0
        acc += int(x)
    sums.append(acc)
    lo.append(len(h))
    return lo, sums


class Pair:
    """One comparison through the C ABI: blocks and indexes resident, damar_match as often as wanted."""

    def __init__(self, L, an, bn, comp, k=14, j=4, identity=0, h=35, blocks=None):
        """blocks: (A block, B block, cross) made in memory, the B block not yet complemented, instead of blocks read from
        an and bn"""
        from damar_amd import api
        self.L, self.comp, self.cross, self.k, self.h = L, comp, int(an != bn) if blocks is None else int(blocks[2]), k, h
        L.Set_Filter_Params(k, 6, 0, h, j)
        L.damar_set_async(0)
        api.set_globals(identity=identity)
        self.adb, self.bdb = (api.read_block(an), api.read_block(bn)) if blocks is None else blocks[:2]
        if comp:
            L.damar_complement_block(C.byref(self.bdb), 1)
        n = C.c_int(0)
        self.ablk = L.damar_block_upload(C.byref(self.adb))
        self.aidx = L.damar_index_build(self.ablk, 0, C.byref(n))
        if self.cross or comp:
            self.bblk = L.damar_block_upload(C.byref(self.bdb))
            self.bidx = L.damar_index_build(self.bblk, 0, C.byref(n))
        else:
            self.bblk, self.bidx = None, self.aidx
        self.spec = L.New_Align_Spec(.70, 100, self.adb.freq, 4, 1, 0, 0, 1)

    def match(self, cap=None, seeds=False, j=None):
        """-> dict(counts, counters[0:5], slabs (b_lo, hits), totals, seeds)"""
        import oracle_api as O
        from damar_amd import api
        L = self.L
        if j is not None:
            L.Set_Filter_Params(self.k, 6, 0, self.h, j)
        if cap is None:
            os.environ.pop(HOOK, None)
        else:
            os.environ[HOOK] = str(int(cap))
        if seeds:
            L.damar_last_seeds(None, 1)
        cnt = (api.c_int64 * 3)()
        L.damar_match(C.byref(self.adb), C.byref(self.bdb), self.aidx, self.bidx, 0 if self.cross else 1, self.comp, self.spec, cnt)
        os.environ.pop(HOOK, None)
        out = dict(counts=list(cnt), counters=api.counters()[:5], slabs=api.last_slabs(), totals=api.slab_totals())
        if seeds:
            got = np.zeros(int(cnt[0]), dtype=O.SEED_DT)
            out["nseeds"] = L.damar_last_seeds(got.ctypes.data, len(got))
            L.damar_last_seeds(None, 0)
            out["seeds"] = got
        L.Reset_Overlap_Buffer(self.spec)
        return out

    def close(self):
        L = self.L
        if self.bblk:
            L.damar_index_free(self.bidx)
            L.damar_block_free(self.bblk)
        L.damar_index_free(self.aidx)
        L.damar_block_free(self.ablk)


def oracle_seeds(an, bn, comp, k=14, identity=0, mem_limit=None):
    import oracle_api as O
    cross = an != bn
    oadb, obdb = O.read_block(an), O.read_block(bn)
    if comp:
        O.lib().damar_complement_block(C.byref(obdb), 1)
    prm = O.params(k=k, identity=identity)
    if mem_limit:
        prm.mem_limit = mem_limit
    pa, na, _ = O.sort_kmers(oadb, prm)
    pb, nb = (O.sort_kmers(obdb, prm)[:2]) if (cross or comp) else (pa, na)
    return O.seed_pairs(oadb, obdb, pa, na, pb, nb, 0 if cross else 1, comp, prm), obdb.nreads


def case_kw(name):
    kw = opts_to_plan_kwargs(read_case(name)["opts"])
    return dict(k=kw.get("k", 14), identity=kw.get("identity", 0))


def comparisons():
    t2 = os.path.join(GOLDEN, "tiny2")
    out = []
    for comp in (0, 1):
        out.append(("tiny2-self-%s" % "NC"[comp], os.path.join(t2, "G.2"), os.path.join(t2, "G.2"), comp, {}))
        out.append(("tiny2-cross-%s" % "NC"[comp], os.path.join(t2, "G.2"), os.path.join(t2, "G.1"), comp, {}))
    td = read_case("tandem")["dbdir"]
    out.append(("tandem-self-N", os.path.join(td, "G.1"), os.path.join(td, "G.1"), 0, {}))
    ti = read_case("tiny_I")["dbdir"]
    out.append(("tiny_I-self-N", os.path.join(ti, "G.1"), os.path.join(ti, "G.1"), 0, case_kw("tiny_I")))
    return out


COMPARISONS = comparisons()


@pytest.mark.parametrize("name,an,bn,comp,kw", COMPARISONS, ids=[c[0] for c in COMPARISONS])
def test_gpu_slab_table_and_seed_list_equal_the_oracle(gpu, name, an, bn, comp, kw):
    """The slab table is the greedy cut of the ORACLE's seed pairs per B read, recomputed here in numpy; the seed list of
    the split run is the oracle's, record for record; work items, Local_Alignment calls, records and trace values are
    those of the run in one piece."""
    want, nrb = oracle_seeds(an, bn, comp, **kw)
    h = np.bincount(want["bread"], minlength=nrb)
    cap = max(int(h.max()), len(want) // 5)
    lo, sums = greedy(h, cap)
    assert len(sums) >= 3                                   # (on the CPU side: the test cannot pass with nothing split)
    p = Pair(gpu, an, bn, comp, **kw)
    try:
        whole = p.match()
        assert whole["slabs"] == ([0, nrb], [len(want)]) and whole["totals"] == (1, 0)
        got = p.match(cap=cap, seeds=True)
        assert got["totals"][1] > 0 and len(got["slabs"][1]) >= 3
        assert got["slabs"] == (lo, sums)
        assert got["totals"] == (sum(1 for x in sums if x > 0), 1)
        assert got["counts"][0] == len(want) and got["nseeds"] == len(want)
        assert np.array_equal(got["seeds"], want)
        again = p.match(cap=cap)                           # (without the seed list kept: the paths of an ordinary run)
        print(name, "slabs", len(sums), "counters whole", whole["counters"], "split", again["counters"])
        assert again["counters"] == whole["counters"]
        assert again["counts"] == whole["counts"]
    finally:
        p.close()


@pytest.mark.parametrize("j", [1, 4, 8])
@pytest.mark.parametrize("name,an,bn,comp,kw", COMPARISONS, ids=[c[0] for c in COMPARISONS])
def test_gpu_slabs_keep_the_reference_thread_slices(gpu, name, an, bn, comp, kw, j):
    """filter.c:2212-2214: a run that starts within minhit seeds of the end of its thread's slice is not entered, and the
    slices are those of the WHOLE sorted list.  Counters 0-4 (seed pairs, work items, Local_Alignment calls, records, trace
    values) of the split run equal those of the run in one piece for -j1, -j4 and -j8; the cap is the largest count of a
    B read, so that most slabs are one or two reads -- far shorter than a slice.  On these comparisons the count of work
    items is the same for -j1 and -j8 (no run lies within minhit seeds of a slice end): the rule at a slice end itself is
    exercised by test_gpu_slabs_where_a_run_lies_at_a_slice_end below."""
    p = Pair(gpu, an, bn, comp, j=j, **kw)
    try:
        first = p.match(cap=1 << 40, seeds=True, j=j)
        h = np.bincount(first["seeds"]["bread"], minlength=p.bdb.nreads)
        cap = int(h.max())
        lo, sums = greedy(h, cap)
        assert len(sums) >= 3 and min(sums) < len(first["seeds"]) // 8       # some slab is shorter than a slice of -j8
        whole = p.match(j=j)
        got = p.match(cap=cap, j=j)
        print(name, "j", j, "slabs", len(sums), "whole", whole["counters"], "split", got["counters"])
        assert got["totals"][1] > 0 and got["slabs"] == (lo, sums)
        assert got["counters"] == whole["counters"]
    finally:
        gpu.Set_Filter_Params(14, 6, 0, 35, 4)
        p.close()


@pytest.mark.parametrize("cross", [0, 1])
def test_gpu_slabs_under_a_lowered_cap_on_mutual_matches(gpu, cross):
    """MEM_LIMIT squeezed as in test_gpu_memory_limit_lowers_the_cap_like_the_oracle: the seed pairs per B read are taken
    under the lowered cap on mutual k-mer matches, which stays a property of the whole code run in every slab."""
    import oracle_api as O
    from damar_amd import api
    L = gpu
    an = os.path.join(GOLDEN, "tandem", "G.1")
    oadb = O.read_block(an)
    full, _ = oracle_seeds(an, an, cross)
    prm_na = O.sort_kmers(oadb, O.params())[1]
    na = nb = prm_na
    dbb = 88 + 32 * (oadb.nreads + 2) + oadb.totlen + oadb.nreads + 4 + len(oadb.path or b"") + 1
    want, mem = None, 0
    for frac in (.9, .8, .7, .6):
        avail = int(len(full) * frac / .98) + 8
        words = (2 * avail + na) if not cross else (avail + na + nb)
        if cross and words > na + 2 * nb:
            words = 2 * avail + na
        mem = 16 * words + 2 * dbb
        w, nrb = oracle_seeds(an, an, cross, mem_limit=mem)
        if 2 < O.LAST_LIMIT < 5000 and 0 < len(w) < len(full):
            want = w
            break
    assert want is not None, "no memory limit found that lowers the cap on this fixture"
    lim = O.LAST_LIMIT
    h = np.bincount(want["bread"], minlength=nrb)
    cap = max(int(h.max()), len(want) // 5)
    lo, sums = greedy(h, cap)
    assert len(sums) >= 3
    memvar = C.c_uint64.in_dll(L, "MEM_LIMIT")
    old = memvar.value
    p = Pair(L, an, an, cross)
    try:
        memvar.value = mem
        got = p.match(cap=cap, seeds=True)
        assert L.damar_last_limit() == lim
        assert got["totals"][1] > 0 and got["slabs"] == (lo, sums)
        assert got["nseeds"] == len(want) and np.array_equal(got["seeds"], want)
    finally:
        memvar.value = old
        p.close()


def case_cap(gpu, case):
    """The largest number of seed pairs of one B read over the case's comparisons, from an in-process pass with the
    case's -k and -I and nothing that only removes k-mers (-t, masks: an upper bound is all that is needed), rounded up
    to a multiple of 64."""
    kw = case_kw(case["name"])
    top = 0
    for a, bs in case["lines"]:
        for b in bs:
            for comp in (0, 1):
                p = Pair(gpu, os.path.join(case["dbdir"], "G." + a), os.path.join(case["dbdir"], "G." + b), comp, **kw)
                try:
                    s = p.match(cap=1 << 40, seeds=True)["seeds"]
                    if len(s):
                        top = max(top, int(np.bincount(s["bread"]).max()))
                finally:
                    p.close()
    from damar_amd import api
    api.set_globals()
    return (top + 63) // 64 * 64


def run_plan_cli(case, work, env):
    from damar_amd import api
    link_db(case["dbdir"], work)
    with open(os.path.join(work, "plan.txt"), "w") as f:
        for a, bs in case["lines"]:
            f.write("daligner %s G.%s %s\n" % (" ".join(case["opts"]), a, " ".join("G." + b for b in bs)))
    st = os.path.join(work, "stats.json")
    subprocess.run([api.daligner_binary(), "-P", "plan.txt"], cwd=work, check=True, stdout=subprocess.DEVNULL,
                   env=dict(os.environ, DAMAR_PLAN_STATS=st, **env))
    return json.load(open(st))


CAPS = {}

MODES = [{}, {"DAMAR_EARLY_CUT": "1"}, {"DAMAR_SORT_PAIR": "0"}, {"DAMAR_SORT_PAIR": "1"}, {"DAMAR_WORK_TWOSTEP": "1"},
         {"DAMAR_PACK_SEEDS": "0"}, {"DAMAR_MERGE_GENERAL": "1"}, {"DAMAR_OVERLAP": "0"}, {"DAMAR_TEST_SMALL_CAPS": "1"},
         {"DAMAR_PACK_POS": "0"}]          # (position words as block offsets: the reads of a B entry through boff / coarse)
CASES = ["tiny2", "tandem", "tandem2", "tiny_I", "tiny_k12", "tiny_t", "tiny_j1", "mask_two", "bias_mask", "fusion", "prod"]
CROSSED = [(n, m) for n in CASES for m in (MODES if n in ("tiny2", "tandem") else MODES[:1])]


@pytest.mark.parametrize("name,mode", CROSSED, ids=["%s-%s" % (n, "".join("%s=%s" % kv for kv in m.items()) or "plain") for n, m in CROSSED])
def test_gpu_cli_plan_in_slabs_equals_reference_golden(gpu, tmp_path, name, mode):
    """The daligner binary in plan mode with the seed stages cut into slabs: the files are the reference's, under every
    variant of the seed stage, and the line of DAMAR_PLAN_STATS says that comparisons were split."""
    case = read_case(name)
    if name not in CAPS:
        CAPS[name] = case_cap(gpu, case)
    st = run_plan_cli(case, str(tmp_path), dict(mode, **{HOOK: str(CAPS[name])}))
    print(name, mode, "cap", CAPS[name], "seed_slabs", st["seed_slabs"], "split_comparisons", st["split_comparisons"])
    assert compare_las(case, str(tmp_path)) == []
    assert st["seed_slabs"] > st["split_comparisons"] > 0


@pytest.mark.parametrize("name", ["tiny2", "tandem"])
def test_gpu_slabs_with_pairs_split_by_b_read_range(gpu, tmp_path, name):
    """The scheme of test_gpu_work_queue_and_split_pairs_equal_reference_golden (upr = 5: every pair split by B-read range,
    damar_set_bread_range) with the seed stages in slabs: the parts merge into the reference's files, and slabs that lie
    wholly outside a part's range are not run -- fewer seed stages than the same comparisons take without a range."""
    from damar_amd import api, multi, driver
    case = read_case(name)
    cap = case_cap(gpu, case)
    work = str(tmp_path)
    link_db(case["dbdir"], work)
    nblocks = int(open(os.path.join(work, "G.db")).read().split("blocks =")[1].split()[0])
    units = multi.work_units(nblocks, 4, units_per_rank=5)
    assert max(n for _, _, _, n in units) > 1
    os.environ[HOOK] = str(cap)
    try:
        runner = multi.GpuRunner(dict(j=4), max_blocks=1)
        mine = multi.run_queue(os.path.join(work, "G"), units, work, multi.LocalQueue(len(units)), runner)
        runner.finish()
        assert len(mine) == len(units)
        ranged_slabs, ranged_split = runner.plan.seed_slabs, runner.plan.split_comparisons
        for r in range(4):
            multi.merge_parts(os.path.join(work, "G"), units, work, r, 4)
        runner.close()
        assert compare_las(case, work) == []
        # the same comparisons, as often as the parts ran them, without a range
        gpu.damar_set_bread_range(0, -1)
        plan = driver.Plan(j=4)
        blocks = {i: driver.Block(os.path.join(work, "G.%d" % i)) for i in range(1, nblocks + 1)}
        out = os.path.join(work, "whole")
        for a, b, _, _ in units:
            plan.run_line(blocks[a], [blocks[b]], out)
        plan.finish()
        print(name, "cap", cap, "ranged", ranged_slabs, ranged_split, "whole", plan.seed_slabs, plan.split_comparisons)
        assert ranged_split > 0 and plan.split_comparisons == ranged_split
        assert ranged_slabs < plan.seed_slabs
    finally:
        os.environ.pop(HOOK, None)
        gpu.damar_set_bread_range(0, -1)


def test_gpu_block_sized_pair_in_slabs_has_the_files_of_the_whole_run(gpu, tmp_path):
    """One cross pair of the config-2 database (two blocks of 25 Mbp) with the figure at a quarter of its seed pairs: the
    only check at a size where tiles, scans and arenas are not toy-sized.  md5s of the split run's files equal those of
    the run in one piece, in the same process."""
    from damar_amd import api, driver
    d = str(tmp_path)
    nb = api.sim_write_db(d, "SIM", 4.6, coverage=87., seed=3, block_mbp=25)
    assert nb >= 2
    blocks = {i: driver.Block(os.path.join(d, "SIM.%d" % i)) for i in (1, 2)}

    def run(out, cap):
        if cap:
            os.environ[HOOK] = str(cap)
        try:
            plan = driver.Plan(j=4)
            plan.run_line(blocks[2], [blocks[1]], out)
            plan.finish()
        finally:
            os.environ.pop(HOOK, None)
        md = {}
        for dp, _, fs in os.walk(out):
            for f in fs:
                if f.endswith(".las"):
                    md[os.path.relpath(os.path.join(dp, f), out)] = hashlib.md5(open(os.path.join(dp, f), "rb").read()).hexdigest()
        return plan, md

    whole, md0 = run(os.path.join(d, "whole"), None)
    assert whole.split_comparisons == 0 and whole.seed_slabs == 2 and len(md0) >= 2
    cap = max(whole.counts[0] // 2 // 4, 1)                 # (two comparisons, N and C, of much the same size)
    split, md1 = run(os.path.join(d, "split"), cap)
    print("config-2 pair: seed pairs", whole.counts[0], "cap", cap, "seed stages", split.seed_slabs, "split", split.split_comparisons)
    assert split.split_comparisons == 2 and split.seed_slabs >= 8
    assert md1 == md0
    assert split.counts == whole.counts


@pytest.mark.parametrize("mode", [{}, {"DAMAR_EARLY_CUT": "1"}, {"DAMAR_OVERLAP": "0"}], ids=["plain", "early_cut", "no_overlap"])
@pytest.mark.parametrize("name,free_mb", [("tandem", 12), ("fusion", 12)])
def test_gpu_cli_plan_under_the_figure_derived_from_free_memory(gpu, tmp_path, name, free_mb, mode):
    """The production figure, not DAMAR_TEST_SEED_CAP: the seed pairs the arenas of one comparison slot and the shared
    seed-stage arenas can be grown to hold in half the free device memory (shim.hip seed_cap).  DAMAR_TEST_FREE_BYTES
    stands for the free memory: 12 MB, of which half counts, against three or four arenas that start empty in a fresh
    process and grow by at least 1 MB each at about 46 B per seed pair (75 B with the early cut) -- room for some 60 000
    (25 000) seed pairs where these comparisons have a few hundred thousand and no B read more than 13 120.  So the
    question to the figure, its bisection and the one-slot rule for the slabs it cuts (each slab's launch completed before
    the next slab's seed stage) all run; the files are the reference's."""
    case = read_case(name)
    st = run_plan_cli(case, str(tmp_path), dict(mode, DAMAR_TEST_FREE_BYTES=str(free_mb << 20)))
    print(name, mode, "free MB", free_mb, "seed_slabs", st["seed_slabs"], "split_comparisons", st["split_comparisons"])
    assert compare_las(case, str(tmp_path)) == []
    assert st["seed_slabs"] > st["split_comparisons"] > 0


def test_gpu_slabs_where_a_run_lies_at_a_slice_end(gpu, tmp_path):
    """A comparison in which the minhit rule at an interior slice end bites (filter.c:2212-2214), found on the CPU with
    the oracle: simulated reads, 1 Mbp genome at 2x coverage (sparse: many short runs), seed 6, block S.1 against its own
    complement with -k14 -h20 (minhit 2).  The oracle enters 36 read pairs with -j1 and -j4 but 34 with -j8: two runs start
    within minhit seeds of the end of a thread's slice.  First the oracle is asked again, so that the case cannot go
    stale unnoticed; then the GPU run in one piece must show the same dependence on -j, and the run in slabs -- at the
    smallest figure possible, the largest count of a B read, and at a fifth of the seed pairs -- must have counters 0-4 of
    the run in one piece for -j1, -j4 and -j8.  An interior slice end put on the wrong bread border changes which runs
    are dropped, and with them work items and Local_Alignment calls."""
    import re
    from damar_amd import api
    d = str(tmp_path)
    assert api.sim_write_db(d, "S", 1.0, coverage=2.0, seed=6, block_mbp=1) >= 1
    seen = {}
    for j in (1, 4, 8):
        o = subprocess.run([os.path.join(ROOT, "oracle", "oracle_daligner"), "-v", "-k14", "-h20", "-j%d" % j, "S.1", "S.1"], cwd=d,
                           check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True).stdout
        m = re.search(r"^C \S+ x \S+: (\d+) hits (\d+) seeds (\d+) confirmed", o, re.M)
        seen[j] = (int(m.group(1)), int(m.group(2)))
    print("oracle (seed pairs, read pairs entered) by -j:", seen)
    assert seen[1][0] == seen[8][0] and seen[1][1] != seen[8][1]
    name = os.path.join(d, "S.1")
    whole = {}
    for j in (1, 4, 8):
        p = Pair(gpu, name, name, 1, j=j, h=20)
        try:
            first = p.match(cap=1 << 40, seeds=True, j=j)
            h = np.bincount(first["seeds"]["bread"], minlength=p.bdb.nreads)
            whole[j] = p.match(j=j)["counters"]
            assert whole[j][0] == seen[j][0] and whole[j][2] == seen[j][1]
            for cap in (int(h.max()), max(int(h.max()), len(first["seeds"]) // 5)):
                lo, sums = greedy(h, cap)
                assert len(sums) >= 3
                got = p.match(cap=cap, j=j)
                print("j", j, "cap", cap, "slabs", len(sums), "whole", whole[j], "split", got["counters"])
                assert got["totals"][1] > 0 and got["slabs"] == (lo, sums)
                assert got["counters"] == whole[j]
        finally:
            gpu.Set_Filter_Params(14, 6, 0, 35, 4)
            p.close()
    assert whole[1] != whole[8]
