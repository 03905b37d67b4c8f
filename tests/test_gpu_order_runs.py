"""The ordering step behind the seed sort over the read pair only (kernels/seed_merge.hip order_waves / order_long, through
the test hook damar_order_runs_test): every listed run of up to 2048 seeds comes out in order of its A positions, equal
positions in the order they had -- what numpy's stable argsort gives -- and every other key is bit-identical to the input.
Then the whole path with the pair sort forced on against the sort over all the bits.  Everything here needs a real MI355X."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import read_case, link_db, compare_las

pytestmark = pytest.mark.gpu

OR_WAVE = 512         # the longest run a wavefront sorts in its registers (seed_merge.hip)
OR_MAX = 2048         # the longest run that is ordered at all
PAIR_BITS = 28

# every length at which the code takes another path: 1 (nothing to do), one key a lane up to 64, then 2, 4 and 8 keys a
# lane (128, 256, OR_WAVE), the workgroup in LDS beyond, its power-of-two padding, and 2048 as the last length ordered
LENGTHS = [1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257,
           OR_WAVE - 1, OR_WAVE, OR_WAVE + 1, 1023, 1025, 2047, 2048]


@pytest.fixture(scope="module")
def gpu(built):
    from damar_amd import api
    L = api.lib()
    assert L.damar_hip_init(0) >= 1
    return L


def make_keys(lengths, listed, ppos, dbits, variant, seed):
    """Runs of the given lengths, one read pair each, one behind the other; work = the heads of those with listed[r]."""
    rng = np.random.default_rng(seed)
    n = int(sum(lengths))
    pair = np.repeat(np.arange(len(lengths), dtype=np.uint64) * np.uint64(2654435761 % (1 << PAIR_BITS) | 1) % np.uint64(1 << PAIR_BITS),
                     lengths)
    # (distinct pairs: an odd multiplier is a bijection modulo 2^28; neighbours differ)
    apos = rng.integers(0, 1 << ppos, n, dtype=np.uint64)
    low = rng.integers(0, 1 << dbits, n, dtype=np.uint64)
    heads = np.concatenate(([0], np.cumsum(lengths)[:-1])).astype(np.int64)
    for h, ln in zip(heads, lengths):
        if variant == "equal":
            apos[h:h + ln] = apos[h]
        elif variant == "sorted":
            apos[h:h + ln] = np.sort(apos[h:h + ln])
        elif variant == "reversed":
            apos[h:h + ln] = np.sort(apos[h:h + ln])[::-1]
        elif variant == "few":                         # many ties among few values
            apos[h:h + ln] = apos[h:h + ln] % np.uint64(5)
    keys = (pair << np.uint64(ppos + dbits)) | (apos << np.uint64(dbits)) | low
    work = np.array([h for h, on in zip(heads, listed) if on], dtype=np.uint32)
    return keys, work


def expected(keys, work, ppos, dbits):
    want = keys.copy()
    pair = keys >> np.uint64(ppos + dbits)
    starts = np.concatenate((np.flatnonzero(pair[1:] != pair[:-1]) + 1, [len(keys)]))      # where the pair changes
    ends = starts[np.searchsorted(starts, work, side="right")]
    for h, e in zip(work, ends):
        h, e = int(h), int(e)
        if e - h <= OR_MAX:
            a = (keys[h:e] >> np.uint64(dbits)) & np.uint64((1 << ppos) - 1)
            want[h:e] = keys[h:e][np.argsort(a, kind="stable")]
    return want


def check(keys, work, ppos, dbits):
    from damar_amd import api
    got = api.order_runs(keys, ppos, dbits, work)
    want = expected(keys, work, ppos, dbits)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, "first difference at seed %d of %d" % (bad[0], len(keys))


@pytest.mark.parametrize("variant", ["random", "equal", "sorted", "reversed", "few"])
@pytest.mark.parametrize("ppos,dbits", [(8, 1), (8, 15), (15, 15), (21, 15), (21, 1)])
def test_gpu_order_runs_every_length_equals_stable_argsort(gpu, ppos, dbits, variant):
    """Every length of LENGTHS as a listed run, with unlisted runs of 1 .. 700 seeds between some of them (they must not
    change), two listed runs adjacent in memory after every third, a listed run of 2049 seeds (left as it is), and 2048 as
    the last run, ending exactly at nhits.  59 work items: not a multiple of the 4 a workgroup takes of a short list (a run
    per wavefront).  ppos 8 and 21 are the bounds of the pair sort (pbits >= 8, pbits + 11 <= 32)."""
    rng = np.random.default_rng(ppos * 100 + dbits)
    lengths, listed = [], []
    for q, ln in enumerate(LENGTHS[:-1]):
        lengths.append(ln)
        listed.append(True)
        if q % 3 != 2:                                 # (else: the next listed run follows at once)
            lengths.append(int(rng.integers(1, 700)))
            listed.append(False)
    lengths += [OR_MAX + 1, 40]
    listed += [True, False]
    for _ in range(36):                                # short runs, so that the list spans two workgroups
        lengths.append(int(rng.integers(2, 100)))
        listed.append(True)
    lengths.append(LENGTHS[-1])
    listed.append(True)
    keys, work = make_keys(lengths, listed, ppos, dbits, variant, seed=7 + ppos + dbits)
    assert len(work) == len(LENGTHS) + 1 + 36 and len(work) % 4 != 0
    assert int(work[-1]) + OR_MAX == len(keys)
    check(keys, work, ppos, dbits)


@pytest.mark.parametrize("nruns", [4 * 2048 + 1, 8 * 2048 + 13])
def test_gpu_order_runs_long_work_lists(gpu, nruns):
    """Work lists long enough for a workgroup to take 16 and 32 items, a wavefront several runs one after the other (the slice
    grows with the list up to 32); neither length is a multiple of its slice.  Runs of 2 .. 40 seeds, every third unlisted,
    and one of 300 and one of 600 seeds among them."""
    rng = np.random.default_rng(nruns)
    lengths = [int(x) for x in rng.integers(2, 41, nruns + nruns // 2)]
    lengths[100], lengths[1000] = 300, 600
    listed = [q % 3 != 2 for q in range(len(lengths))]
    keys, work = make_keys(lengths, listed, 15, 15, "random", seed=5)
    assert len(work) == nruns and nruns % (4 * (nruns // 2048)) != 0
    check(keys, work, 15, 15)


@pytest.mark.parametrize("nwork", [0, 1])
def test_gpu_order_runs_empty_and_single_work_list(gpu, nwork):
    """nwork = 0 changes nothing; nwork = 1 orders that run alone, the other runs stay (one of them longer than a wavefront's)."""
    keys, work = make_keys([100, 600, 30], [False, True, False], 15, 15, "random", seed=3)
    check(keys, work[:nwork], 15, 15)


def test_gpu_order_runs_whole_array_is_one_run(gpu):
    """One run that is the whole array, at a length a wavefront probes twice (65) and at one of a single probe (64): the probe
    must not read behind nhits."""
    for n in (64, 65, OR_WAVE, OR_WAVE + 1):
        keys, work = make_keys([n], [True], 15, 15, "random", seed=n)
        check(keys, work, 15, 15)


def _plan(case, d, env):
    link_db(case["dbdir"], d)
    with open(os.path.join(d, "plan.txt"), "w") as f:
        for a, bs in case["lines"]:
            f.write("daligner %s G.%s %s\n" % (" ".join(case["opts"]), a, " ".join("G." + b for b in bs)))
    from damar_amd import api
    st = os.path.join(d, "stats.json")
    subprocess.run([api.daligner_binary(), "-P", "plan.txt"], cwd=d, check=True, stdout=subprocess.DEVNULL,
                   env=dict(os.environ, DAMAR_PLAN_STATS=st, **env))
    return json.load(open(st))


def test_gpu_order_runs_too_long_a_run_goes_to_the_full_sort(gpu, tmp_path):
    """DAMAR_TEST_RUN_MAX=6: kept runs of more than 6 seeds count as too long to order, the comparison is sorted over all the
    bits after all (the path of a run beyond 2048 seeds); the records are the golden ones."""
    case = read_case("tandem")
    st = _plan(case, str(tmp_path), {"DAMAR_SORT_PAIR": "1", "DAMAR_TEST_RUN_MAX": "6"})
    assert compare_las(case, str(tmp_path)) == []
    assert st["resorted"] > 0


@pytest.mark.parametrize("name", ["tandem", "fusion", "noisy"])
def test_gpu_pair_sort_on_and_off_give_the_same_plan(gpu, tmp_path, name):
    """DAMAR_SORT_PAIR=1 against =0, a child process each: the same work items, alignments and records, and the same files
    (records and trace values byte for byte)."""
    case = read_case(name)
    dirs = [os.path.join(str(tmp_path), x) for x in ("on", "off")]
    stats = [_plan(case, d, {"DAMAR_SORT_PAIR": v}) for d, v in zip(dirs, ("1", "0"))]
    for k in ("work_items", "seed_pairs", "local_alignments", "records"):
        assert stats[0][k] == stats[1][k], k
    assert stats[0]["work_items"] > 0 and stats[0]["resorted"] == 0
    n = 0
    for dp, _, fs in os.walk(dirs[1]):
        for f in fs:
            if f.endswith(".las"):
                rel = os.path.relpath(os.path.join(dp, f), dirs[1])
                assert open(os.path.join(dp, f), "rb").read() == open(os.path.join(dirs[0], rel), "rb").read(), rel
                n += 1
    assert n >= len(case["las"])
    assert compare_las(case, dirs[0]) == []
