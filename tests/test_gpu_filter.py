"""LAfilter on the device path (kernels/pile_filter.hip, and kernels/box_align.hip under -T) against the fixtures the
reference's LAfilter left in tests/golden/filter/, and damar_pile_filter on the planted and on seeded random piles against
the plain routine of host/filter.c."""
import os

import numpy as np
import pytest

import filter_common as fc
import q_common

pytestmark = pytest.mark.gpu
CASES = fc.load_cases()
DROP = ("DAMAR_PILES", "DAMAR_TRIM", "DAMAR_TEST_FILTER_LEN", "DAMAR_TEST_FILTER_GROUP", "DAMAR_TEST_FILTER_GRID", "DAMAR_TEST_BOX_LIMIT",
        "DAMAR_PILE_BATCH")
NAMES = ("flags", "aepos", "bepos", "diffs", "tlen", "reason", "cont_by", "cnt")
# the option sets of the pile call: what the cases run on the planted file, without the options only the file pass sees
SETS = {c["name"][:-6]: [o for o in c["opts"] if o not in ("-v", "-p", "-T", "-L")] for c in CASES if c["input"] == "fsynth"}


@pytest.fixture(autouse=True)
def device_path(monkeypatch):
    for k in DROP:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def planted():
    return fc.trace_batch(os.path.join(fc.FDIR, "synth.las")), q_common.db_read_len("tiny2"), fc.load_cases("files")


@pytest.fixture(scope="module")
def random_piles():
    return fc.random_piles()


def both_paths(batch, rl, monkeypatch, **kw):
    from damar_amd import api
    dev = api.pile_filter(batch, rl, **kw)
    last = api.filter_last()
    monkeypatch.setenv("DAMAR_PILES", "host")
    host = api.pile_filter(batch, rl, **kw)
    monkeypatch.delenv("DAMAR_PILES")
    for k in NAMES:
        bad = np.flatnonzero(np.any(dev[k] != host[k], axis=1) if k == "cnt" else dev[k] != host[k])
        assert len(bad) == 0, "%s differs in %d places, the first %d: %s against %s" % (k, len(bad), bad[0], dev[k][bad[0]], host[k][bad[0]])
    return host, last


@pytest.mark.parametrize("name", sorted(SETS))
def test_planted_piles_match_the_host_routine(planted, name, monkeypatch):
    batch, rl, files = planted
    _, (ms, npiles, host_piles, _) = both_paths(batch, rl, monkeypatch, **fc.opts_to_params(SETS[name], "fsynth", files))
    # the kernel leaves exactly the pile with a run of more records of one B read than a lane takes
    assert (npiles, host_piles) == (len(batch["pile_aread"]), 1)
    assert ms["kernel"] > 0


@pytest.mark.parametrize("name", sorted(SETS))
def test_random_piles_match_the_host_routine(random_piles, planted, name, monkeypatch):
    batch, rl = random_piles
    _, (ms, npiles, host_piles, _) = both_paths(batch, rl, monkeypatch, **fc.opts_to_params(SETS[name], "fsynth", planted[2]))
    assert (npiles, host_piles) == (len(batch["pile_aread"]), 0)


def test_pre_step_alone(planted, random_piles, monkeypatch):
    from damar_amd import api
    for batch, rl in (planted[:2], random_piles):
        host, _ = both_paths(batch, rl, monkeypatch, steps=api.FILTER_PRE, downsample=50, seg_rate=30, stitch=300, remove=0x40)
        assert np.array_equal(host["aepos"], batch["aepos"]) and not np.any(host["reason"])


def test_limits_leave_only_the_planted_piles(planted, monkeypatch):
    """the run of MAXGROUP + 1 records under every option set; with the length limit lowered to the second-longest planted
    read also the longest, but only under -z with -u, which alone needs the coverage bits"""
    from damar_amd import api
    batch, rl, files = planted
    plants = fc.load_cases("plants")
    assert api.filter_limits()[0] == fc.MAXGROUP
    lens = np.sort(rl[batch["pile_aread"]])
    assert lens[-1] == rl[plants["longest"]["aread"]] and lens[-2] < lens[-1]
    monkeypatch.setenv("DAMAR_TEST_FILTER_LEN", str(int(lens[-2])))
    _, (_, _, host_piles, _) = both_paths(batch, rl, monkeypatch, **fc.opts_to_params(["-z", "2", "-u", "200"], "fsynth", files))
    assert host_piles == 2
    _, (_, _, host_piles, _) = both_paths(batch, rl, monkeypatch, **fc.opts_to_params(["-z", "2"], "fsynth", files))
    assert host_piles == 1
    monkeypatch.delenv("DAMAR_TEST_FILTER_LEN")
    monkeypatch.setenv("DAMAR_TEST_FILTER_GROUP", str(fc.MAXGROUP - 1))
    _, (_, _, host_piles, _) = both_paths(batch, rl, monkeypatch, **fc.opts_to_params(["-s", "300"], "fsynth", files))
    assert host_piles == 2                             # the run of exactly MAXGROUP as well


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_tool_case_whole_and_in_small_batches(case, tmp_path):
    dev, small = os.path.join(str(tmp_path), "dev"), os.path.join(str(tmp_path), "small")
    os.makedirs(dev)
    os.makedirs(small)
    fc.run_case(case, dev, timeout_s=120, drop=DROP)
    fc.run_case(case, small, {"DAMAR_PILE_BATCH": "40"}, timeout_s=120, drop=DROP)
    if fc.keeps_traces(case):
        r = fc.lacheck(dev)
        assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.parametrize("name", ["plan_synth", "zu_synth", "plan_tandem"])
def test_api_counts_the_host_piles(name, tmp_path, monkeypatch):
    """through api.filter_las, which shows the count the command does not: the host routine does the planted run of
    MAXGROUP + 1 records and no other pile"""
    from damar_amd import api
    case = next(c for c in CASES if c["name"] == name)
    tmp = fc.workdir(str(tmp_path), case["input"])
    kw = fc.opts_to_params(case["opts"], case["input"], fc.load_cases("files"))
    for k in ("trim", "repeats", "sym", "read_state", "include"):
        kw.pop(k, None)
    p = lambda f: os.path.join(tmp, f)
    st = api.filter_las(p("G"), p(fc.LAS), p("api.las"), purge="-p" in case["opts"], do_trim="-T" in case["opts"], **kw)
    assert fc.tc.md5(p("api.las")) == case["md5"]
    # under -T the two halves of a batch are two calls, each of which leaves the planted pile to the host routine
    assert st["host_piles"] == (1 if case["input"] == "fsynth" else 0)
