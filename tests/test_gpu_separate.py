"""LAseparate on the device path (kernels/pile_chains.hip) against the fixtures the reference's LAseparate left in
tests/golden/separate/, and damar_pile_chains on the planted and on random piles against the plain routine of
host/separate.c field for field."""
import os

import numpy as np
import pytest

import q_common
import separate_common as sc

pytestmark = pytest.mark.gpu
CASES = sc.load_cases()
DROP = ("DAMAR_PILES", "DAMAR_TEST_SEPARATE_GROUP", "DAMAR_TEST_SEPARATE_CHAINS", "DAMAR_TEST_SEPARATE_GRID", "DAMAR_PILE_BATCH")


@pytest.fixture(autouse=True)
def device_path(monkeypatch):
    for k in DROP:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def planted():
    return sc.batch_of(os.path.join(sc.SDIR, "synth.las")), q_common.db_read_len("tiny2"), sc.tracks("ssynth")["rep"]


def both_paths(batch, rl, rep, kind, monkeypatch):
    from damar_amd import api
    dev = api.pile_chains(batch, rl, rep[0], rep[1], sc.TW, kind)
    last = api.separate_last()
    monkeypatch.setenv("DAMAR_PILES", "host")
    host = api.pile_chains(batch, rl, rep[0], rep[1], sc.TW, kind)
    monkeypatch.delenv("DAMAR_PILES")
    assert np.array_equal(dev[0], host[0]), "flags differ in records %s" % np.flatnonzero(dev[0] != host[0])[:8]
    assert len(dev[1]) == len(host[1])
    for i, (d, h) in enumerate(zip(dev[1], host[1])):
        assert d == h, "group %d: %s against the host routine's %s" % (i, d, h)
    return host, last


def beyond(batch, rl, rep, kind, maxgroup, maxchains):
    """the groups the model finds beyond the limits: the host routine's"""
    _, _, full = sc.model_batch(batch, rl, rep, sc.TW, kind)
    return sum(1 for m, (_, recs) in zip(full, sc.groups_of(batch)) if sc.beyond_limits(m, len(recs), maxgroup, maxchains))


@pytest.mark.parametrize("kind", [0, 1])
def test_planted_groups_match_the_host_routine(planted, kind, monkeypatch):
    from damar_amd import api
    batch, rl, rep = planted
    host, (ms, ngroups, host_groups, multi) = both_paths(batch, rl, rep, kind, monkeypatch)
    _, mgroups, _ = sc.model_batch(batch, rl, rep, sc.TW, kind)
    assert host[1] == mgroups
    # the host routine did exactly the three groups planted beyond the limits: 65 records, 17 chains, a chain of 65 members
    assert beyond(batch, rl, rep, kind, *api.separate_limits()) == 3
    assert (ngroups, host_groups, multi) == (len(mgroups), 3, sum(1 for _, recs in sc.groups_of(batch) if len(recs) > 1))
    assert ms["kernel"] > 0


@pytest.mark.parametrize("kind", [0, 1])
def test_random_piles_match_the_host_routine(kind, monkeypatch):
    batch, rl, rep = sc.random_piles()
    host, (_, ngroups, host_groups, _) = both_paths(batch, rl, rep, kind, monkeypatch)
    assert (ngroups, host_groups) == (len(host[1]), 0)


@pytest.mark.parametrize("env, limits", [({"DAMAR_TEST_SEPARATE_CHAINS": "15"}, (64, 15)), ({"DAMAR_TEST_SEPARATE_GROUP": "63"}, (63, 16)),
                                         ({"DAMAR_TEST_SEPARATE_CHAINS": "1"}, (64, 1)), ({"DAMAR_TEST_SEPARATE_GRID": "3"}, (64, 16))],
                         ids=["chains_15", "group_63", "chains_1", "grid_3"])
def test_lowered_limits_leave_what_the_model_finds_beyond_them(planted, env, limits, monkeypatch):
    batch, rl, rep = planted
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    host, (_, _, host_groups, _) = both_paths(batch, rl, rep, 0, monkeypatch)
    assert host_groups == beyond(batch, rl, rep, 0, *limits)


def test_temp_on_input_is_not_looked_at(monkeypatch):
    batch, rl, rep = sc.random_piles()
    marked = dict(batch, flags=batch["flags"] | np.where(np.arange(len(batch["flags"])) % 3 == 0, sc.TEMP, 0).astype(np.int32))
    host, _ = both_paths(marked, rl, rep, 0, monkeypatch)
    assert not np.any(host[0][[g0 for g0, recs in sc.groups_of(batch) if len(recs) == 1]] & sc.TEMP)


def test_error_runs_on_the_device_path(tmp_path):
    tmp = sc.workdir(str(tmp_path), "tiny2")
    for e in sc.load_cases("errors"):
        r = sc.run_tool([], tmp, args=e["args"], timeout_s=60, drop=DROP)
        assert (r.returncode, r.stdout, r.stderr) == (e["rc"], e["stdout"], e["stderr"]), e["name"]


def test_group_that_comes_all_flagged_is_an_error_run_on_the_device_path(tmp_path):
    tmp = sc.workdir(str(tmp_path), "fusion")
    pair = sc.flag_first_pair(os.path.join(tmp, sc.LAS))
    r = sc.run_tool(["-T0"], tmp, timeout_s=60, drop=DROP)
    rc, out, err = sc.ALL_FLAGGED
    assert (r.returncode, r.stdout, r.stderr) == (rc, out, err % pair)


def test_no_track(monkeypatch):
    batch, rl, _ = sc.random_piles()
    both_paths(batch, rl, (None, None), 0, monkeypatch)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_tool_case_small_batches_and_host_count(case, tmp_path, monkeypatch):
    """the command on the device path, whole and in small batches, against the fixture; then the same through
    api.separate_las, which shows the count the command does not: the host routine does the three planted groups beyond the
    limits and no group of a real file"""
    from damar_amd import api
    dev, small = os.path.join(str(tmp_path), "dev"), os.path.join(str(tmp_path), "small")
    os.makedirs(dev)
    os.makedirs(small)
    sc.run_case(case, dev, timeout_s=120, drop=DROP)
    sc.run_case(case, small, {"DAMAR_PILE_BATCH": "40"}, timeout_s=120, drop=DROP)
    p = lambda f: os.path.join(dev, f)
    st = api.separate_las(p("G"), p(sc.LAS), p("api.las"), p("api2.las"), kind=sc.kind_of(case["opts"]), repeats=sc.track_of(case["opts"]))
    assert [sc.tc.md5(p("api.las")), sc.tc.md5(p("api2.las"))] == [case["md5"], case["md5_discard"]], case["name"]
    assert st["host_groups"] == case["host_groups"] == (3 if case["input"] == "ssynth" else 0), (case["name"], st)
