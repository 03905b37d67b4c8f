"""LAseparate on the plain host path (DAMAR_PILES=host: host/separate.c) against the fixtures the reference's LAseparate left
in tests/golden/separate/: both output files, stdout, stderr and exit status of every case; and the host routine against
tests/separate_model.py field for field."""
import ctypes
import os

import numpy as np
import pytest

import q_common
import separate_common as sc

CASES = sc.load_cases()
HOST = {"DAMAR_PILES": "host"}
SMALL = dict(HOST, DAMAR_PILE_BATCH="40")


@pytest.fixture(autouse=True)
def host_path(monkeypatch):
    monkeypatch.setenv("DAMAR_PILES", "host")


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_tool_case(case, tmp_path):
    sc.run_case(case, str(tmp_path), HOST)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_small_batches_give_the_same(case, tmp_path):
    sc.run_case(case, str(tmp_path), SMALL)


def check_against_model(batch, rl, rep, twidth=sc.TW):
    from damar_amd import api
    for kind in (0, 1):
        flags, groups = api.pile_chains(batch, rl, rep[0], rep[1], twidth, kind)
        mflags, mgroups, _ = sc.model_batch(batch, rl, rep, twidth, kind)
        assert np.array_equal(flags, mflags), "kind %d: flags differ in records %s" % (kind, np.flatnonzero(flags != mflags)[:8])
        assert len(groups) == len(mgroups)
        for i, (g, m) in enumerate(zip(groups, mgroups)):
            assert g == m, "kind %d, group %d: %s against the model's %s" % (kind, i, g, m)
        if kind == 0:
            first = mgroups
    return first


def test_planted_groups_match_the_model():
    batch = sc.batch_of(os.path.join(sc.SDIR, "synth.las"))
    mgroups = check_against_model(batch, q_common.db_read_len("tiny2"), sc.tracks("ssynth")["rep"])
    # what the generator saw of every plant is what the model still makes of it
    groups = sc.groups_of(batch)
    for tag, pl in sc.load_cases("plants").items():
        if "groups" in pl:                                 # a pile of that many groups of two records, one chain each
            mine = [g for g, (_, recs) in zip(mgroups, groups) if recs[0]["aread"] == pl["aread"]]
            assert len(mine) == pl["groups"] and all(g[:2] == (1, [0, 1]) for g in mine), tag
            continue
        gi = next(i for i, (_, recs) in enumerate(groups) if (recs[0]["aread"], recs[0]["bread"]) == (pl["aread"], pl["bread"]))
        assert [mgroups[gi][0], mgroups[gi][1], mgroups[gi][2]] == pl["seen"], tag


def test_random_piles_match_the_model():
    batch, rl, rep = sc.random_piles()
    sizes = [len(recs) for _, recs in sc.groups_of(batch)]
    assert len(batch["pile_off"]) == 61 and min(sizes) == 1 and max(sizes) == 12
    assert set(np.unique(batch["flags"])) == {0, 1}
    mgroups = check_against_model(batch, rl, rep)
    assert sum(1 for g in mgroups if g[0] > 1) > 20            # the piles do reach the order of the chains


def test_seed_plants_depend_on_the_track_and_on_the_trace_spacing():
    """the host routine follows the model where the repeat counts and the trace spacing decide the seed, and so the files"""
    from damar_amd import api
    batch, rl, rep = sc.batch_of(os.path.join(sc.SDIR, "synth.las")), q_common.db_read_len("tiny2"), sc.tracks("ssynth")["rep"]
    groups = sc.groups_of(batch)
    plants = sc.load_cases("plants")
    at = lambda tag: next(i for i, (_, recs) in enumerate(groups) if (recs[0]["aread"], recs[0]["bread"]) == (plants[tag]["aread"], plants[tag]["bread"]))
    base = api.pile_chains(batch, rl, rep[0], rep[1], sc.TW, 0)[1]
    for tag, r, tw in (("seed_unique", (None, None), sc.TW), ("seed_fallback", rep, 0)):
        flags, other = api.pile_chains(batch, rl, r[0], r[1], tw, 0)
        mflags, mother, _ = sc.model_batch(batch, rl, None if r[0] is None else r, tw, 0)
        assert np.array_equal(flags, mflags) and other == mother
        assert base[at(tag)][1] != other[at(tag)][1] and base[at(tag)][2] != other[at(tag)][2], tag


def test_filler_taken_twice_makes_a_chain_longer_than_its_group():
    """the host routine begins with member lists of the group's size, so these two groups go through its second run"""
    batch, rl, rep = sc.batch_of(os.path.join(sc.SDIR, "synth.las")), q_common.db_read_len("tiny2"), sc.tracks("ssynth")["rep"]
    _, _, full = sc.model_batch(batch, rl, rep, sc.TW, 0)
    longer = [len(m["best"]) - len(recs) for m, (_, recs) in zip(full, sc.groups_of(batch)) if len(m["best"]) > len(recs)]
    assert longer == [1, 1]                               # fill_twice and fill_twice_64; that the routine equals the model on them is
    #                                                       test_planted_groups_match_the_model


def test_temp_on_input_is_not_looked_at():
    from damar_amd import api
    batch, rl, rep = sc.random_piles()
    marked = dict(batch, flags=batch["flags"] | np.where(np.arange(len(batch["flags"])) % 3 == 0, sc.TEMP, 0).astype(np.int32))
    for kind in (0, 1):
        flags, groups = api.pile_chains(marked, rl, rep[0], rep[1], sc.TW, kind)
        plain = api.pile_chains(batch, rl, rep[0], rep[1], sc.TW, kind)
        assert np.array_equal(flags, plain[0]) and groups == plain[1]


def test_no_track_gives_no_repeat_bases():
    from damar_amd import api
    batch, rl, _ = sc.random_piles()
    flags, groups = api.pile_chains(batch, rl, None, None, sc.TW, 0)
    mflags, mgroups, _ = sc.model_batch(batch, rl, None, sc.TW, 0)
    assert np.array_equal(flags, mflags) and groups == mgroups


def test_error_runs(tmp_path):
    tmp = sc.workdir(str(tmp_path), "tiny2")
    for e in sc.load_cases("errors"):
        r = sc.run_tool([], tmp, HOST, args=e["args"])
        assert (r.returncode, r.stdout, r.stderr) == (e["rc"], e["stdout"], e["stderr"]), e["name"]


def test_group_that_comes_all_flagged_is_an_error_run(tmp_path):
    """two records of one read pair that both come discarded: the reference leaves chain() without a chain, counts one of
    the two and aborts on its own assert after the first file; here a message names the group"""
    tmp = sc.workdir(str(tmp_path), "fusion")
    pair = sc.flag_first_pair(os.path.join(tmp, sc.LAS))
    r = sc.run_tool(["-T0"], tmp, HOST)
    rc, out, err = sc.ALL_FLAGGED
    assert (r.returncode, r.stdout, r.stderr) == (rc, out, err % pair)
    assert sc.load_cases("reference_aborts")["rc"] == -6    # what the generator saw the reference do with this file


@pytest.mark.parametrize("name", ["T0_ssynth", "T1r_ssynth", "T1_tandem"])
def test_api_agrees_with_the_command(name, tmp_path, capfd):
    from damar_amd import api
    case = next(c for c in CASES if c["name"] == name)
    tmp = sc.workdir(str(tmp_path), case["input"])
    p = lambda f: os.path.join(tmp, f)
    st = api.separate_las(p("G"), p(sc.LAS), p(sc.OUT), p(sc.OUT2), kind=sc.kind_of(case["opts"]), repeats=sc.track_of(case["opts"]))
    assert [sc.tc.md5(p(sc.OUT)), sc.tc.md5(p(sc.OUT2))] == [case["md5"], case["md5_discard"]]
    want = sc.expected_flags(name)
    assert (st["written"], st["written_discard"]) == (int(np.sum((want & sc.DISCARD) == 0)), int(np.sum((want & sc.DISCARD) != 0)))
    assert (st["kept"], st["discarded"], st["host_groups"]) == (st["written"], st["written_discard"], 0)
    assert capfd.readouterr().out == case["stdout"]


def test_refused_write(tmp_path):
    tmp = sc.workdir(str(tmp_path), "tiny2")
    r = sc.run_tool([], tmp, HOST, args=("G", sc.LAS, sc.OUT, sc.tc.FULL))
    assert (r.returncode, r.stderr) == (1, sc.tc.CANNOT_WRITE)


def test_symbols_and_command_exist():
    from damar_amd import api
    lib = ctypes.CDLL(os.path.join(sc.ROOT, "damar_amd", "libdamar_hip.so"))
    for name in ("damar_pile_chains", "damar_host_chain_group", "damar_separate_inputs_valid", "damar_separate_las", "damar_separate_last",
                 "damar_separate_limits", "damar_separate_release"):
        assert hasattr(lib, name), name
    assert os.access(os.path.join(sc.BIN, "LAseparate"), os.X_OK)
    assert api.separate_limits() == (64, 16)
