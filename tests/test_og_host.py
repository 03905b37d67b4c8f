"""OGbuild by the plain host routine (DAMAR_PILES=host) against the reference's runs kept in tests/golden/og/: graph files,
stdout, stderr and exit status of every case, whole and in batches of 40 records, and the error runs."""
import os
import tempfile

import pytest

import og_common as oc
import q_common

HOST = {"DAMAR_PILES": "host"}
CASES = oc.load_cases()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_host_equals_reference(built, case):
    with tempfile.TemporaryDirectory() as tmp:
        oc.run_case(case, tmp, HOST)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_host_in_batches(built, case):
    with tempfile.TemporaryDirectory() as tmp:
        oc.run_case(case, tmp, dict(HOST, DAMAR_PILE_BATCH="40"))


@pytest.mark.parametrize("err", oc.load_cases("errors"), ids=[e["name"] for e in oc.load_cases("errors")])
def test_error_runs(built, err):
    with tempfile.TemporaryDirectory() as tmp:
        oc.workdir(tmp, "synth")
        r = oc.run_tool(err["args"], tmp, HOST)
        assert (r.returncode, r.stdout, r.stderr) == (err["rc"], err["stdout"], err["stderr"])


def test_edges_call_on_host(built, monkeypatch):
    """api.og_edges by the host routine: the counters the reference prints for the planted file"""
    monkeypatch.setenv("DAMAR_PILES", "host")
    from damar_amd import api
    case = next(c for c in CASES if c["name"] == "def_synth")
    with tempfile.TemporaryDirectory() as tmp:
        oc.workdir(tmp, "synth")
        g = api.og_edges(os.path.join(tmp, "G"), os.path.join(tmp, oc.LAS))
    out = case["stdout"]
    assert "%d left edges\n%d right edges\n" % (g["cnt_left"], g["cnt_right"]) in out
    assert "  %d edges\n  %d redges\n  %d symmetric discards\n" % (g["edges"], g["redges"], g["symdiscard"]) in out
    assert "  %d parallel edges\nremoved %d edges\n" % (g["parallel"], g["removed"]) in out
    assert g["left"].shape[0] == g["loff"][-1] and g["right"].shape[0] == g["roff"][-1] and g["neg_rec"] == -1


def test_host_arrays_equal_model_on_planted_file(built, monkeypatch):
    """offsets, edge fields, statuses and counters of the host routine against tests/og_model.py, field for field"""
    monkeypatch.setenv("DAMAR_PILES", "host")
    from damar_amd import api
    rl = q_common.db_read_len("tiny2")
    ta, td, _, _ = oc.tracks("synth")
    with tempfile.TemporaryDirectory() as tmp:
        oc.workdir(tmp, "synth")
        host = api.og_edges(os.path.join(tmp, "G"), os.path.join(tmp, oc.LAS))
        model = oc.model_of(os.path.join(tmp, oc.LAS), rl, oc.trim_pairs(ta, td))
    oc.same_edges(host, model)
    assert model["symdiscard"] == 5 and model["cnt_left"] > model["edges"] - model["redges"]


@pytest.mark.parametrize("inp", oc.REAL)
def test_host_arrays_equal_model_on_real_files(built, monkeypatch, inp):
    monkeypatch.setenv("DAMAR_PILES", "host")
    from damar_amd import api
    rl = q_common.db_read_len(oc.DB_OF[inp])
    ta, td, _, _ = oc.tracks(inp)
    with tempfile.TemporaryDirectory() as tmp:
        oc.workdir(tmp, inp)
        host = api.og_edges(os.path.join(tmp, "G"), os.path.join(tmp, oc.LAS))
        model = oc.model_of(os.path.join(tmp, oc.LAS), rl, oc.trim_pairs(ta, td))
    oc.same_edges(host, model)


def test_host_arrays_equal_model_on_random_piles(built, monkeypatch):
    """60 seeded random piles: every flag the tool looks at, runs of one B read, containments, symmetric discards that hit"""
    monkeypatch.setenv("DAMAR_PILES", "host")
    from damar_amd import api
    with tempfile.TemporaryDirectory() as tmp:
        db, las, rl, pairs = oc.random_workdir(tmp)
        host = api.og_edges(db, las, trim="rtrim")
        model = oc.model_of(las, rl, pairs)
    oc.same_edges(host, model)
    assert model["edges"] > 100 and model["parallel"] > 0 and model["symdiscard"] > 0 and model["cnt_left"] + model["cnt_right"] > model["edges"] + model["redges"]
