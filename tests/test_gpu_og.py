"""OGbuild with its edges made on the GPU (kernels/graph_edges.hip) against the reference's runs kept in tests/golden/og/,
whole and in batches of 40 records, and against the host routine field for field."""
import os
import tempfile

import pytest

import og_common as oc
import q_common

pytestmark = pytest.mark.gpu
CASES = oc.load_cases()


def dev_env(case, **more):
    """the planted file runs with the limit its degrees are sized by; the real files with the limit the library was built with,
    so that the kernel's own dedupe is what is held against the reference"""
    env = {"DAMAR_TEST_GRAPH_MAXDEG": str(oc.MAXDEG_TEST)} if case["input"] == "synth" else {}
    return dict(env, **more)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_device_equals_reference(built, case):
    with tempfile.TemporaryDirectory() as tmp:
        oc.run_case(case, tmp, dev_env(case), timeout_s=120)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_device_in_batches(built, case):
    with tempfile.TemporaryDirectory() as tmp:
        oc.run_case(case, tmp, dev_env(case, DAMAR_PILE_BATCH="40"), timeout_s=120)


def both(api, monkeypatch, db, las):
    monkeypatch.delenv("DAMAR_PILES", raising=False)
    dev = api.og_edges(db, las)
    last = api.og_last()
    monkeypatch.setenv("DAMAR_PILES", "host")
    host = api.og_edges(db, las)
    monkeypatch.delenv("DAMAR_PILES")
    return dev, host, last


@pytest.mark.parametrize("batch", [None, "40"])
def test_edges_equal_host_on_planted_file(built, monkeypatch, batch):
    """field for field; the host routine finishes exactly the read planted over the limit"""
    from damar_amd import api
    monkeypatch.setenv("DAMAR_TEST_GRAPH_MAXDEG", str(oc.MAXDEG_TEST))
    if batch:
        monkeypatch.setenv("DAMAR_PILE_BATCH", batch)
    with tempfile.TemporaryDirectory() as tmp:
        oc.workdir(tmp, "synth")
        dev, host, last = both(api, monkeypatch, os.path.join(tmp, "G"), os.path.join(tmp, oc.LAS))
    oc.same_edges(dev, host)
    over = oc.load_cases("plants")["degree"]["over"]
    assert host["loff"][over + 1] - host["loff"][over] == oc.MAXDEG_TEST + 1
    assert last[3] == 1                        # reads the host routine finished: the one planted over the limit
    assert last[4] == len(dev["left"]) + len(dev["right"])


def test_edges_equal_host_and_model_on_random_piles(built, monkeypatch):
    """at the limit the library was built with: the kernel's dedupe and its count, against the host routine and the model"""
    from damar_amd import api
    with tempfile.TemporaryDirectory() as tmp:
        db, las, rl, pairs = oc.random_workdir(tmp)
        monkeypatch.delenv("DAMAR_PILES", raising=False)
        dev = api.og_edges(db, las, trim="rtrim")
        last = api.og_last()
        monkeypatch.setenv("DAMAR_PILES", "host")
        host = api.og_edges(db, las, trim="rtrim")
        model = oc.model_of(las, rl, pairs)
    oc.same_edges(dev, host)
    oc.same_edges(dev, model)
    assert last[3] == 0 and host["edges"] > 100 and host["parallel"] > 0


@pytest.mark.parametrize("inp", oc.REAL)
def test_edges_equal_model_on_real_files(built, monkeypatch, inp):
    from damar_amd import api
    monkeypatch.delenv("DAMAR_PILES", raising=False)
    rl = q_common.db_read_len(oc.DB_OF[inp])
    ta, td, _, _ = oc.tracks(inp)
    with tempfile.TemporaryDirectory() as tmp:
        oc.workdir(tmp, inp)
        dev = api.og_edges(os.path.join(tmp, "G"), os.path.join(tmp, oc.LAS))
        last = api.og_last()
        model = oc.model_of(os.path.join(tmp, oc.LAS), rl, oc.trim_pairs(ta, td))
    oc.same_edges(dev, model)
    assert last[3] == 0
