"""LAgap on the plain host path (DAMAR_PILES=host DAMAR_TRIM=host: host/gap.c, host/trim.c) against the fixtures the
reference's LAgap left in tests/golden/gap/: output file, stdout, stderr and exit status of every case."""
import os

import pytest

import gap_common as gc

CASES = gc.load_cases()
HOST = {"DAMAR_PILES": "host", "DAMAR_TRIM": "host"}
SMALL = dict(HOST, DAMAR_PILE_BATCH="40")             # the planted file's 202 records in several batches


@pytest.fixture(autouse=True)
def host_path(monkeypatch):
    for k, v in HOST.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_tool_case(case, tmp_path):
    tmp = str(tmp_path)
    gc.run_case(case, tmp, HOST)
    r = gc.lacheck(tmp)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_small_batches_give_the_same(case, tmp_path):
    gc.run_case(case, str(tmp_path), SMALL)


def test_error_runs(tmp_path):
    tmp = gc.workdir(str(tmp_path), "tiny2")
    for e in gc.load_cases("errors"):
        r = gc.run_tool([], tmp, HOST, args=e["args"])
        assert (r.returncode, r.stdout, r.stderr) == (e["rc"], e["stdout"], e["stderr"]), e["name"]
    r = gc.run_tool(["-C", "x"], tmp, HOST)
    assert (r.returncode, r.stdout, r.stderr) == gc.NO_CHIMER
    assert not os.path.exists(os.path.join(tmp, "x"))


@pytest.mark.parametrize("name", ["es_synth", "tps_synth", "t_tiny2"])
def test_api_agrees_with_the_command(name, tmp_path, capfd):
    from damar_amd import api
    case = next(c for c in CASES if c["name"] == name)
    tmp = gc.workdir(str(tmp_path), case["input"])
    p = lambda f: os.path.join(tmp, f)
    st = api.gap_las(p("G"), p(gc.LAS), p(gc.OUT), **gc.opts_to_kwargs(case["opts"]))
    assert gc.tc.md5(p(gc.OUT)) == case["md5"]
    exp = gc.expected(name)
    assert st["written"] == int(exp["novl"]) and st["host_piles"] == 0
    tail = case["stdout"].splitlines()[-2:]
    assert tail == ["dropped %d containments" % st["contained"], "dropped %d overlaps in %d break/gaps" % (st["dropped"], st["breaks"])]
    assert capfd.readouterr().out == case["stdout"]
