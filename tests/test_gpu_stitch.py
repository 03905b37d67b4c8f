"""LAstitch and the exact box alignment into trace pairs under it on the device (kernels/box_trace.hip), against the fixtures
the reference's LAstitch and Compute_Alignment(DIFF_TRACE) left in tests/golden/stitch/."""
import os

import numpy as np
import pytest

import stitch_common as sc

pytestmark = pytest.mark.gpu
CASES = sc.load_cases()
DROP = ("DAMAR_STITCH", "DAMAR_TEST_BOX_LIMIT")


@pytest.fixture(autouse=True)
def device_path(monkeypatch):
    for k in DROP:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def bx():
    return sc.tboxes()


def test_box_runs(bx):
    from damar_amd import api
    runs = np.arange(len(bx["run_box"]))
    a, b, at = sc.run_seqs(bx, runs)
    diffs, traces = api.trace_boxes(a, b, at, sc.TW)
    sc.check_runs(bx, runs, diffs, traces)
    ms, boxes, fallback, values = api.tbox_last()
    assert (boxes, values) == (len(runs), len(bx["trace"]))
    big = np.maximum(bx["m"], bx["n"])[bx["run_box"]]
    assert fallback == int(np.sum(big > 4096)) > 0           # only what the kernel's LDS does not hold
    assert ms["kernel"] > 0


def test_lowered_limit_falls_back(bx, monkeypatch):
    from damar_amd import api
    big = np.maximum(bx["m"], bx["n"])[bx["run_box"]]
    limit = int(np.sort(big)[2 * len(big) // 3])             # a third of the runs lie above it
    monkeypatch.setenv("DAMAR_TEST_BOX_LIMIT", str(limit))
    runs = np.arange(len(big))
    a, b, at = sc.run_seqs(bx, runs)
    diffs, traces = api.trace_boxes(a, b, at, sc.TW)
    sc.check_runs(bx, runs, diffs, traces)
    _, boxes, fallback, _ = api.tbox_last()
    above = int(np.sum(big > limit))
    assert boxes == len(runs) and fallback == above and len(runs) // 4 < above < len(runs) // 2


def test_batch_sizes(bx):
    from damar_amd import api
    diffs, traces = api.trace_boxes([], [], [], sc.TW)
    assert len(diffs) == 0 and traces == []
    fam = list(bx["families"]).index("large_unrelated")
    one = np.flatnonzero(bx["family"][bx["run_box"]] == fam)[:1]
    a, b, at = sc.run_seqs(bx, one)
    diffs, traces = api.trace_boxes(a, b, at, sc.TW)
    sc.check_runs(bx, one, diffs, traces)
    assert api.tbox_last()[1:3] == (1, 0)
    grid = api.lib().damar_tbox_grid()
    small = np.flatnonzero(np.maximum(bx["m"], bx["n"])[bx["run_box"]] <= 130)
    runs = np.tile(small, grid // len(small) + 2)[:grid + 777]         # more boxes than workgroups
    a, b, at = sc.run_seqs(bx, runs)
    diffs, traces = api.trace_boxes(a, b, at, sc.TW)
    sc.check_runs(bx, runs, diffs, traces)
    assert api.tbox_last()[1:3] == (len(runs), 0)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_tool_case_and_host_path_agree(case, tmp_path):
    dev, host = os.path.join(str(tmp_path), "dev"), os.path.join(str(tmp_path), "host")
    os.makedirs(dev)
    os.makedirs(host)
    sc.run_case(case, dev, timeout_s=120, drop=DROP)
    sc.run_case(case, host, {"DAMAR_STITCH": "host"}, drop=DROP)
    assert open(os.path.join(dev, sc.OUT), "rb").read() == open(os.path.join(host, sc.OUT), "rb").read()
    r = sc.lacheck(dev, sort_order=case["input"] != "ssynth")
    assert r.returncode == 0, r.stdout + r.stderr


def test_synth_boxes_stay_on_the_device(tmp_path):
    from damar_amd import api
    case = next(c for c in CASES if c["name"] == "synth_f150")
    sc.workdir(str(tmp_path), case["input"])
    p = lambda f: os.path.join(str(tmp_path), f)
    st = api.stitch_las(p("G"), p(sc.LAS), p(sc.OUT), fuzz=150)
    assert sc.tc.md5(p(sc.OUT)) == case["md5"]
    _, boxes, fallback, _ = api.tbox_last()                   # the last round's
    assert boxes == st["round_boxes"][-1] > 0 and fallback == 0 and st["rounds"] >= 2
