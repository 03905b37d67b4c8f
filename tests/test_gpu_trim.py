"""LAtrim and the exact box alignment under it on the device (kernels/box_align.hip), against the fixtures the reference's
LAtrim and Compute_Alignment(DIFF_ALIGN) left in tests/golden/trim/."""
import os

import numpy as np
import pytest

import trim_common as tc

pytestmark = pytest.mark.gpu
CASES = [c for c in tc.load_cases() if c["name"] in tc.GPU_CASES]


@pytest.fixture(autouse=True)
def device_path(monkeypatch):
    monkeypatch.delenv("DAMAR_TRIM", raising=False)
    monkeypatch.delenv("DAMAR_TEST_BOX_LIMIT", raising=False)


@pytest.fixture(scope="module")
def bx():
    return tc.boxes()


def test_box_cases(bx):
    from damar_amd import api
    a, b = tc.box_seqs(bx)
    diffs, scripts = api.align_boxes(a, b)
    tc.check_boxes(bx, diffs, scripts)
    ms, boxes, fallback, values = api.box_last()
    assert (boxes, values) == (len(a), len(bx["script"]))
    assert fallback == int(np.sum(np.maximum(bx["m"], bx["n"]) > 1000)) > 0          # only what the kernel's LDS does not hold
    assert ms["kernel"] > 0


def test_lowered_limit_falls_back(bx, monkeypatch):
    from damar_amd import api
    monkeypatch.setenv("DAMAR_TEST_BOX_LIMIT", "40")
    idx = list(range(0, len(bx["m"]), 3))
    a, b = tc.box_seqs(bx, idx)
    diffs, scripts = api.align_boxes(a, b)
    tc.check_boxes(bx, diffs, scripts, idx)
    _, boxes, fallback, _ = api.box_last()
    big = int(np.sum(np.maximum(bx["m"][idx], bx["n"][idx]) > 40))
    assert boxes == len(idx) and fallback == big and 0 < big < len(idx)


def test_batch_sizes(bx):
    from damar_amd import api
    diffs, scripts = api.align_boxes([], [])
    assert len(diffs) == 0 and scripts == []
    one = [int(np.flatnonzero((bx["m"] == 125) & (bx["n"] == 255))[0])]
    a, b = tc.box_seqs(bx, one)
    diffs, scripts = api.align_boxes(a, b)
    tc.check_boxes(bx, diffs, scripts, one)
    grid = api.lib().damar_box_grid()
    idx = (list(range(int(bx["small"]))) * (grid // int(bx["small"]) + 2))[:grid + 777]       # more boxes than workgroups
    a, b = tc.box_seqs(bx, idx)
    diffs, scripts = api.align_boxes(a, b)
    tc.check_boxes(bx, diffs, scripts, idx)
    assert api.box_last()[1:3] == (len(idx), 0)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_tool_case(case, tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("DAMAR_TRIM", "DAMAR_TEST_BOX_LIMIT")}
    exp = tc.expected(case["name"])
    tc.workdir(str(tmp_path), case, exp)
    cmd = ["timeout", "-k", "10", "120", os.path.join(tc.BIN, "LAtrim")] + case["opts"] + ["G", tc.LAS, tc.OUT]
    r = tc.subprocess.run(cmd, cwd=str(tmp_path), env=env, stdout=tc.subprocess.PIPE, stderr=tc.subprocess.PIPE, text=True)
    tc.check_output(case, exp, r, os.path.join(str(tmp_path), tc.OUT))


def test_tiny2_boxes_stay_on_the_device(tmp_path):
    from damar_amd import api
    case = next(c for c in CASES if c["name"] == "def_tiny2")
    exp = tc.expected(case["name"])
    tc.workdir(str(tmp_path), case, exp)
    p = lambda f: os.path.join(str(tmp_path), f)
    st = api.trim_las(p("G"), p(tc.LAS), p(tc.OUT))
    assert tc.md5(p(tc.OUT)) == case["md5"]
    _, boxes, fallback, _ = api.box_last()
    assert boxes == st["boxes"] > 0 and fallback == 0
