"""The box kernels (kernels/box_align.hip, kernels/box_trace.hip, the search of kernels/box_search.h under both) at every size
they admit, against what the reference's Compute_Alignment left in tests/golden/trim/boxes_wide.npz and
tests/golden/stitch/tboxes_wide.npz (tests/golden/make_box_edges_golden.py).  Every comparison is exact, and after every
call the host routine has done exactly the boxes that lie beyond the kernel's limits: a box inside them that comes back
from the kernel with length -1 is a failure here."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import stitch_common as sc                             # noqa: E402
import trim_common as tc                               # noqa: E402

pytestmark = pytest.mark.gpu
DROP = ("DAMAR_TRIM", "DAMAR_STITCH", "DAMAR_TEST_BOX_LIMIT")
# the kernel time allowed to the eight worst-case runs.  A frontier step of d differences is (2d + 1) / 64 chunks, so the
# search of an all-differences box of 4096 is some 2 * 2048^2 / 64 = 131 000 chunk steps of one wavefront and the halves
# under it as many again: at a microsecond a chunk step a quarter of a second, and the four large runs go side by side.
WORST_MS = 3000.


@pytest.fixture(autouse=True)
def device_path(monkeypatch):
    for k in DROP:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def bx():
    return tc.boxes_wide()


@pytest.fixture(scope="module")
def tbx():
    return sc.tboxes_wide()


# ---- box_align: every box up to 1000 ---------------------------------------------------------------------------------

@pytest.mark.parametrize("family", ["limit", "worst", "ladder", "skew", "ties", "random"])
def test_align_family(bx, family):
    from damar_amd import api
    idx = tc.family_rows(bx, family)
    a, b = tc.box_seqs(bx, idx)
    diffs, scripts = api.align_boxes(a, b)
    tc.check_boxes(bx, diffs, scripts, idx)
    ms, boxes, fallback, values = api.box_last()
    beyond = int(np.sum(np.maximum(bx["m"], bx["n"])[idx] > tc.BOX_MAX))
    assert (boxes, values) == (len(idx), int(np.sum(bx["soff"][idx + 1] - bx["soff"][idx])))
    assert fallback == beyond == (3 if family == "limit" else 0)         # the kernel holds every box up to its limit
    assert ms["kernel"] > 0


# ---- box_trace: both builds, other spacings, the ledger's bound ------------------------------------------------------

@pytest.mark.parametrize("family", ["build_border", "middle", "spacing", "ledger"])
def test_trace_family(tbx, family):
    kernel_ms, fallback, beyond = sc.trace_runs(tbx, sc.family_runs(tbx, family))
    assert fallback == beyond == (2 if family == "ledger" else 0)        # 514 cells: the host routine's, and counted
    assert kernel_ms > 0


def test_trace_worst_case_of_both_builds(tbx):
    """all of one base against all of another: max(M, N) differences, the last frontier step of box_trace<1032> at 1024
    and of box_trace<4104> at 4096; a large one keeps a wavefront busy for the whole search"""
    env = {k: v for k, v in os.environ.items() if k not in DROP}
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__)], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:]
    runs, kernel_ms, fallback, beyond = r.stdout.split()[-4:]
    assert (int(runs), int(fallback), int(beyond)) == (len(sc.family_runs(tbx, "worst")), 0, 0)
    assert 0 < float(kernel_ms) < WORST_MS


def border_runs(tbx):
    runs = sc.family_runs(tbx, "build_border")
    big = np.maximum(tbx["m"], tbx["n"])[tbx["run_box"][runs]]
    return runs[big <= sc.TB_SMALL], runs[big > sc.TB_SMALL]


def test_trace_build_border_in_one_call(tbx):
    small, large = border_runs(tbx)
    assert len(small) == len(large) > 0
    mixed = np.stack([large, small], axis=1).reshape(-1)                 # large and small boxes alternate
    _, fallback, beyond = sc.trace_runs(tbx, mixed)
    assert fallback == beyond == 0


def test_trace_large_boxes_alone(tbx):
    _, large = border_runs(tbx)                                          # nothing for the first launch to do
    _, fallback, beyond = sc.trace_runs(tbx, large)
    assert fallback == beyond == 0


@pytest.mark.parametrize("which", ["mixed", "large"])
def test_trace_limit_on_the_build_border(tbx, which, monkeypatch):
    """with the limit on the border the second launch does not run: its boxes are the host routine's, the others are not"""
    monkeypatch.setenv("DAMAR_TEST_BOX_LIMIT", str(sc.TB_SMALL))
    small, large = border_runs(tbx)
    runs = np.stack([large, small], axis=1).reshape(-1) if which == "mixed" else large
    kernel_ms, fallback, beyond = sc.trace_runs(tbx, runs, limit=sc.TB_SMALL)
    assert fallback == beyond == len(large) and kernel_ms > 0


if __name__ == "__main__":                                 # the child of the worst-case test: runs, kernel ms, hand-offs
    wide = sc.tboxes_wide()
    worst = sc.family_runs(wide, "worst")
    kernel_ms, fallback, beyond = sc.trace_runs(wide, worst)
    print("%d %.3f %d %d" % (len(worst), kernel_ms, fallback, beyond))
