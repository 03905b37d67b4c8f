"""The whole-read alignment on the GPU (kernels/read_align.hip, the search of kernels/read_search.h under it) against what
the reference's Compute_Alignment(DIFF_ALIGN) left in tests/golden/correct/read_boxes.npz
(tests/golden/make_read_align_golden.py), and LAcorrect with its postrace on the device.  Every comparison is exact, and
after every call the host routine has done exactly the boxes beyond the kernel's bounds: a box inside them that comes back
with length -1 counts as handed over and fails the test."""
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import correct_common as cc                            # noqa: E402
import read_align_common as rc                         # noqa: E402

pytestmark = pytest.mark.gpu
DROP = ("DAMAR_PILES", "DAMAR_POSTRACE", "DAMAR_TEST_READ_DIFFS", "DAMAR_TEST_READ_GRID")
FAMILIES = ("border", "ladder", "skew", "ties", "worst", "cap", "many")
# the kernel time allowed to the `worst` and `cap` calls together.  A frontier step of d differences is ceil((2d + 1) / 512)
# chunk steps of the workgroup.  The box of 9000 differences is searched until either side has passed 4000 and is then
# given up: 2 * sum(ceil((2d + 1) / 512), d = 1 .. 4000) = 2 * (4000 * 4001 / 512 + 2000) = 66 500 chunk steps.  The box of
# 1500 differences takes 2 * (750^2 / 512 + 750) = 3 700 for its top search and, differences halving over 11 levels of one
# chunk a step, 11 * 1500 = 16 500 under it; an unrelated pair of 2000 (some 1060 differences) less than that.  The boxes
# of a call run side by side, so the two calls are some 66 500 + 20 200 = 86 700 chunk steps deep: at a microsecond a chunk
# step under a tenth of a second, and twelve times that is allowed, the factor test_gpu_box_edges.py allows its WORST_MS.
WORST_MS = 1200.


@pytest.fixture(autouse=True)
def device_path(monkeypatch):
    for k in DROP:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def bx():
    return rc.boxes()


@pytest.mark.parametrize("family", FAMILIES)
def test_family_equals_reference(bx, family):
    last, beyond = rc.run_family(bx, rc.family_rows(bx, family))
    print(family, last)
    assert last[2] == beyond == (1 if family == "cap" else 0)            # the kernel holds every box inside its bounds
    assert last[0]["kernel"] > 0


def test_lowered_bound_hands_over_what_lies_beyond_it(bx, monkeypatch):
    monkeypatch.setenv("DAMAR_TEST_READ_DIFFS", "400")
    cap = rc.family_rows(bx, "cap")
    assert [int(bx["diffs"][i]) for i in cap] == [400, 402, 9000]
    last, beyond = rc.run_family(bx, cap, limit=400)
    assert last[2] == beyond == 2
    for row, handed in zip(cap, (0, 1, 1)):                              # which ones: not the box of exactly 400
        last, beyond = rc.run_family(bx, [row], limit=400)
        assert last[2] == beyond == handed
    last, beyond = rc.run_family(bx, rc.family_rows(bx, "ladder"), limit=400)
    assert last[2] == beyond == 3                                        # 511, 512, 513


def test_long_and_short_boxes_alternate_in_one_call(bx):
    long_, short = rc.family_rows(bx, "border"), rc.family_rows(bx, "many")[:len(rc.family_rows(bx, "border"))]
    mixed = np.stack([short, long_], axis=1).reshape(-1)
    last, beyond = rc.run_family(bx, mixed)
    assert last[2] == beyond == 0


def test_single_box(bx):
    last, beyond = rc.run_family(bx, rc.family_rows(bx, "skew")[:1])
    assert last[1:3] == (1, 0) and beyond == 0


def test_workgroups_take_several_boxes(bx, monkeypatch):
    """no fixture call holds more boxes than damar_read_grid(); with the grid lowered to 7 the forty boxes of `many` and
    the ladder are some six to a workgroup"""
    from damar_amd import api
    assert api.lib().damar_read_grid() >= len(bx["m"])
    monkeypatch.setenv("DAMAR_TEST_READ_GRID", "7")
    rows = np.concatenate([rc.family_rows(bx, "many"), rc.family_rows(bx, "ladder")])
    last, beyond = rc.run_family(bx, rows)
    assert last[2] == beyond == 0


def test_worst_cases_stay_inside_their_time(bx):
    ms = 0.
    for family in ("worst", "cap"):
        last, _ = rc.run_family(bx, rc.family_rows(bx, family))
        print(family, last)
        ms += last[0]["kernel"]
    assert 0 < ms < WORST_MS


@pytest.mark.parametrize("case", [c for c in cc.load_cases() if c["name"].split("_")[0] in ("plain", "rj")], ids=lambda c: c["name"])
def test_pass_with_postrace_on_the_device(case, tmp_path):
    from damar_amd import api
    tmp = cc.workdir(str(tmp_path), case["input"])
    opts = case["opts"]
    st = api.correct_las(os.path.join(tmp, "G"), os.path.join(tmp, cc.LAS), os.path.join(tmp, cc.OUT),
                         parts=int(opts[opts.index("-j") + 1]) if "-j" in opts else 1,
                         read_ids=os.path.join(tmp, "ids.txt") if "-r" in opts else None)
    # the files against the fixture; what the pass printed is the command's to check (tests/test_gpu_correct.py)
    cc.check_output(case, types.SimpleNamespace(returncode=case["rc"], stdout=case["stdout"], stderr=case["stderr"]), tmp)
    heads = [ln for f in cc.out_files(tmp) for ln in open(os.path.join(tmp, f)) if ln[0] == ">" and not ln.startswith(">copy.")]
    traced = sum(" postrace=" in h for h in heads)
    print(case["name"], st, traced)
    assert st["postrace_host"] == 0
    assert traced <= st["postrace_boxes"] == st["reads"] == len(heads) > 0        # a read equal to its correction has no postrace
    assert st["ms_postrace_kernel"] > 0 and st["ms_postrace_call"] >= st["ms_postrace_kernel"] and st["ms_postrace"] == 0
