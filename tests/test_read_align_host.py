"""damar_align_reads and LAcorrect's postrace without a GPU: with DAMAR_POSTRACE=host the host routine does every box of
tests/golden/correct/read_boxes.npz (made by the reference, tests/golden/make_read_align_golden.py) and the results are the
fixture's; the command with DAMAR_PILES=host DAMAR_POSTRACE=host gives the reference's files."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import correct_common as cc                            # noqa: E402
import read_align_common as rc                         # noqa: E402

FAMILIES = ("border", "ladder", "skew", "ties", "worst", "cap", "many")


@pytest.fixture(autouse=True)
def host_path(monkeypatch):
    monkeypatch.setenv("DAMAR_POSTRACE", "host")
    monkeypatch.delenv("DAMAR_TEST_READ_DIFFS", raising=False)


def test_fixture_holds_the_families():
    bx = rc.boxes()
    assert tuple(bx["families"]) == FAMILIES
    assert int(bx["boff"][-1] + bx["n"][-1]) == len(bx["bases"]) and len(bx["soff"]) == len(bx["m"]) + 1
    assert int((bx["diffs"] > rc.MAXDIFF).sum()) == 1


@pytest.mark.parametrize("family", FAMILIES)
def test_host_routine_equals_reference(family):
    bx = rc.boxes()
    last, _ = rc.run_family(bx, rc.family_rows(bx, family))
    assert last[2] == 0 and last[0]["kernel"] == 0                       # no box counts as handed over: nothing ran on a GPU


def test_malformed_batches_are_refused():
    from damar_amd import api
    with pytest.raises(ValueError):
        api.align_reads([[0, 1]], [[]])
    diffs, scripts = api.align_reads([], [])
    assert len(diffs) == 0 and scripts == [] and api.read_last()[1:] == (0, 0, 0)


def test_command_on_the_host(tmp_path):
    case = next(c for c in cc.load_cases() if c["name"] == "rj_tiny2")
    cc.run_case(case, str(tmp_path), dict(DAMAR_PILES="host", DAMAR_POSTRACE="host"), timeout_s=120)


def test_pass_on_the_host_counts_no_device_box(tmp_path, monkeypatch):
    from damar_amd import api
    monkeypatch.setenv("DAMAR_PILES", "host")
    case = next(c for c in cc.load_cases() if c["name"] == "r_tiny2")
    tmp = cc.workdir(str(tmp_path), case["input"])
    st = api.correct_las(os.path.join(tmp, "G"), os.path.join(tmp, cc.LAS), os.path.join(tmp, cc.OUT), read_ids=os.path.join(tmp, "ids.txt"))
    assert {f: cc.fc.md5(os.path.join(tmp, f)) for f in cc.out_files(tmp)} == case["md5"]
    assert (st["postrace_boxes"], st["postrace_host"], st["ms_postrace_kernel"], st["ms_postrace_call"]) == (0, 0, 0, 0)
    assert st["reads"] > 0 and st["ms_postrace"] > 0
