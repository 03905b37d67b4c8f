"""LAtrim and the exact box alignment under it on the host path (DAMAR_TRIM=host), against the fixtures the reference's
LAtrim and Compute_Alignment(DIFF_ALIGN) left in tests/golden/trim/ (tests/golden/make_trim_golden.py)."""
import os
import subprocess

import numpy as np
import pytest

import trim_common as tc

HOST = {"DAMAR_TRIM": "host"}
CASES = tc.load_cases()


@pytest.fixture(autouse=True)
def host_path(monkeypatch):
    monkeypatch.setenv("DAMAR_TRIM", "host")


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_tool_case(case, tmp_path):
    tc.run_case(case, str(tmp_path), HOST)


def test_box_cases():
    from damar_amd import api
    bx = tc.boxes()
    a, b = tc.box_seqs(bx)
    diffs, scripts = api.align_boxes(a, b)
    tc.check_boxes(bx, diffs, scripts)
    _, boxes, fallback, values = api.box_last()
    assert (boxes, fallback, values) == (len(a), 0, len(bx["script"]))


WIDE_FAMILIES = ("limit", "worst", "ladder", "skew", "ties", "random")


@pytest.mark.parametrize("family", WIDE_FAMILIES)
def test_wide_box_cases(family):
    """boxes_wide.npz (tests/golden/make_box_edges_golden.py): boxes of every size up to the kernel's 1000 and just beyond"""
    from damar_amd import api
    bx = tc.boxes_wide()
    idx = tc.family_rows(bx, family)
    a, b = tc.box_seqs(bx, idx)
    diffs, scripts = api.align_boxes(a, b)
    tc.check_boxes(bx, diffs, scripts, idx)
    assert api.box_last()[1:3] == (len(idx), 0)


def test_wide_families_hold_what_they_were_planted_for():
    bx = tc.boxes_wide()
    assert sorted(bx["families"]) == sorted(WIDE_FAMILIES)
    big = np.maximum(bx["m"], bx["n"])
    worst = tc.family_rows(bx, "worst")
    assert len(worst) == 5 and np.all(bx["diffs"][worst] == big[worst]) and big[worst].max() == tc.BOX_MAX
    ladder = tc.family_rows(bx, "ladder")
    pure = ladder[bx["planted"][ladder] >= 0]
    assert np.array_equal(bx["diffs"][pure], bx["planted"][pure])
    assert sorted(bx["planted"][pure]) == list(range(61, 68)) + list(range(125, 132)) + list(range(253, 260)) + [300]
    assert len(ladder) == 2 * len(pure) and np.all(bx["soff"][pure + 1] == bx["soff"][pure])        # substitutions leave no entry
    limit = tc.family_rows(bx, "limit")
    assert np.sum(big[limit] == tc.BOX_MAX) == 14 and np.sum(big[limit] > tc.BOX_MAX) == 3
    assert np.sum(big > tc.BOX_MAX) == 3 and np.sum((big >= 256) & (big <= tc.BOX_MAX)) >= 300
    skew = tc.family_rows(bx, "skew")
    assert set(np.abs(bx["m"] - bx["n"])[skew].tolist()) == {70, 130, 200, 450, 700}
    assert set(np.sign(bx["m"] - bx["n"])[skew].tolist()) == {-1, 1}


def test_no_boxes():
    from damar_amd import api
    diffs, scripts = api.align_boxes([], [])
    assert len(diffs) == 0 and scripts == []


@pytest.mark.parametrize("name", ["def_tiny2", "p_tiny2", "synth_p", "def_tandem"])
def test_L_changes_nothing(name, tmp_path):
    case = next(c for c in CASES if c["name"] == name)
    tc.run_case(case, str(tmp_path), HOST, opts=case["opts"] + ["-L"])


def test_uncompressed_track(tmp_path):
    tc.run_case(next(c for c in CASES if c["name"] == "synth"), str(tmp_path), HOST, plain=True)


@pytest.mark.parametrize("err", tc.load_cases("errors"), ids=[e["name"] for e in tc.load_cases("errors")])
def test_error_paths(err, tmp_path):
    case = next(c for c in CASES if c["name"] == "def_tiny2")
    tc.workdir(str(tmp_path), case, tc.expected(case["name"]))
    r = tc.run_tool([], str(tmp_path), HOST, args=err["args"])
    assert (r.returncode, r.stdout, r.stderr) == (err["rc"], err["stdout"], err["stderr"])


@pytest.mark.parametrize("case", [c for c in CASES if "-p" in c["opts"]], ids=[c["name"] for c in CASES if "-p" in c["opts"]])
def test_lacheck_accepts_purged(case, tmp_path):
    tc.run_case(case, str(tmp_path), HOST)
    r = subprocess.run([os.path.join(tc.BIN, "LAcheck"), "-p", "-s", "G", tc.OUT], cwd=str(tmp_path), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_api_trim_las(tmp_path):
    from damar_amd import api
    case = next(c for c in CASES if c["name"] == "p_tiny2")
    exp = tc.expected(case["name"])
    tc.workdir(str(tmp_path), case, exp)
    p = lambda f: os.path.join(str(tmp_path), f)
    st = api.trim_las(p("G"), p(tc.LAS), p(tc.OUT), purge=True)
    assert tc.md5(p(tc.OUT)) == case["md5"]
    assert (st["novl"], st["ntrimmed"], st["written"]) == (1746, 1500, int(exp["novl"])) and st["boxes"] > 0


@pytest.mark.parametrize("small", [False, True], ids=["records", "close"])
def test_refused_write(small, tmp_path):
    """the output on a device that refuses the data: at a record, and (one record, all of it in the stream's buffer) at the close"""
    case = next(c for c in CASES if c["name"] == "def_tiny2")
    tc.workdir(str(tmp_path), case, tc.expected(case["name"]))
    if small:
        tc.keep_first_record(str(tmp_path / tc.LAS))
    r = tc.run_tool([], str(tmp_path), HOST, args=("G", tc.LAS, tc.FULL))
    assert (r.returncode, r.stdout, r.stderr) == (1, "", tc.CANNOT_WRITE)


def test_reads_the_database_does_not_have(tmp_path):
    case = next(c for c in CASES if c["name"] == "def_tiny2")
    tc.workdir(str(tmp_path), case, tc.expected(case["name"]))
    tc.foreign_aread(str(tmp_path / tc.LAS), tc.nreads_of("tiny2"))
    r = tc.run_tool([], str(tmp_path), HOST)
    assert (r.returncode, r.stdout, r.stderr) == (1, "", tc.FOREIGN)
