"""LAstitch and the exact box alignment into trace pairs under it on the host path (DAMAR_STITCH=host), against the fixtures
the reference's LAstitch and Compute_Alignment(DIFF_TRACE) left in tests/golden/stitch/ (tests/golden/make_stitch_golden.py)."""
import os

import numpy as np
import pytest

import stitch_common as sc

HOST = {"DAMAR_STITCH": "host"}
CASES = sc.load_cases()


@pytest.fixture(autouse=True)
def host_path(monkeypatch):
    monkeypatch.setenv("DAMAR_STITCH", "host")


def test_box_runs():
    from damar_amd import api
    bx = sc.tboxes()
    runs = np.arange(len(bx["run_box"]))
    a, b, at = sc.run_seqs(bx, runs)
    diffs, traces = api.trace_boxes(a, b, at, sc.TW)
    sc.check_runs(bx, runs, diffs, traces)
    _, boxes, fallback, values = api.tbox_last()
    assert (boxes, fallback, values) == (len(runs), 0, len(bx["trace"]))


WIDE_FAMILIES = ("build_border", "middle", "worst", "spacing", "ledger")


@pytest.mark.parametrize("family", WIDE_FAMILIES)
def test_wide_box_runs(family):
    """tboxes_wide.npz (tests/golden/make_box_edges_golden.py): the border between the kernel's two builds, the sizes
    between the old fixtures, the most differences a box can hold, other spacings than 100 and the ledger's bound"""
    bx = sc.tboxes_wide()
    _, fallback, _ = sc.trace_runs(bx, sc.family_runs(bx, family))
    assert fallback == 0


def test_wide_families_hold_what_they_were_planted_for():
    bx = sc.tboxes_wide()
    assert sorted(bx["families"]) == sorted(WIDE_FAMILIES)
    runs = np.arange(len(bx["run_box"]))
    m, n = bx["m"][bx["run_box"]], bx["n"][bx["run_box"]]
    big, ts, cells = np.maximum(m, n), sc.run_spacing(bx, runs), sc.run_cells(bx, runs)
    assert big.max() == sc.TBOX_MAX
    worst = sc.family_runs(bx, "worst")
    assert len(worst) == 8 and np.all(bx["diffs"][worst] == big[worst]) and set(bx["run_abpos"][worst] % sc.TW) == {0, 99}
    assert set(big[worst].tolist()) == {sc.TB_SMALL, sc.TBOX_MAX} and set((m - n)[worst].tolist()) > {0}
    border = sc.family_runs(bx, "build_border")
    for side in (m, n):                                      # either side the larger one, related and unrelated
        for size in (1023, 1024, 1025, 1026):
            at_size = border[(side[border] == size) & (big[border] == size)]
            assert np.any(bx["diffs"][at_size] < size // 3) and np.any(bx["diffs"][at_size] > size // 3)
    middle = sc.family_runs(bx, "middle")
    assert np.all((m[middle] > 700) & (m[middle] <= 2000)) and np.any(big[middle] <= sc.TB_SMALL) and np.any(big[middle] > sc.TB_SMALL)
    assert np.all(ts[np.concatenate([worst, border, middle])] == sc.TW)
    spacing = sc.family_runs(bx, "spacing")
    assert set(ts[spacing].tolist()) == {16, 64, 126, 255, 1000}
    for t in (16, 64, 126, 255, 1000):
        assert set((bx["run_abpos"] % ts)[spacing[ts[spacing] == t]].tolist()) == {0, 1, t - 1, 7}
    ledger = sc.family_runs(bx, "ledger")
    assert sorted(cells[ledger].tolist()) == [sc.TB_CELLS, sc.TB_CELLS + 2, sc.TB_CELLS + 2] and np.all(ts[ledger] == 16)
    assert np.all(cells[np.setdiff1d(runs, ledger)] <= sc.TB_CELLS)


def test_start_modulo_spacing_is_enough():
    from damar_amd import api
    bx = sc.tboxes()
    runs = np.arange(0, len(bx["run_box"]), 7)
    a, b, at = sc.run_seqs(bx, runs)
    diffs, traces = api.trace_boxes(a, b, at % sc.TW, sc.TW)
    sc.check_runs(bx, runs, diffs, traces)


def test_no_boxes():
    from damar_amd import api
    diffs, traces = api.trace_boxes([], [], [], sc.TW)
    assert len(diffs) == 0 and traces == []


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_tool_case(case, tmp_path):
    sc.run_case(case, str(tmp_path), HOST)
    r = sc.lacheck(str(tmp_path), sort_order=case["input"] != "ssynth")
    assert r.returncode == 0, r.stdout + r.stderr


PLANTED = [c for c in CASES if c["name"] in sc.PLANT_KEY]


@pytest.mark.parametrize("case", PLANTED, ids=[c["name"] for c in PLANTED])
def test_planted_records(case, tmp_path):
    """synth.las: every planted group ends up as its plant says, by the branch it is planted for"""
    from damar_amd import api
    sc.workdir(str(tmp_path), case["input"])
    p = lambda f: os.path.join(str(tmp_path), f)
    st = api.stitch_las(p("G"), p(sc.LAS), p(sc.OUT), **sc.opts_to_kwargs(case["opts"]))
    assert sc.tc.md5(p(sc.OUT)) == case["md5"]
    cols, _, _, _ = sc.tc.read_records(p(sc.OUT))
    plants = sc.check_plants(case, cols, st)
    if sc.PLANT_KEY[case["name"]] == "def":
        rows = np.flatnonzero((cols[:, 7] == plants["chain3"]["aread"]) & (cols[:, 8] == plants["chain3"]["bread"]))
        assert tuple(cols[rows[0], [4, 5]]) == tuple(cols[rows[2], [4, 5]])      # the head took the last piece's end
        comp = [pl["expect"]["def"] for tag, pl in plants.items() if tag.startswith("comp")]
        assert 0 in comp and 1 in comp                                           # complement joints: refused ones and stitched ones


def test_every_planted_branch_is_taken_somewhere():
    plants = sc.load_cases("plants")
    taken = lambda what: set(k for pl in plants.values() for k in pl.get(what, []))
    assert taken("refused") and taken("widened") and taken("no_box") >= {"wide", "far"}
    assert len([t for t, pl in plants.items() if pl["refused"]]) >= 5
    assert "td" in plants["lc_250"]["refused"]                                   # a value above 250


@pytest.mark.parametrize("err", sc.load_cases("errors"), ids=[e["name"] for e in sc.load_cases("errors")])
def test_error_paths(err, tmp_path):
    sc.workdir(str(tmp_path), "tiny2")
    r = sc.run_tool([], str(tmp_path), HOST, args=err["args"])
    assert (r.returncode, r.stdout, r.stderr) == (err["rc"], err["stdout"], err["stderr"])


def test_api_stitch_las(tmp_path):
    from damar_amd import api
    case = next(c for c in CASES if c["name"] == "synth_f150")
    sc.workdir(str(tmp_path), case["input"])
    p = lambda f: os.path.join(str(tmp_path), f)
    st = api.stitch_las(p("G"), p(sc.LAS), p(sc.OUT), fuzz=150)
    assert sc.tc.md5(p(sc.OUT)) == case["md5"]
    exp = sc.expected(case["name"])
    assert (st["novl"], st["written"], st["stitched"]) == (int(exp["novl"]), int(exp["novl"]), int(np.sum((exp["cols"][:, 6] & 0x80) != 0)))
    assert st["boxes"] == st["stitched"] + st["refused"] == sum(st["round_boxes"])
    assert st["rounds"] >= 2 and st["round_boxes"][0] > st["round_boxes"][1] > 0     # the chain's second joint waits for the first
    case = next(c for c in CASES if c["name"] == "synth_t")
    st = api.stitch_las(p("G"), p(sc.LAS), p(sc.OUT), track=sc.LC_TRACK)
    assert sc.tc.md5(p(sc.OUT)) == case["md5"] and st["stitched_lc"] == 1


@pytest.mark.parametrize("small", [False, True], ids=["records", "close"])
def test_refused_write(small, tmp_path):
    """the output on a device that refuses the data: at a record, and (one record, all of it in the stream's buffer) at the close"""
    sc.workdir(str(tmp_path), "tiny2")
    if small:
        sc.tc.keep_first_record(str(tmp_path / sc.LAS))
    r = sc.run_tool([], str(tmp_path), HOST, args=("G", sc.LAS, sc.tc.FULL))
    assert (r.returncode, r.stdout, r.stderr) == (1, "", sc.tc.CANNOT_WRITE)


def test_reads_the_database_does_not_have(tmp_path):
    sc.workdir(str(tmp_path), "tiny2")
    sc.tc.foreign_aread(str(tmp_path / sc.LAS), sc.tc.nreads_of("tiny2"))
    r = sc.run_tool([], str(tmp_path), HOST)
    assert (r.returncode, r.stdout, r.stderr) == (1, "", sc.tc.FOREIGN)


def test_uncompressed_track(tmp_path):
    """-t from .anno / .data, what the loader falls back to"""
    case = next(c for c in CASES if c["name"] == "synth_t")
    sc.workdir(str(tmp_path), case["input"])
    for ext in (".a2", ".d2"):
        os.remove(str(tmp_path / (".G." + sc.LC_TRACK + ext)))
    anno, data = sc.lc_track()
    sc.tc.write_track_anno(str(tmp_path / (".G." + sc.LC_TRACK)), len(anno) - 1, anno, data)
    r = sc.run_tool(case["opts"], str(tmp_path), HOST)
    sc.check_output(case, r, str(tmp_path / sc.OUT))
