"""LArepeat and TANmask without a GPU (DAMAR_PILES=host): the commands and the plain model against the fixtures the
reference's own tools wrote (tests/golden/make_masks_golden.py), the pile reader against hand-built files, the tracks we
write through the existing track loader, and the new names of the C-ABI."""
import os
import struct
import subprocess

import numpy as np
import pytest

import masks_model
from conftest import GOLDEN, ROOT
from masks_common import (BIN, REP, REP_CASES, TAN, TAN_CASES, case_las, check_repeat_arrays, opts_to_kwargs, rep_workdir, run_larepeat,
                          run_tanmask)

HOST = {"DAMAR_PILES": "host"}


@pytest.fixture(autouse=True)
def host_path(monkeypatch, built):
    monkeypatch.setenv("DAMAR_PILES", "host")


def test_abi_names_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "damar_amd", "libdamar_hip.so")], check=True,
                         stdout=subprocess.PIPE, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    for n in ("damar_pile_coverage", "damar_pile_repeats", "damar_pile_tandem", "damar_pile_release", "damar_pile_last"):
        assert n in exported
    for exe in ("LArepeat", "TANmask"):
        assert os.path.exists(os.path.join(BIN, exe))


@pytest.mark.parametrize("case", REP_CASES, ids=[c["name"] for c in REP_CASES])
def test_larepeat_command_equals_reference(case, tmp_path):
    run_larepeat(case, str(tmp_path), HOST)


@pytest.mark.parametrize("case", TAN_CASES, ids=[c["name"] for c in TAN_CASES])
def test_tanmask_command_equals_reference(case, tmp_path):
    run_tanmask(case, str(tmp_path), HOST)


@pytest.mark.parametrize("case", [c for c in REP_CASES if c["name"] in ("c", "Cm", "m", "I", "o", "hl", "c_f", "I_f")], ids=lambda c: c["name"])
def test_model_equals_reference_repeats(case):
    from damar_amd import api
    rl, rf, _ = api.db_info(os.path.join(REP, "G"))
    (p,) = api.read_piles(os.path.join(REP, case_las(case)))
    exp = np.load(os.path.join(REP, "expected_%s.npz" % case["name"]))
    count, data, merged, rbases = masks_model.repeats(p, rl, **opts_to_kwargs(case["opts"]))
    anno = np.zeros(len(rl) + 1, dtype=np.uint64)
    anno[p["pile_aread"] + 1] = 4 * count.astype(np.uint64)
    check_repeat_arrays(case, np.cumsum(anno).astype(np.uint64), data, exp)
    assert (merged, rbases) == (int(exp["MERGED"]), int(exp["BASES_REPEAT"]))


def test_model_equals_reference_estimate_and_tandem():
    from damar_amd import api
    rl, rf, _ = api.db_info(os.path.join(REP, "G"))
    for name, las in (("est", "G.1.las"), ("est_f", "G.1f.las")):
        (p,) = api.read_piles(os.path.join(REP, las))
        exp = np.load(os.path.join(REP, "expected_%s.npz" % name))
        histo, bases, inactive = masks_model.coverage(p, rl, rf)
        assert np.array_equal(histo, exp["histo"]) and (inactive, bases) == (int(exp["INACTIVE"][0]), int(exp["INACTIVE"][2]))
    for case in TAN_CASES:
        if case["whole"]:
            continue
        (p,) = api.read_piles(os.path.join(GOLDEN, case["las"]))
        e = np.load(os.path.join(TAN, "expected_%s.npz" % case["name"]))
        _count, data = masks_model.tandem(p, 0)
        assert data.astype("<i4").tobytes() == e["data"].tobytes()


def test_python_calls_equal_reference():
    from damar_amd import api
    for case in REP_CASES:
        exp = np.load(os.path.join(REP, "expected_%s.npz" % case["name"]))
        anno, data, stats = api.repeat_track(os.path.join(REP, "G"), os.path.join(REP, case_las(case)), **opts_to_kwargs(case["opts"]))
        check_repeat_arrays(case, anno, data, exp)
        assert stats["merged"] == int(exp["MERGED"]) and stats["bases_repeat"] == int(exp["BASES_REPEAT"])
    for case in TAN_CASES:
        e = np.load(os.path.join(TAN, "expected_%s.npz" % case["name"]))
        offs, data = api.tan_track(os.path.join(GOLDEN, case["db"], "G"), os.path.join(GOLDEN, case["las"]), 0, 0 if case["whole"] else 1)
        assert offs.astype("<i8").tobytes() == e["anno"].tobytes()[8:] and data.astype("<i4").tobytes() == e["data"].tobytes()
    # an honest threshold removes intervals (the command inherits the reference's -l, which does not)
    case = TAN_CASES[0]
    _o, all_ = api.tan_track(os.path.join(GOLDEN, case["db"], "G"), os.path.join(GOLDEN, case["las"]), 0, 1)
    _o, few = api.tan_track(os.path.join(GOLDEN, case["db"], "G"), os.path.join(GOLDEN, case["las"]), 3000, 1)
    assert len(few) < len(all_)


def _las(path, recs, tspace=100):
    """recs: (aread, bread, abpos, aepos, tlen)"""
    tb = 1 if tspace <= 125 else 2
    with open(path, "wb") as f:
        f.write(struct.pack("<qi", len(recs), tspace))
        for a, b, ab, ae, tlen in recs:
            f.write(struct.pack("<iiiiiiIiii", tlen, 0, ab, ab + 1, ae, ae + 1, 0, a, b, 0))
            f.write(b"\x07" * (tb * tlen))


def test_pile_reader(tmp_path, monkeypatch):
    from damar_amd import api
    p = str(tmp_path / "x.las")
    open(p, "wb").close()
    assert api.read_piles(p) == []                                   # an empty file
    _las(p, [])
    assert api.read_piles(p) == []
    for tspace in (100, 500):                                        # 1-byte and 2-byte traces
        _las(p, [(3, 1, 10, 20, 4)], tspace)
        (b,) = api.read_piles(p)
        assert list(b["pile_off"]) == [0, 1] and list(b["pile_aread"]) == [3] and list(b["aepos"]) == [20]
        recs = [(0, 1, 0, 5, 2), (0, 2, 1, 6, 0), (2, 0, 2, 7, 6), (2, 1, 3, 8, 2), (2, 3, 4, 9, 2), (2, 4, 5, 10, 2), (5, 0, 6, 11, 4)]
        _las(p, recs, tspace)
        (b,) = api.read_piles(p)                                     # a pile ends the file
        assert list(b["pile_off"]) == [0, 2, 6, 7] and list(b["pile_aread"]) == [0, 2, 5]
        assert list(b["abpos"]) == [r[2] for r in recs] and list(b["bread"]) == [r[1] for r in recs]
        assert list(b["bbpos"]) == [r[2] + 1 for r in recs] and list(b["bepos"]) == [r[3] + 1 for r in recs]
        monkeypatch.setenv("DAMAR_PILE_BATCH", "3")                  # cuts between piles, never inside one
        bs = api.read_piles(p)
        assert [list(x["pile_aread"]) for x in bs] == [[0], [2], [5]]
        assert [len(x["abpos"]) for x in bs] == [2, 4, 1]
        monkeypatch.setenv("DAMAR_PILE_BATCH", "6")
        assert [list(x["pile_aread"]) for x in api.read_piles(p)] == [[0, 2], [5]]
        monkeypatch.delenv("DAMAR_PILE_BATCH")


def test_tracks_load_through_the_daligner_loader(tmp_path):
    """what we write is what the existing mask loader (damar_load_masks, daligner -m) reads"""
    import ctypes as C
    import shutil
    from damar_amd import api

    class Track(C.Structure):                                        # include/damar_db.h HITS_TRACK
        _fields_ = [("next", C.c_void_p), ("name", C.c_char_p), ("size", C.c_int), ("anno", C.c_void_p), ("data", C.c_void_p)]
    d = str(tmp_path)
    for f in ("G.db", ".G.idx", ".G.bps"):
        shutil.copy(os.path.join(GOLDEN, "tandem", f), os.path.join(d, f))
    shutil.copy(os.path.join(GOLDEN, "tan_tandem/las/tan/G.1.G.1.las"), os.path.join(d, "G.1.G.1.las"))
    env = dict(os.environ, **HOST)
    subprocess.run([os.path.join(BIN, "TANmask"), "G", "G.1.G.1.las"], cwd=d, env=env, check=True)
    subprocess.run([os.path.join(BIN, "LArepeat"), "-c", "1", "-I", "-t", "rp", "G", "G.1.G.1.las"], cwd=d, env=env, check=True,
                   stdout=subprocess.DEVNULL)
    L = api.lib()
    for name, ref in (("tan", api.read_track(os.path.join(d, "G"), "tan", 1)), ("rp", api.read_track(os.path.join(d, "G"), "rp"))):
        blk = api.read_block(os.path.join(d, "G.1"))
        names = (C.c_char_p * 1)(name.encode())
        assert L.damar_load_masks(C.byref(blk), names, 1) == 0
        assert blk.tracks
        trk = C.cast(blk.tracks, C.POINTER(Track)).contents
        got_anno = np.ctypeslib.as_array(C.cast(trk.anno, C.POINTER(C.c_int64)), shape=(blk.nreads + 1,)).copy()
        got_data = np.ctypeslib.as_array(C.cast(trk.data, C.POINTER(C.c_int)), shape=(max(int(got_anno[-1]), 1),))[:int(got_anno[-1])].copy()
        # what was written, for the block's reads, in the loader's form: offsets in ints, intervals that touch fused
        first = 0 if name == "tan" else blk.ufirst
        offs = ref["anno"][first:first + blk.nreads + 1].astype(np.int64) // 4
        want_anno, want_data = [0], []
        for i in range(blk.nreads):
            mine = []
            for a in range(int(offs[i]), int(offs[i + 1]) - 1, 2):
                b, e = int(ref["data"][a]), int(ref["data"][a + 1])
                if mine and b <= mine[-1]:
                    mine[-1] = max(mine[-1], e)
                else:
                    mine += [b, e]
            want_data += mine
            want_anno.append(len(want_data))
        assert len(want_data) >= 40                                   # the comparison has something to compare
        assert np.array_equal(got_anno, want_anno) and np.array_equal(got_data, want_data), name
        L.damar_close_block(C.byref(blk))


def test_usage_errors_and_exit_codes(tmp_path):
    d = rep_workdir(str(tmp_path))
    run = lambda exe, *a: subprocess.run([os.path.join(BIN, exe)] + list(a), cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    r = run("LArepeat")
    assert r.returncode == 1 and r.stdout.startswith("usage:")
    r = run("LArepeat", "-x", "G", "G.1.las")
    assert r.returncode == 1 and r.stdout.startswith("usage:")
    r = run("LArepeat", "-h", "1", "-l", "2", "G", "G.1.las")
    assert r.returncode == 1 and r.stderr == "invalid arguments: low 2.00 > high 1.00\n"
    r = run("LArepeat", "-n", "10", "G", "G.1.las")
    assert r.returncode == 1 and "should be larger than 1000" in r.stderr
    r = run("LArepeat", "G", "none.las")
    assert r.returncode == 1 and r.stderr == "could not open 'none.las'\n"
    r = run("LArepeat", "-M", "50", "G", "G.1.las")
    assert r.returncode == 1 and "maximum coverage cannot be smallert than '100'" in r.stderr
    r = run("LArepeat", "-E", "G", "G.1.las")
    assert r.returncode == 0 and "MAX " in r.stdout and "REGIONS" not in r.stdout
    r = run("TANmask", "G")
    assert r.returncode == 1 and "at least one subject block and one LAS file are required" in r.stderr
    r = run("TANmask", "-q", "G", "G.1.las")
    assert r.returncode == 1 and r.stderr.startswith("Unsupported option: -q")
    r = run("TANmask", "G.1", "G.1.las")
    assert r.returncode == 1 and "Cannot be called on a block" in r.stderr


def test_truncated_las_is_an_error(tmp_path):
    """a file that stops before the records its header counts, on a record boundary, inside a record or inside a trace, is
    damaged: no short track is written"""
    from damar_amd import api
    p = str(tmp_path / "G.1.las")
    recs = [(0, 1, 0, 5, 2), (0, 2, 1, 6, 0), (2, 0, 2, 7, 6), (2, 1, 3, 8, 2)]
    _las(p, recs)
    whole = open(p, "rb").read()
    assert len(api.read_piles(p)) == 1
    for cut in (12 + 42 + 40, 12 + 42 + 40 + 46 + 17, len(whole) - 1, 12):           # after record 2, inside record 4, in the last trace, no record
        open(p, "wb").write(whole[:cut])
        with pytest.raises(RuntimeError):
            api.read_piles(p)
    d = rep_workdir(str(tmp_path))
    whole = open(os.path.join(d, "G.1.las"), "rb").read()
    open(os.path.join(d, "G.1.las"), "wb").write(whole[:12 + 40 * 5000])
    for opts in (["-c", "8"], []):                                   # the repeat pass and the estimate pass
        r = subprocess.run([os.path.join(BIN, "LArepeat")] + opts + ["G", "G.1.las"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode != 0 and "ends before" in r.stderr
        assert not os.path.exists(os.path.join(d, ".G.repeats.a2"))


def test_calls_refuse_what_they_cannot_compute():
    """enter below leave: the device's last-set scan and the reference's walk are the same thing only for enter >= leave, so
    the call refuses it on either path, as the command does; a block the database does not have"""
    from damar_amd import api
    rl, rf = np.full(4, 1000, dtype=np.int32), np.full(4, 0x0800, dtype=np.int32)
    p = dict(pile_off=np.array([0, 2], dtype=np.int64), pile_aread=np.array([1], dtype=np.int32), abpos=np.array([0, 10], dtype=np.int32),
             aepos=np.array([500, 600], dtype=np.int32), bbpos=np.zeros(2, dtype=np.int32), bepos=np.ones(2, dtype=np.int32),
             bread=np.array([2, 3], dtype=np.int32), flags=np.zeros(2, dtype=np.int32))
    count, data, _m, _b = api.pile_repeats(p, rl, rf, api.repeat_params(cov=1, xcov_enter=1.0, xcov_leave=1.0))
    assert list(data) == [10, 599]                                   # depth 2 at 10; below 1 only after the second end
    with pytest.raises(RuntimeError):
        api.pile_repeats(p, rl, rf, api.repeat_params(cov=1, xcov_enter=1.0, xcov_leave=2.0))
    case = TAN_CASES[0]
    with pytest.raises(ValueError):
        api.tan_track(os.path.join(GOLDEN, case["db"], "G"), os.path.join(GOLDEN, case["las"]), 0, 99)


@pytest.mark.parametrize("opts", [["-c", "8"], []], ids=["repeat_pass", "estimate_pass"])
def test_reads_the_database_does_not_have(opts, tmp_path):
    import q_common
    import trim_common
    tmp = q_common.workdir(str(tmp_path), "tiny2")
    trim_common.foreign_aread(os.path.join(tmp, q_common.LAS), trim_common.nreads_of("tiny2"))
    r = q_common.run_tool(os.path.join(BIN, "LArepeat"), opts, tmp, env=dict(os.environ, DAMAR_PILES="host"))
    assert (r.returncode, r.stderr) == (1, trim_common.FOREIGN)
