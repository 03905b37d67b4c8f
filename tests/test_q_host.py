"""LAq on the host path (DAMAR_PILES=host; host/quality.c, the traces-on reader of host/piles.c): every fixture of
tests/golden/q/ through bin/LAq and the Python calls, the command's error paths, batching, a damaged file, the integer
form of the reference's float rounding, and the plain model of tests/q_model.py against the fixtures."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import q_common
import q_model
from q_common import BIN, GOLDEN, INPUTS, LAS

CASES = q_common.load_cases()
IDS = [c["name"] for c in CASES]


@pytest.fixture(autouse=True)
def host_path(monkeypatch, built):
    monkeypatch.setenv("DAMAR_PILES", "host")


def test_cases_are_the_generators():
    assert [(c["name"], c["opts"], c["input"]) for c in CASES] == [(n, o, i) for n, o, i in q_common.CASES]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_laq_command(case, tmp_path):
    q_common.run_case(case, str(tmp_path), {"DAMAR_PILES": "host"})


def _laq(tmp, opts, las=LAS):
    return q_common.run_tool(os.path.join(BIN, "LAq"), opts, tmp, env=dict(os.environ, DAMAR_PILES="host"), las=las)


def test_laq_error_paths(tmp_path):
    tmp = q_common.workdir(str(tmp_path), "tiny2")
    usage = "[-uc] [-mbdsS <int>] [-L <file>] [-tT <track>] <db> <overlaps>\n"
    for opts, msg in ((["-d0"], "error: -q not specified\n"), (["-s0"], "error: invalid -s\n"),
                      (["-s5", "-S3"], "error: invalid -s -S combination\n")):
        r = _laq(tmp, opts)
        assert (r.returncode, r.stdout, r.stderr) == (1, "", msg)
    r = _laq(tmp, [], las="nofile.las")
    assert (r.returncode, r.stdout, r.stderr) == (1, "", "could not open 'nofile.las'\n")
    r = _laq(tmp, ["-x"])
    assert r.returncode == 1 and r.stdout == "" and r.stderr.startswith(usage) and r.stderr.endswith("allow quality values of 0!\n")
    r = subprocess.run([os.path.join(BIN, "LAq"), "G"], cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 1 and r.stderr.startswith(usage)
    # -u without the tracks: the pass is announced, then the reference's message (its DB library's own line before it is not kept)
    r = _laq(tmp, ["-u"])
    assert (r.returncode, r.stdout) == (1, "\x1b[32mPASS update quality estimate and trimming\x1b[0m\n")
    assert r.stderr.splitlines()[-1] == "could not open q track"
    assert _laq(tmp, ["-Tkeep"]).returncode == 0                     # a q track, and no trim track of the name -t asks for
    r = _laq(tmp, ["-u", "-tnone"])
    assert r.returncode == 1 and r.stderr.splitlines()[-1] == "could not open none track"
    assert not os.path.exists(os.path.join(tmp, ".G.trim.a2"))


def _api_case(case, tmp):
    """a case through api.q_track / api.trim_update -> the arrays, in the fixture's order"""
    from damar_amd import api
    db = os.path.join(GOLDEN, INPUTS[case["input"]][0], "G")
    las = q_common.input_path(case["input"], tmp)
    kw = q_common.opts_to_kwargs(case["opts"])
    if "-u" in case["opts"]:
        plain = api.q_track(db, q_common.input_path("tiny2", tmp))
        ta, td = api.trim_update(db, las, plain[:2], plain[2:], **{k: v for k, v in kw.items() if k in ("trim_q", "min_len", "ccs")})
        return plain[0], plain[1], ta, td
    return api.q_track(db, las, **kw)


def _equal_fixture(got, exp):
    for g, key in zip(got, ("q_anno", "q_data", "trim_anno", "trim_data")):
        assert g.dtype == exp[key].dtype and np.array_equal(g, exp[key]), key


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_python_calls(case, tmp_path):
    _equal_fixture(_api_case(case, str(tmp_path)), q_common.expected(case["name"]))


@pytest.mark.parametrize("name", ["def_tiny2", "def_tiny_s", "def_synth", "u"])
def test_many_batches_give_the_same_tracks(name, tmp_path, monkeypatch):
    from damar_amd import api
    case = [c for c in CASES if c["name"] == name][0]
    monkeypatch.setenv("DAMAR_PILE_BATCH", "1000")
    _equal_fixture(_api_case(case, str(tmp_path)), q_common.expected(name))
    monkeypatch.delenv("DAMAR_PILE_BATCH")
    monkeypatch.setenv("DAMAR_PILE_TRACE_BYTES", "3000")             # a pile of tiny2 holds more: every pile its own batch
    _equal_fixture(_api_case(case, str(tmp_path)), q_common.expected(name))


def test_byte_bound_cuts_batches(tmp_path):
    """the reader itself: whole piles, the same records and trace bytes whatever the bounds, and the bounds kept"""
    from damar_amd import api
    las = q_common.input_path("tiny2", str(tmp_path))
    whole = q_common.read_las(las)
    for bound, tbound in ((0, 0), (1000, 0), (0, 20000), (7, 100)):
        batches = api.read_trace_piles(las, bound, tbound)
        assert (len(batches) == 1) == (bound == 0 and tbound == 0)
        assert sum(len(b["pile_aread"]) for b in batches) == len(whole["pile_aread"])
        for k in ("abpos", "aepos", "bread", "flags", "tlen", "pile_aread"):
            assert np.array_equal(np.concatenate([b[k] for b in batches]), whole[k]), k
        assert np.concatenate([b["trace"] for b in batches]).tobytes() == whole["trace"].tobytes()
        for b in batches:
            assert b["tbytes"] == 1 and b["tspace"] == 100 and b["trace_off"][0] == 0
            assert np.array_equal(np.diff(b["trace_off"]), b["tlen"][:-1].astype(np.int64))
            if len(b["pile_aread"]) > 1:
                assert (bound == 0 or len(b["abpos"]) <= bound) and (tbound == 0 or len(b["trace"]) <= tbound)


def test_truncated_las_fails(tmp_path):
    from damar_amd import api
    tmp = q_common.workdir(str(tmp_path), "tiny2")
    buf = open(os.path.join(tmp, LAS), "rb").read()
    for cut in (len(buf) - 1, len(buf) - 30, len(buf) // 2):
        open(os.path.join(tmp, "cut.las"), "wb").write(buf[:cut])
        r = _laq(tmp, [], las="cut.las")
        assert r.returncode == 1 and "ends before" in r.stderr
        with pytest.raises(RuntimeError):
            api.q_track(os.path.join(tmp, "G"), os.path.join(tmp, "cut.las"))


def test_integer_rounding_equals_the_float_form():
    """(int) ((float) sum / count + 0.5) == (2 sum + count) / (2 count) for every count <= 255 and sum <= 255 count: what the
    one-byte traces of a default run can reach (a value is below 256, segmax is at most 255 there)"""
    for count in range(1, 256):
        s = np.arange(0, 255 * count + 1, dtype=np.int64)
        d = (s.astype(np.float32) / np.float32(count)).astype(np.float64) + 0.5       # a float division, then a double addition
        assert np.array_equal(d.astype(np.int64), (2 * s + count) // (2 * count)), count


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_model_equals_fixtures(case, tmp_path):
    exp = q_common.expected(case["name"])
    rl = q_common.db_read_len(INPUTS[case["input"]][0])
    b = q_common.read_las(q_common.input_path(case["input"], str(tmp_path)))
    kw = q_common.opts_to_kwargs(case["opts"])
    assert np.all(b["tlen"] >= 4)
    if "-u" in case["opts"]:
        plain = q_model.q_track(q_common.read_las(q_common.input_path("tiny2", str(tmp_path))), rl, strict=True)
        ta, td, tight, emptied = q_model.trim_update(b, rl, *plain, strict=True, **kw)
        assert tight >= 1 and emptied >= 1
        got = (plain[0], plain[1], ta, td)
    else:
        got = q_model.q_track(b, rl, strict=True, **kw)
    _equal_fixture(got, exp)


def test_host_batches_equal_model():
    """damar_pile_quality on arrays (the host path) at a few of the shapes tests/test_gpu_q.py runs on the device"""
    from damar_amd import api
    import q_shapes
    for shape in (0, 3, 5):
        b, rl, kw = q_shapes.make(shape)
        q, tile0, depth, nseg = q_model.tile_q(b, rl, **kw)
        assert np.array_equal(api.pile_quality(b, rl, **kw), q), shape
    b, rl, kw = q_shapes.make(0)
    with pytest.raises(RuntimeError):
        api.pile_quality(b, rl, segmin=0)
    with pytest.raises(RuntimeError):
        api.pile_quality(dict(b, trace=b["trace"][:-1]), rl)


def test_reads_the_database_does_not_have(tmp_path):
    import trim_common
    tmp = q_common.workdir(str(tmp_path), "tiny2")
    trim_common.foreign_aread(os.path.join(tmp, LAS), trim_common.nreads_of("tiny2"))
    r = q_common.run_tool(os.path.join(BIN, "LAq"), [], tmp, env=dict(os.environ, DAMAR_PILES="host"))
    assert (r.returncode, r.stdout, r.stderr) == (1, "\x1b[32mPASS quality estimate and trimming\x1b[0m\n", trim_common.FOREIGN)
