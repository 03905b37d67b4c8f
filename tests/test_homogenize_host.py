"""TKhomogenize on the host path (DAMAR_PILES=host; host/homogenize.c): every fixture of tests/golden/homogenize/ through
bin/TKhomogenize and the Python call, the planted shapes of tests/hom_shapes.py through api.pile_homogenize against the model
and the reference's fixtures, batching, and the command's error paths."""
import numpy as np
import pytest

import hom_checks
import hom_common as hc

CASES = hc.load_cases("cases") + hc.load_cases("synth")
IDS = [c["name"] for c in CASES]
HOST = {"DAMAR_PILES": "host"}


@pytest.fixture(autouse=True)
def host_path(monkeypatch, built):
    monkeypatch.setenv("DAMAR_PILES", "host")
    monkeypatch.delenv("DAMAR_PILE_BATCH", raising=False)


def test_cases_are_the_generators():
    assert [(c["name"], c["input"], c["opts"]) for c in CASES] == [(n, i, o) for n, i, _, _, o in hc.CASES + hc.SYNTH_CASES]
    assert sum(1 for c in CASES if len(hc.expected(c["name"])["data"]) == 0) == 1


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_command(case, tmp_path):
    hc.run_case(case, str(tmp_path), HOST)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_homogenize_track_equals_command(case, tmp_path):
    hom_checks.check_python_equals_command(case, str(tmp_path), HOST)


@pytest.mark.parametrize("name", ["def_tiny2", "def_tiny_s", "e2000_tandem"])
def test_many_batches_give_the_same_track(name, tmp_path, monkeypatch):
    case = [c for c in CASES if c["name"] == name][0]
    monkeypatch.setenv("DAMAR_PILE_BATCH", "500")
    hom_checks.check_python_equals_command(case, str(tmp_path), HOST)


@pytest.mark.parametrize("name", sorted(hom_checks.SYNTH_KW))
def test_planted_shapes_equal_model_and_reference(name):
    hom_checks.check_synth(name)


def test_planted_records_do_what_they_are_there_for():
    hom_checks.check_roles()


@pytest.mark.parametrize("name", ["synth", "synth_m_r7", "synth_e"])
def test_piles_in_different_batches(name):
    hom_checks.check_batches(name)


def test_four_piles_in_three_batches(tmp_path, monkeypatch):
    hom_checks.check_reader_batches(str(tmp_path), monkeypatch)


def test_two_byte_traces():
    hom_checks.check_two_byte()


def test_empty_batch_list():
    hom_checks.check_empty_list()


def test_bit_range_helper_equals_the_reference_loop():
    """damar_bits_set_range against a line-for-line ba_assign_range, over every pair of ends in three bytes and some wide ones"""
    import ctypes
    import hom_model
    from damar_amd import api
    L = api.lib()
    L.damar_bits_set_range.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64]
    L.damar_bits_set_range.restype = None
    pairs = [(b, e) for b in range(24) for e in range(24)] + [(31, 31), (31, 32), (32, 63), (0, 95), (33, 70), (5, 12895), (7, 4000)]
    for beg, end in pairs:
        for fill in (0, 0x5a):
            want = np.unpackbits(np.full(2048, fill, dtype=np.uint8), bitorder="little").astype(bool)
            hom_model.assign_range(want, beg, end)
            got = np.full(2048, fill, dtype=np.uint8)
            L.damar_bits_set_range(got.ctypes.data, 2048 * 8, beg, end)
            assert np.array_equal(np.unpackbits(got, bitorder="little").astype(bool), want), (beg, end, fill)


def test_error_paths(tmp_path):
    tmp = str(tmp_path)
    hc.copy_db(tmp, "tiny2")
    for e in hc.load_cases("errors"):
        r = hc.run_tool([], tmp, HOST, args=e["args"])
        assert (r.returncode, r.stdout) == (e["rc"], e["stdout"]), e["name"]
        if e["name"] == "no_trim":                   # the reference's DB library puts a line of its own in front
            assert r.stderr.splitlines()[-1] == e["stderr"].splitlines()[-1] == "-e requires a trim track"
        else:
            assert r.stderr == e["stderr"], e["name"]
    r = hc.run_tool(["-i", "nosuch"], tmp, HOST)
    assert r.returncode == 1 and r.stdout == "\x1b[32mPASS homogenising\n\x1b[0m" and r.stderr.splitlines()[-1] == "could not load track nosuch"


def test_calls_refuse_what_they_cannot_index():
    from damar_amd import api
    p, _ = hom_checks.plan()
    ra, rd = p.track()
    b = p.batch()
    with pytest.raises(RuntimeError):
        api.pile_homogenize([dict(b, trace=b["trace"][:-1])], p.rl, ra, rd)
    with pytest.raises(RuntimeError):
        api.pile_homogenize([dict(b, bepos=b["bepos"] + 100000)], p.rl, ra, rd)
    with pytest.raises(RuntimeError):
        api.pile_homogenize([b], p.rl, ra, rd, res=0)
    with pytest.raises(ValueError):
        api.pile_homogenize([b], p.rl, ra, rd, ends=1500)


def test_reads_the_database_does_not_have(tmp_path):
    case = next(c for c in CASES if c["name"] == "def_tiny2")
    tmp = hc.workdir(str(tmp_path), case, hc.expected(case["name"]))
    hc.trim_common.foreign_aread(str(tmp_path / hc.LAS), hc.trim_common.nreads_of("tiny2"))
    r = hc.run_tool(case["opts"], tmp, HOST)
    assert (r.returncode, r.stderr) == (1, hc.trim_common.FOREIGN)
    assert r.stdout.startswith("\x1b[32mPASS homogenising\n\x1b[0m")
