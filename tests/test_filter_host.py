"""LAfilter on the plain host path (DAMAR_PILES=host DAMAR_TRIM=host: host/filter.c, host/trim.c) against the fixtures the
reference's LAfilter left in tests/golden/filter/: output file, -a file, stdout, stderr and exit status of every case."""
import os

import pytest

import filter_common as fc

CASES = fc.load_cases()
HOST = {"DAMAR_PILES": "host", "DAMAR_TRIM": "host"}
SMALL = dict(HOST, DAMAR_PILE_BATCH="40")


@pytest.fixture(autouse=True)
def host_path(monkeypatch):
    for k, v in HOST.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_tool_case(case, tmp_path):
    tmp = str(tmp_path)
    fc.run_case(case, tmp, HOST)
    if fc.keeps_traces(case):
        r = fc.lacheck(tmp)
        assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_small_batches_give_the_same(case, tmp_path):
    fc.run_case(case, str(tmp_path), SMALL)


def test_error_runs(tmp_path):
    tmp = fc.workdir(str(tmp_path), "tiny2")
    for e in fc.load_cases("errors"):
        r = fc.run_tool([], tmp, HOST, args=e["args"])
        assert (r.returncode, r.stdout, r.stderr) == (e["rc"], e["stdout"], e["stderr"]), e["name"]


def test_unsupported_options_say_so(tmp_path):
    tmp = fc.workdir(str(tmp_path), "tiny2")
    for opt, val, what in fc.UNSUPPORTED:
        r = fc.run_tool([opt] + ([val] if val else []), tmp, HOST)
        assert (r.returncode, r.stdout, r.stderr) == (1, "", "LAfilter: %s is not supported\n" % what), opt
    assert not os.path.exists(os.path.join(tmp, "sp.txt"))


def test_T_without_the_trim_track_is_an_error(tmp_path):
    tmp = fc.workdir(str(tmp_path), "tiny2")
    r = fc.run_tool(["-T", "-t", "nosuch"], tmp, HOST)
    assert (r.returncode, r.stdout) == (1, "") and "nosuch" in r.stderr
    r = fc.run_tool(["-t", "nosuch"], tmp, HOST)               # without -T: said, and done without, as in the reference
    assert r.returncode == 0 and r.stderr == "(null): Track 'nosuch' does not exist\ncould not load track nosuch\n"


def test_unsorted_A_file_is_a_message(tmp_path):
    tmp = fc.workdir(str(tmp_path), "tiny2")
    open(os.path.join(tmp, "bad.txt"), "w").write("5 9\n3 4\n")
    r = fc.run_tool(["-A", "bad.txt"], tmp, HOST)
    assert r.returncode == 1 and "not sorted" in r.stderr


# ---- the plain routine against the model of the method (tests/filter_model.py) ------------------------------------------

SETS = {c["name"][:-6]: [o for o in c["opts"] if o not in ("-v", "-p", "-T", "-L")] for c in CASES if c["input"] == "fsynth"}
NAMES = ("flags", "aepos", "bepos", "diffs", "tlen", "reason", "cont_by", "cnt")


@pytest.fixture(scope="module")
def batches():
    import q_common
    rl = q_common.db_read_len("tiny2")
    return {"planted": fc.trace_batch(os.path.join(fc.FDIR, "synth.las")), "random": fc.random_piles()[0]}, rl, fc.load_cases("files")


@pytest.mark.parametrize("which", ["planted", "random"])
@pytest.mark.parametrize("name", sorted(SETS))
def test_host_routine_equals_the_model(batches, name, which):
    import numpy as np
    import filter_model
    from damar_amd import api
    both, rl, files = batches
    kw = fc.opts_to_params(SETS[name], "fsynth", files)
    got = api.pile_filter(both[which], rl, **kw)
    want = filter_model.run_batch(both[which], rl, **kw)
    for k in NAMES:
        bad = np.flatnonzero(np.any(got[k] != want[k], axis=1) if k == "cnt" else got[k] != want[k])
        assert len(bad) == 0, "%s differs in %d places, the first %d: %s against the model's %s" % (k, len(bad), bad[0], got[k][bad[0]], want[k][bad[0]])


def test_pre_step_equals_the_model(batches):
    import numpy as np
    import filter_model
    from damar_amd import api
    both, rl, _ = batches
    for which in both:
        kw = dict(steps=api.FILTER_PRE, downsample=50, seg_rate=30)
        got, want = api.pile_filter(both[which], rl, **kw), filter_model.run_batch(both[which], rl, **kw)
        for k in NAMES:
            assert np.array_equal(got[k], want[k]), (which, k)


PASS = "\x1b[32mPASS filtering\n\x1b[0m"
# what the one-record file leaves on stdout before the close fails: the closing lines are out by then
CLOSE_STDOUT = {(): PASS, ("-T",): PASS + "trimmed 1 of 1 overlaps\ntrimmed 0 of 3108 bases\n"}


@pytest.mark.parametrize("opts", [(), ("-T",)], ids=["plain", "T"])
@pytest.mark.parametrize("small", [False, True], ids=["records", "close"])
def test_refused_write(small, opts, tmp_path):
    """the output on a device that refuses the data: at a record, and (one record, all of it in the stream's buffer) at the close"""
    tmp = fc.workdir(str(tmp_path), "tiny2")
    if small:
        fc.tc.keep_first_record(os.path.join(tmp, fc.LAS))
    r = fc.run_tool(opts, tmp, HOST, args=("G", fc.LAS, fc.tc.FULL))
    assert (r.returncode, r.stdout, r.stderr) == (1, CLOSE_STDOUT[opts] if small else PASS, fc.tc.CANNOT_WRITE)


@pytest.mark.parametrize("opts", [(), ("-T",)], ids=["plain", "T"])
def test_reads_the_database_does_not_have(opts, tmp_path):
    tmp = fc.workdir(str(tmp_path), "tiny2")
    fc.tc.foreign_aread(os.path.join(tmp, fc.LAS), fc.tc.nreads_of("tiny2"))
    r = fc.run_tool(opts, tmp, HOST)
    assert (r.returncode, r.stdout, r.stderr) == (1, PASS, fc.tc.FOREIGN)
