"""LAgap on the plain host path (DAMAR_PILES=host DAMAR_TRIM=host: host/gap.c, host/trim.c) against the fixtures the
reference's LAgap left in tests/golden/gap/: output file, stdout, stderr and exit status of every case."""
import os

import pytest

import gap_common as gc

CASES = gc.load_cases()
HOST = {"DAMAR_PILES": "host", "DAMAR_TRIM": "host"}
SMALL = dict(HOST, DAMAR_PILE_BATCH="40")             # the planted file's 202 records in several batches


@pytest.fixture(autouse=True)
def host_path(monkeypatch):
    for k, v in HOST.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_tool_case(case, tmp_path):
    tmp = str(tmp_path)
    gc.run_case(case, tmp, HOST)
    r = gc.lacheck(tmp)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_small_batches_give_the_same(case, tmp_path):
    gc.run_case(case, str(tmp_path), SMALL)


def test_error_runs(tmp_path):
    tmp = gc.workdir(str(tmp_path), "tiny2")
    for e in gc.load_cases("errors"):
        r = gc.run_tool([], tmp, HOST, args=e["args"])
        assert (r.returncode, r.stdout, r.stderr) == (e["rc"], e["stdout"], e["stderr"]), e["name"]
    r = gc.run_tool(["-C", "x"], tmp, HOST)
    assert (r.returncode, r.stdout, r.stderr) == gc.NO_CHIMER
    assert not os.path.exists(os.path.join(tmp, "x"))


@pytest.mark.parametrize("name", ["es_synth", "tps_synth", "t_tiny2"])
def test_api_agrees_with_the_command(name, tmp_path, capfd):
    from damar_amd import api
    case = next(c for c in CASES if c["name"] == name)
    tmp = gc.workdir(str(tmp_path), case["input"])
    p = lambda f: os.path.join(tmp, f)
    st = api.gap_las(p("G"), p(gc.LAS), p(gc.OUT), **gc.opts_to_kwargs(case["opts"]))
    assert gc.tc.md5(p(gc.OUT)) == case["md5"]
    exp = gc.expected(name)
    assert st["written"] == int(exp["novl"]) and st["host_piles"] == 0
    tail = case["stdout"].splitlines()[-2:]
    assert tail == ["dropped %d containments" % st["contained"], "dropped %d overlaps in %d break/gaps" % (st["dropped"], st["breaks"])]
    assert capfd.readouterr().out == case["stdout"]


PASS = "\x1b[32mPASS gaps\x1b[0m\n"
# what the one-record file leaves on stdout before the close fails: the closing lines are out by then
CLOSE_STDOUT = {(): PASS + "DROP R @ 10400..11300\ndropped 0 containments\ndropped 1 overlaps in 1 break/gaps\n",
                ("-t", "trim"): PASS + "            1 of             1 overlaps trimmed\n            0 of          3108 bases trimmed\n"
                                "dropped 0 containments\ndropped 0 overlaps in 0 break/gaps\n"}


@pytest.mark.parametrize("opts", [(), ("-t", "trim")], ids=["plain", "t"])
@pytest.mark.parametrize("small", [False, True], ids=["records", "close"])
def test_refused_write(small, opts, tmp_path):
    """the output on a device that refuses the data: at a record, and (one record, all of it in the stream's buffer) at the close"""
    tmp = gc.workdir(str(tmp_path), "tiny2")
    if small:
        gc.tc.keep_first_record(os.path.join(tmp, gc.LAS))
    r = gc.run_tool(opts, tmp, HOST, args=("G", gc.LAS, gc.tc.FULL))
    assert (r.returncode, r.stderr) == (1, gc.tc.CANNOT_WRITE)
    if small:
        assert r.stdout == CLOSE_STDOUT[opts]
    else:
        assert r.stdout.startswith(PASS) and "dropped" not in r.stdout


@pytest.mark.parametrize("opts", [(), ("-t", "trim")], ids=["plain", "t"])
def test_reads_the_database_does_not_have(opts, tmp_path):
    tmp = gc.workdir(str(tmp_path), "tiny2")
    gc.tc.foreign_aread(os.path.join(tmp, gc.LAS), gc.tc.nreads_of("tiny2"))
    r = gc.run_tool(opts, tmp, HOST)
    assert (r.returncode, r.stdout, r.stderr) == (1, PASS, gc.tc.FOREIGN)
