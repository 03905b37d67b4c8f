"""What tests/test_homogenize_host.py, tests/test_gpu_homogenize.py and tests/golden/make_homogenize_golden.py share: the
cases of the TKhomogenize fixtures (tests/golden/homogenize/), a case's input tracks written back into a working directory,
and how a command's output is compared with the fixtures."""
import json
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np

import q_common
import trim_common

ROOT = q_common.ROOT
GOLDEN = q_common.GOLDEN
HDIR = os.path.join(GOLDEN, "homogenize")
BIN = q_common.BIN
LAS = "in.las"

INPUTS = dict(q_common.INPUTS, hsynth=("tiny2", "homogenize/synth.las"), masks_rep=("masks_rep", "masks_rep/G.1.las"))

# name, input, options of the LArepeat run the input track comes from ("synth": written by tests/hom_shapes.py), whether a
# default LAq run supplies the trim track ("synth": hom_shapes's), options of TKhomogenize
CASES = [
    ("def_fusion", "fusion", [], False, []), ("c12_fusion", "fusion", ["-c", "12"], False, []),
    ("def_tandem", "tandem", [], False, []), ("def_tiny2", "tiny2", [], False, []),
    ("m_tiny2", "tiny2", [], False, ["-m"]), ("r10_tiny2", "tiny2", [], False, ["-r", "10"]),
    ("m_r10_tiny2", "tiny2", [], False, ["-m", "-r", "10"]), ("e2000_tandem", "tandem", [], True, ["-e", "2000"]),
    ("e2000_m_fusion", "fusion", ["-c", "12"], True, ["-e", "2000", "-m"]),
    ("b_iI_tiny2", "tiny2", ["-t", "rep2"], False, ["-b", "1", "-i", "rep2", "-I", "hrep2"]),
    ("def_tiny_s", "tiny_s", ["-c", "6"], False, []),
    ("empty_tiny2", "tiny2", ["-c", "12"], False, []),
    ("m_masks_rep", "masks_rep", ["-c", "8"], False, ["-m"]),
]
SYNTH_CASES = [                                 # the planted file: kept apart, the generator's shares are for real inputs
    ("synth", "hsynth", "synth", False, []), ("synth_m", "hsynth", "synth", False, ["-m"]),
    ("synth_r10", "hsynth", "synth", False, ["-r", "10"]), ("synth_m_r7", "hsynth", "synth", False, ["-m", "-r", "7"]),
    ("synth_e", "hsynth", "synth", "synth", ["-e", "1500"]), ("synth_e_r10", "hsynth", "synth", "synth", ["-e", "1500", "-r", "10"]),
]


def opt(opts, flag, default):
    return opts[opts.index(flag) + 1] if flag in opts else default


def track_names(opts):
    """(block, input track, output track, trim track) of a run"""
    return int(opt(opts, "-b", "0")), opt(opts, "-i", "repeats"), opt(opts, "-I", "hrepeats"), opt(opts, "-t", "trim")


def opts_to_kwargs(opts):
    return dict(merge="-m" in opts, ends=int(opt(opts, "-e", "-1")), res=int(opt(opts, "-r", "1")), track_in=opt(opts, "-i", "repeats"),
                trim=opt(opts, "-t", "trim"))


def load_cases(what="cases"):
    """the tool cases on real inputs ("cases"), on the planted file ("synth"), or the runs that end with a message ("errors")"""
    return json.load(open(os.path.join(HDIR, "cases.json")))[what]


def expected(name):
    return np.load(os.path.join(HDIR, "expected_%s.npz" % name))


def copy_db(tmp, inp):
    db = INPUTS[inp][0]
    for f in ("G.db", ".G.idx", ".G.bps"):
        src = os.path.join(GOLDEN, db, f)
        if os.path.exists(src):
            shutil.copy(src, os.path.join(tmp, f))
        else:
            open(os.path.join(tmp, f), "wb").close()          # masks_rep keeps no bases; the tools only open the file
    shutil.copy(os.path.join(GOLDEN, INPUTS[inp][1]), os.path.join(tmp, LAS))


def workdir(tmp, case, exp):
    """the database, the input and the input tracks of a case in tmp"""
    copy_db(tmp, case["input"])
    _, tin, _, ttrim = track_names(case["opts"])
    nreads = int(exp["nreads"])
    trim_common.write_track_a2(os.path.join(tmp, ".G." + tin), nreads, exp["rep_anno"], exp["rep_data"])
    if "trim_anno" in exp.files:
        trim_common.write_track_a2(os.path.join(tmp, ".G." + ttrim), nreads, exp["trim_anno"], exp["trim_data"])
    return tmp


def run_tool(opts, tmp, env_extra=None, timeout_s=60, args=("G", LAS), exe=None):
    cmd = ["timeout", "-k", "10", str(timeout_s), exe or os.path.join(BIN, "TKhomogenize")] + list(opts) + list(args)
    return subprocess.run(cmd, cwd=tmp, env=dict(os.environ, **(env_extra or {})), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True)


def inflate(buf):
    out, at = [], 0
    while at < len(buf):
        n = struct.unpack_from("<Q", buf, at)[0]
        out.append(zlib.decompress(buf[at + 8:at + 8 + n]))
        at += 8 + n
    return b"".join(out)


def read_written(tmp, name, block=0):
    """a track as a run left it: the header's words and everything behind them inflated, whatever the header says of the
    lengths (the empty result's header says 0: see check_output)"""
    pre = os.path.join(tmp, ".G.%s%s" % ("%d." % block if block else "", name))
    a = open(pre + ".a2", "rb").read()
    version, size, _pad, length, clen, cdlen = struct.unpack_from("<HHIQQQ", a, 0)
    d = open(pre + ".d2", "rb").read()
    return dict(version=version, size=size, len=length, clen=clen, cdlen=cdlen, a2_bytes=len(a), d2_bytes=len(d),
                anno=np.frombuffer(inflate(a[64:]), dtype="<u8"), data=np.frombuffer(inflate(d), dtype="<i4"))


def check_output(case, exp, r, tmp):
    """exit status, stdout, stderr and the inflated track against the fixture.  A run that tags nothing ends like the
    reference's: its message, an empty .d2 and an .a2 whose header was not written a second time (clen 0)."""
    assert (r.returncode, r.stdout, r.stderr) == (case["rc"], case["stdout"], case["stderr"])
    block, _, tout, _ = track_names(case["opts"])
    got = read_written(tmp, tout, block)
    assert (got["version"], got["size"], got["len"]) == (2, 8, int(exp["nreads"]))
    assert got["anno"].tobytes() == exp["anno"].astype("<u8").tobytes()
    assert got["data"].tobytes() == exp["data"].astype("<i4").tobytes()
    assert (got["clen"] == 0, got["cdlen"] == 0, got["d2_bytes"] == 0) == tuple(bool(x) for x in exp["header_zero"])
    if len(exp["data"]):
        assert got["clen"] == got["a2_bytes"] - 64 and got["cdlen"] == got["d2_bytes"]


def run_case(case, tmp, env_extra, timeout_s=60):
    exp = expected(case["name"])
    workdir(tmp, case, exp)
    r = run_tool(case["opts"], tmp, env_extra, timeout_s)
    check_output(case, exp, r, tmp)
    return r
