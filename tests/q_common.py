"""What tests/test_q_host.py, tests/test_gpu_q.py and tests/golden/make_q_golden.py share: the inputs of the LAq fixtures
(tests/golden/q/), a .las file as the batch tests/q_model.py reads, the flagged copy -u runs on, and how a command's
output is compared with the fixtures."""
import json
import os
import shutil
import struct
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, ".."))
GOLDEN = os.path.join(HERE, "golden")
QDIR = os.path.join(GOLDEN, "q")
BIN = os.path.join(ROOT, "damar_amd", "bin")

INPUTS = {                  # name: (database, .las file under tests/golden/)
    "tandem": ("tandem", "tandem/las/d001_00001/G.1.G.1.las"),
    "fusion": ("fusion", "fusion/las/d001_00001/G.1.G.1.las"),
    "tiny2": ("tiny2", "tiny2/las/d001_00001/G.1.G.1.las"),
    "long": ("long", "long/las/d001_00001/G.1.G.1.las"),
    "tiny_s": ("tiny2", "tiny_s/las/d001_00002/G.2.G.1.las"),
    "tan_k10": ("tandem", "tan_k10/las/tan/G.1.G.1.las"),
    "synth": ("tiny2", "q/synth.las"),
    "flagged": ("tiny2", None),             # made by flag_records from tiny2's file
}
CASES = [                   # name, options, input
    ("def_tandem", [], "tandem"), ("def_fusion", [], "fusion"), ("def_tiny2", [], "tiny2"), ("def_long", [], "long"),
    ("def_tiny_s", [], "tiny_s"), ("def_tan_k10", [], "tan_k10"), ("def_synth", [], "synth"), ("def_flagged", [], "flagged"),
    ("s3S5", ["-s3", "-S5"], "tiny2"), ("S1", ["-S1"], "tiny2"), ("d20", ["-d20"], "tiny2"),
    ("d30o3000", ["-d30", "-o3000"], "tiny2"), ("c", ["-c"], "tiny2"), ("c_synth", ["-c"], "synth"),
    ("bTQ", ["-b1", "-Tt2", "-Qq2"], "tiny2"), ("L", ["-L", "qlog.txt"], "tiny2"),
    ("u", ["-u"], "flagged"),               # after a default run on tiny2's own file, as a pipeline would
]
LAS = "in.las"              # what every case's input is called in its working directory


def db_read_len(db):
    """the read lengths of a fixture database, from its index"""
    buf = open(os.path.join(GOLDEN, db, ".G.idx"), "rb").read()
    n = struct.unpack_from("<i", buf, 0)[0]
    return np.frombuffer(buf, dtype="<i4", offset=len(buf) - 32 * n).reshape(n, 8)[:, 0].copy()


def flag_records(src, dst):
    """tiny2's file with one record in nine marked OVL_DISCARD, in every fourth pile the leftmost and the rightmost record
    discarded too (so that -u has something to tighten) and two records made identity overlaps, and all of the sixth
    pile's records discarded (so that -u empties one).  Deterministic: the generator and the tests make the same bytes."""
    buf = bytearray(open(src, "rb").read())
    novl, tspace = struct.unpack_from("<qi", buf, 0)
    tb = 1 if tspace <= 125 else 2
    rng = np.random.default_rng(20251018)
    at, recs = 12, []
    for _ in range(novl):
        tlen = struct.unpack_from("<i", buf, at)[0]
        recs.append(at)
        at += 40 + tb * tlen
    aread = [struct.unpack_from("<i", buf, r + 28)[0] for r in recs]
    cuts = [0] + [i for i in range(1, novl) if aread[i] != aread[i - 1]] + [novl]
    draw = rng.random(novl)

    def discard(r):
        struct.pack_into("<I", buf, r + 24, struct.unpack_from("<I", buf, r + 24)[0] | 2)
    for p in range(len(cuts) - 1):
        mine = recs[cuts[p]:cuts[p + 1]]
        for k, r in enumerate(mine):
            if draw[cuts[p] + k] < 1 / 9 or p == 5:
                discard(r)
        if p % 4 == 0:
            discard(min(mine, key=lambda r: struct.unpack_from("<i", buf, r + 8)[0]))
            discard(max(mine, key=lambda r: struct.unpack_from("<i", buf, r + 16)[0]))
            for r in mine[1:3]:
                struct.pack_into("<i", buf, r + 32, aread[cuts[p]])
    open(dst, "wb").write(bytes(buf))


def input_path(name, tmp):
    """the .las file of an input (the flagged copy is written into tmp)"""
    if name == "flagged":
        dst = os.path.join(tmp, "flagged_src.las")
        flag_records(os.path.join(GOLDEN, INPUTS["tiny2"][1]), dst)
        return dst
    return os.path.join(GOLDEN, INPUTS[name][1])


def read_las(path):
    """a whole .las file as one batch: the columns, the trace bytes back to back and where each record's begin"""
    buf = open(path, "rb").read()
    novl, tspace = struct.unpack_from("<qi", buf, 0)
    tb = 1 if tspace <= 125 else 2
    cols = np.zeros((novl, 10), dtype=np.int32)
    toff = np.zeros(novl, dtype=np.int64)
    trace, at, top = [], 12, 0
    for i in range(novl):
        cols[i] = np.frombuffer(buf, dtype="<i4", count=10, offset=at)
        n = tb * int(cols[i, 0])
        trace.append(buf[at + 40:at + 40 + n])
        toff[i] = top
        top += n
        at += 40 + n
    aread = cols[:, 7]
    off = np.concatenate([[0], np.flatnonzero(np.diff(aread)) + 1, [novl]]).astype(np.int64) if novl else np.zeros(1, dtype=np.int64)
    return dict(pile_off=off, pile_aread=aread[off[:-1]].copy(), abpos=cols[:, 2].copy(), aepos=cols[:, 4].copy(),
                bbpos=cols[:, 3].copy(), bepos=cols[:, 5].copy(), bread=cols[:, 8].copy(), flags=cols[:, 6].copy(),
                tlen=cols[:, 0].copy(), trace=np.frombuffer(b"".join(trace), dtype=np.uint8), trace_off=toff, tbytes=tb, tspace=tspace)


def opts_to_kwargs(opts):
    kw = {}
    names = {"s": "segmin", "S": "segmax", "d": "trim_q", "o": "min_len"}
    i = 0
    while i < len(opts):
        f, v = opts[i][1], opts[i][2:]
        if f in names:
            kw[names[f]] = int(v)
        elif f == "c":
            kw["ccs"] = True
        elif f == "L":
            i += 1
        i += 1                                # -u -b -T -Q -t -q: which pass and where the command writes
    return kw


def track_names(opts):
    """(block, q track, trim track) the options make the command write"""
    block, q, t = 0, "q", "trim"
    for o in opts:
        if o.startswith("-b"):
            block = int(o[2:])
        elif o.startswith("-Q"):
            q = o[2:]
        elif o.startswith("-T"):
            t = o[2:]
    return block, q, t


def workdir(tmp, inp):
    """the database of an input and the input itself as in.las, in tmp"""
    db = INPUTS[inp][0]
    for f in ("G.db", ".G.idx", ".G.bps"):
        shutil.copy(os.path.join(GOLDEN, db, f), os.path.join(tmp, f))
    shutil.copy(input_path(inp, tmp), os.path.join(tmp, LAS))
    return tmp


def run_tool(exe, opts, tmp, env=None, timeout_s=None, las=LAS):
    cmd = [exe] + opts + ["G", las]
    if timeout_s:
        cmd = ["timeout", "-k", "10", str(timeout_s)] + cmd
    return subprocess.run(cmd, cwd=tmp, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def prepare_update(exe, tmp, env=None):
    """what -u starts from: the default tracks of tiny2's own file"""
    shutil.copy(os.path.join(GOLDEN, INPUTS["tiny2"][1]), os.path.join(tmp, "plain.las"))
    r = run_tool(exe, [], tmp, env=env, las="plain.las")
    assert r.returncode == 0, r.stderr


def load_cases():
    return json.load(open(os.path.join(QDIR, "cases.json")))


def expected(name):
    return np.load(os.path.join(QDIR, "expected_%s.npz" % name))


def check_tracks(case, tmp, exp):
    """the track files the command left in tmp, inflated, against the fixture"""
    from damar_amd import api
    block, q, t = track_names(case["opts"])
    names = [("trim", t)] if "-u" in case["opts"] else [("q", q), ("trim", t)]
    for key, name in names:
        got = api.read_track(os.path.join(tmp, "G"), name, block)
        assert (got["version"], got["size"], got["len"]) == (2, 8, int(exp["nreads"])), name
        assert got["anno"].tobytes() == exp[key + "_anno"].astype("<u8").tobytes(), name
        assert got["data"].tobytes() == exp[key + "_data"].astype("<i4").tobytes(), name


def run_case(case, tmp, env_extra, timeout_s=None):
    """one fixture case through bin/LAq: exit status, stdout, stderr, the -L file and the tracks"""
    exe = os.path.join(BIN, "LAq")
    env = dict(os.environ, **env_extra)
    workdir(tmp, case["input"])
    if "-u" in case["opts"]:
        prepare_update(exe, tmp, env)
    r = run_tool(exe, case["opts"], tmp, env=env, timeout_s=timeout_s)
    assert (r.returncode, r.stdout, r.stderr) == (case["rc"], case["stdout"], case["stderr"])
    if "-L" in case["opts"]:
        assert open(os.path.join(tmp, "qlog.txt")).read() == case["qlog"]
    check_tracks(case, tmp, expected(case["name"]))
