"""What tests/test_trim_host.py, tests/test_gpu_trim.py and tests/golden/make_trim_golden.py share: the cases of the LAtrim
fixtures (tests/golden/trim/), the trim track of a case written back into a working directory, and how a command's output
is compared with the fixtures."""
import hashlib
import json
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np

import q_common

ROOT = q_common.ROOT
GOLDEN = q_common.GOLDEN
TDIR = os.path.join(GOLDEN, "trim")
BIN = q_common.BIN
LAS = "in.las"
OUT = "out.las"

INPUTS = dict(q_common.INPUTS, tsynth=("tiny2", "trim/synth.las"))

# name, input, what the trim track comes from (options of LAq, or "synth": written by hand), options of LAtrim
CASES = [
    ("def_tiny2", "tiny2", [], ["-v"]), ("def_tandem", "tandem", [], ["-v"]), ("def_fusion", "fusion", [], ["-v"]),
    ("def_long", "long", [], ["-v"]), ("def_tiny_s", "tiny_s", [], ["-v"]),
    ("p_tiny2", "tiny2", [], ["-p"]), ("p_fusion", "fusion", [], ["-v", "-p"]),
    ("t2_tiny2", "tiny2", ["-d30", "-Tt2"], ["-v", "-t", "t2"]),
    ("d20_tandem", "tandem", ["-d20"], ["-v"]), ("d20_tandem_p", "tandem", ["-d20"], ["-v", "-p"]),
    ("synth", "tsynth", "synth", ["-v"]), ("synth_p", "tsynth", "synth", ["-v", "-p"]),
]
GPU_CASES = ("def_tiny2", "synth", "synth_p", "def_tandem", "d20_tandem", "d20_tandem_p")


def track_name(opts):
    return opts[opts.index("-t") + 1] if "-t" in opts else "trim"


def md5(path):
    return hashlib.md5(open(path, "rb").read()).hexdigest()


def write_track_a2(prefix, nreads, anno, data):
    """<prefix>.a2 / .d2 as lib/tracks.c writes them: a 64-byte header, then runs of {u64 n, n bytes of a zlib stream}"""
    chunk = lambda b: struct.pack("<Q", len(zlib.compress(b))) + zlib.compress(b)
    ca = chunk(np.ascontiguousarray(anno, dtype="<u8").tobytes())
    cd = chunk(np.ascontiguousarray(data, dtype="<i4").tobytes())
    with open(prefix + ".a2", "wb") as f:
        f.write(struct.pack("<HHIQQQ4Q", 2, 8, 0, nreads, len(ca), len(cd), 0, 0, 0, 0) + ca)
    with open(prefix + ".d2", "wb") as f:
        f.write(cd)


def write_track_anno(prefix, nreads, anno, data):
    """the uncompressed form (db/DB.c Load_Track): what the loaders fall back to"""
    with open(prefix + ".anno", "wb") as f:
        f.write(struct.pack("<ii", nreads, 8) + np.ascontiguousarray(anno, dtype="<i8").tobytes())
    with open(prefix + ".data", "wb") as f:
        f.write(np.ascontiguousarray(data, dtype="<i4").tobytes())


def load_cases(what="cases"):
    """the tool cases, or ("errors") the runs that end with a message"""
    return json.load(open(os.path.join(TDIR, "cases.json")))[what]


def expected(name):
    return np.load(os.path.join(TDIR, "expected_%s.npz" % name))


def workdir(tmp, case, exp, plain=False):
    """the database and the input of a case in tmp, and its trim track (plain: in the uncompressed form)"""
    db = INPUTS[case["input"]][0]
    for f in ("G.db", ".G.idx", ".G.bps"):
        shutil.copy(os.path.join(GOLDEN, db, f), os.path.join(tmp, f))
    shutil.copy(os.path.join(GOLDEN, INPUTS[case["input"]][1]), os.path.join(tmp, LAS))
    nreads = len(exp["trim_anno"]) - 1
    (write_track_anno if plain else write_track_a2)(os.path.join(tmp, ".G." + track_name(case["opts"])), nreads,
                                                    exp["trim_anno"], exp["trim_data"])
    return tmp


def run_tool(opts, tmp, env_extra=None, timeout_s=None, args=("G", LAS, OUT)):
    cmd = [os.path.join(BIN, "LAtrim")] + list(opts) + list(args)
    if timeout_s:
        cmd = ["timeout", "-k", "10", str(timeout_s)] + cmd
    return subprocess.run(cmd, cwd=tmp, env=dict(os.environ, **(env_extra or {})), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True)


def read_records(path):
    """(the ten words of every record, the trace bytes back to back, header count, spacing)"""
    b = q_common.read_las(path)
    buf = open(path, "rb").read()
    novl, tspace = struct.unpack_from("<qi", buf, 0)
    cols = np.zeros((novl, 10), dtype=np.int32)
    at, tb = 12, b["tbytes"]
    for i in range(novl):
        cols[i] = np.frombuffer(buf, dtype="<i4", count=10, offset=at)
        at += 40 + tb * int(cols[i, 0])
    return cols, b["trace"], novl, tspace


def check_output(case, exp, r, out):
    """exit status, stdout, stderr and the output file of a run against the fixture; on a mismatch of the file, where"""
    assert (r.returncode, r.stdout, r.stderr) == (case["rc"], case["stdout"], case["stderr"])
    if md5(out) == case["md5"]:
        return
    cols, trace, novl, tspace = read_records(out)
    assert (novl, tspace) == (int(exp["novl"]), int(exp["tspace"])), "header"
    names = ("tlen", "diffs", "abpos", "bbpos", "aepos", "bepos", "flags", "aread", "bread", "last word")
    for k, name in enumerate(names):
        bad = np.flatnonzero(cols[:, k] != exp["cols"][:, k])
        assert len(bad) == 0, "%s differs in %d records, the first %d: %d against %d" % (name, len(bad), bad[0], cols[bad[0], k],
                                                                                         exp["cols"][bad[0], k])
    if "trace" in exp.files:
        bad = np.flatnonzero(trace != exp["trace"])
        assert len(bad) == 0, "trace bytes differ, the first at %d" % bad[0]
    assert False, "the output's md5 differs and no column does"


def run_case(case, tmp, env_extra, timeout_s=None, plain=False, opts=None):
    exp = expected(case["name"])
    workdir(tmp, case, exp, plain=plain)
    r = run_tool(case["opts"] if opts is None else opts, tmp, env_extra, timeout_s)
    check_output(case, exp, r, os.path.join(tmp, OUT))
    return r


def boxes():
    """the box cases: m, n, aoff, boff, bases and what the reference's Compute_Alignment(DIFF_ALIGN) made of them"""
    return np.load(os.path.join(TDIR, "boxes.npz"))


BOX_MAX = 1000                          # DAMAR_BOX_MAXLEN: the largest box kernels/box_align.hip keeps
_WIDE = None


def boxes_wide():
    """the box cases of tests/golden/make_box_edges_golden.py, loaded once: the layout of boxes(), and family[i] (an index
    into families) and planted[i] (the substitutions planted into a ladder box, -1 elsewhere) of every box"""
    global _WIDE
    if _WIDE is None:
        z = np.load(os.path.join(TDIR, "boxes_wide.npz"))
        _WIDE = {k: z[k] for k in z.files}
        for v in _WIDE.values():
            v.setflags(write=False)
    return _WIDE


def family_rows(bx, name):
    return np.flatnonzero(bx["family"] == list(bx["families"]).index(name))


def box_seqs(bx, idx=None):
    idx = range(len(bx["m"])) if idx is None else idx
    a = [bx["bases"][bx["aoff"][i]:bx["aoff"][i] + bx["m"][i]] for i in idx]
    b = [bx["bases"][bx["boff"][i]:bx["boff"][i] + bx["n"][i]] for i in idx]
    return a, b


def check_boxes(bx, diffs, scripts, idx=None):
    idx = list(range(len(bx["m"]))) if idx is None else list(idx)
    assert len(diffs) == len(idx) and len(scripts) == len(idx)
    for j, i in enumerate(idx):
        want = bx["script"][bx["soff"][i]:bx["soff"][i + 1]]
        assert int(diffs[j]) == int(bx["diffs"][i]), "box %d (%d x %d): %d differences against %d" % (i, bx["m"][i], bx["n"][i],
                                                                                                     diffs[j], bx["diffs"][i])
        assert np.array_equal(scripts[j], want), "box %d (%d x %d): the scripts part ways" % (i, bx["m"][i], bx["n"][i])


# ---- what the passes over a .las file share: a refused write, reads the database does not have -----------------------

FULL = "/dev/full"                      # takes the open and refuses the data
CANNOT_WRITE = "damar: cannot write %s\n" % FULL
FOREIGN = "damar: %s holds reads the database does not have\n" % LAS


def record_offsets(buf):
    """where every record of a .las file begins, and where the last one ends"""
    novl, tspace = struct.unpack_from("<qi", buf, 0)
    tb, at, offs = (1 if tspace <= 125 else 2), 12, []
    for _ in range(novl):
        offs.append(at)
        at += 40 + tb * struct.unpack_from("<i", buf, at)[0]
    return offs, at


def keep_first_record(path):
    """the file cut to its first record: what a run writes of it fits the stream's buffer, the refusal comes at the close"""
    buf = open(path, "rb").read()
    offs, _ = record_offsets(buf)
    open(path, "wb").write(struct.pack("<q", 1) + buf[8:offs[1]])


def foreign_aread(path, nreads):
    """the A read of the file's last record set to nreads: the first read the database does not have"""
    buf = bytearray(open(path, "rb").read())
    offs, _ = record_offsets(buf)
    struct.pack_into("<i", buf, offs[-1] + 28, nreads)
    open(path, "wb").write(buf)


def nreads_of(db):
    return len(q_common.db_read_len(db))
