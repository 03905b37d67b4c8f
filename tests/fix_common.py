"""What tests/test_fix_host.py, tests/test_gpu_fix.py and tests/golden/make_fix_golden.py share: the inputs of the LAfix
fixtures (tests/golden/fix/), the working directory of a case, and how a command's output is compared with the fixtures."""
import hashlib
import json
import os
import shutil
import subprocess
import zlib

import numpy as np

import q_common
import trim_common as tc

ROOT = q_common.ROOT
GOLDEN = q_common.GOLDEN
FDIR = os.path.join(GOLDEN, "fix")
BIN = q_common.BIN
LAS = "in.las"
OUT = "patched.fasta"
TOUT = "trims.txt"
TW = 100

REAL = ("tiny2", "fusion", "tandem", "long", "tiny_s")       # the inputs LAgap's fixtures use
INPUTS = dict(q_common.INPUTS, fsynth=("tiny2", "fix/synth.las"))
Q_OF = dict(tiny2="def_tiny2", tandem="def_tandem", fusion="def_fusion", long="def_long", tiny_s="def_tiny_s")
Q_LIST = (25, 22, 20, 18, 15)           # what the generator picks -Q from: below the default, so that it makes weak segments
BIG = "fusion"                          # the largest real fixture file

ERRORS = (("no_q_track", ["-q", "nosuch", "G", LAS, OUT]), ("no_t_track", ["-t", "nosuch", "G", LAS, OUT]),
          ("no_r_track", ["-r", "nosuch", "G", LAS, OUT]), ("no_c_track", ["-c", "nosuch", "G", LAS, OUT]),
          ("no_las", ["G", "nosuch.las", OUT]), ("no_args", ["G", LAS]), ("bad_option", ["-z", "G", LAS, OUT]),
          ("R_101", ["-R", "101", "G", LAS, OUT]),
          # the two sanity exits: a q track that lacks a read's values, a trim interval beyond its read (see workdir)
          ("q_count", ["-q", "qbad", "-t", "trim", "G", LAS, OUT]), ("trim_outside", ["-t", "tbad", "G", LAS, OUT]))
# this project's own: the reference's experimental chimer code and its quality streams are not built
NO_CHIMER = (1, "", "LAfix: -X (chimer detection) is not supported\n")
NO_QUIVA = (1, "", "LAfix: -f (quality streams) is not supported\n")


def variants(qv):
    """the option sets of every input, qv the -Q value the generator picked"""
    return [("def", ["-t", "trim"]), ("not", []), ("l", ["-t", "trim", "-l"]), ("Q", ["-t", "trim", "-Q", str(qv)]),
            ("g", ["-t", "trim", "-Q", str(qv), "-g", "300"]), ("x", ["-t", "trim", "-x", "6000"]),
            ("c", ["-t", "trim", "-Q", str(qv), "-c", "cv1", "-c", "cv2"]), ("T", ["-t", "trim", "-T", TOUT]),
            ("r", ["-t", "trim", "-r", "rep"]), ("g0", ["-t", "trim", "-g", "-1"])]


def load_cases(what="cases"):
    return json.load(open(os.path.join(FDIR, "cases.json")))[what]


def expected(name):
    return np.load(os.path.join(FDIR, "expected_%s.npz" % name))


def tracks(inp):
    """{track name: (anno, data)} of an input: q, trim, rep, cv1, cv2"""
    if inp == "fsynth":
        t = np.load(os.path.join(FDIR, "synth_tracks.npz"))
        return {k: (t[k + "_anno"], t[k + "_data"]) for k in ("q", "trim", "rep", "cv1", "cv2")}
    t = q_common.expected(Q_OF[inp])
    trim = (t["trim_anno"], t["trim_data"])
    return dict(q=(t["q_anno"], t["q_data"]), trim=trim, rep=trim, cv1=trim, cv2=trim)


def workdir(tmp, inp):
    """the database, the input and its tracks in tmp"""
    db = INPUTS[inp][0]
    for f in ("G.db", ".G.idx", ".G.bps"):
        shutil.copy(os.path.join(GOLDEN, db, f), os.path.join(tmp, f))
    shutil.copy(os.path.join(GOLDEN, INPUTS[inp][1]), os.path.join(tmp, LAS))
    tr = tracks(inp)
    for name, (anno, data) in tr.items():
        tc.write_track_a2(os.path.join(tmp, ".G." + name), len(anno) - 1, anno, data)
    # for the error runs: the q track without the values of the tenth pile's read, the trim track with that read's
    # interval running 100 bases past its end
    rl = q_common.db_read_len(db)
    a = int(q_common.read_las(os.path.join(tmp, LAS))["pile_aread"][9])
    qa, qd = np.array(tr["q"][0], dtype=np.int64), np.asarray(tr["q"][1])
    n = qa[a + 1] - qa[a]
    qbad = np.concatenate([qa[:a + 1], qa[a + 1:] - n])
    tc.write_track_a2(os.path.join(tmp, ".G.qbad"), len(qbad) - 1, qbad, np.concatenate([qd[:qa[a] // 4], qd[qa[a + 1] // 4:]]))
    ta, td = np.array(tr["trim"][0], dtype=np.int64), np.array(tr["trim"][1])
    if ta[a + 1] - ta[a] == 8:
        td[ta[a] // 4 + 1] = rl[a] + 100
    tc.write_track_a2(os.path.join(tmp, ".G.tbad"), len(ta) - 1, ta, td)
    return tmp


def run_tool(opts, tmp, env_extra=None, timeout_s=None, args=("G", LAS, OUT), drop=(), exe=None):
    cmd = [exe or os.path.join(BIN, "LAfix")] + list(opts) + list(args)
    if timeout_s:
        cmd = ["timeout", "-k", "10", str(timeout_s)] + cmd
    env = {k: v for k, v in os.environ.items() if k not in drop}
    env.update(env_extra or {})
    return subprocess.run(cmd, cwd=tmp, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def md5(path):
    return hashlib.md5(open(path, "rb").read()).hexdigest() if os.path.exists(path) else None


def digest(buf):
    """a FASTA file as (header lines, bases per read, crc32 of each read's lines)"""
    heads, lens, crcs = [], [], []
    for block in buf.split(b">")[1:]:
        head, _, body = block.partition(b"\n")
        heads.append(head.decode("latin-1"))
        lens.append(len(body.replace(b"\n", b"")))
        crcs.append(zlib.crc32(body))
    return heads, np.array(lens, dtype=np.int64), np.array(crcs, dtype=np.uint32)


def check_output(case, r, tmp):
    """exit status, stdout, stderr, the FASTA and the -T file of a run against the fixture; on a mismatch, where"""
    assert (r.returncode, r.stdout, r.stderr) == (case["rc"], case["stdout"], case["stderr"])
    assert md5(os.path.join(tmp, TOUT)) == case["md5_T"]
    if md5(os.path.join(tmp, OUT)) == case["md5"]:
        return
    exp = expected(case["name"])
    heads, lens, crcs = digest(open(os.path.join(tmp, OUT), "rb").read())
    assert heads == [str(h) for h in exp["heads"]], "the header lines differ"
    bad = np.flatnonzero(lens != exp["lens"])
    assert len(bad) == 0, "%s holds %d bases, %d expected" % (heads[bad[0]], lens[bad[0]], exp["lens"][bad[0]])
    bad = np.flatnonzero(crcs != exp["crcs"])
    assert len(bad) == 0, "the bases of %s differ" % heads[bad[0]]
    assert False, "the FASTA's md5 differs and no read does"


def run_case(case, tmp, env_extra=None, timeout_s=None, drop=()):
    workdir(tmp, case["input"])
    r = run_tool(case["opts"], tmp, env_extra, timeout_s, drop=drop)
    check_output(case, r, tmp)
    return r


def opts_to_kwargs(opts):
    """the options of a case as api.fix_las takes them"""
    names = {"-x": ("min_len", int), "-Q": ("low_q", int), "-g": ("max_gap", int), "-t": ("trim", str), "-q": ("q", str),
             "-r": ("repeats", str), "-T": ("trim_out", str)}
    kw, i = dict(convert=[]), 0
    while i < len(opts):
        if opts[i] == "-l":
            kw["low_coverage"] = True
        elif opts[i] == "-c":
            kw["convert"].append(opts[i + 1])
            i += 1
        elif opts[i] in names:
            kw[names[opts[i]][0]] = names[opts[i]][1](opts[i + 1])
            i += 1
        i += 1
    return kw


def batch_of(inp):
    """an input's .las file as api.pile_patches takes it, with the database's read lengths"""
    return q_common.read_las(os.path.join(GOLDEN, INPUTS[inp][1])), q_common.db_read_len(INPUTS[inp][0])


def trims_of(batch, rl, trim):
    """the trim track's interval of every pile's A read, as get_trim reads it"""
    anno, data = np.asarray(trim[0], dtype=np.int64) // 4, trim[1]
    out = np.zeros((len(batch["pile_aread"]), 2), dtype=np.int32)
    for i, a in enumerate(batch["pile_aread"]):
        if anno[a + 1] - anno[a] == 2 and data[anno[a]] < data[anno[a] + 1]:
            out[i] = data[anno[a]], data[anno[a] + 1]
    return out
