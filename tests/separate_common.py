"""What tests/test_separate_host.py, tests/test_gpu_separate.py and tests/golden/make_separate_golden.py share: the cases of
the LAseparate fixtures (tests/golden/separate/), the working directory of a case, the groups of a file as
tests/separate_model.py takes them, and how a command's two output files are compared with the fixtures."""
import json
import os
import shutil
import struct
import subprocess

import numpy as np

import filter_common as fc
import q_common
import separate_model as sm
import trim_common as tc

ROOT = q_common.ROOT
GOLDEN = q_common.GOLDEN
SDIR = os.path.join(GOLDEN, "separate")
BIN = q_common.BIN
LAS = tc.LAS
OUT = tc.OUT
OUT2 = "out_discard.las"
TW = 100
DISCARD, TEMP = 0x2, 0x800

INPUTS = dict(q_common.INPUTS, ssynth=("tiny2", "separate/synth.las"))
REAL = ("tiny2", "fusion", "tandem", "long", "tiny_s")
VARIANTS = [("T0", ["-T0"]), ("T1", ["-T", "1"]), ("T1r", ["-T1", "-r", "rep2"]), ("T0L", ["-T0", "-L", "-o", "500", "-l", "1000", "-v"])]
CASES = [("%s_%s" % (v, inp), inp, o) for inp in REAL + ("ssynth",) for v, o in VARIANTS]
ARGS = ("G", LAS, OUT, OUT2)
ERRORS = (("no_track", ["-r", "nosuch"] + list(ARGS)), ("bad_type", ["-T", "2"] + list(ARGS)), ("no_las", ["G", "nosuch.las", OUT, OUT2]),
          ("no_args", ["G", LAS, OUT]), ("bad_option", ["-x"] + list(ARGS)))
BIG = "fusion"                          # the largest real fixture file
PASS = "\x1b[32mPASS separate\n\x1b[0m"
# this project's own: the group the reference aborts on after its first file (two records that come discarded)
ALL_FLAGGED = (1, PASS, "damar: separate: the 2 overlaps of reads %d and %d all come discarded or contained\n")


def kind_of(opts):
    return 1 if ("-T1" in opts or ("-T" in opts and opts[opts.index("-T") + 1] == "1")) else 0


def track_of(opts):
    return opts[opts.index("-r") + 1] if "-r" in opts else "rep"


def load_cases(what="cases"):
    """the tool cases, ("errors") the runs that end with a message, or ("plants") what synth.las plants"""
    return json.load(open(os.path.join(SDIR, "cases.json")))[what]


def tracks(inp):
    """{name: (anno, data)} of an input: rep is the repeat track the LAfilter fixtures hold for a real file (LArepeat's),
    rep2 its trim track; the planted file has two of its own"""
    if inp == "ssynth":
        t = np.load(os.path.join(SDIR, "synth_tracks.npz"))
        return {k: (t[k + "_anno"], t[k + "_data"]) for k in ("rep", "rep2")}
    ta, td, ra, rd = fc.tracks(inp)
    return dict(rep=(ra, rd), rep2=(ta, td))


def workdir(tmp, inp):
    db = INPUTS[inp][0]
    for f in ("G.db", ".G.idx", ".G.bps"):
        shutil.copy(os.path.join(GOLDEN, db, f), os.path.join(tmp, f))
    shutil.copy(os.path.join(GOLDEN, INPUTS[inp][1]), os.path.join(tmp, LAS))
    for name, (anno, data) in tracks(inp).items():
        tc.write_track_a2(os.path.join(tmp, ".G." + name), len(anno) - 1, anno, data)
    return tmp


def run_tool(opts, tmp, env_extra=None, timeout_s=None, args=ARGS, drop=(), exe=None):
    cmd = [exe or os.path.join(BIN, "LAseparate")] + list(opts) + list(args)
    if timeout_s:
        cmd = ["timeout", "-k", "10", str(timeout_s)] + cmd
    env = {k: v for k, v in os.environ.items() if k not in drop}
    env.update(env_extra or {})
    return subprocess.run(cmd, cwd=tmp, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


_FLAGS = None


def expected_flags(name):
    """per record of the case's input the flags word the reference's first pass leaves (without OVL_TEMP): its first file
    holds the records without OVL_DISCARD, its second the others with the bit taken off"""
    global _FLAGS
    if _FLAGS is None:
        _FLAGS = np.load(os.path.join(SDIR, "expected.npz"))
    return _FLAGS[name]


def check_output(case, r, tmp):
    """exit status, stdout, stderr and both files of a run against the fixture; on a mismatch of a file, where"""
    assert (r.returncode, r.stdout, r.stderr) == (case["rc"], case["stdout"], case["stderr"])
    got = [tc.md5(os.path.join(tmp, f)) for f in (OUT, OUT2)]
    if got == [case["md5"], case["md5_discard"]]:
        return
    cols = tc.read_records(os.path.join(tmp, LAS))[0]
    want = expected_flags(case.get("same_as", case["name"]))
    for f, sel, flags in ((OUT, (want & DISCARD) == 0, want), (OUT2, (want & DISCARD) != 0, want ^ DISCARD)):
        exp = cols[sel].copy()
        exp[:, 6] = flags[sel]
        have = tc.read_records(os.path.join(tmp, f))[0]
        assert len(have) == len(exp), "%s holds %d records, the reference's %d" % (f, len(have), len(exp))
        bad = np.flatnonzero(np.any(have != exp, axis=1))
        assert len(bad) == 0, "%s differs in %d records, the first %d: %s against %s" % (f, len(bad), bad[0], have[bad[0]], exp[bad[0]])
    assert False, "an output's md5 differs and no record does"


def run_case(case, tmp, env_extra=None, timeout_s=None, drop=()):
    workdir(tmp, case["input"])
    r = run_tool(case["opts"], tmp, env_extra, timeout_s, drop=drop)
    check_output(case, r, tmp)
    return r


def flag_first_pair(path):
    """the first group of exactly two records of a file marked OVL_DISCARD in both: -> (A read, B read)"""
    buf = bytearray(open(path, "rb").read())
    offs, _ = tc.record_offsets(buf)
    cols = tc.read_records(path)[0]
    pair = lambda k: tuple(cols[k, 7:9]) if 0 <= k < len(cols) else None
    i = next(i for i in range(len(cols) - 1) if pair(i) == pair(i + 1) and pair(i + 2) != pair(i) and pair(i - 1) != pair(i))
    for k in (i, i + 1):
        struct.pack_into("<i", buf, offs[k] + 24, int(cols[k, 6]) | DISCARD)
    open(path, "wb").write(buf)
    return int(cols[i, 7]), int(cols[i, 8])


def beyond_limits(m, nrec, maxgroup, maxchains, maxmembers=64):
    """whether a group of nrec records, as the model's dict m has it, is the host routine's under these limits.  (The model
    keeps the best chain alone: a chain of more than maxmembers that is not the best one is not seen here; no fixture has one.)"""
    return nrec > maxgroup or m["nchains"] > maxchains or (nrec <= maxgroup and len(m["best"]) > maxmembers)


def batch_of(path):
    """a .las file as api.pile_chains takes it"""
    b = q_common.read_las(path)
    return {k: b[k] for k in ("pile_off", "pile_aread", "abpos", "aepos", "bbpos", "bepos", "bread", "flags")}


def groups_of(batch):
    """[(first record, records as the model takes them)] of a batch, in file order"""
    out = []
    off = batch["pile_off"]
    for p in range(len(off) - 1):
        g0 = int(off[p])
        for i in range(int(off[p]), int(off[p + 1])):
            if i + 1 == off[p + 1] or batch["bread"][i + 1] != batch["bread"][g0]:
                out.append((g0, [dict(aread=int(batch["pile_aread"][p]), bread=int(batch["bread"][k]), ab=int(batch["abpos"][k]),
                                      ae=int(batch["aepos"][k]), bb=int(batch["bbpos"][k]), be=int(batch["bepos"][k]),
                                      flags=int(batch["flags"][k])) for k in range(g0, i + 1)]))
                g0 = i + 1
    return out


def model_batch(batch, read_len, rep, twidth, kind):
    """the model over every group of a batch: -> (flags per record, [(nchains, best, proper)] per group, the model's dicts)"""
    flags = np.zeros(len(batch["abpos"]), dtype=np.int32)
    groups, full = [], []
    for g0, recs in groups_of(batch):
        m = sm.group(recs, int(read_len[recs[0]["aread"]]), int(read_len[recs[0]["bread"]]), twidth, rep, kind)
        flags[g0:g0 + len(recs)] = m["flags"]
        groups.append((m["nchains"], m["best"][:len(recs)], m["proper"]))
        full.append(m)
    return flags, groups, full


def random_piles(seed=20261021, npiles=60):
    """seeded random piles on tiny2: groups of 1 to 12 records in both orientations whose records follow one another closely
    enough to chain, overlap, nest and leave gaps, and a repeat track of random intervals.  -> (batch, read_len, (anno, data))"""
    rng = np.random.default_rng(seed)
    rl = q_common.db_read_len("tiny2")
    nreads = len(rl)
    cols = {k: [] for k in ("abpos", "aepos", "bbpos", "bepos", "bread", "flags")}
    off, aread = [0], []
    for a in rng.choice(nreads, npiles, replace=False):
        for b in sorted(rng.choice(nreads, int(rng.integers(1, 6)), replace=False)):
            n = int(rng.integers(1, 13))
            pa, pb = int(rng.integers(0, 3000)), int(rng.integers(0, 3000))
            for _ in range(n):
                la = int(rng.integers(300, 5000))
                lb = max(1, la + int(rng.integers(-200, 200)))
                step = int(rng.choice([-2500, -900, 0, 90, 101, 800, 4000, 5001, 12000, 31000]))
                ab, bb = max(0, pa + step + int(rng.integers(-50, 50))), max(0, pb + step + int(rng.integers(-50, 50)))
                for k, v in zip(cols, (ab, ab + la, bb, bb + lb, int(b), int(rng.integers(0, 2)))):
                    cols[k].append(v)
                pa, pb = ab + la, bb + lb
        off.append(len(cols["abpos"]))
        aread.append(int(a))
    anno, data = [0], []
    for r in range(nreads):
        at = 0
        for _ in range(int(rng.integers(0, 4))):
            at += int(rng.integers(0, 4000))
            e = at + int(rng.integers(1, 3000))
            data += [at, e]
            at = e if rng.random() < 0.8 else at          # now and then an interval that begins where the last one did
        anno.append(4 * len(data))
    batch = dict(pile_off=np.array(off, dtype=np.int64), pile_aread=np.array(aread, dtype=np.int32),
                 **{k: np.array(v, dtype=np.int32) for k, v in cols.items()})
    return batch, rl, (np.array(anno, dtype=np.uint64), np.array(data, dtype=np.int32))
