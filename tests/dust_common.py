"""What tests/test_dust_host.py, tests/test_gpu_dust.py and tests/golden/make_dust_golden.py share: the option sets, the
fixtures of tests/golden/dust/, the seeded synthetic reads and how a command's tracks are compared."""
import json
import os
import random
import shutil
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DUST = os.path.join(GOLDEN, "dust")
BIN = os.path.join(ROOT, "damar_amd", "bin")

# name -> the command's options.  -m1 is an error of the reference (its test is on -m minus one), recorded as such; -m2 is
# the smallest it takes.
OPTION_SETS = {
    "default": [],
    "w32": ["-w32"],
    "w16t15": ["-w16", "-t1.5"],
    "t35": ["-t3.5"],
    "m1": ["-m1"],
    "m2": ["-m2"],
    "m30": ["-m30"],
    "b": ["-b"],
    "w80": ["-w80"],
}
ERROR_SETS = ("m1",)
HOST_SETS = ("b", "w80")                       # what the kernel leaves to the host routine
INTEGER_SETS = [k for k in OPTION_SETS if k not in ERROR_SETS and k != "b"]
ERROR_RUNS = {"noarg": [], "w0": ["-w0", "P"], "t0": ["-t0", "P"], "m0": ["-m0", "P"], "unknown": ["-q", "P"]}
DB_FILES = ("P.db", ".P.idx", ".P.bps")
MASK_DUST = os.path.join(GOLDEN, "mask_dust")


def kwargs_of(opts):
    kw = {}
    for o in opts:
        if o == "-b":
            kw["biased"] = True
        elif o[:2] == "-w":
            kw["window"] = int(o[2:])
        elif o[:2] == "-t":
            kw["thresh"] = float(o[2:])
        elif o[:2] == "-m":
            kw["minlen"] = int(o[2:])
    return kw


def db_reads(dbdir, root):
    """-> (the reads of a database as uint8 arrays of 0..3, its four base frequencies as float32)"""
    idx = np.fromfile(os.path.join(dbdir, ".%s.idx" % root), dtype=np.uint8)
    nreads = int(idx[:4].view("<i4")[0])
    freq = idx[4:20].view("<f4").copy()
    recs = idx[88:88 + 32 * nreads].reshape(nreads, 32)
    bps = np.fromfile(os.path.join(dbdir, ".%s.bps" % root), dtype=np.uint8)
    reads = []
    for r in recs:
        rlen = int(r[0:4].copy().view("<i4")[0])
        boff = int(r[8:16].copy().view("<i8")[0])
        b = bps[boff:boff + (rlen + 3) // 4]
        reads.append(np.stack([(b >> 6) & 3, (b >> 4) & 3, (b >> 2) & 3, b & 3], axis=1).reshape(-1)[:rlen].astype(np.uint8))
    return reads, freq


def block_ranges(dbdir, root):
    """first read of every block and the end, from the stub"""
    lines = open(os.path.join(dbdir, root + ".db")).read().split("\n")
    at = [i for i, ln in enumerate(lines) if ln.startswith("blocks =")]
    if not at:
        return None
    n = int(lines[at[0]].split("=")[1])
    return [int(lines[at[0] + 2 + i].split()[0]) for i in range(n + 1)]


def track_intervals(anno, data):
    """the bytes of a .anno / .data pair -> a list of [n, 2] arrays"""
    nreads, size = np.frombuffer(anno[:8], dtype="<i4")
    assert size == 8
    offs = np.frombuffer(anno[8:], dtype="<i8")
    assert len(offs) == nreads + 1 and offs[-1] == len(data)
    d = np.frombuffer(data, dtype="<i4")
    return [d[offs[i] // 4:offs[i + 1] // 4].reshape(-1, 2) for i in range(nreads)]


def track_bytes(ivs):
    offs = np.zeros(len(ivs) + 1, dtype="<i8")
    offs[1:] = np.cumsum([8 * len(v) for v in ivs])
    data = np.concatenate([np.asarray(v, dtype="<i4").reshape(-1) for v in ivs] + [np.zeros(0, dtype="<i4")])
    return np.array([len(ivs), 8], dtype="<i4").tobytes() + offs.tobytes(), data.astype("<i4").tobytes()


def expected(name):
    """the recorded track files of one run: {file name: bytes}"""
    z = np.load(os.path.join(DUST, "expected.npz"))
    return {k.split("/", 1)[1]: z[k].tobytes() for k in z.files if k.split("/", 1)[0] == name}


def cases():
    return json.load(open(os.path.join(DUST, "cases.json")))


def planted_workdir(tmp, files=DB_FILES, src=DUST):
    for f in files:
        shutil.copy(os.path.join(src, f), os.path.join(tmp, f))
    return tmp


def run_dbdust(args, cwd, env_extra, timeout_s=None):
    cmd = [os.path.join(BIN, "DBdust")] + list(args)
    if timeout_s:
        cmd = ["timeout", "-k", "10", str(timeout_s)] + cmd
    return subprocess.run(cmd, cwd=cwd, env=dict(os.environ, **env_extra), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def dust_files(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if ".dust." in f}


def _stats(stderr):
    w = stderr.split()
    return dict(zip(w[1::2], map(int, w[2::2])))


def check_option_set(name, tmp, env_extra, timeout_s=None):
    """one option set on the planted database's block and on the database itself against the record -> the runs' counters"""
    planted_workdir(tmp)
    out, stats = {}, []
    for blk in ("P.1", "P"):
        r = run_dbdust(OPTION_SETS[name] + [blk], tmp, dict(env_extra, DAMAR_DUST_STATS="1"), timeout_s)
        if name in ERROR_SETS:
            out[blk + ".stderr"] = ("%s\nrc %d\n" % (r.stderr, r.returncode)).encode()
        else:
            assert r.returncode == 0, r.stderr
            stats.append(_stats(r.stderr))
    out.update(dust_files(tmp))
    assert out == expected(name), name
    return stats


def check_mask_dust(tmp, env_extra, timeout_s=None):
    planted_workdir(tmp, ("G.db", ".G.idx", ".G.bps"), MASK_DUST)
    for blk in ("G.1", "G.2"):
        r = run_dbdust([blk], tmp, env_extra, timeout_s)
        assert r.returncode == 0, r.stderr
    assert dust_files(tmp) == expected("mask_dust")


def check_append(tmp, env_extra, timeout_s=None):
    """the track of the database before two reads were added, then the command on the grown database, and once more"""
    planted_workdir(tmp, ("A.db", ".A.idx", ".A.bps"))
    for f, b in expected("append_before").items():
        open(os.path.join(tmp, f), "wb").write(b)
    r = run_dbdust(["A"], tmp, dict(env_extra, DAMAR_DUST_STATS="1"), timeout_s)
    assert r.returncode == 0, r.stderr
    assert dust_files(tmp) == expected("append_after")
    r2 = run_dbdust(["A"], tmp, env_extra, timeout_s)               # nothing to add: untouched
    assert r2.returncode == 0 and dust_files(tmp) == expected("append_after")
    return _stats(r.stderr)


def synthetic_reads(n=300, seed=20240613, lo=200, hi=6200):
    """reads mixed from random, short-period, two-letter and near-homopolymer stretches"""
    rng = random.Random(seed)
    reads = []
    for _ in range(n):
        length = rng.randrange(lo, hi)
        s = []
        while len(s) < length:
            mode, run = rng.randrange(4), rng.randrange(10, 160)
            if mode == 0:
                s += [rng.randrange(4) for _ in range(run)]
            elif mode == 1:
                unit = [rng.randrange(4) for _ in range(rng.randrange(1, 7))]
                s += [rng.randrange(4) if rng.randrange(12) == 0 else unit[k % len(unit)] for k in range(run)]
            elif mode == 2:
                x, y = rng.randrange(4), rng.randrange(4)
                s += [x if rng.randrange(3) else y for _ in range(run)]
            else:
                x = rng.randrange(4)
                s += [x if rng.randrange(8) else rng.randrange(4) for _ in range(run)]
        reads.append(np.array(s[:length], dtype=np.uint8))
    return reads
