"""What tests/test_correct_host.py, tests/test_gpu_correct.py and tests/golden/make_correct_golden.py share: the inputs of
the LAcorrect fixtures (tests/golden/correct/), the working directory of a case, how a command's output is compared with the
fixtures, and the seeded random tiles."""
import functools
import json
import os
import shutil
import subprocess

import numpy as np

import fix_common as fc
import q_common
import trim_common as tc

ROOT = fc.ROOT
GOLDEN = fc.GOLDEN
CDIR = os.path.join(GOLDEN, "correct")
BIN = fc.BIN
LAS = "in.las"
OUT = "out"
TW = 100
LOW_COLS = 110            # what the tests lower the kernel's column limit to (DAMAR_TEST_CORRECT_COLS)

INPUTS = dict(q_common.INPUTS, csynth=("tiny2", "correct/synth.las"))
# -r lists on the larger files: reads with piles, two or three each; none on `long`, whose whole-read alignment alone
# takes seconds per read
R_LISTS = dict(fusion=(3, 40, 77), tandem=(5, 60), tiny2=(2, 50, 101), tiny_s=(97, 100))
WHOLE = ("tiny_s", "tiny2", "csynth")
VARIANTS = [("plain", []), ("j3", ["-j", "3"]), ("r", ["-r", "ids.txt"]), ("b2", ["-b", "2"]), ("q", ["-q", "q2"]), ("v", ["-v"]),
            ("rj", ["-r", "ids.txt", "-j", "2", "-v"])]
ERRORS = (("no_track", ["-q", "nosuch", "G", LAS, OUT]), ("no_las", ["G", "nosuch.las", OUT]), ("bad_option", ["-z", "G", LAS, OUT]),
          ("x_1", ["-x", "1", "G", LAS, OUT]), ("no_args", ["G", LAS]), ("no_ids", ["-r", "nosuch.txt", "G", LAS, OUT]))


def load_cases(what="cases"):
    return json.load(open(os.path.join(CDIR, "cases.json")))[what]


def expected(name):
    return np.load(os.path.join(CDIR, "expected_%s.npz" % name))


def q_track(inp):
    if inp == "csynth":
        t = np.load(os.path.join(CDIR, "synth_q.npz"))
        return t["q_anno"], t["q_data"]
    t = q_common.expected(fc.Q_OF[inp])
    return t["q_anno"], t["q_data"]


def workdir(tmp, inp):
    """the database, the input, its q track under two names and the -r list in tmp"""
    db = INPUTS[inp][0]
    for f in ("G.db", ".G.idx", ".G.bps"):
        shutil.copy(os.path.join(GOLDEN, db, f), os.path.join(tmp, f))
    shutil.copy(os.path.join(GOLDEN, INPUTS[inp][1]), os.path.join(tmp, LAS))
    anno, data = q_track(inp)
    for name in ("q", "q2"):
        tc.write_track_a2(os.path.join(tmp, ".G." + name), len(anno) - 1, anno, data)
    ids = R_LISTS.get(inp) or tuple(int(a) for a in q_common.read_las(os.path.join(tmp, LAS))["pile_aread"][::5])
    open(os.path.join(tmp, "ids.txt"), "w").write("".join("%d\n" % i for i in ids))
    return tmp


def run_tool(opts, tmp, env_extra=None, timeout_s=None, args=("G", LAS, OUT), drop=(), exe=None):
    cmd = [exe or os.path.join(BIN, "LAcorrect")] + list(opts) + list(args)
    if timeout_s:
        cmd = ["timeout", "-k", "10", str(timeout_s)] + cmd
    env = {k: v for k, v in os.environ.items() if k not in drop}
    env.update(env_extra or {})
    return subprocess.run(cmd, cwd=tmp, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def out_files(tmp):
    return sorted(f for f in os.listdir(tmp) if f.startswith(OUT + ".") and f.endswith(".fasta"))


def check_output(case, r, tmp):
    """exit status, stdout, stderr and every output file of a run against the fixture; on a mismatch, where"""
    assert (r.returncode, r.stdout, r.stderr) == (case["rc"], case["stdout"], case["stderr"])
    assert out_files(tmp) == sorted(case["md5"])
    exp = None
    for f in out_files(tmp):
        if fc.md5(os.path.join(tmp, f)) == case["md5"][f]:
            continue
        exp = exp if exp is not None else expected(case["name"])
        heads, lens, crcs = fc.digest(open(os.path.join(tmp, f), "rb").read())
        want = [str(h) for h in exp["heads_" + f]]
        assert len(heads) == len(want), "%s holds %d reads, %d expected" % (f, len(heads), len(want))
        for i, (h, w) in enumerate(zip(heads, want)):
            assert h == w, "header %d of %s differs:\n%s\n%s" % (i, f, h[:400], w[:400])
        bad = np.flatnonzero(crcs != exp["crcs_" + f])
        assert len(bad) == 0, "the bases of %s differ" % heads[bad[0]][:80]
        assert False, "the md5 of %s differs and no read does" % f


def run_case(case, tmp, env_extra=None, timeout_s=None, drop=()):
    workdir(tmp, case["input"])
    r = run_tool(case["opts"], tmp, env_extra, timeout_s, drop=drop)
    check_output(case, r, tmp)
    return r


def random_tiles(n=200, seed=20261020):
    """seeded tiles: coverage 1 to 20, a template of 20 to 140 bases, every sequence the template with 0 to 30 %
    differences (substitutions, insertions and deletions alike), 20 bases at the least"""
    rng = np.random.default_rng(seed)
    tiles = []
    for _ in range(n):
        cov, length, rate = int(rng.integers(1, 21)), int(rng.integers(20, 141)), float(rng.uniform(0, 0.3))
        tmpl = rng.integers(0, 4, size=length)
        tile = []
        for _ in range(cov):
            s = []
            for base in tmpl:
                u = rng.random()
                if u < rate / 3:
                    continue
                if u < 2 * rate / 3:
                    s.append(int(rng.integers(0, 4)))
                    s.append(int(base))
                elif u < rate:
                    s.append(int((base + 1 + rng.integers(0, 3)) % 4))
                else:
                    s.append(int(base))
            while len(s) < 20:
                s.append(int(rng.integers(0, 4)))
            tile.append(np.array(s[:140], dtype=np.uint8))
        tiles.append(tile)
    return tiles



@functools.lru_cache(maxsize=None)
def planted_piles():
    """the piles of the planted file as tests/correct_model.py lays them out"""
    import correct_model as cm
    qa, qd = q_track("csynth")
    return cm.piles(q_common.read_las(os.path.join(CDIR, "synth.las")), cm.db_reads(os.path.join(GOLDEN, "tiny2")), qa, qd)


@functools.lru_cache(maxsize=None)
def model_calls(which):
    """the model's consensus of every tile of `which` ("random" or "planted"): (tiles, [(bases, added, facts)])"""
    import correct_model as cm
    tiles = random_tiles() if which == "random" else [t for p in planted_piles() for t in p["tiles"]]
    return tiles, [cm.consensus(t) for t in tiles]


def over(facts, limits):
    """whether the kernel at limits = (seg, cols, cells) has to leave a tile with these facts to the host routine"""
    return facts["seg"] > limits[0] or facts["cols"] > limits[1] or facts["cells"] > limits[2]
