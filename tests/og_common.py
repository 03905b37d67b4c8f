"""What tests/test_og_host.py, tests/test_gpu_og.py and tests/golden/make_og_golden.py share: the cases of the OGbuild
fixtures (tests/golden/og/), the working directory of a case, and how a command's output is compared with the fixtures."""
import glob
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np

import filter_common as fc
import q_common
import trim_common as tc

ROOT = q_common.ROOT
GOLDEN = q_common.GOLDEN
ODIR = os.path.join(GOLDEN, "og")
BIN = q_common.BIN
LAS = tc.LAS
OUT = "og.out"
MAXDEG_TEST = 8                         # DAMAR_TEST_GRAPH_MAXDEG in the tests: what the planted degrees are sized by

REAL = ("tiny2", "fusion")              # filtered by the reference's LAfilter under the plan's options
DB_OF = dict(tiny2="tiny2", fusion="fusion", synth="tiny2", noedge="tiny2", neg="tiny2")
VARIANTS = [("def", []), ("gml", ["-f", "gml"]), ("tgf", ["-f", "tgf"]), ("s", ["-s"]), ("s_gml", ["-s", "-f", "gml"]), ("s_tgf", ["-s", "-f", "tgf"]),
            ("c1", ["-c", "1"]), ("call", ["-c", "-1"]), ("c2ovh", ["-c", "2", "-p", "ovh"]), ("t2", ["-t", "trim2"])]
CASES = ([("%s_%s" % (v, inp), inp, o) for inp in REAL + ("synth",) for v, o in VARIANTS] +
         [("def_noedge", "noedge", []), ("s_noedge", "noedge", ["-s"]), ("def_neg", "neg", [])])
ERRORS = (("bad_format", ["-f", "dot", "G", LAS, OUT]), ("bad_prio", ["-p", "len", "G", LAS, OUT]), ("no_track", ["-t", "nosuch", "G", LAS, OUT]),
          ("no_las", ["G", "nosuch.las", OUT]), ("no_args", ["G", LAS]), ("bad_option", ["-x", "G", LAS, OUT]), ("bad_c", ["-c", "-2", "G", LAS, OUT]))


def load_cases(what="cases"):
    return json.load(open(os.path.join(ODIR, "cases.json")))[what]


def tracks(inp):
    """(trim anno, trim data, second track's anno, its data) of an input"""
    if inp in REAL:
        t = tc.expected(fc.TRIM_OF[inp])
        return t["trim_anno"], t["trim_data"], t["trim_anno"], t["trim_data"]
    t = np.load(os.path.join(ODIR, "synth_tracks.npz"))
    return t["trim_anno"], t["trim_data"], t["trim2_anno"], t["trim2_data"]


def workdir(tmp, inp):
    """the database, the input and both trim tracks of a case in tmp"""
    for f in ("G.db", ".G.idx", ".G.bps"):
        shutil.copy(os.path.join(GOLDEN, DB_OF[inp], f), os.path.join(tmp, f))
    shutil.copy(os.path.join(ODIR, inp + ".las"), os.path.join(tmp, LAS))
    ta, td, ua, ud = tracks(inp)
    tc.write_track_a2(os.path.join(tmp, ".G.trim"), len(ta) - 1, ta, td)
    tc.write_track_a2(os.path.join(tmp, ".G.trim2"), len(ua) - 1, ua, ud)
    return tmp


def run_tool(args, tmp, env_extra=None, timeout_s=None, tool=None):
    cmd = [tool or os.path.join(BIN, "OGbuild")] + list(args)
    if timeout_s:
        cmd = ["timeout", "-k", "10", str(timeout_s)] + cmd
    env = dict(os.environ)
    env.update(env_extra or {})
    return subprocess.run(cmd, cwd=tmp, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def outputs(tmp):
    """{file name: md5} of what a run wrote: the graph, or one file per component"""
    return {os.path.basename(p): hashlib.md5(open(p, "rb").read()).hexdigest() for p in sorted(glob.glob(os.path.join(tmp, OUT + "*")))}


def check_output(case, r, tmp):
    assert r.returncode == case["rc"], (case["name"], r.returncode, r.stderr[-2000:])
    assert r.stdout == case["stdout"], "%s: stdout differs\n%s\n--- expected\n%s" % (case["name"], r.stdout[-3000:], case["stdout"][-3000:])
    assert r.stderr == case["stderr"], "%s: stderr differs\n%s\n--- expected\n%s" % (case["name"], r.stderr[-3000:], case["stderr"][-3000:])
    got = outputs(tmp)
    assert got == case["md5"], "%s: the graph files differ: %s" % (case["name"], sorted(set(got.items()) ^ set(case["md5"].items())))
    kept = os.path.join(ODIR, "expected_%s.txt" % case["name"])
    if os.path.exists(kept) and os.path.exists(os.path.join(tmp, OUT)):
        assert open(os.path.join(tmp, OUT)).read() == open(kept).read()


def run_case(case, tmp, env_extra=None, timeout_s=None):
    workdir(tmp, case["input"])
    r = run_tool(case["opts"] + ["G", LAS, OUT], tmp, env_extra, timeout_s)
    check_output(case, r, tmp)
    return r


EDGE_FIELDS = ("loff", "roff", "left", "right", "status")
COUNTERS = ("cnt_left", "cnt_right", "edges", "redges", "symdiscard", "parallel", "removed", "neg_rec")


def same_edges(x, y):
    for k in EDGE_FIELDS:
        assert np.array_equal(x[k], y[k]), k
    for k in COUNTERS:
        assert x[k] == y[k], (k, x[k], y[k])


def random_las(path, rl, seed=20261021):
    """60 seeded piles on the reads of tiny2 for a trim of (100, length - 100): records at either border of A's interval or
    inside it, runs of one B read of 1 to 4 records, containments, complements, every flag the tool looks at"""
    import struct
    rng = np.random.default_rng(seed)
    body, n = [], 0
    for a in sorted(int(x) for x in rng.choice(len(rl), size=60, replace=False)):
        alen, recs = int(rl[a]), []
        for _ in range(int(rng.integers(1, 140))):
            b = a if rng.integers(25) == 0 else int(rng.integers(len(rl)))
            blen = int(rl[b])
            for _ in range(int(rng.integers(1, 5)) if rng.integers(6) == 0 else 1):
                comp = int(rng.integers(2))
                tbb, tbe = 100, blen - 100
                kind = int(rng.integers(6))
                ab = 100 if kind in (0, 2, 3) else int(rng.integers(101, alen - 700))
                ae = alen - 100 if kind in (1, 2) else int(rng.integers(ab + 300, alen - 100))
                span = ae - ab
                if kind == 4 or span >= tbe - tbb:            # B contained
                    bb, be = tbb, tbe
                elif kind in (0, 3):
                    bb = tbb + int(rng.integers(0, 3)) * int(rng.integers(1, 200))
                    be = min(bb + span, tbe)
                else:
                    be = tbe - int(rng.integers(0, 3)) * int(rng.integers(1, 200))
                    bb = max(be - span, tbb)
                flags = comp | (int(rng.choice([0x2, 0x100, 0x102, 0x80000, 0x8002])) if rng.integers(5) == 0 else 0)
                recs.append((b, ab, struct.pack("<10i", 0, int(rng.integers(0, 400)), ab, bb, ae, be, flags, a, b, 0)))
        recs.sort(key=lambda x: (x[0], x[1]))
        body += [x[2] for x in recs]
        n += len(recs)
    open(path, "wb").write(struct.pack("<qi", n, 100) + b"".join(body))
    return n


def trim_pairs(anno, data):
    """get_trim of every read"""
    return fc.trim_pairs(anno, data)


def random_workdir(tmp):
    """tiny2 with random.las (random_las) and the track rtrim it was made for -> (db, las, read lengths, trim pairs)"""
    rl = q_common.db_read_len("tiny2")
    workdir(tmp, "synth")
    las = os.path.join(tmp, "random.las")
    assert random_las(las, rl) > 1000
    data = np.array([v for r in range(len(rl)) for v in (100, int(rl[r]) - 100)], dtype=np.int32)
    anno = np.arange(len(rl) + 1, dtype=np.uint64) * 8
    tc.write_track_a2(os.path.join(tmp, ".G.rtrim"), len(rl), anno, data)
    return os.path.join(tmp, "G"), las, rl, data


def model_of(las, rl, pairs):
    import og_model
    return og_model.build(tc.read_records(las)[0], rl, pairs)
