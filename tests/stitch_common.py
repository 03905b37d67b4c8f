"""What tests/test_stitch_host.py, tests/test_gpu_stitch.py and tests/golden/make_stitch_golden.py share: the cases of the
LAstitch fixtures (tests/golden/stitch/), the working directory of a case, and how a command's output and the trace pairs
of a box are compared with the fixtures."""
import json
import os
import shutil
import subprocess

import numpy as np

import q_common
import trim_common as tc

ROOT = q_common.ROOT
GOLDEN = q_common.GOLDEN
SDIR = os.path.join(GOLDEN, "stitch")
BIN = q_common.BIN
LAS = tc.LAS
OUT = tc.OUT
TW = 100
OFFSETS = (0, 1, 50, 99)                # where a box begins in its first trace interval

INPUTS = dict(q_common.INPUTS, ssynth=("tiny2", "stitch/synth.las"))
LC_TRACK = "lc"                         # the track the generator writes for the -t cases (synth's reads)

# name, input, options
CASES = [
    ("def_tiny2", "tiny2", []), ("def_fusion", "fusion", []), ("p_fusion", "fusion", ["-p"]), ("f150_tiny2", "tiny2", ["-f", "150"]),
    ("L_tiny2", "tiny2", ["-L"]),
    ("synth", "ssynth", []), ("synth_p", "ssynth", ["-p", "-v"]), ("synth_f150", "ssynth", ["-f", "150"]),
    ("synth_f0", "ssynth", ["-f", "0"]), ("synth_L", "ssynth", ["-L"]),
    ("synth_t", "ssynth", ["-t", LC_TRACK]), ("synth_t_d", "ssynth", ["-t", LC_TRACK, "-d", "0.6"]),
    ("synth_wide", "ssynth", ["-f", "250", "-a", "100"]), ("synth_far", "ssynth", ["-f", "2400"]),
    ("synth_t_r", "ssynth", ["-p", "-t", LC_TRACK, "-r", LC_TRACK, "-m", "50", "-M", "100", "-l", "400", "-d", "0.2"]),
]
# which expectation of a plant (cases.json "plants": expect) a case of the planted file is held to; -p cases: the md5 alone
PLANT_KEY = dict(synth="def", synth_L="def", synth_f150="f150", synth_f0="f0", synth_t="t", synth_t_d="td", synth_wide="wide",
                 synth_far="far")
ERRORS = (("no_track", ["-t", "nosuch", "G", LAS, OUT]), ("no_las", ["G", "nosuch.las", OUT]), ("no_args", ["G", LAS]),
          ("bad_option", ["-x", "G", LAS, OUT]))


def opts_to_kwargs(opts):
    """the options of a case as api.stitch_las takes them"""
    names = {"-f": ("fuzz", int), "-t": ("track", str), "-r": ("repeats", str), "-a": ("anchor", int), "-m": ("merge", int),
             "-l": ("min_len", int), "-M": ("min_merge", int), "-d": ("gap_diff", float)}
    kw, i = {}, 0
    while i < len(opts):
        if opts[i] == "-p":
            kw["purge"] = True
        elif opts[i] in names:
            kw[names[opts[i]][0]] = names[opts[i]][1](opts[i + 1])
            i += 1
        i += 1
    return kw


def check_plants(case, cols, st):
    """a case of the planted file: every planted group ends up as its plant says, and the run's counters show that the
    branches the plants are there for were taken: Check_Bridge refusals, widened joints, candidates left without a box"""
    key = PLANT_KEY[case["name"]]
    plants = load_cases("plants")
    for tag, pl in plants.items():
        rows = np.flatnonzero((cols[:, 7] == pl["aread"]) & (cols[:, 8] == pl["bread"]))
        assert len(rows) == pl["pieces"], tag
        gone = int(np.sum((cols[rows, 6] & 0x82) == 0x82))
        assert gone == pl["expect"][key], "%s: %d records of plant %s stitched away, planted %d" % (case["name"], gone, tag, pl["expect"][key])
    count = lambda what: sum(1 for pl in plants.values() if key in pl.get(what, []))
    assert st["stitched"] + st["stitched_lc"] == sum(pl["expect"][key] for pl in plants.values())
    assert (st["refused"], st["widened"], st["no_box"]) == (count("refused"), count("widened"), count("no_box")), (case["name"], st)
    assert st["candidates"] == st["boxes"] + st["no_box"] and st["boxes"] == st["stitched"] + st["stitched_lc"] + st["refused"]
    return plants


def load_cases(what="cases"):
    """the tool cases, ("errors") the runs that end with a message, or ("plants") what synth.las plants"""
    return json.load(open(os.path.join(SDIR, "cases.json")))[what]


def expected(name):
    return np.load(os.path.join(SDIR, "expected_%s.npz" % name))


def lc_track():
    t = np.load(os.path.join(SDIR, "lc_track.npz"))
    return t["anno"], t["data"]


def workdir(tmp, inp):
    """the database and the input of a case in tmp, and the track of the -t cases"""
    db = INPUTS[inp][0]
    for f in ("G.db", ".G.idx", ".G.bps"):
        shutil.copy(os.path.join(GOLDEN, db, f), os.path.join(tmp, f))
    shutil.copy(os.path.join(GOLDEN, INPUTS[inp][1]), os.path.join(tmp, LAS))
    if inp == "ssynth":
        anno, data = lc_track()
        tc.write_track_a2(os.path.join(tmp, ".G." + LC_TRACK), len(anno) - 1, anno, data)
    return tmp


def run_tool(opts, tmp, env_extra=None, timeout_s=None, args=("G", LAS, OUT), drop=()):
    cmd = [os.path.join(BIN, "LAstitch")] + list(opts) + list(args)
    if timeout_s:
        cmd = ["timeout", "-k", "10", str(timeout_s)] + cmd
    env = {k: v for k, v in os.environ.items() if k not in drop}
    env.update(env_extra or {})
    return subprocess.run(cmd, cwd=tmp, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def check_output(case, r, out):
    tc.check_output(case, expected(case["name"]), r, out)


def run_case(case, tmp, env_extra=None, timeout_s=None, drop=()):
    workdir(tmp, case["input"])
    r = run_tool(case["opts"], tmp, env_extra, timeout_s, drop=drop)
    check_output(case, r, os.path.join(tmp, OUT))
    return r


def lacheck(tmp, sort_order):
    """bin/LAcheck on a case's output: the pass-through points of every record, stitched ones included, and (the real files;
    synth.las plants records out of order) the sort order"""
    return subprocess.run([os.path.join(BIN, "LAcheck"), "-p"] + (["-s"] if sort_order else []) + ["G", OUT], cwd=tmp,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


# ---- the box cases ---------------------------------------------------------------------------------------------------

_TBOXES = None


def tboxes():
    """the box cases, loaded once: m, n, aoff, boff, bases of every box, and the runs -- box run_box[j] beginning run_abpos[j]
    bases into A -- with what the reference's Compute_Alignment(DIFF_TRACE) at spacing 100 made of them: diffs, and the
    values [toff[j], toff[j + 1]) of trace"""
    global _TBOXES
    if _TBOXES is None:
        z = np.load(os.path.join(SDIR, "tboxes.npz"))
        _TBOXES = {k: z[k] for k in z.files}
        for v in _TBOXES.values():
            v.setflags(write=False)
    return _TBOXES


TBOX_MAX = 4096                         # DAMAR_TBOX_MAXLEN: the largest box kernels/box_trace.hip keeps
TB_SMALL = 1024                         # the largest box of its first build
TB_CELLS = 512                          # the ledger cells of a box
_TBOXES_WIDE = None


def tboxes_wide():
    """the box cases of tests/golden/make_box_edges_golden.py, loaded once: the layout of tboxes(), and run_tspace[j], the
    spacing run j was made at"""
    global _TBOXES_WIDE
    if _TBOXES_WIDE is None:
        z = np.load(os.path.join(SDIR, "tboxes_wide.npz"))
        _TBOXES_WIDE = {k: z[k] for k in z.files}
        for v in _TBOXES_WIDE.values():
            v.setflags(write=False)
    return _TBOXES_WIDE


def family_runs(bx, name):
    return np.flatnonzero(bx["family"][bx["run_box"]] == list(bx["families"]).index(name))


def run_spacing(bx, runs):
    """the spacing of every run: a file without run_tspace was made at TW throughout"""
    return bx["run_tspace"][runs] if "run_tspace" in bx else np.full(len(runs), TW, dtype=np.int32)


def run_cells(bx, runs):
    """the ledger cells kernels/box_trace.hip needs for every run: two per interval the box touches and a spare pair"""
    ts = run_spacing(bx, runs).astype(np.int64)
    return 2 * ((bx["run_abpos"][runs] % ts + bx["m"][bx["run_box"][runs]] + ts - 1) // ts + 1)


def trace_runs(bx, runs, limit=TBOX_MAX):
    """api.trace_boxes on the runs, one call per spacing among them, against the fixture: -> (the device's kernel time in ms,
    boxes the host routine did beside the kernel, and how many of the runs lie beyond what the kernel keeps: a side above
    `limit`, or more ledger cells than it has) summed over the calls"""
    from damar_amd import api
    runs = np.asarray(runs)
    spacing = run_spacing(bx, runs)
    kernel_ms, fallback = 0., 0
    for ts in sorted(set(spacing.tolist())):
        part = runs[spacing == ts]
        a, b, at = run_seqs(bx, part)
        diffs, traces = api.trace_boxes(a, b, at, ts)
        check_runs(bx, part, diffs, traces)
        ms, boxes, fb, _ = api.tbox_last()
        assert boxes == len(part)
        kernel_ms += ms["kernel"]
        fallback += fb
    big = np.maximum(bx["m"], bx["n"])[bx["run_box"][runs]]
    return kernel_ms, fallback, int(np.sum((big > limit) | (run_cells(bx, runs) > TB_CELLS)))


def run_seqs(bx, runs):
    a = [bx["bases"][bx["aoff"][i]:bx["aoff"][i] + bx["m"][i]] for i in bx["run_box"][runs]]
    b = [bx["bases"][bx["boff"][i]:bx["boff"][i] + bx["n"][i]] for i in bx["run_box"][runs]]
    return a, b, bx["run_abpos"][runs]


def check_runs(bx, runs, diffs, traces):
    assert len(diffs) == len(runs) and len(traces) == len(runs)
    for j, r in enumerate(runs):
        i = bx["run_box"][r]
        what = "run %d: box %d (%d x %d) at %d" % (r, i, bx["m"][i], bx["n"][i], bx["run_abpos"][r])
        want = bx["trace"][bx["toff"][r]:bx["toff"][r + 1]]
        assert int(diffs[j]) == int(bx["diffs"][r]), "%s: %d differences against %d" % (what, diffs[j], bx["diffs"][r])
        assert len(traces[j]) == len(want), "%s: %d values against %d" % (what, len(traces[j]), len(want))
        assert np.array_equal(traces[j], want), "%s: the pairs part ways: %s against %s" % (what, traces[j], want)
