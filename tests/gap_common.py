"""What tests/test_gap_host.py, tests/test_gpu_gap.py and tests/golden/make_gap_golden.py share: the cases of the LAgap
fixtures (tests/golden/gap/), the working directory of a case, and how a command's output is compared with the fixtures."""
import json
import os
import shutil
import subprocess

import numpy as np

import q_common
import trim_common as tc

ROOT = q_common.ROOT
GOLDEN = q_common.GOLDEN
GDIR = os.path.join(GOLDEN, "gap")
BIN = q_common.BIN
LAS = tc.LAS
OUT = tc.OUT
TW = 100

INPUTS = dict(q_common.INPUTS, gsynth=("tiny2", "gap/synth.las"))
# the trim track of a real input: what the LAtrim fixtures hold for it; the planted file's tracks: tests/golden/gap/
TRIM_OF = dict(tiny2="def_tiny2", tandem="def_tandem", fusion="def_fusion", long="def_long", tiny_s="def_tiny_s")
EX_TRACK = "ex"                         # the -e track: the planted file's own, a real file's trim track under that name

VARIANTS = [("def", []), ("p", ["-p"]), ("s100", ["-s", "100"]), ("s300", ["-s", "300"]), ("t", ["-t", "trim"]),
            ("tps", ["-t", "trim", "-p", "-s", "300"]), ("tL", ["-t", "trim", "-L"]), ("e", ["-e", EX_TRACK])]
# name, input, options
REAL = ("tiny2", "fusion", "tandem", "long", "tiny_s")       # the inputs whose trim tracks the LAtrim fixtures hold
CASES = ([("%s_%s" % (v, inp), inp, o) for inp in REAL for v, o in VARIANTS] +
         [("%s_synth" % v, "gsynth", o) for v, o in VARIANTS] +
         [("es_synth", "gsynth", ["-e", EX_TRACK, "-s", "300"]), ("R_synth", "gsynth", ["-R", EX_TRACK])])
ERRORS = (("no_e_track", ["-e", "nosuch", "G", LAS, OUT]), ("no_t_track", ["-t", "nosuch", "G", LAS, OUT]),
          ("no_R_track", ["-R", "nosuch", "G", LAS, OUT]), ("no_las", ["G", "nosuch.las", OUT]), ("no_args", ["G", LAS]),
          ("bad_option", ["-x", "G", LAS, OUT]))
# this project's own: the reference's experimental chimer code is not built
NO_CHIMER = (1, "", "LAgap: -C (chimer detection) is not supported\n")
BIG = "fusion"                          # the largest real fixture file


def host_piles_of(inp):
    """the piles damar_pile_gaps may leave to the host routine on an input: the one pile the planted file holds with more
    events than the kernel's slot, and none anywhere else"""
    return 1 if inp == "gsynth" else 0


def opts_to_kwargs(opts):
    """the options of a case as api.gap_las takes them"""
    names = {"-s": ("stitch", int), "-t": ("trim", str), "-e": ("exclude", str), "-R": ("repeats", str)}
    kw, i = {}, 0
    while i < len(opts):
        if opts[i] == "-p":
            kw["purge"] = True
        elif opts[i] in names:
            kw[names[opts[i]][0]] = names[opts[i]][1](opts[i + 1])
            i += 1
        i += 1
    return kw


def load_cases(what="cases"):
    """the tool cases, ("errors") the runs that end with a message, or ("plants") what synth.las plants"""
    return json.load(open(os.path.join(GDIR, "cases.json")))[what]


def expected(name):
    return np.load(os.path.join(GDIR, "expected_%s.npz" % name))


def tracks(inp):
    """(trim anno, trim data, exclude anno, exclude data) of an input"""
    if inp == "gsynth":
        t = np.load(os.path.join(GDIR, "synth_tracks.npz"))
        return t["trim_anno"], t["trim_data"], t["ex_anno"], t["ex_data"]
    t = tc.expected(TRIM_OF[inp])
    return t["trim_anno"], t["trim_data"], t["trim_anno"], t["trim_data"]


def workdir(tmp, inp):
    """the database, the input and both tracks of a case in tmp"""
    db = INPUTS[inp][0]
    for f in ("G.db", ".G.idx", ".G.bps"):
        shutil.copy(os.path.join(GOLDEN, db, f), os.path.join(tmp, f))
    shutil.copy(os.path.join(GOLDEN, INPUTS[inp][1]), os.path.join(tmp, LAS))
    ta, td, ea, ed = tracks(inp)
    tc.write_track_a2(os.path.join(tmp, ".G.trim"), len(ta) - 1, ta, td)
    tc.write_track_a2(os.path.join(tmp, ".G." + EX_TRACK), len(ea) - 1, ea, ed)
    return tmp


def run_tool(opts, tmp, env_extra=None, timeout_s=None, args=("G", LAS, OUT), drop=()):
    cmd = [os.path.join(BIN, "LAgap")] + list(opts) + list(args)
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


def lacheck(tmp):
    return subprocess.run([os.path.join(BIN, "LAcheck"), "-p", "G", OUT], cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True)


def pile_arrays(path):
    """a .las file as api.pile_gaps takes it: (pile_off, pile_aread, abpos, aepos, bbpos, bepos, bread, flags)"""
    cols = tc.read_records(path)[0]
    aread = cols[:, 7]
    starts = np.flatnonzero(np.concatenate([[True], aread[1:] != aread[:-1]])) if len(aread) else np.zeros(0, dtype=np.int64)
    off = np.concatenate([starts, [len(aread)]]).astype(np.int64)
    return off, aread[starts].astype(np.int32), cols[:, 2], cols[:, 4], cols[:, 3], cols[:, 5], cols[:, 8], cols[:, 6]
