"""What tests/test_masks_host.py and tests/test_gpu_masks.py share: the fixtures of tests/golden/masks_*/ and how a command's
output is compared with them."""
import json
import os
import re
import shutil
import subprocess

import numpy as np

from conftest import GOLDEN, ROOT

REP = os.path.join(GOLDEN, "masks_rep")
TAN = os.path.join(GOLDEN, "masks_tan")
REP_CASES = json.load(open(os.path.join(REP, "cases.json")))
TAN_CASES = json.load(open(os.path.join(TAN, "cases.json")))
BIN = os.path.join(ROOT, "damar_amd", "bin")


def opts_to_kwargs(opts):
    kw, i = {}, 0
    names = {"-c": ("cov", int), "-h": ("xcov_enter", float), "-l": ("xcov_leave", float), "-m": ("merge_dist", int),
             "-o": ("min_aln_len", int), "-M": ("max_cov", int)}
    while i < len(opts):
        o = opts[i]
        if o == "-C":
            kw["inccov"] = 1
        elif o == "-I":
            kw["inc_identity"] = 1
        elif o in names:
            kw[names[o][0]] = names[o][1](opts[i + 1])
            i += 1
        else:
            i += 1                      # -b -t: where the command writes, not what
        i += 1
    return kw


def stdout_numbers(text):
    out = {}
    hist = [int(m.group(2)) for m in re.finditer(r"^COV (\d+) READS (-?\d+)$", text, re.M)]
    if hist:
        out["histo"] = np.array(hist, dtype=np.int64)
    for key in ("MAX", "AVG_RLEN", "REGIONS", "MERGED", "BASES_TOTAL", "BASES_REPEAT"):
        m = re.search(r"^%s (-?\d+)" % key, text, re.M)
        if m:
            out[key] = int(m.group(1))
    m = re.search(r"^INACTIVE (-?\d+) \((-?\d+)%\) OF (-?\d+)", text, re.M)
    if m:
        out["INACTIVE"] = np.array([int(m.group(1)), int(m.group(2)), int(m.group(3))], dtype=np.int64)
    return out


def case_las(case):
    """the fixture's .las file: G.1.las as the reference's daligner and LAmerge wrote it, or G.1f.las, the same records with
    identity overlaps and discarded records planted by the generator"""
    return case.get("las", "G.1.las")


def rep_workdir(tmp):
    for f in ("G.db", ".G.idx", "G.1.las", "G.1f.las"):
        shutil.copy(os.path.join(REP, f), os.path.join(tmp, f))
    return tmp


def check_repeat_arrays(case, anno, data, exp):
    """data always equals the reference's; anno too, except for -m without -C, where the reference's under-counts by four
    bytes per merge (LArepeat.c:398-399) and ours is checked to be the consistent one instead"""
    assert np.array_equal(data, exp["data"])
    if "-m" in case["opts"] and "-C" not in case["opts"]:
        assert int(anno[0]) == 0 and int(anno[-1]) == 4 * len(data) and np.all(np.diff(anno.astype(np.int64)) >= 0)
        assert np.all(np.diff(anno.astype(np.int64)) % 8 == 0)
        assert int(exp["anno"][-1]) == 4 * len(data) - 4 * int(exp["MERGED"])         # the quirk, as recorded
    else:
        assert np.array_equal(anno, exp["anno"])


def run_larepeat(case, tmp, env_extra, timeout_s=None):
    from damar_amd import api
    rep_workdir(tmp)
    env = dict(os.environ, **env_extra)
    cmd = [os.path.join(BIN, "LArepeat")] + case["opts"] + ["G", case_las(case)]
    if timeout_s:
        cmd = ["timeout", "-k", "10", str(timeout_s)] + cmd
    r = subprocess.run(cmd, cwd=tmp, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    exp = np.load(os.path.join(REP, "expected_%s.npz" % case["name"]))
    t = api.read_track(os.path.join(tmp, "G"), case["track"], case["block"])
    assert (t["version"], t["size"], t["len"]) == (int(exp["version"]), int(exp["size"]), int(exp["len"]))
    check_repeat_arrays(case, t["anno"], t["data"], exp)
    num = stdout_numbers(r.stdout)
    for k in ("REGIONS", "MERGED", "BASES_TOTAL", "BASES_REPEAT", "MAX", "AVG_RLEN"):
        if k in exp.files:
            assert num[k] == int(exp[k]), k
    for k in ("histo", "INACTIVE"):
        if k in exp.files:
            assert np.array_equal(num[k], exp[k]), k


def run_tanmask(case, tmp, env_extra, timeout_s=None):
    for f in ("G.db", ".G.idx"):
        shutil.copy(os.path.join(GOLDEN, case["db"], f), os.path.join(tmp, f))
    las = "Gall.las" if case["whole"] else "G.1.G.1.las"
    shutil.copy(os.path.join(GOLDEN, case["las"]), os.path.join(tmp, las))
    cmd = [os.path.join(BIN, "TANmask"), "-l500", "G", las]
    if timeout_s:
        cmd = ["timeout", "-k", "10", str(timeout_s)] + cmd
    r = subprocess.run(cmd, cwd=tmp, env=dict(os.environ, **env_extra), stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    exp = np.load(os.path.join(TAN, "expected_%s.npz" % case["name"]))
    pre = os.path.join(tmp, ".G.tan" if case["whole"] else ".G.1.tan")
    assert open(pre + ".anno", "rb").read() == exp["anno"].tobytes()
    assert open(pre + ".data", "rb").read() == exp["data"].tobytes()
