#!/usr/bin/env python3
"""Fixtures of TKhomogenize (tests/golden/homogenize/) from the REFERENCE.

Runs only where the reference sources lie (REF_SRC, default /root/reference): LArepeat, LAq and TKhomogenize are compiled
with plain gcc lines into a temporary directory outside the repository, run on .las files this repository already holds
(tests/hom_common.py INPUTS) and on the planted file tests/hom_shapes.py writes, and only data is kept: synth.las,
cases.json (options, exit status, stdout, stderr) and expected_<case>.npz (the input interval track, the trim track where
the case reads one, and the expected anno and data).  Nothing compiled is kept.  The asserts hold the real cases to an
effect worth testing and the planted file to its shapes, and pin tests/hom_model.py to the reference.

    python tests/golden/make_homogenize_golden.py
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
SRC = os.environ.get("REF_SRC", "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import q_common                                        # noqa: E402
import hom_common as hc                                # noqa: E402
import hom_model                                       # noqa: E402
import hom_shapes                                      # noqa: E402
import trim_common                                     # noqa: E402
from make_q_golden import build_tool as build_laq      # noqa: E402

OUT = hc.HDIR
MAX_FILE = 1 << 20


def build_tools(tmp):
    s = lambda *p: os.path.join(SRC, *p)
    cc = ["gcc", "-O3", "-w", "-fno-strict-aliasing", "-I" + SRC]
    subprocess.run(cc + ["-o", os.path.join(tmp, "TKhomogenize"), s("scrub", "TKhomogenize.c"), s("lib", "borders.c"), s("lib", "utils.c"),
                         s("lib", "tracks.c"), s("lib", "pass.c"), s("lib", "compression.c"), s("lib", "trim.c"), s("lib", "read_loader.c"),
                         s("lib.ext", "bitarr.c"), s("db", "DB.c"), s("db", "QV.c"), s("dalign", "align.c"), "-lm", "-lz", "-lpthread"],
                   cwd=tmp, check=True)
    subprocess.run(cc + ["-o", os.path.join(tmp, "LArepeat"), s("scrub", "LArepeat.c"), s("lib", "borders.c"), s("lib", "utils.c"),
                         s("lib", "tracks.c"), s("lib", "pass.c"), s("db", "QV.c"), s("dalign", "align.c"), s("db", "DB.c"),
                         s("lib", "compression.c"), "-lm", "-lz", "-lpthread"], cwd=tmp, check=True)
    return os.path.join(tmp, "LArepeat"), build_laq(tmp), os.path.join(tmp, "TKhomogenize")


def borders_inside(las, rep_anno, rep_data):
    """records with a border of one of their A read's long intervals strictly inside (abpos, aepos)"""
    b = q_common.read_las(las)
    n, p = 0, 0
    for i in range(len(b["abpos"])):
        while b["pile_off"][p + 1] <= i:
            p += 1
        a = int(b["pile_aread"][p])
        iv = rep_data[int(rep_anno[a]) // 4:int(rep_anno[a + 1]) // 4].reshape(-1, 2)
        iv = iv[iv[:, 1] - iv[:, 0] >= 500]
        ab, ae = int(b["abpos"][i]), int(b["aepos"][i])
        if b["bread"][i] != a and np.any((iv > ab) & (iv < ae)):
            n += 1
    return n


def run_case(tools, tmp, name, inp, rep, laq, opts, plan):
    larepeat, laq_exe, tk = tools
    work = tempfile.mkdtemp(dir=tmp)
    hc.copy_db(work, inp)
    block, tin, tout, ttrim = hc.track_names(opts)
    nreads = len(q_common.db_read_len(hc.INPUTS[inp][0])) if inp != "masks_rep" else None
    extra = {}
    if rep == "synth":
        ra, rd = plan.track()
        trim_common.write_track_a2(os.path.join(work, ".G." + tin), nreads, ra, rd)
    else:
        r = subprocess.run([larepeat] + rep + ["G", hc.LAS], cwd=work, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0, (name, r.stderr)
        got = hc.read_written(work, tin)
        nreads, ra, rd = got["len"], got["anno"], got["data"]
    if laq == "synth":
        ta, td = plan.trim_track()
        trim_common.write_track_a2(os.path.join(work, ".G." + ttrim), nreads, ta, td)
        extra = dict(trim_anno=ta, trim_data=td)
    elif laq:
        r = q_common.run_tool(laq_exe, [], work)
        assert r.returncode == 0, (name, r.stderr)
        got = hc.read_written(work, ttrim)
        extra = dict(trim_anno=got["anno"], trim_data=got["data"])
    r = hc.run_tool(opts, work, exe=tk)
    got = hc.read_written(work, tout, block)
    assert got["len"] == nreads and len(got["anno"]) == nreads + 1
    np.savez_compressed(os.path.join(OUT, "expected_%s.npz" % name), nreads=nreads, rep_anno=ra, rep_data=rd, anno=got["anno"],
                        data=got["data"], header_zero=np.array([got["clen"] == 0, got["cdlen"] == 0, got["d2_bytes"] == 0]), **extra)
    assert os.path.getsize(os.path.join(OUT, "expected_%s.npz" % name)) < MAX_FILE
    case = dict(name=name, input=inp, opts=opts, rc=r.returncode, stdout=r.stdout, stderr=r.stderr)
    return case, got, (ra, rd), extra, os.path.join(work, hc.LAS)


def main():
    tmp = tempfile.mkdtemp(prefix="homogenize_golden_")
    try:
        tools = build_tools(tmp)
        shutil.rmtree(OUT, ignore_errors=True)
        os.makedirs(OUT)
        hom_shapes.write_synth(os.path.join(OUT, "synth.las"))
        assert os.path.getsize(os.path.join(OUT, "synth.las")) < 16384
        plan, role = hom_shapes.synth()
        cases, synth, empty = [], [], 0
        for name, inp, rep, laq, opts in hc.CASES:
            case, got, (ra, rd), extra, las = run_case(tools, tmp, name, inp, rep, laq, opts, plan)
            cases.append(case)
            assert case["rc"] == 0, (name, case["stderr"])
            rl = q_common.db_read_len(hc.INPUTS[inp][0])
            tagged = int(np.sum(got["data"][1::2].astype(np.int64) - got["data"][0::2]))
            assert "tagged %d as repeat\n" % tagged in case["stdout"]
            inside = borders_inside(las, ra, rd)
            print("%-16s reads %4d  input intervals %5d  tagged %8d of %8d (%4.1f%%)  records with a border inside %6d"
                  % (name, len(rl), len(rd) // 2, tagged, rl.sum(), 100. * tagged / rl.sum(), inside))
            if len(got["data"]) == 0:
                empty += 1
                assert case["stderr"] == "failed to write track data of 0 (0) bytes\n" and list(got["header_zero"] if "header_zero" in got else [1]) \
                    and got["clen"] == 0 and got["d2_bytes"] == 0
                continue
            assert .05 * rl.sum() <= tagged <= .80 * rl.sum(), (name, tagged, int(rl.sum()))
            if name == "m_masks_rep":                        # no traces: the copy alone
                assert np.array_equal(got["data"].reshape(-1, 2)[:, 0], rd.reshape(-1, 2)[(rd[1::2] - rd[0::2]) >= 500][:, 0])
            else:
                assert inside >= 100, (name, inside)
        assert empty == 1
        for name, inp, rep, laq, opts in hc.SYNTH_CASES:
            case, got, (ra, rd), extra, las = run_case(tools, tmp, name, inp, rep, laq, opts, plan)
            synth.append(case)
            assert case["rc"] == 0, (name, case["stderr"])
            kw = hc.opts_to_kwargs(opts)
            seen = {}
            anno, data, tagged, nranges = hom_model.homogenize([plan.batch()], plan.rl, ra, rd, merge=kw["merge"], ends=kw["ends"], res=kw["res"],
                                                               trim=(extra["trim_anno"], extra["trim_data"]) if extra else None, seen=seen)
            assert np.array_equal(anno, got["anno"]) and np.array_equal(data, got["data"]), "the model and the reference part ways on " + name
            assert "tagged %d as repeat\n" % tagged in case["stdout"]
            missing = [k for k in hom_shapes.PLANTED if k not in seen and ((kw["res"] == 1 and kw["ends"] == -1) or k not in ("spare_bit", "ends_before_last"))]
            assert not missing and seen.get("min_bites", 0) == 0, (name, missing)
            if kw["ends"] != -1:
                assert all(seen.get("e_" + k, 0) >= 1 for k in ("left", "right", "both", "neither")), seen
            if kw["res"] == 10 and kw["ends"] == -1:
                assert seen.get("single_bit", 0) >= 1
            print("%-16s tagged %6d, %3d ranges set, the model agrees" % (name, tagged, nranges))
        # the runs that end with a message
        work = tempfile.mkdtemp(dir=tmp)
        hc.copy_db(work, "tiny2")
        errors = []
        for name, args in (("bad_e0", ["-e", "0", "G", hc.LAS]), ("bad_e_neg", ["-e", "-5", "G", hc.LAS]), ("no_trim", ["-e", "2000", "G", hc.LAS]),
                           ("no_las", ["G", "nosuch.las"]), ("no_args", ["G"]), ("bad_option", ["-x", "G", hc.LAS])):
            r = hc.run_tool([], work, args=args, exe=tools[2])
            errors.append(dict(name=name, args=args, rc=r.returncode, stdout=r.stdout, stderr=r.stderr))
            assert r.returncode == 1, (name, r.returncode, r.stderr)
            print("%-10s %r %r" % (name, r.stdout[:60], r.stderr))
        json.dump(dict(cases=cases, synth=synth, errors=errors), open(os.path.join(OUT, "cases.json"), "w"), indent=1)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
