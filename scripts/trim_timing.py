#!/usr/bin/env python3
"""LAtrim on the tandem and fusion fixtures, device path against host path (DAMAR_TRIM=host): wall time of the command,
start-up included, the two alternating, and the split of damar_box_last from a run inside this process.

    python scripts/trim_timing.py [out.txt]
"""
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import trim_common as tc                               # noqa: E402
from damar_amd import api                              # noqa: E402

REPS = 5


def wall(case, tmp, env):
    t0 = time.perf_counter()
    r = subprocess.run(["timeout", "-k", "10", "120", os.path.join(tc.BIN, "LAtrim")] + case["opts"] + ["G", tc.LAS, tc.OUT], cwd=tmp,
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    dt = time.perf_counter() - t0
    if r.returncode != 0 or tc.md5(os.path.join(tmp, tc.OUT)) != case["md5"]:
        raise RuntimeError("%s: the run failed or its output is not the fixture's\n%s" % (case["name"], r.stderr))
    return 1000. * dt


def main():
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout
    dev = {k: v for k, v in os.environ.items() if k != "DAMAR_TRIM"}
    host = dict(dev, DAMAR_TRIM="host")
    out.write("LAtrim -v on fixture inputs, %s; times in ms; wall = the whole command, start-up included, %d runs each, alternating\n"
              % (api.lib().damar_hip_device_name().decode(), REPS))
    for name in ("def_tandem", "def_fusion"):
        case = next(c for c in tc.load_cases() if c["name"] == name)
        with tempfile.TemporaryDirectory() as tmp:
            tc.workdir(tmp, case, tc.expected(name))
            wall(case, tmp, dev)                       # warm the file cache
            d, h = [], []
            for _ in range(REPS):
                d.append(wall(case, tmp, dev))
                h.append(wall(case, tmp, host))
            p = lambda f: os.path.join(tmp, f)
            os.environ.pop("DAMAR_TRIM", None)
            api.trim_las(p("G"), p(tc.LAS), p(tc.OUT))
            t0 = time.perf_counter()
            st = api.trim_las(p("G"), p(tc.LAS), p(tc.OUT))
            call_dev = 1000. * (time.perf_counter() - t0)
            ms, boxes, fallback, values = api.box_last()
            os.environ["DAMAR_TRIM"] = "host"
            t0 = time.perf_counter()
            api.trim_las(p("G"), p(tc.LAS), p(tc.OUT))
            call_host = 1000. * (time.perf_counter() - t0)
            hms = api.box_last()[0]
            os.environ.pop("DAMAR_TRIM", None)
        fmt = lambda v: " ".join("%.1f" % x for x in v)
        out.write("\n%s: %d records, %d cut, %d boxes (mean M %.1f, mean N %.1f), %d to the host routine, %d script values\n"
                  % (name, st["novl"], st["ntrimmed"], boxes, st["box_a"] / max(boxes, 1), st["box_b"] / max(boxes, 1), fallback, values))
        out.write("  wall, device path: %s   median %.1f\n" % (fmt(d), sorted(d)[REPS // 2]))
        out.write("  wall, host path  : %s   median %.1f\n" % (fmt(h), sorted(h)[REPS // 2]))
        out.write("  inside a warm process, whole file: device path %.1f, host path %.1f\n" % (call_dev, call_host))
        out.write("  damar_box_last, device path: upload %.3f kernel %.3f download %.3f whole call %.3f\n"
                  % (ms["upload"], ms["kernel"], ms["download"], ms["call"]))
        out.write("  damar_box_last, host path  : whole call %.3f\n" % hms["call"])
    return 0


if __name__ == "__main__":
    sys.exit(main())
