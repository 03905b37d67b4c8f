#!/usr/bin/env python3
"""TKhomogenize on the fusion and tandem fixtures, device path against host path (DAMAR_PILES=host): wall time of the
command, start-up included, the two alternating, and the split of damar_homog_last from a run inside this process.

    python scripts/homogenize_timing.py [out.txt]
"""
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hom_common as hc                                # noqa: E402
from damar_amd import api                              # noqa: E402

REPS = 5


def wall(case, exp, tmp, env_extra):
    t0 = time.perf_counter()
    r = hc.run_tool(case["opts"], tmp, env_extra, timeout_s=120)
    dt = time.perf_counter() - t0
    hc.check_output(case, exp, r, tmp)
    return 1000. * dt


def main():
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout
    os.environ.pop("DAMAR_PILES", None)
    out.write("TKhomogenize on fixture inputs, %s; times in ms; wall = the whole command, start-up included, %d runs each, alternating\n"
              % (api.lib().damar_hip_device_name().decode(), REPS))
    for name in ("c12_fusion", "def_tandem"):
        case = next(c for c in hc.load_cases() if c["name"] == name)
        exp = hc.expected(name)
        with tempfile.TemporaryDirectory() as tmp:
            hc.workdir(tmp, case, exp)
            wall(case, exp, tmp, {})                   # warm the file cache
            d, h = [], []
            for _ in range(REPS):
                d.append(wall(case, exp, tmp, {}))
                h.append(wall(case, exp, tmp, {"DAMAR_PILES": "host"}))
            p = lambda f: os.path.join(tmp, f)
            api.homogenize_track(p("G"), p(hc.LAS))
            t0 = time.perf_counter()
            anno, data, tagged = api.homogenize_track(p("G"), p(hc.LAS))
            call_dev = 1000. * (time.perf_counter() - t0)
            ms, records, ranges, intervals = api.homog_last()
            os.environ["DAMAR_PILES"] = "host"
            t0 = time.perf_counter()
            api.homogenize_track(p("G"), p(hc.LAS))
            call_host = 1000. * (time.perf_counter() - t0)
            os.environ.pop("DAMAR_PILES", None)
        fmt = lambda v: " ".join("%.1f" % x for x in v)
        out.write("\n%s: %d records, %d ranges set, %d intervals out, %d bases tagged\n" % (name, records, ranges, intervals, tagged))
        out.write("  wall, device path: %s   median %.1f\n" % (fmt(d), sorted(d)[REPS // 2]))
        out.write("  wall, host path  : %s   median %.1f\n" % (fmt(h), sorted(h)[REPS // 2]))
        out.write("  inside a warm process, whole file (reading it included): device path %.1f, host path %.1f\n" % (call_dev, call_host))
        out.write("  damar_homog_last, device path: upload %.3f mark %.3f read-out %.3f download %.3f\n"
                  % (ms["upload"], ms["mark"], ms["readout"], ms["download"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
