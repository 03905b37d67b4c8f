#!/usr/bin/env python3
"""Timings of LAcorrect on the largest fixture file (fusion), best of 5 after an untimed run: the consensus kernel, the
whole damar_tile_consensus calls, the host routine's consensus, the host postrace alignment and its share, and the command
with start-up on both paths.  Prints what profiles/correct_timing.txt holds.

    python scripts/correct_timing.py [reference LAcorrect binary]
"""
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import correct_common as cc                            # noqa: E402
from damar_amd import api                              # noqa: E402

REPS = 5


def main():
    tmp = cc.workdir(tempfile.mkdtemp(), "fusion")
    args = (os.path.join(tmp, "G"), os.path.join(tmp, cc.LAS), os.path.join(tmp, cc.OUT))
    paths = [("host", dict(DAMAR_PILES="host"))] + ([] if os.environ.get("DAMAR_PILES") == "host" else [("device", {})])
    for name, env in paths:
        os.environ.update(env)
        runs = [api.correct_las(*args) for _ in range(REPS + 1)][1:]
        best = lambda k: min(r[k] for r in runs)
        r = runs[0]
        print("%-6s pass: %d tiles (%d by the host routine beside the kernel), %d reads" % (name, r["tiles"], r["host_tiles"], r["reads"]))
        print("       consensus calls %.1f ms (kernel %.1f ms), postrace %.1f ms of thread time in 8 threads, waited for %.1f ms, "
              "whole pass %.1f ms" % (best("ms_consensus"), best("ms_kernel"), best("ms_postrace"), best("ms_postrace_wait"), best("ms_total")))
        os.environ["DAMAR_CORRECT_THREADS"] = "1"
        one = [api.correct_las(*args) for _ in range(2)][1]
        del os.environ["DAMAR_CORRECT_THREADS"]
        print("       with one postrace thread: postrace %.1f ms = %.0f %% of a pass of %.1f ms" %
              (one["ms_postrace"], 100 * one["ms_postrace"] / one["ms_total"], one["ms_total"]))
        for k in env:
            del os.environ[k]
        t = []
        for _ in range(REPS + 1):
            t0 = time.time()
            subprocess.run([os.path.join(cc.BIN, "LAcorrect"), "G", cc.LAS, cc.OUT], cwd=tmp, env=dict(os.environ, **env), check=True)
            t.append(time.time() - t0)
        print("       command with start-up: %.2f s" % min(t[1:]))
    if len(sys.argv) > 1:
        t0 = time.time()
        subprocess.run([sys.argv[1], "-j", "1", "G", cc.LAS, "ref"], cwd=tmp, check=True)
        print("reference -j 1 (gcc -O3), one run: %.2f s" % (time.time() - t0))


if __name__ == "__main__":
    main()
