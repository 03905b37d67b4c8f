#!/usr/bin/env python3
"""Times of LAfix on the largest real fixture file and on the planted file, for profiles/fix_timing.txt: the damar_fix_last
split of one damar_pile_patches call over the whole file on the device path, the same call on the host path
(damar_host_fix_pile) in the same process, and the whole command on both paths, start-up included, each run under a time
limit of its own.

    python scripts/fix_timing.py > profiles/fix_timing.txt
"""
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fix_common as fc                                # noqa: E402
from damar_amd import api                              # noqa: E402

REPEAT = 5


def main():
    print("# ms; every line is the best of %d runs after one that is not timed, its split the same run's" % REPEAT)
    for inp in (fc.BIG, "fsynth"):
        with tempfile.TemporaryDirectory() as tmp:
            fc.workdir(tmp, inp)
            batch, rl = fc.batch_of(inp)
            tr = fc.tracks(inp)
            trims = fc.trims_of(batch, rl, tr["trim"])
            for path in ("device", "host"):
                if path == "host":
                    os.environ["DAMAR_PILES"] = "host"
                else:
                    os.environ.pop("DAMAR_PILES", None)
                api.pile_patches(batch, rl, trims, tr["q"])    # not timed: the first call of a path in this process
                best = None
                for _ in range(REPEAT):
                    api.pile_patches(batch, rl, trims, tr["q"])
                    split, npiles, host_piles, n = api.fix_last()
                    if best is None or split["call"] < best[0]["call"]:
                        best = (split, npiles, host_piles, n)
                split, npiles, host_piles, n = best
                print("%-7s %-6s damar_pile_patches: upload %.3f  kernel %.3f  download %.3f  whole call %.3f  (%d records, %d piles, %d by "
                      "the host routine, %d repairs)" % (inp, path, split["upload"], split["kernel"], split["download"], split["call"],
                                                         len(batch["abpos"]), npiles, host_piles, n))
            os.environ.pop("DAMAR_PILES", None)
            for path in ("device", "host"):
                env = {k: v for k, v in os.environ.items() if k != "DAMAR_PILES"}
                if path == "host":
                    env["DAMAR_PILES"] = "host"
                best = None
                for run in range(REPEAT + 1):
                    t0 = time.perf_counter()
                    subprocess.run(["timeout", "-k", "10", "60", os.path.join(fc.BIN, "LAfix"), "-t", "trim", "G", fc.LAS, fc.OUT], cwd=tmp,
                                   env=env, check=True, stdout=subprocess.DEVNULL)
                    dt = (time.perf_counter() - t0) * 1e3
                    if run > 0:                                # the first run of a path is not timed
                        best = dt if best is None or dt < best else best
                print("%-7s %-6s whole command %8.2f" % (inp, path, best))
    return 0


if __name__ == "__main__":
    sys.exit(main())
