#!/usr/bin/env python3
"""Times of LAgap on the largest real fixture file and on the planted file, for profiles/gap_timing.txt: the damar_gap_last
split of one damar_pile_gaps call over the whole file on the device path, the same call on the host path in the same
process, and the whole command on both paths, start-up included, each run under a time limit of its own.

    python scripts/gap_timing.py > profiles/gap_timing.txt
"""
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gap_common as gc                                # noqa: E402
import q_common                                        # noqa: E402
from damar_amd import api                              # noqa: E402

REPEAT = 5


def main():
    print("# ms; every line is the best of %d runs after one that is not timed, its split the same run's" % REPEAT)
    for inp in (gc.BIG, "gsynth"):
        with tempfile.TemporaryDirectory() as tmp:
            gc.workdir(tmp, inp)
            off, aread, ab, ae, bb, be, br, fl = gc.pile_arrays(os.path.join(tmp, gc.LAS))
            piles = dict(pile_off=off, pile_aread=aread, abpos=ab, aepos=ae, bbpos=bb, bepos=be, bread=br, flags=fl)
            rl = q_common.db_read_len(gc.INPUTS[inp][0])
            for path in ("device", "host"):
                if path == "host":
                    os.environ["DAMAR_PILES"] = "host"
                else:
                    os.environ.pop("DAMAR_PILES", None)
                api.pile_gaps(piles, rl)                       # not timed: the first call of a path in this process
                best = None
                for _ in range(REPEAT):
                    api.pile_gaps(piles, rl)
                    split, npiles, host_piles, nev = api.gap_last()
                    if best is None or split["call"] < best[0]["call"]:
                        best = (split, npiles, host_piles, nev)
                split, npiles, host_piles, nev = best
                print("%-7s %-6s damar_pile_gaps: upload %.3f  kernel %.3f  download %.3f  whole call %.3f  (%d records, %d piles, %d by the "
                      "host routine, %d events)" % (inp, path, split["upload"], split["kernel"], split["download"], split["call"], len(ab),
                                                    npiles, host_piles, nev))
            os.environ.pop("DAMAR_PILES", None)
            for path in ("device", "host"):
                env = {k: v for k, v in os.environ.items() if k not in ("DAMAR_PILES", "DAMAR_TRIM")}
                if path == "host":
                    env["DAMAR_PILES"] = "host"
                best = None
                for run in range(REPEAT + 1):
                    t0 = time.perf_counter()
                    subprocess.run(["timeout", "-k", "10", "60", os.path.join(gc.BIN, "LAgap"), "G", gc.LAS, gc.OUT], cwd=tmp, env=env,
                                   check=True, stdout=subprocess.DEVNULL)
                    dt = (time.perf_counter() - t0) * 1e3
                    if run > 0:                                # the first run of a path is not timed
                        best = dt if best is None or dt < best else best
                print("%-7s %-6s whole command %8.2f" % (inp, path, best))
    return 0


if __name__ == "__main__":
    sys.exit(main())
