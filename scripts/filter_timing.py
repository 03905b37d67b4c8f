#!/usr/bin/env python3
"""Times of LAfilter on the largest real fixture file under the plan's option set, for profiles/filter_timing.txt: the
damar_filter_last split of one damar_pile_filter call over the whole file on the device path (the options of the plan that
the pile call sees; -T lies outside it), the same call on the host path (damar_host_filter_pile) in the same process, and
the whole command with the full set on both paths, start-up included, each run under a time limit of its own.

    python scripts/filter_timing.py > profiles/filter_timing.txt
"""
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import filter_common as fc                             # noqa: E402
import q_common                                        # noqa: E402
from damar_amd import api                              # noqa: E402

REPEAT = 5


def main():
    inp = fc.BIG
    case = next(c for c in fc.load_cases() if c["name"] == "plan_" + inp)
    print("# ms; every line is the best of %d runs after one that is not timed, its split the same run's" % REPEAT)
    print("# %s, options %s" % (inp, " ".join(case["opts"])))
    with tempfile.TemporaryDirectory() as tmp:
        fc.workdir(tmp, inp)
        batch = fc.trace_batch(os.path.join(tmp, fc.LAS))
        rl = q_common.db_read_len(fc.INPUTS[inp][0])
        kw = fc.opts_to_params(case["opts"], inp, fc.load_cases("files"))
        for path in ("device", "host"):
            if path == "host":
                os.environ["DAMAR_PILES"] = "host"
            else:
                os.environ.pop("DAMAR_PILES", None)
            api.pile_filter(batch, rl, **kw)               # not timed: the first call of a path in this process
            best = None
            for _ in range(REPEAT):
                api.pile_filter(batch, rl, **kw)
                got = api.filter_last()
                if best is None or got[0]["call"] < best[0]["call"]:
                    best = got
            split, npiles, host_piles, gone = best
            print("%-7s %-6s damar_pile_filter: upload %.3f  kernel %.3f  download %.3f  whole call %.3f  (%d records, %d piles, %d by the "
                  "host routine, %d records discarded)" % (inp, path, split["upload"], split["kernel"], split["download"], split["call"],
                                                           len(batch["abpos"]), npiles, host_piles, gone))
        os.environ.pop("DAMAR_PILES", None)
        for path in ("device", "host"):
            env = {k: v for k, v in os.environ.items() if k not in ("DAMAR_PILES", "DAMAR_TRIM")}
            if path == "host":
                env.update(DAMAR_PILES="host", DAMAR_TRIM="host")
            best = None
            for run in range(REPEAT + 1):
                t0 = time.perf_counter()
                subprocess.run(["timeout", "-k", "10", "60", os.path.join(fc.BIN, "LAfilter")] + case["opts"] + ["G", fc.LAS, fc.OUT], cwd=tmp,
                               env=env, check=True, stdout=subprocess.DEVNULL)
                dt = (time.perf_counter() - t0) * 1e3
                if run > 0:                                # the first run of a path is not timed
                    best = dt if best is None or dt < best else best
            print("%-7s %-6s whole command %8.2f" % (inp, path, best))
    return 0


if __name__ == "__main__":
    sys.exit(main())
