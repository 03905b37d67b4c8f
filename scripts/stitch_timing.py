#!/usr/bin/env python3
"""Times of LAstitch on the fixture files and of the box kernel under it, for profiles/stitch_timing.txt: per file the
damar_tbox_last split of the last round and the boxes per round on the device path, the same call on the host path in the
same process, and the whole command on both paths, start-up included; then the 400-to-700-base boxes of
tests/golden/stitch/tboxes.npz, the shape of a stitch box at spacing 100, as one batch on either path.

    python scripts/stitch_timing.py > profiles/stitch_timing.txt
"""
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import stitch_common as sc                             # noqa: E402
from damar_amd import api                              # noqa: E402

REPEAT = 5


def call(path, fn):
    if path == "host":
        os.environ["DAMAR_STITCH"] = "host"
    else:
        os.environ.pop("DAMAR_STITCH", None)
    fn()                                                   # not timed: the first call of a path in this process
    best, res, last = None, None, None
    for _ in range(REPEAT):
        t0 = time.perf_counter()
        r = fn()
        dt = (time.perf_counter() - t0) * 1e3
        if best is None or dt < best:                      # the split printed beside a time is that run's
            best, res, last = dt, r, api.tbox_last()
    return best, res, last


def main():
    print("# ms; every line is the best of %d runs after one that is not timed, its split the same run's" % REPEAT)
    for inp, opts in (("tiny2", []), ("fusion", []), ("ssynth", ["-f", "150"])):
        with tempfile.TemporaryDirectory() as tmp:
            sc.workdir(tmp, inp)
            p = lambda f: os.path.join(tmp, f)
            kw = dict(fuzz=150) if opts else {}
            for path in ("device", "host"):
                ms, st, (split, boxes, fallback, values) = call(path, lambda: api.stitch_las(p("G"), p(sc.LAS), p(sc.OUT), **kw))
                print("%-7s %-6s call %8.2f  records %6d  boxes per round %s  stitched %d  refused %d" %
                      (inp, path, ms, st["novl"], st["round_boxes"] if st["boxes"] else [], st["stitched"], st["refused"]))
                if st["boxes"] and path == "device":
                    print("%-7s %-6s last round: upload %.3f  kernel %.3f  download %.3f  whole call %.3f  (%d boxes, %d by the host routine)" %
                          (inp, path, split["upload"], split["kernel"], split["download"], split["call"], boxes, fallback))
            for path in ("device", "host"):
                env = {k: v for k, v in os.environ.items() if k != "DAMAR_STITCH"}
                if path == "host":
                    env["DAMAR_STITCH"] = "host"
                best = None
                for _ in range(REPEAT + 1):
                    t0 = time.perf_counter()
                    subprocess.run([os.path.join(sc.BIN, "LAstitch")] + opts + ["G", sc.LAS, sc.OUT], cwd=tmp, env=env, check=True,
                                   stdout=subprocess.DEVNULL)
                    dt = (time.perf_counter() - t0) * 1e3
                    best = dt if best is None or dt < best else best
                print("%-7s %-6s whole command %8.2f" % (inp, path, best))
    bx = sc.tboxes()
    fams = list(bx["families"])
    for names in (("stitch",), ("unrelated",), ("large", "large_unrelated")):
        runs = np.flatnonzero(np.isin(bx["family"][bx["run_box"]], [fams.index(n) for n in names]))
        a, b, at = sc.run_seqs(bx, runs)
        for path in ("device", "host"):
            ms, _, (split, boxes, fallback, values) = call(path, lambda: api.trace_boxes(a, b, at, sc.TW))
            print("boxes %-22s %-6s %5d boxes  upload %.3f  kernel %.3f  download %.3f  whole call %.3f  (Python round trip %.2f)" %
                  ("+".join(names), path, boxes, split["upload"], split["kernel"], split["download"], split["call"], ms))
    return 0


if __name__ == "__main__":
    sys.exit(main())
