#!/usr/bin/env python3
"""Times of OGbuild for profiles/og_timing.txt, on one GPU: the largest filtered fixture file, and a larger file made here
from a simulated block (api.sim_write_db as bin/simdb does, the daligner stage, bin/LAq for the trim track, bin/LAfilter
-T -p).  Per input and path (device, DAMAR_PILES=host), best of 5 after an untimed run, in one process: the kernels and
the copies (HIP events, damar_graph_last), the whole call (api.og_edges), and the command with start-up.

    python scripts/og_timing.py [genome Mbp] > profiles/og_timing.txt
"""
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import og_common as oc                                 # noqa: E402
from damar_amd import api, driver                      # noqa: E402

REPEAT = 5


def tool(name, args, cwd, limit=300):
    subprocess.run(["timeout", "-k", "10", str(limit), os.path.join(oc.BIN, name)] + args, cwd=cwd, check=True, stdout=subprocess.DEVNULL)


def measure(label, tmp, db, las):
    for path in ("device", "host"):
        if path == "host":
            os.environ["DAMAR_PILES"] = "host"
        else:
            os.environ.pop("DAMAR_PILES", None)
        best = None
        for run in range(REPEAT + 1):
            t0 = time.perf_counter()
            g = api.og_edges(os.path.join(tmp, db), os.path.join(tmp, las))
            call = (time.perf_counter() - t0) * 1e3
            ms, nrec, ncand, nhost, kept = api.og_last()
            t0 = time.perf_counter()
            tool("OGbuild", [db, las, "og.timing.out"], tmp)
            cmd = (time.perf_counter() - t0) * 1e3
            row = (ms["piles"] + ms["finish"], ms["upload"] + ms["download"], call, cmd) if path == "device" else (0.0, 0.0, call, cmd)
            if run > 0:
                best = row if best is None else tuple(min(x, y) for x, y in zip(best, row))
        print("%-8s %-6s kernels %8.3f  copies %8.3f  whole call %9.2f  command with start-up %9.1f   (%d records, %d + %d slots, %d edges kept)"
              % (label, path, best[0], best[1], best[2], best[3], records(tmp, las),
                 g["cnt_left"], g["cnt_right"], len(g["left"]) + len(g["right"])))
        sys.stdout.flush()
    os.environ.pop("DAMAR_PILES", None)


def records(tmp, las):
    import struct
    return struct.unpack("<q", open(os.path.join(tmp, las), "rb").read(8))[0]


def main():
    mbp = float(sys.argv[1]) if len(sys.argv) > 1 else 4.0
    print("# ms; every line is the best of %d runs after one that is not timed; the host routine runs no kernel and copies nothing" % REPEAT)
    with tempfile.TemporaryDirectory() as tmp:
        oc.workdir(tmp, "fusion")
        measure("fixture", tmp, "G", oc.LAS)
    with tempfile.TemporaryDirectory() as tmp:
        api.sim_write_db(tmp, "SIM", mbp, coverage=20., seed=11)
        blk = driver.Block(os.path.join(tmp, "SIM.1"))
        plan = driver.Plan(j=4)
        plan.run_line(blk, [blk], os.path.join(tmp, "las"))
        plan.finish()
        shutil.copy(os.path.join(tmp, "las", "d001_00001", "SIM.1.SIM.1.las"), os.path.join(tmp, "SIM.las"))
        tool("LAq", ["SIM", "SIM.las"], tmp)
        tool("LAfilter", ["-t", "trim", "-T", "-p", "-o", "1000", "-s", "300", "SIM", "SIM.las", "SIM.filtered.las"], tmp)
        print("# simulated: %.1f Mbp at 20x, one block, %d records, %d after LAfilter -t trim -T -p -o 1000 -s 300"
              % (mbp, records(tmp, "SIM.las"), records(tmp, "SIM.filtered.las")))
        measure("simulated", tmp, "SIM", "SIM.filtered.las")
    return 0


if __name__ == "__main__":
    sys.exit(main())
