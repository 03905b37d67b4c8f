#!/usr/bin/env python3
"""Times of LAseparate for profiles/separate_timing.txt, on one GPU: the largest fixture file, and one simulated block
pair's daligner output made here (api.sim_write_db as bin/simdb does, the daligner stage, bin/LArepeat for the rep track).
Per input and path (device, DAMAR_PILES=host), best of 5 after an untimed run, in one process: the kernels and the copies
(HIP events, damar_separate_last), the whole call (api.pile_chains on the file as one batch), and the command with start-up.
With a reference binary given (REF_LASEPARATE, built outside the repository as tests/golden/make_separate_golden.py builds
it) its command is timed beside them; without one that column is left out and said so.

    python scripts/separate_timing.py [genome Mbp] > profiles/separate_timing.txt
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
import separate_common as sc                           # noqa: E402
from damar_amd import api, driver                      # noqa: E402

REPEAT = 5
REF = os.environ.get("REF_LASEPARATE")


def tool(exe, args, cwd, limit=300):
    subprocess.run(["timeout", "-k", "10", str(limit), exe] + args, cwd=cwd, check=True, stdout=subprocess.DEVNULL)


def measure(label, tmp, db, las, track):
    batch = sc.batch_of(os.path.join(tmp, las))
    read_len = api.db_info(os.path.join(tmp, db))[0]
    rep = api.read_track(os.path.join(tmp, db), track)
    sizes = [len(recs) for _, recs in sc.groups_of(batch)]
    print("# %s: %d records, %d groups, %d of more than one record (%.1f %%), the longest %d"
          % (label, len(batch["abpos"]), len(sizes), sum(1 for s in sizes if s > 1), 100.0 * sum(1 for s in sizes if s > 1) / max(len(sizes), 1),
             max(sizes)))
    args = ["-T0", "-r", track, db, las, "sep.keep.las", "sep.rest.las"]
    for path in ("device", "host"):
        if path == "host":
            os.environ["DAMAR_PILES"] = "host"
        else:
            os.environ.pop("DAMAR_PILES", None)
        best = None
        for run in range(REPEAT + 1):
            t0 = time.perf_counter()
            api.pile_chains(batch, read_len, rep["anno"], rep["data"], 100, 0)
            call = (time.perf_counter() - t0) * 1e3
            ms, ngroups, nhost, multi = api.separate_last()
            t0 = time.perf_counter()
            tool(os.path.join(sc.BIN, "LAseparate"), args, tmp)
            cmd = (time.perf_counter() - t0) * 1e3
            row = (ms["kernel"], ms["upload"] + ms["download"], ms["call"], call, cmd)
            if run > 0:
                best = row if best is None else tuple(min(x, y) for x, y in zip(best, row))
        print("%-9s %-6s kernels %8.3f  copies %8.3f  the C call %9.2f  api.pile_chains %9.2f  command with start-up %9.1f   (%d groups by the host routine)"
              % ((label, path) + best + (nhost,)))
        sys.stdout.flush()
    os.environ.pop("DAMAR_PILES", None)
    if REF:
        best = None
        for run in range(REPEAT + 1):
            t0 = time.perf_counter()
            tool(REF, args, tmp)
            cmd = (time.perf_counter() - t0) * 1e3
            if run > 0:
                best = cmd if best is None else min(best, cmd)
        print("%-9s %-6s command with start-up %9.1f" % (label, "ref", best))
    else:
        print("# %s: no reference binary given (REF_LASEPARATE): its command is not timed" % label)


def main():
    mbp = float(sys.argv[1]) if len(sys.argv) > 1 else 4.0
    print("# ms; every line is the best of %d runs after one that is not timed; the host routine runs no kernel and copies nothing" % REPEAT)
    with tempfile.TemporaryDirectory() as tmp:
        sc.workdir(tmp, sc.BIG)
        measure("fixture", tmp, "G", sc.LAS, "rep")
    with tempfile.TemporaryDirectory() as tmp:
        api.sim_write_db(tmp, "SIM", mbp, coverage=20., seed=11)
        blk = driver.Block(os.path.join(tmp, "SIM.1"))
        plan = driver.Plan(j=4)
        plan.run_line(blk, [blk], os.path.join(tmp, "las"))
        plan.finish()
        shutil.copy(os.path.join(tmp, "las", "d001_00001", "SIM.1.SIM.1.las"), os.path.join(tmp, "SIM.las"))
        tool(os.path.join(sc.BIN, "LArepeat"), ["-c", "20", "-t", "rep", "SIM", "SIM.las"], tmp)
        measure("simulated", tmp, "SIM", "SIM.las", "rep")
    return 0


if __name__ == "__main__":
    sys.exit(main())
