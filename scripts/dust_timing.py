#!/usr/bin/env python3
"""DBdust on the largest fixture and on a simulated block of the config-2 size: the call, and the commands with start-up, on
the device path, with DAMAR_DUST=host and with the reference binary of oracle/_ref/ (profiles/dust_timing.txt).  Run from the
repository root on a machine with the GPU."""
import os, shutil, subprocess, sys, tempfile, time
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import numpy as np
from damar_amd import api
import dust_common as dc
ROOT = os.getcwd()
reads, _ = dc.db_reads(dc.MASK_DUST, "G")
nb = sum(len(r) for r in reads)
def best(f, n=5):
    f(); ts = []
    for _ in range(n):
        t0 = time.perf_counter(); f(); ts.append(time.perf_counter() - t0)
    return min(ts) * 1e3
ms = best(lambda: api.dust_reads(reads))
last = api.dust_last()
print("mask_dust database: %d reads %d bases; call best-of-5 %.2f ms; last %s; walk share %.3f" % (len(reads), nb, ms, last[0], last[5] / last[4]))
os.environ["DAMAR_DUST"] = "host"
print("same call DAMAR_DUST=host best-of-5 %.2f ms" % best(lambda: api.dust_reads(reads)))
del os.environ["DAMAR_DUST"]
def cmd_ms(exe, args, cwd, env=None, n=3):
    ts = []
    for _ in range(n + 1):
        t0 = time.perf_counter()
        subprocess.run(["timeout", "-k", "10", "120", exe] + args, cwd=cwd, env=env, check=True, stderr=subprocess.PIPE)
        ts.append(time.perf_counter() - t0)
    return min(ts[1:]) * 1e3
with tempfile.TemporaryDirectory() as tmp:
    dc.planted_workdir(tmp, ("G.db", ".G.idx", ".G.bps"), dc.MASK_DUST)
    print("command G.1 (1.0 Mbp, with start-up): device %.0f ms, DAMAR_DUST=host %.0f ms, reference %.0f ms" % (
        cmd_ms(os.path.join(dc.BIN, "DBdust"), ["G.1"], tmp), cmd_ms(os.path.join(dc.BIN, "DBdust"), ["G.1"], tmp, dict(os.environ, DAMAR_DUST="host")),
        cmd_ms(os.path.join(ROOT, "oracle", "_ref", "DBdust"), ["G.1"], tmp)))
    # a block of simulated reads at the config-2 block size
    api.sim_write_db(tmp, "S", 9.0, coverage=15., seed=11, block_mbp=135)
    env = dict(os.environ, DAMAR_DUST_STATS="1")
    t0 = time.perf_counter(); r = subprocess.run(["timeout", "-k", "10", "200", os.path.join(dc.BIN, "DBdust"), "S.1"], cwd=tmp, env=env, stderr=subprocess.PIPE, text=True, check=True); d = time.perf_counter() - t0
    print("simulated block S.1:", r.stderr.strip())
    dev = {f: open(os.path.join(tmp, f), "rb").read() for f in (".S.1.dust.anno", ".S.1.dust.data")}
    print("command S.1 with start-up: device %.0f ms (first run)" % (d * 1e3))
    print("command S.1: device %.0f ms, DAMAR_DUST=host %.0f ms, reference %.0f ms" % (
        cmd_ms(os.path.join(dc.BIN, "DBdust"), ["S.1"], tmp, n=2), cmd_ms(os.path.join(dc.BIN, "DBdust"), ["S.1"], tmp, dict(os.environ, DAMAR_DUST="host"), n=1),
        cmd_ms(os.path.join(ROOT, "oracle", "_ref", "DBdust"), ["S.1"], tmp, n=1)))
    ref = {f: open(os.path.join(tmp, f), "rb").read() for f in (".S.1.dust.anno", ".S.1.dust.data")}
    print("S.1 device track equals the reference's:", dev == ref, len(ref[".S.1.dust.data"]) // 8, "intervals")
