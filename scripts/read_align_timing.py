#!/usr/bin/env python3
"""Timings of the whole-read alignment behind LAcorrect's " postrace=" on the largest fixture file (fusion), best of 5 after
an untimed run: damar_align_reads on the file's (read, correction) boxes, kernel and whole call; the same boxes through
damar_exact_box in one thread and in eight; the whole warm pass and the command with start-up with the postrace on the
device and in the worker threads, and, given a built checkout of the parent commit, the parent's.  Prints what
profiles/read_align_timing.txt holds.

    python scripts/read_align_timing.py [built checkout of the parent commit]
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
import correct_common as cc                            # noqa: E402
import correct_model as cm                             # noqa: E402
from damar_amd import api                              # noqa: E402

REPS = 5
PARENT = """
import sys
sys.path.insert(0, sys.argv[1])
from damar_amd import api
runs = [api.correct_las(*sys.argv[2:5])["ms_total"] for _ in range(%d)][1:]
print(" ".join("%%.1f" %% x for x in runs))
""" % (REPS + 1)


def file_boxes(tmp):
    """the (read, correction) pairs of the pass's output"""
    reads = cm.db_reads(os.path.join(cc.GOLDEN, cc.INPUTS["fusion"][0]))
    code = np.zeros(256, dtype=np.uint8)
    for i, c in enumerate(b"acgt"):
        code[c] = i
    a, b = [], []
    for rec in open(os.path.join(tmp, cc.OUT + ".00.fasta"), "rb").read().split(b">")[1:]:
        head, _, body = rec.partition(b"\n")
        if head.startswith(b"copy."):
            continue
        a.append(reads[int(head.split(b".")[0])])
        b.append(code[np.frombuffer(body.replace(b"\n", b""), dtype=np.uint8)])
    return a, b


def passes(args, env):
    os.environ.update(env)
    runs = [api.correct_las(*args) for _ in range(REPS + 1)][1:]
    for k in env:
        del os.environ[k]
    return runs


def command(exe, tmp, env):
    t = []
    for _ in range(REPS + 1):
        t0 = time.time()
        subprocess.run([exe, "G", cc.LAS, cc.OUT], cwd=tmp, env=dict(os.environ, **env), check=True)
        t.append(time.time() - t0)
    return min(t[1:])


def main():
    tmp = cc.workdir(tempfile.mkdtemp(), "fusion")
    args = (os.path.join(tmp, "G"), os.path.join(tmp, cc.LAS), os.path.join(tmp, cc.OUT))
    api.correct_las(*args)
    a, b = file_boxes(tmp)
    big = [max(len(x), len(y)) for x, y in zip(a, b)]
    dev = []
    for _ in range(REPS + 1):
        diffs, _ = api.align_reads(a, b)
        dev.append(api.read_last())
    dev = dev[1:]
    print("boxes: %d whole reads of %d to %d bases, %d to %d differences (%d in all), %d script values, %d by the host routine beside "
          "the kernel" % (len(a), min(big), max(big), diffs.min(), diffs.max(), diffs.sum(), dev[0][3], dev[0][2]))
    print("damar_align_reads: kernel %.1f ms, whole call %.1f ms (upload %.1f, download %.1f)" %
          (min(d[0]["kernel"] for d in dev), min(d[0]["call"] for d in dev), min(d[0]["upload"] for d in dev), min(d[0]["download"] for d in dev)))
    os.environ["DAMAR_POSTRACE"] = "host"
    one = []
    for _ in range(REPS + 1):
        api.align_reads(a, b)
        one.append(api.read_last()[0]["call"])
    del os.environ["DAMAR_POSTRACE"]
    print("damar_exact_box, the same boxes in one thread: %.1f ms" % min(one[1:]))
    for name, env in (("device", {}), ("threads", dict(DAMAR_POSTRACE="host"))):
        runs = passes(args, env)
        tot = sorted(r["ms_total"] for r in runs)
        best = lambda k: min(r[k] for r in runs)
        print("pass, postrace on the %s: %.1f ms (five runs %s); consensus calls %.1f ms" %
              (name, tot[0], " ".join("%.1f" % x for x in tot), best("ms_consensus")))
        if name == "device":
            print("      damar_align_reads calls %.1f ms (kernels %.1f ms), %d boxes, %d by the host routine" %
                  (best("ms_postrace_call"), best("ms_postrace_kernel"), runs[0]["postrace_boxes"], runs[0]["postrace_host"]))
        else:
            print("      eight threads: %.1f ms of thread time, waited for %.1f ms" % (best("ms_postrace"), best("ms_postrace_wait")))
        print("      command with start-up: %.2f s" % command(os.path.join(cc.BIN, "LAcorrect"), tmp, env))
    if len(sys.argv) > 1:
        parent = os.path.abspath(sys.argv[1])
        r = subprocess.run([sys.executable, "-c", PARENT, parent] + list(args), stdout=subprocess.PIPE, text=True, check=True)
        tot = sorted(float(x) for x in r.stdout.split())
        print("parent commit, pass: %.1f ms (five runs %s)" % (tot[0], " ".join("%.1f" % x for x in tot)))
        print("      command with start-up: %.2f s" % command(os.path.join(parent, "damar_amd", "bin", "LAcorrect"), tmp, {}))


if __name__ == "__main__":
    main()
