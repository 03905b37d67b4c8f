#!/usr/bin/env python3
"""Boxes of read length for the whole-read alignment (kernels/read_align.hip, damar_align_reads) from the REFERENCE:
tests/golden/correct/read_boxes.npz.

Runs only where the reference sources lie (REF_SRC, default /root/reference): the driver of make_trim_golden.py around
Compute_Alignment(DIFF_ALIGN) is compiled into a temporary directory outside the repository, and only data is kept: the
boxes' bases, four to a byte, and the differences and the script the reference left for each.  Nothing compiled is kept.
The asserts hold every family to what it was planted for, as the reference reports it.

    python tests/golden/make_read_align_golden.py
"""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import read_align_common as rc                         # noqa: E402
from make_trim_golden import DRIVER, SRC, MAX_FILE, mutate, run_boxes        # noqa: E402

FAMILIES = ("border", "ladder", "skew", "ties", "worst", "cap", "many")
BORDER = (1000, 1001, 32767, 32768, 32769, 70000)      # the first size box_align refuses, the short border, past uint16
LADDER = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, rc.THREADS - 1, rc.THREADS, rc.THREADS + 1)
SKEW = ((5000, 3000), (3000, 5000), (2000, 1), (1, 2000))


def build_driver(tmp):
    s = lambda *p: os.path.join(SRC, *p)
    open(os.path.join(tmp, "boxdriver.c"), "w").write(DRIVER)
    subprocess.run(["gcc", "-O3", "-w", "-fno-strict-aliasing", "-I" + SRC, "-o", os.path.join(tmp, "boxdriver"),
                    os.path.join(tmp, "boxdriver.c"), s("dalign", "align.c"), s("db", "DB.c"), s("db", "QV.c"), "-lm", "-lpthread"],
                   cwd=tmp, check=True)
    return os.path.join(tmp, "boxdriver")


def substituted(rng, a, count):
    """`count` bases of a changed, evenly spread and never next to each other"""
    b = a.copy()
    if count:
        at = (np.arange(count) * len(a)) // count + int(rng.integers(0, max(1, len(a) // count - 1)))
        b[at] = (b[at] + 1 + rng.integers(0, 3, count)) % 4
    return b


def box_list():
    rng = np.random.default_rng(20261020)
    rnd = lambda n: rng.integers(0, 4, n).astype(np.uint8)
    bx = []                                            # (family, planted, a, b)
    for big in BORDER:
        a = rnd(big)
        bx.append(("border", -1, a, mutate(rng, a, .02, big)))
    for d in LADDER:
        a = rnd(3000)
        bx.append(("ladder", d, a, substituted(rng, a, d)))
    a = rnd(3000)                                      # one difference: a base of A alone, a base of B alone
    bx.append(("ladder", 1, a, np.delete(a, 1700)))
    bx.append(("ladder", 1, np.delete(a, 1300), a))
    for m, n in SKEW:
        long_ = rnd(max(m, n))
        short = long_[np.sort(rng.choice(max(m, n), min(m, n), replace=False))]
        bx.append(("skew", -1, long_, short) if m > n else ("skew", -1, short, long_))
    for m, n in ((500, 537), (1200, 1100), (2000, 1900), (1000, 1001)):
        bx.append(("ties", -1, np.zeros(m, dtype=np.uint8), np.zeros(n, dtype=np.uint8)))
        bx.append(("ties", -1, np.arange(m, dtype=np.uint8) % 2, np.arange(n, dtype=np.uint8) % 2))
        bx.append(("ties", -1, np.arange(m, dtype=np.uint8) % 2, (np.arange(n, dtype=np.uint8) + 1) % 2))
        core = np.zeros(m, dtype=np.uint8)             # a run between unique flanks, bases of the run missing on one side
        bx.append(("ties", -1, np.concatenate([rnd(300), core, rnd(300)]), None))
        a = bx[-1][2]
        bx[-1] = ("ties", -1, a, np.delete(a, 300 + np.sort(rng.choice(m, abs(m - n) + 3, replace=False))))
    bx.append(("worst", -1, rnd(2000), rnd(2000)))
    bx.append(("worst", -1, rnd(2000), rnd(2000)))
    bx.append(("worst", -1, np.zeros(1500, dtype=np.uint8), np.ones(1500, dtype=np.uint8)))
    for d in (400, 402):
        a = rnd(6000)
        bx.append(("cap", d, a, substituted(rng, a, d)))
    bx.append(("cap", -1, np.zeros(9000, dtype=np.uint8), np.ones(9000, dtype=np.uint8)))
    for _ in range(40):
        a = rnd(int(rng.integers(1001, 1201)))
        bx.append(("many", -1, a, mutate(rng, a, .05, len(a))))
    return bx


def main():
    tmp = tempfile.mkdtemp(prefix="read_golden_")
    try:
        driver = build_driver(tmp)
        bx = box_list()
        diffs, soff, script = run_boxes(driver, tmp, [(a, b) for _, _, a, b in bx])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    m = np.array([len(a) for _, _, a, _ in bx], dtype=np.int32)
    n = np.array([len(b) for _, _, _, b in bx], dtype=np.int32)
    big = np.maximum(m, n)
    aoff = np.concatenate([[0], np.cumsum(m + n)[:-1]]).astype(np.int64)
    bases = np.concatenate([np.concatenate([a, b]) for _, _, a, b in bx]).astype(np.uint8)
    family = np.array([FAMILIES.index(f) for f, _, _, _ in bx], dtype=np.int32)
    planted = np.array([p for _, p, _, _ in bx], dtype=np.int32)
    slen = np.diff(soff)
    rows = lambda f: np.flatnonzero(family == FAMILIES.index(f))

    r = rows("border")
    assert tuple(big[r]) == BORDER and np.all(diffs[r] > big[r] // 100) and np.all(diffs[r] < big[r] // 25) and np.all(slen[r] > 0)
    r = rows("ladder")
    assert np.array_equal(diffs[r], planted[r]) and tuple(planted[r][:len(LADDER)]) == LADDER
    one = r[planted[r] == 1]
    assert sorted((int(m[i] - n[i]), int(slen[i])) for i in one) == [(-1, 1), (0, 0), (1, 1)]
    r = rows("skew")
    assert tuple(zip(m[r], n[r])) == SKEW and np.all(diffs[r] == np.abs(m[r] - n[r])) and np.all(slen[r] == diffs[r])
    r = rows("ties")
    assert np.all(diffs[r] >= np.abs(m[r] - n[r])) and np.all(slen[r] >= np.abs(m[r] - n[r])) and np.all(slen[r] > 0)
    r = rows("worst")
    assert np.all(diffs[r[:2]] > 900) and diffs[r[2]] == 1500 and slen[r[2]] == 0
    r = rows("cap")
    assert tuple(diffs[r]) == (400, 402, 9000) and diffs[r[2]] > rc.MAXDIFF
    r = rows("many")
    assert len(r) == 40 and big[r].min() >= 1001 and big[r].max() <= 1200 and np.all(diffs[r] > 0)
    assert np.sum(diffs > rc.MAXDIFF) == 1

    os.makedirs(os.path.dirname(rc.PATH), exist_ok=True)
    np.savez_compressed(rc.PATH, m=m, n=n, aoff=aoff, boff=aoff + m, packed=rc.pack(bases), nbases=len(bases), diffs=diffs, soff=soff,
                        script=script, family=family, families=np.array(FAMILIES), planted=planted)
    assert os.path.getsize(rc.PATH) < MAX_FILE
    assert np.array_equal(rc.unpack(np.load(rc.PATH)["packed"], len(bases)), bases)
    print("read boxes: %d, %d bases, %d script values, %d bytes" % (len(bx), len(bases), len(script), os.path.getsize(rc.PATH)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
