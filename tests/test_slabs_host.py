"""A comparison with more seed pairs than one seed stage holds runs in slabs of B reads: the parts that need no GPU --
the new entry points are declared and exported, and the greedy cut (host arithmetic of libdamar_hip.so) does what
include/damar_hip.h says."""
import os
import subprocess

import numpy as np

from conftest import ROOT


def test_slab_entry_points_are_declared_and_exported(built):
    lib = os.path.join(ROOT, "damar_amd", "libdamar_hip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, stdout=subprocess.PIPE, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    hdr = open(os.path.join(ROOT, "include", "damar_hip.h")).read()
    for fn in ("damar_last_slabs", "damar_slab_totals", "damar_slab_cut"):
        assert fn in exported
        assert fn + "(" in hdr


def greedy(h, cap):
    """The rule of include/damar_hip.h, restated: a slab takes B reads while its sum stays <= cap, at least one."""
    lo, sums, acc = [0], [], 0
    for r, x in enumerate(h):
        if r > lo[-1] and acc + x > cap:
            sums.append(acc)
            lo.append(r)
            acc = 0
        acc += x
    sums.append(acc)
    lo.append(len(h))
    return lo, sums


def test_greedy_cut_of_b_reads(built):
    from damar_amd import api
    assert api.slab_cut([0, 3, 0, 5, 2, 0, 9, 1], 9) == ([0, 4, 6, 7, 8], [8, 2, 9, 1])
    assert api.slab_cut([1, 2, 3], 100) == ([0, 3], [6])                 # cap above the total: one slab
    assert api.slab_cut([0, 0, 0], 5) == ([0, 3], [0])                   # reads without seeds
    assert api.slab_cut([], 5) == ([0, 0], [0])
    assert api.slab_cut([1, 2, 30, 1], 9) == -3                          # read 2 alone is above the cap
    assert api.slab_cut([4, 4, 4], 4) == ([0, 1, 2, 3], [4, 4, 4])       # "<= cap": a read that fills a slab exactly
    rng = np.random.RandomState(5)
    for _ in range(50):
        h = [int(x) for x in rng.randint(0, 40, size=rng.randint(1, 200)) * (rng.rand() < .8)]
        cap = max(max(h), int(rng.randint(1, 400)))
        assert api.slab_cut(h, cap) == greedy(h, cap)
    big = [2 ** 33, 5, 2 ** 33 - 5, 7]                                   # sums beyond 32 bits
    assert api.slab_cut(big, 2 ** 33) == greedy(big, 2 ** 33)
