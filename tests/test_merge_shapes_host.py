"""The planted shapes of tests/merge_shapes.py on the CPU: every case is built, run through the oracle (sort_kmers,
seed_pairs) and the geometry it is named for is asserted on the oracle's own index arrays -- a run starts 65 entries before
a tile border, a tile's B piece has exactly 3073 entries, a tile has no seed between two that have.  A case that has
drifted off its border fails here, without a GPU.  Cross comparisons must have the closed-form seed count (the sum over
codes of na * nb where na * nb is below the cap), runs of N identical reads in a self comparison N (N - 1) / 2 seeds or
none, and every planted run the fate its maker wrote into the table: that pins the oracle on these shapes independently of
the device.

Reads shorter than k are not among the shapes: the reference refuses a block that has one (daligner.c:499-504)."""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import merge_shapes as M


@pytest.mark.parametrize("cid", M.IDS)
def test_planted_case_sits_on_its_border_and_the_oracle_counts_it(built, cid):
    case = M.BY_ID[cid]
    x = M.context(case)
    assert len(x.acode) > 0 and len(case.checks) >= 2
    for chk in case.checks:
        chk(x)
    if not case.lowmem:
        assert x.limit == M.MAXGRAM
    flagged = M.flagged_tiles(x)                            # what the GPU file asserts of damar_last_merge_flagged()
    if case.flagged == ">0":
        assert 0 < len(flagged) < x.ntiles
    elif case.flagged is not None:
        assert len(flagged) == case.flagged


def test_the_gpu_file_runs_every_case_of_the_table():
    """what pytest collects from the GPU file: every test function of it that takes a case runs every case id of the
    table, and every group of the table has both code widths where it should"""
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-m", "pytest", "--collect-only", "-q", os.path.join(here, "test_gpu_merge_shapes.py")],
                       cwd=os.path.dirname(here), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    seen = {}
    for m in re.finditer(r"::(test_\w+)\[([^\]]+)\]", r.stdout):
        seen.setdefault(m.group(1), []).append(m.group(2))
    assert sorted(seen["test_gpu_planted_merge_equals_oracle"]) == sorted(M.IDS)
    modes = sorted(set(i.split("-", 1)[0] for i in seen["test_gpu_planted_merge_equals_oracle_under_switch"]))
    assert modes == ["general", "pack_pos0", "pack_seeds0"]
    for mode in modes:
        assert sorted(i.split("-", 1)[1] for i in seen["test_gpu_planted_merge_equals_oracle_under_switch"]
                      if i.startswith(mode + "-")) == sorted(M.IDS)
    for g in "ABCD":
        ids14 = sorted(c.id[:-4] for c in M.CASES if c.group == g and c.k == M.K32)
        ids17 = sorted(c.id[:-4] for c in M.CASES if c.group == g and c.k == M.K64)
        assert ids14 == ids17 and len(ids14) > 0
    assert sorted(c.k for c in M.CASES if c.group == "E") == [M.K32, M.K32]
    assert all(len(c.a.runs) + len(c.a.extra) and c.a.at <= 40 * M.MT_A for c in M.CASES)
