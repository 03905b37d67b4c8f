"""Trace-point expansion: the oracle's restatement (oracle/trace.c) against the REAL reference on the planted border
records of tests/trace_shapes.py -- the records tests/test_gpu_trace_shapes.py then holds the kernels to.

tests/golden/trace_shapes_ref_md5.txt holds, per (family, file, mode, pts|mid), the md5 of what oracle/_ref/ref_lastrace
wrote around the reference's Compute_Trace_PTS / Compute_Trace_MID (made by tests/golden/make_trace_shapes_golden.py).
oracle_lastrace's dump must have that md5, and where the reference build is present it is run live and compared record by
record.

Before the md5s were recorded, oracle/ref_lastrace.c and the reference's sources were built once as a stand-alone program
with -fsanitize=address,undefined and run over every file in every mode: a record on which the reference is undefined proves
nothing and belongs in trace_shapes.REMOVED (which stayed empty: the row arithmetic of trace_shapes._wellformed keeps the
planted segments inside the reference's wave rows)."""
import hashlib
import os

import pytest

from conftest import GOLDEN

import trace_shapes as S


def recorded():
    out = {}
    for ln in open(os.path.join(GOLDEN, "trace_shapes_ref_md5.txt")):
        md5, fam, name, mode, kind = ln.split()
        out[(fam, name, int(mode), 1 if kind == "mid" else 0)] = md5
    return out


def test_every_run_is_recorded():
    assert set(recorded()) == {(fam, f.name, m, k) for fam in S.FAMILIES for f in S.family(fam) for m, k in S.jobs(f)}
    for fam in S.FAMILIES:                                     # three modes; MID everywhere, PTS but for mid_drift
        for f in S.family(fam):
            assert f.mid and f.pts == (fam != "mid_drift") and len(S.jobs(f)) == 3 * (f.mid + f.pts)


def test_removed_records_stay_within_their_cap():
    """family() itself refuses more than 2 % of a family or a whole sub-shape"""
    assert set(S.REMOVED) <= set(S.FAMILIES)
    for fam in S.FAMILIES:
        S.family(fam)
    assert sum(len(v) for v in S.REMOVED.values()) == 0        # what the list ended up holding


@pytest.mark.parametrize("fam", list(S.FAMILIES))
def test_family_is_well_formed(fam):
    for f in S.family(fam):
        ts = f.tspace
        assert 0 < ts <= 8192 and f.recs and len(f.reads) <= 2000 and max(len(r) for r in f.reads) <= 13000
        for r in f.recs:
            alen, blen = len(f.reads[r.aread]), len(f.reads[r.bread])
            assert r.aread != r.bread and r.comp in (0, 1)
            assert 0 <= r.abpos < r.aepos <= alen and 0 <= r.bbpos < r.bepos <= blen
            assert r.bbpos + sum(n for _, n in r.pairs[:-1]) < r.bepos
            if r.pairs:
                assert r.bbpos + sum(n for _, n in r.pairs) == r.bepos
                assert len(r.pairs) == (r.aepos - 1) // ts - r.abpos // ts + 1
            assert r.aepos - r.abpos <= 32000 and r.bepos - r.bbpos <= 32000


def test_planted_distance_of_the_heavy_construction():
    """the argument in the module docstring, held against the Levenshtein table for both signs of del"""
    import numpy as np
    rng = np.random.default_rng(11)
    for M, N, D in ((100, 100, 70), (100, 80, 40), (80, 100, 40), (120, 120, 62), (50, 50, 30), (80, 100, 36)):
        a, b = S.plant_heavy(M, N, D, rng)
        assert (len(a), len(b)) == (M, N) and S.edit_distance(a, b) == D + abs(M - N)
    assert S.edit_distance(np.array([0, 1, 2, 3]), np.array([0, 2, 3, 3, 1])) == 3


@pytest.mark.parametrize("fam", list(S.FAMILIES))
def test_oracle_trace_expansion_equals_reference(built, fam):
    want = recorded()
    mine = S.oracle(fam)
    for f in S.family(fam):
        db, las = S.materialize(fam, f)
        for mode, mid in S.jobs(f):
            dump = mine[(f.name, mode, mid)]
            if os.path.exists(S.REF):
                out = las + ".r"
                r = S.run_tool(S.REF, db, las, out, mode, mid)
                assert r.returncode == 0, (fam, f.name, mode, mid, r.stderr)
                live = open(out, "rb").read()
                assert live == dump, "%s mode %d %s: oracle, then reference: %s" % (fam, mode, "mid" if mid else "pts",
                                                                                   S.first_difference(f, dump, live))
                assert hashlib.md5(live).hexdigest() == want[(fam, f.name, mode, mid)], \
                    "the reference no longer answers what was recorded for %s/%s" % (fam, f.name)
            assert hashlib.md5(dump).hexdigest() == want[(fam, f.name, mode, mid)], (fam, f.name, mode, mid)


def test_families_reach_what_they_are_for(built):
    """from the definitions and the oracle's own dumps (tests/test_gpu_trace_shapes.py asserts the same before it trusts a
    family on the GPU)"""
    S.check_reach()


def test_oracle_refuses_the_error_records(built, tmp_path):
    """the two loud exits of the reference (align.c:5575 TP_Error, :4890 TP_Align): the oracle returns -1 on the same records,
    and only there -- the good records in front of them are written"""
    for name, f in S.error_files().items():
        d = str(tmp_path / name)
        S.write_db(d, f.reads)
        las = os.path.join(d, "x.las")
        with open(las, "wb") as o:
            o.write(f.las_bytes())
        r = S.run_tool(S.ORACLE, os.path.join(d, "G"), las, las + ".o", 0, 0)
        assert r.returncode != 0 and "record %d" % (len(f.recs) - 1) in r.stderr, (name, r.stderr)
        if os.path.exists(S.REF):
            r = S.run_tool(S.REF, os.path.join(d, "G"), las, las + ".r", 0, 0)
            msg = "Trace point out of bounds" if name.endswith("points") else "Bad alignment between trace points"
            assert r.returncode != 0 and msg in r.stderr, (name, r.stderr)
