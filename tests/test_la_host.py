"""Local_Alignment: the oracle's restatement (oracle/wave.c) against the REAL reference on the task families of
tests/la_shapes.py -- the shapes tests/test_gpu_la_shapes.py then holds the kernels to.

tests/golden/la_ref_md5.txt holds, per family, the md5 of what the reference's Local_Alignment (align.c:1904, called the way
filter.c:2316 calls it by oracle/ref_localalign.c) leaves in both paths and both traces of every task (made by
tests/golden/make_la_golden.py).  The oracle's answers, written in the same format, must have that md5, and where the
reference build is present (oracle/_ref) they must equal the reference run live, task for task.

Before a family was recorded, the driver and the reference's sources were built once as a stand-alone program with
-fsanitize=address,undefined and run over every family: a task on which the reference reads out of bounds or is otherwise
undefined, or on which the oracle reports an empty band, proves nothing and is listed in la_shapes.REMOVED."""
import hashlib
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import la_shapes as S


def recorded():
    out = {}
    for ln in open(os.path.join(GOLDEN, "la_ref_md5.txt")):
        md5, name, n = ln.split()
        out[name] = (md5, int(n))
    return out


def test_every_family_is_recorded():
    assert set(recorded()) == set(S.FAMILIES)


def test_removed_tasks_stay_within_their_cap():
    """family() itself refuses more than 2 % of a family or a whole sub-shape; nothing may be listed for a family that is gone"""
    assert set(S.REMOVED) <= set(S.FAMILIES)
    for name in S.FAMILIES:
        S.family(name)


@pytest.mark.parametrize("name", list(S.FAMILIES))
def test_family_is_well_formed(name):
    for g in S.family(name):
        assert 0 < g.tspace <= 8192 and g.comp in (0, 1) and len(g.tasks) == len(g.tags) > 0
        for t, (ar, br, dg, anti) in enumerate(g.tasks):
            al, bl = g.lens(t)
            assert (anti + dg) % 2 == 0
            x, y = g.point(t)
            assert 0 <= x <= al and 0 <= y <= bl
            assert max(al, bl) <= 20600


@pytest.mark.parametrize("name", list(S.FAMILIES))
def test_oracle_local_alignment_equals_reference(built, tmp_path, name):
    md5, ntasks = recorded()[name]
    groups = S.family(name)
    assert sum(len(g.tasks) for g in groups) == ntasks
    res = S.oracle(name)
    empty = [(g.name, t, g.tags[t]) for g, (_, stats) in zip(groups, res) for t, st in enumerate(stats) if st.empty_band]
    assert not empty, "the oracle ran a wave on an empty band (undefined in the reference): %s" % empty
    mine = b"".join(S.dump(ans) for ans, _ in res)
    ref = os.path.join(ROOT, "oracle", "_ref", "ref_localalign")
    if os.path.exists(ref):
        fam, out = str(tmp_path / "f.fam"), str(tmp_path / "f.bin")
        S.write_family(fam, groups)
        subprocess.run([ref, fam, out], check=True)
        live = open(out, "rb").read()
        if live != mine:                                   # say which task, which field
            pos = 0
            for g, (ans, _) in zip(groups, res):
                for t, (p, at, bt) in enumerate(ans):
                    rp = list(struct.unpack("<12i", live[pos:pos + 48]))
                    pos += 48
                    rat = np.frombuffer(live[pos:pos + 2 * rp[5]], "<u2").tolist()
                    pos += 2 * rp[5]
                    rbt = np.frombuffer(live[pos:pos + 2 * rp[11]], "<u2").tolist()
                    pos += 2 * rp[11]
                    assert (rp, rat, rbt) == (p, list(at), list(bt)), \
                        "%s task %d (%s) reads %s seed %s: reference, then oracle" % (g.name, t, g.tags[t], g.lens(t), g.point(t))
        assert hashlib.md5(live).hexdigest() == md5, "the reference no longer answers what was recorded for %s" % name
    assert hashlib.md5(mine).hexdigest() == md5


def test_wave_stats_mirror_follows_oracle_h(built):
    """maxband, empty_band and the rest are read through a ctypes mirror of OWaveStats: oracle_api.lib() checks its size and
    four field offsets against the C struct; here the fields of one task with a single mismatch are held against each other"""
    import oracle_api as O
    a = np.array([0, 1, 2, 3] * 10, dtype=np.uint8)
    b = a.copy()
    b[20] ^= 1
    adb, bdb = S.make_db([a]), S.make_db([b])
    spec = O.lib().New_Align_Spec(.70, 100, adb.freq, 1, 1, 0, 0, 1)
    st = O.OWaveStats()
    p, at, bt = O.local_alignment(adb, bdb, 0, 0, 0, 0, 40, spec, 8, st)
    assert p[:5] == [0, 0, 40, 40, 1]
    assert st.empty_band == 0 and st.dirs == 2 and st.waves == sum(st.bandhist) > 0
    assert 0 <= st.maxband <= 5 and st.cells <= st.maxband * st.waves
    assert sum(i * n for i, n in enumerate(st.bandhist)) in (3, 6)      # one or two steps of the three diagonals behind a mismatch
    assert st.steps_narrow + st.steps_wide == st.waves and st.pebbles > 0


def test_families_reach_what_they_are_for(built):
    """the reach of each family, from the oracle's own statistics (tests/test_gpu_la_shapes.py asserts the same before it
    trusts a family on the GPU)"""
    S.check_reach()
