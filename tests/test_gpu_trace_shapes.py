"""kernels/trace_pts.hip at its own borders: the planted records of tests/trace_shapes.py through damar_amd/bin/lastrace,
every dump byte for byte the oracle's (integer work: no tolerance), which tests/test_trace_shapes_host.py pins to the
reference's Compute_Trace_PTS / Compute_Trace_MID on the very same files.

The switches of the expansion are read once per process, so each variant is ONE lastrace -L process that does every file of
every family in all three modes, PTS and MID:

  default    the slot kernel, the stripe kernel behind it for what the documented limits defer
  deferred   DAMAR_TRACE_ROWS=9 DAMAR_TRACE_BLOCKS=7: nine rows, so almost every segment is deferred
  one_block  DAMAR_TRACE_BLOCKS=1: one wavefront takes every batch in turn and reuses its slot area across batches
  unordered  DAMAR_TRACE_ORDER=0: no work order, mixed shapes share a wavefront
  batches    DAMAR_TRACE_MAXSEGS=64: batch borders inside `counts` and `record_walk`

What a family reaches is asserted by trace_shapes.check_reach() on the definitions and the ORACLE's dumps, never on the code
under test.  The two loud exits of the reference are handled error returns of lastrace; each runs in a process of its own
(four: a process ends at its first bad file, so the two "last in a file of good records" cases cannot share one).

Time limits: the default variant's process (135 jobs) took 0.65 s on an MI355X when this was written (SECONDS_DEFAULT; the
other variants 0.56 - 0.84 s, an error process 0.1 s); every process runs under ten times that."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import trace_shapes as S

pytestmark = pytest.mark.gpu

SECONDS_DEFAULT = 0.65
LIMIT = 10 * SECONDS_DEFAULT
LASTRACE = os.path.join(ROOT, "damar_amd", "bin", "lastrace")
SWITCHES = ("DAMAR_TRACE_ROWS", "DAMAR_TRACE_BLOCKS", "DAMAR_TRACE_ORDER", "DAMAR_TRACE_MAXSEGS")
VARIANTS = {
    "default":   {},
    "deferred":  {"DAMAR_TRACE_ROWS": "9", "DAMAR_TRACE_BLOCKS": "7"},
    "one_block": {"DAMAR_TRACE_BLOCKS": "1"},
    "unordered": {"DAMAR_TRACE_ORDER": "0"},
    "batches":   {"DAMAR_TRACE_MAXSEGS": "64"},
}


def _env(extra):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(extra)
    return env


@pytest.fixture(scope="module")
def reach(built):
    S.check_reach()
    return True


_children = {}


@pytest.fixture(scope="module")
def child(built, tmp_path_factory):
    """variant -> ({(family, file, mode, mid): dump}, {the same: deferred segments lastrace -v reports}); one process, once"""
    tmp = tmp_path_factory.mktemp("trace_shapes")

    def get(variant):
        if variant not in _children:
            import time
            keys, lst = [], str(tmp / (variant + ".jobs"))
            with open(lst, "w") as o:
                for fam in S.FAMILIES:
                    for f in S.family(fam):
                        db, las = S.materialize(fam, f)
                        for mode, mid in S.jobs(f):
                            keys.append((fam, f.name, mode, mid))
                            o.write("%d %d %s %s %s %s\n" % (mode, mid, db, db, las, str(tmp / ("%s.%d.bin" % (variant, len(keys))))))
            t0 = time.time()
            r = subprocess.run([LASTRACE, "-v", "-L" + lst], env=_env(VARIANTS[variant]), timeout=LIMIT,
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            print("lastrace, variant %s: %d jobs in %.2f s" % (variant, len(keys), time.time() - t0))
            assert r.returncode == 0, "lastrace (%s): exit %d\n%s" % (variant, r.returncode, r.stderr[-3000:])
            said = re.findall(r"lastrace: (\d+) records, (\d+) segments \((\d+) deferred\)", r.stdout)
            assert len(said) == len(keys)
            dumps, deferred = {}, {}
            for i, k in enumerate(keys):
                with open(str(tmp / ("%s.%d.bin" % (variant, i + 1))), "rb") as fh:
                    dumps[k] = fh.read()
                deferred[k] = int(said[i][2])
            _children[variant] = (dumps, deferred)
        return _children[variant]
    return get


@pytest.mark.parametrize("fam", list(S.FAMILIES))
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_gpu_trace_family_equals_oracle(child, reach, variant, fam):
    dumps, _ = child(variant)
    want = S.oracle(fam)
    bad = []
    for f in S.family(fam):
        for mode, mid in S.jobs(f):
            got = dumps[(fam, f.name, mode, mid)]
            if got != want[(f.name, mode, mid)]:
                bad.append("%s/%s mode %d %s: GPU, then oracle: %s" % (variant, fam, mode, "mid" if mid else "pts",
                                                                      S.first_difference(f, got, want[(f.name, mode, mid)])))
    for b in bad[:20]:
        print(b)
    assert not bad, "%d dump(s) differ, the first: %s" % (len(bad), bad[0])


def test_gpu_trace_deferred_segments_are_those_beyond_the_documented_limits(child, reach):
    """lastrace -v reports how many segments the slot kernel left to the stripe kernel (damar_trace_last, cnt[2]): on the
    single-segment files, PTS, that is the number of records with M or N above 240, |del| + D/2 + 1 >= 40 or D + 2 >= 64,
    D from the oracle's answer"""
    _, deferred = child("default")
    seen = 0
    for fam, f in [(fam, f) for fam in S.SINGLE for f in S.family(fam)] + [("counts", S.family("counts")[-1])]:
        want = sum(S.slot_defers(r.M, r.N, D) for r, D in zip(f.recs, S.oracle_D(fam, f)))
        seen += want
        for mode in S.MODES:
            assert deferred[(fam, f.name, mode, 0)] == want, (fam, f.name, mode)
    assert seen > 400


@pytest.mark.parametrize("name", ["points", "align", "good_then_points", "good_then_align"])
def test_gpu_trace_loud_errors(built, tmp_path, name):
    """`Trace point out of bounds` (a pair that pushes be past blen) and `Bad alignment between trace points` (dmax one
    less than the planted D), alone and as the last record of a file of good ones: lastrace exits non-zero with the
    reference's words, the oracle refuses the same record"""
    f = S.error_files()[name]
    d = str(tmp_path / name)
    S.write_db(d, f.reads)
    las, db = os.path.join(d, "x.las"), os.path.join(d, "G")
    with open(las, "wb") as o:
        o.write(f.las_bytes())
    r = S.run_tool(S.ORACLE, db, las, las + ".o", 0, 0)
    assert r.returncode != 0 and "record %d" % (len(f.recs) - 1) in r.stderr
    msg = "Trace point out of bounds (Compute_Trace), source DB likely incorrect" if name.endswith("points") else \
          "Bad alignment between trace points (Compute_Trace), source DB likely incorrect"
    for mid in ([], ["-M"]):
        r = subprocess.run([LASTRACE, "-m0"] + mid + [db, db, las, las + ".g"], env=_env({}), timeout=LIMIT,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 1 and msg in r.stderr, (name, mid, r.returncode, r.stderr[-1000:])
        assert not os.path.exists(las + ".g")


def test_gpu_trace_same_buffer_against_oracle(built):
    """flags & 2, align.c:4930-4947: A and B are ONE buffer, the band is clipped at the identity diagonal (posl / posh).
    ref_lastrace loads B into a buffer of its own and cannot reach this, so this leg is pinned to the ORACLE only, not to
    the reference.  Through the C entry (Compute_Trace_PTS / _MID) with aseq == bseq and bbpos ahead of and behind abpos by
    1, 5 and 50, on random sequence, where D / 2 of a segment exceeds the offset: the oracle's answer with B in a copy of
    the buffer (no clipping) is a different one at every offset."""
    from damar_amd import api
    lib = api.lib()
    ora = ctypes.CDLL(os.path.join(ROOT, "oracle", "liboracle.so"))

    class Path(ctypes.Structure):
        _fields_ = [("trace", ctypes.c_void_p), ("tlen", ctypes.c_int), ("diffs", ctypes.c_int),
                    ("abpos", ctypes.c_int), ("bbpos", ctypes.c_int), ("aepos", ctypes.c_int), ("bepos", ctypes.c_int)]

    class Alignment(ctypes.Structure):
        _fields_ = [("path", ctypes.POINTER(Path)), ("flags", ctypes.c_uint32), ("aseq", ctypes.c_void_p),
                    ("bseq", ctypes.c_void_p), ("alen", ctypes.c_int), ("blen", ctypes.c_int)]

    sig = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(Path), ctypes.c_int, ctypes.c_int,
           ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
    ora.oracle_compute_trace_pts.argtypes = ora.oracle_compute_trace_mid.argtypes = sig
    lib.New_Work_Data.restype = ctypes.c_void_p
    lib.Free_Work_Data.argtypes = [ctypes.c_void_p]
    lib.Compute_Trace_PTS.argtypes = lib.Compute_Trace_MID.argtypes = [ctypes.POINTER(Alignment), ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    rng = np.random.default_rng(17)
    n = 720
    buf = np.concatenate([[4], rng.integers(0, 4, n), [4]]).astype(np.int8)
    copy = buf.copy()
    seq = buf.ctypes.data + 1
    work = lib.New_Work_Data()
    # (tspace, abpos, aepos, offset of B): one segment each, and two segments at +-5
    cases = [(100, 100, 200, o) for o in (1, -1, 5, -5)] + [(300, 300, 600, o) for o in (50, -50)] + [(100, 100, 300, o) for o in (5, -5)]

    def oracle(kind, bptr, ts, ab, ae, off, mode):
        tp = np.array([ts, ts] * ((ae - ab) // ts), dtype=np.uint16)
        p = Path(tp.ctypes.data, len(tp), 0, ab, ab + off, ae, ae + off)
        script = np.zeros(2 * n + 16, dtype=np.int32)
        d = ctypes.c_int(0)
        k = (ora.oracle_compute_trace_mid if kind else ora.oracle_compute_trace_pts)(seq, n, bptr, n, ctypes.byref(p), ts, mode,
                                                                                    script.ctypes.data, ctypes.byref(d))
        assert k >= 0
        return script[:k].tolist(), d.value

    for ts, ab, ae, off in cases:
        for kind in (0, 1):
            for mode in S.MODES:
                want = oracle(kind, seq, ts, ab, ae, off, mode)
                assert want != oracle(kind, copy.ctypes.data + 1, ts, ab, ae, off, mode), "the band is not clipped at offset %d" % off
                tp = np.array([ts, ts] * ((ae - ab) // ts), dtype=np.uint16)
                p = Path(tp.ctypes.data, len(tp), 0, ab, ab + off, ae, ae + off)
                al = Alignment(ctypes.pointer(p), 0, seq, seq, n, n)
                assert (lib.Compute_Trace_MID if kind else lib.Compute_Trace_PTS)(ctypes.byref(al), work, ts, mode) == 0
                got = np.ctypeslib.as_array(ctypes.cast(p.trace, ctypes.POINTER(ctypes.c_int)), shape=(max(p.tlen, 1),))[:p.tlen].tolist()
                assert (got, p.diffs) == want, "offset %d spacing %d mode %d %s" % (off, ts, mode, "mid" if kind else "pts")
    lib.Free_Work_Data(work)
