"""bin/LAcheck and the checking routine behind it (csrc/host/lascheck.c) against the reference suite's own LAcheck
(oracle/_ref/LAcheck, built by build() from the reference's sources): clean goldens, files damaged at run time, the
strict set the reference does not have, and the routine itself through ctypes.  No GPU needed."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT, GOLDEN, golden_cases, read_case

OURS = os.path.join(ROOT, "damar_amd", "bin", "LAcheck")
REF = os.path.join(ROOT, "oracle", "_ref", "LAcheck")

SUBSETS = [["-p"], ["-s"], ["-d"], ["-p", "-s", "-d"], ["-i", "-p", "-s", "-d"]]


@pytest.fixture(scope="module")
def ref(built):
    if not os.path.exists(REF):
        pytest.skip("oracle/_ref/LAcheck not built (needs the reference's sources at build time)")
    return REF


def run(exe, opts, db, las):
    r = subprocess.run([exe] + list(opts) + [db, las], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    return r.returncode, r.stderr, r.stdout


# ---- .las files as lists of records ------------------------------------------------------------------------------------

TLEN, DIFFS, ABPOS, BBPOS, AEPOS, BEPOS, FLAGS, AREAD, BREAD, PAD = range(10)


def read_las(path):
    """-> (novl, tspace, [[10 int32 fields as a list, trace bytes as a bytearray], ...])"""
    raw = open(path, "rb").read()
    novl, tspace = struct.unpack_from("<qi", raw, 0)
    tbytes = 1 if tspace <= 125 else 2
    recs, off = [], 12
    for _ in range(novl):
        f = list(struct.unpack_from("<10i", raw, off))
        n = tbytes * f[TLEN]
        recs.append([f, bytearray(raw[off + 40:off + 40 + n])])
        off += 40 + n
    assert off == len(raw)
    return novl, tspace, recs


def write_las(path, tspace, recs, novl=None):
    with open(path, "wb") as f:
        f.write(struct.pack("<qi", len(recs) if novl is None else novl, tspace))
        for fields, trace in recs:
            f.write(struct.pack("<10i", *fields))
            f.write(bytes(trace))
    return path


def copy(recs):
    return [[list(f), bytearray(t)] for f, t in recs]


def read_lengths(dbdir, root="G"):
    """rlen of every read of the whole database (the .idx file: an 88-byte header, then 32 bytes per read, rlen first)"""
    x = np.fromfile(os.path.join(dbdir, ".%s.idx" % root), dtype=np.uint8)[88:]
    return x.reshape(-1, 32)[:, :4].copy().view("<i4").ravel()


def sort_key(f):
    return (f[AREAD], f[BREAD], f[FLAGS] & 1, f[ABPOS])


BASE_CASE, BASE_LAS = "tiny2", os.path.join("d001_00001", "G.1.G.1.las")


@pytest.fixture(scope="module")
def base():
    case = read_case(BASE_CASE)
    novl, tspace, recs = read_las(os.path.join(case["lasdir"], BASE_LAS))
    assert novl >= 300 and tspace == 100
    return dict(db=os.path.join(case["dbdir"], "G"), lens=read_lengths(case["dbdir"]), tspace=tspace, recs=recs)


def middle(recs, ok):
    """the first index from the middle of the file on for which ok(i) holds"""
    for i in range(len(recs) // 2, len(recs) - 1):
        if ok(i):
            return i
    raise AssertionError("the golden file has no record the case can be made from")


def groups(recs):
    """[(aread, first, end)] of the runs of equal A read"""
    out, s = [], 0
    for i in range(1, len(recs) + 1):
        if i == len(recs) or recs[i][0][AREAD] != recs[s][0][AREAD]:
            out.append((recs[s][0][AREAD], s, i))
            s = i
    return out


def damage(kind, b):
    """-> (records, announced count or None) of damaged file `kind`, made from the golden records b['recs']"""
    r = copy(b["recs"])
    novl = None
    if kind == "a_swapped":
        i = middle(r, lambda i: r[i][0][AREAD] == r[i + 1][0][AREAD] and sort_key(r[i][0]) < sort_key(r[i + 1][0]))
        r[i], r[i + 1] = r[i + 1], r[i]
    elif kind == "b_twice":
        i = middle(r, lambda i: True)
        r.insert(i, [list(r[i][0]), bytearray(r[i][1])])
    elif kind in ("c_bvalue_up", "c_bvalue_down"):
        i = middle(r, lambda i: r[i][0][TLEN] >= 6 and 1 <= r[i][1][3] <= 254)
        r[i][1][3] += 1 if kind.endswith("up") else -1
    elif kind == "d_aepos":
        i = middle(r, lambda i: True)
        r[i][0][AEPOS] = int(b["lens"][r[i][0][AREAD]]) + 1
    elif kind == "e_abpos":
        i = middle(r, lambda i: True)
        r[i][0][ABPOS] = -1
    elif kind == "f_count_high":
        novl = len(r) + 1
    elif kind == "f_count_low":
        novl = len(r) - 1
    elif kind == "g_group_moved":
        g = groups(r)
        assert len(g) >= 8
        (_, s0, e0), (_, s1, e1) = g[len(g) // 3], g[2 * len(g) // 3]
        r = r[:s0] + r[s1:e1] + r[s0:s1] + r[e1:]
    elif kind == "h_diff":
        i = middle(r, lambda i: r[i][0][TLEN] >= 6 and r[i][1][2] <= 254)
        r[i][1][2] += 1
    elif kind == "i_pair_removed":
        i = middle(r, lambda i: r[i][0][TLEN] >= 8 and r[i][1][3] + r[i][1][5] <= 255 and r[i][1][2] + r[i][1][4] <= 255)
        t = r[i][1]
        t[4] += t[2]                       # (the differences move along too: only the number of pairs is wrong)
        t[5] += t[3]
        del t[2:4]
        r[i][0][TLEN] -= 2
    elif kind == "j_padding":
        i = middle(r, lambda i: True)
        r[i][0][PAD] = 0x00010000
    else:
        raise AssertionError(kind)
    return r, novl


DAMAGED = ["a_swapped", "b_twice", "c_bvalue_up", "c_bvalue_down", "d_aepos", "e_abpos", "f_count_high", "f_count_low",
           "g_group_moved"]
STRICT_ONLY = ["h_diff", "i_pair_removed", "j_padding"]


# ---- clean files -------------------------------------------------------------------------------------------------------

def cases_with_files():
    return [n for n in golden_cases() if read_case(n)["las"]]


@pytest.mark.parametrize("name", cases_with_files())
def test_clean_goldens_pass_like_the_reference_and_pass_strict(ref, name):
    """Every golden .las with its database: -p -s -d is silent with status 0 for both tools, and -x (every golden was
    written by daligner or datander) finds nothing either.  The one exception is the reference's own doing: a case run
    with -T has records without trace points, of which the reference's -p says "pass-through points inconsistent"
    (status 1).  There the two tools must still agree on that text, and -s -d must be clean, with -x as well."""
    case = read_case(name)
    db = os.path.join(case["dbdir"], "G")
    assert case["las"]
    for rel in case["las"]:
        las = os.path.join(case["lasdir"], rel)
        want = run(ref, ["-p", "-s", "-d"], db, las)
        got = run(OURS, ["-p", "-s", "-d"], db, las)
        if "-T" in case["opts"]:
            assert got == want and want[0] == 1, (rel, want, got)
            assert run(ref, ["-s", "-d"], db, las) == (0, "", "") == run(OURS, ["-s", "-d"], db, las), rel
            assert run(OURS, ["-x", "-s", "-d"], db, las) == (0, "", ""), rel
            continue
        assert want == (0, "", "") and got == want, (rel, want, got)
        assert run(OURS, ["-x", "-p", "-s", "-d"], db, las) == (0, "", ""), rel


# ---- damaged files -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("opts", SUBSETS, ids=["".join(o) for o in SUBSETS])
@pytest.mark.parametrize("kind", DAMAGED)
def test_damaged_files_are_reported_like_the_reference(ref, base, tmp_path, kind, opts):
    """Exit status, stderr and stdout of bin/LAcheck equal the reference tool's on a golden file damaged in one place
    (cases (a) to (g) of the checker's specification), under every option subset.  The reference reads on until the count
    of the header is reached: with the count one too high it looks once more at the slot behind its last group, which
    holds a record of an earlier, larger group -- the golden file used here ends in a group that is smaller than an
    earlier one, so what it finds there is defined, and the tool must say the same."""
    recs, novl = damage(kind, base)
    if kind == "f_count_high":
        g = groups(recs)
        assert max(e - s for _, s, e in g[:-1]) > g[-1][2] - g[-1][1]
    las = write_las(str(tmp_path / "damaged.las"), base["tspace"], recs, novl)
    want = run(ref, opts, base["db"], las)
    got = run(OURS, opts, base["db"], las)
    print(kind, opts, want)
    assert want[0] in (0, 1)
    assert got == want


def test_every_damage_is_seen_by_some_reference_option(ref, base, tmp_path):
    """(the cases above are not vacuous: under -p -s -d the reference reports each of them)"""
    for kind in DAMAGED:
        recs, novl = damage(kind, base)
        las = write_las(str(tmp_path / ("%s.las" % kind)), base["tspace"], recs, novl)
        st, err, _ = run(ref, ["-p", "-s", "-d"], base["db"], las)
        assert st == 1 and err != "", kind


# ---- the strict set ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", STRICT_ONLY)
def test_strict_set_reports_what_the_reference_options_do_not(ref, base, tmp_path, kind):
    recs, novl = damage(kind, base)
    las = write_las(str(tmp_path / "damaged.las"), base["tspace"], recs, novl)
    assert run(ref, ["-p", "-s", "-d"], base["db"], las) == (0, "", "")
    assert run(OURS, ["-p", "-s", "-d"], base["db"], las) == (0, "", "")
    st, err, out = run(OURS, ["-x", "-p", "-s", "-d"], base["db"], las)
    lines = err.splitlines()
    print(kind, lines)
    assert st == 1 and len(lines) == 1 and lines[0].startswith("strict: overlap ")
    want = {"h_diff": "differences", "i_pair_removed": "trace pairs", "j_padding": "padding"}[kind]
    assert want in lines[0]


def test_usage_and_missing_file_status(built, tmp_path):
    assert subprocess.run([OURS], stderr=subprocess.PIPE).returncode == 1
    r = subprocess.run([OURS, os.path.join(GOLDEN, BASE_CASE, "G"), str(tmp_path / "none.las")], stderr=subprocess.PIPE, text=True)
    assert r.returncode == 1 and "could not open" in r.stderr


# ---- the routine itself --------------------------------------------------------------------------------------------------

class Path(C.Structure):
    _fields_ = [("trace", C.c_void_p), ("tlen", C.c_int), ("diffs", C.c_int), ("abpos", C.c_int), ("bbpos", C.c_int),
                ("aepos", C.c_int), ("bepos", C.c_int)]


class Overlap(C.Structure):
    _fields_ = [("path", Path), ("flags", C.c_uint32), ("aread", C.c_int), ("bread", C.c_int), ("pad", C.c_uint32)]


REPORT = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_char_p)


class Checker(C.Structure):                          # include/damar_check.h: damar_lascheck
    _fields_ = [("tspace", C.c_int), ("options", C.c_int), ("report", REPORT), ("arg", C.c_void_p),
                ("seen", C.c_int64), ("looked", C.c_int64), ("violations", C.c_int64),
                ("stopped", C.c_int), ("have_prev", C.c_int), ("split", C.c_int), ("prev_a", C.c_int), ("prev", Overlap)]


PTP, SORT, DUPES, IGNORE, STRICT, PADBIT, ALL = 1, 2, 4, 8, 16, 32, 64
WRITER = PTP | SORT | DUPES | STRICT | ALL           # what `daligner -C` runs over every file it writes


def feed_all(L, recs, lens, tspace, options, novl=None):
    """-> (violations, records seen, records looked at, messages) of the routine fed with recs"""
    assert C.sizeof(Overlap) == 48
    said = []
    cb = REPORT(lambda arg, kind, text: said.append((kind, text.decode())))
    ck = Checker()
    L.damar_lascheck_begin.argtypes = [C.POINTER(Checker), C.c_int, C.c_int, REPORT, C.c_void_p]
    L.damar_lascheck_feed.argtypes = [C.POINTER(Checker), C.POINTER(Overlap), C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.damar_lascheck_end.argtypes = [C.POINTER(Checker), C.c_int64]
    L.damar_lascheck_end.restype = C.c_int64
    L.damar_lascheck_begin(C.byref(ck), tspace, options, cb, None)
    for f, t in recs:
        o = Overlap()
        o.path.tlen, o.path.diffs, o.path.abpos, o.path.bbpos, o.path.aepos, o.path.bepos = f[:6]
        o.flags, o.aread, o.bread, o.pad = f[FLAGS] & 0xffffffff, f[AREAD], f[BREAD], f[PAD] & 0xffffffff
        buf = (C.c_uint8 * max(len(t), 1)).from_buffer_copy(bytes(t) or b"\0")
        L.damar_lascheck_feed(C.byref(ck), C.byref(o), buf, 1, int(lens[f[AREAD]]), int(lens[f[BREAD]]))
    v = L.damar_lascheck_end(C.byref(ck), len(recs) if novl is None else novl)
    return v, ck.seen, ck.looked, said


def test_routine_on_a_clean_golden_counts_and_finds_nothing(built, base):
    from damar_amd import api
    L = api.lib()
    v, seen, looked, said = feed_all(L, base["recs"], base["lens"], base["tspace"], WRITER | PADBIT)
    assert (v, seen, looked, said) == (0, len(base["recs"]), len(base["recs"]), [])
    # -i: a record flagged as discarded is counted, not looked at
    r = copy(base["recs"])
    r[5][0][FLAGS] |= 2
    r[5][0][ABPOS] = -1
    v, seen, looked, said = feed_all(L, r, base["lens"], base["tspace"], PTP | SORT | DUPES | IGNORE)
    assert (v, seen, looked) == (0, len(r), len(r) - 1)
    v, seen, looked, said = feed_all(L, r, base["lens"], base["tspace"], PTP | SORT | DUPES)
    assert v >= 1 and any("abpos < 0" in m for _, m in said)


@pytest.mark.parametrize("kind", DAMAGED + STRICT_ONLY)
def test_writer_option_set_fires_on_damaged_record_arrays(built, base, kind):
    """What `daligner -C` runs in the thread that writes a file (-p -s -d, the strict set, no stop at the first A read
    with a violation), driven here on damaged record arrays: every kind of damage is counted, and the records behind
    it are still looked at."""
    from damar_amd import api
    L = api.lib()
    recs, novl = damage(kind, base)
    options = WRITER | (PADBIT if kind == "j_padding" else 0)
    v, seen, looked, said = feed_all(L, recs, base["lens"], base["tspace"], options, novl)
    print(kind, v, said[:4])
    assert v >= 1 and seen == len(recs) == looked
    assert len([1 for k, _ in said if k == 0]) == v


# ---- the writer of las.c with the check on (what `daligner -C` switches on), driven on the CPU ---------------------------

def write_through_las_c(L, api, recs, tspace, block, outdir):
    """recs through New_Align_Spec / AddOverlapToBuffer / Write_Overlap_Buffer as the block pair G.1 x G.1 -> the file"""
    L.OVL_IO_Buffer.restype = C.c_void_p
    L.OVL_IO_Buffer.argtypes = [C.c_void_p]
    L.AddOverlapToBuffer.argtypes = [C.c_void_p, C.POINTER(Overlap), C.c_int]
    spec = L.New_Align_Spec(.70, tspace, block.freq, 1, 1, 0, 0, 1)
    L.damar_check_note_blocks(spec, C.byref(block), None)
    buf = L.OVL_IO_Buffer(spec)
    for f, t in reversed(recs):                      # (any order: the writer sorts)
        o = Overlap()
        raw = (C.c_uint8 * max(len(t), 1)).from_buffer_copy(bytes(t) or b"\0")
        o.path.trace = C.addressof(raw)
        o.path.tlen, o.path.diffs, o.path.abpos, o.path.bbpos, o.path.aepos, o.path.bepos = f[:6]
        o.flags, o.aread, o.bread = f[FLAGS] & 0xffffffff, f[AREAD], f[BREAD]
        assert L.AddOverlapToBuffer(buf, C.byref(o), 1) == 0
    L.Write_Overlap_Buffer(spec, outdir.encode(), outdir.encode(), b"G.1", b"G.1", block.ufirst + block.nreads - 1)
    L.Reset_Overlap_Buffer(spec)
    L.Free_Align_Spec(spec)
    return os.path.join(outdir, "G.1.G.1.las")


def test_writer_with_the_check_on_counts_reports_and_still_writes(built, base, tmp_path, capfd):
    """damar_set_check(1): a clean set of records is written as the golden file and counted; with damaged records every
    violation is a `damar: CHECK <file>: ...` line (16 per file at most, then the total), the totals carry them, and the
    file is written all the same.  With the check off the same damaged records pass without a word."""
    from damar_amd import api
    L = api.lib()
    case = read_case(BASE_CASE)
    block = api.read_block(os.path.join(case["dbdir"], "G.1"))
    golden = open(os.path.join(case["lasdir"], BASE_LAS), "rb").read()
    n = len(base["recs"])
    try:
        api.set_check(True)
        t0 = api.check_totals()
        os.makedirs(str(tmp_path / "clean"))
        out = write_through_las_c(L, api, base["recs"], base["tspace"], block, str(tmp_path / "clean"))
        t1 = api.check_totals()
        assert open(out, "rb").read() == golden
        assert [y - x for x, y in zip(t0, t1)] == [1, n, 0, 0]
        assert "CHECK" not in capfd.readouterr().err

        one, _ = damage("c_bvalue_up", base)
        os.makedirs(str(tmp_path / "one"))
        out = write_through_las_c(L, api, one, base["tspace"], block, str(tmp_path / "one"))
        t2 = api.check_totals()
        err = capfd.readouterr().err.splitlines()
        assert [y - x for x, y in zip(t1, t2)] == [1, n, 1, 0]
        assert len(err) == 1 and err[0].startswith("damar: CHECK %s: overlap " % out) and "pass-through points inconsistent" in err[0]
        assert read_las(out)[0] == n                                     # (written all the same)

        many = copy(base["recs"])
        for i in range(10, 50):
            many[i][0][AEPOS] = int(base["lens"][many[i][0][AREAD]]) + 1  # aepos > lena, and a panel count that no longer fits
        os.makedirs(str(tmp_path / "many"))
        out = write_through_las_c(L, api, many, base["tspace"], block, str(tmp_path / "many"))
        t3 = api.check_totals()
        err = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("damar: CHECK")]
        assert t3[2] - t2[2] >= 40 and t3[1] - t2[1] == n
        assert len(err) == 17 and "violations in all" in err[-1] and any("aepos > lena" in ln for ln in err)

        api.set_check(False)
        os.makedirs(str(tmp_path / "off"))
        write_through_las_c(L, api, many, base["tspace"], block, str(tmp_path / "off"))
        assert api.check_totals() == t3 and capfd.readouterr().err == ""
    finally:
        api.set_check(False)
