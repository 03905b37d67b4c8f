"""Deterministic piles at the borders of kernels/pile_filter.hip (runs of one B read met 64 records at a time and walked by one
lane; the -R 4 count; the hand-overs between its steps; FL_REPCAP repeat values in LDS; one coverage bit per base in words of
32, the lanes over the words; the divisions in double; two-byte traces), one pile each on an A read of its own length, and
seeded random piles with runs of up to 70 records.  The reads are the shapes' own: read 0 and the last read serve the -A, -x
and -I lists, reads 1 .. are the A reads, then a pool of B reads of BLEN bases, BREP (a B read of 513 repeat intervals) and LB
(one B read for every run that needs no other).

shapes() -> the Shapes on traces of spacing 100, shapes200() -> the few on spacing 200 (two-byte traces); arrays(S) -> the
batch api.pile_filter takes; tracks() -> trim and repeat track; params(key) -> the keywords of an option set.  Every shape
states under `expect` the letter (code()) of each of its records under the option sets it is meant for; '?' stands for any."""
import hashlib

import numpy as np

import filter_common as fc
import filter_model as fm
from filter_model import DISCARD, LOCAL

WAVE, GROUP, U = 64, 64, 32              # lanes; DAMAR_FILTER_MAXGROUP; the -u of the coverage shapes
NA = 120                                 # reads 1 .. NA: the shapes' A reads
POOL, NPOOL = NA + 1, 220                # the pool of B reads
BREP = POOL + NPOOL
LB = BREP + 1
LAST = LB + 1
NREADS = LAST + 1
BLEN = 8000
SELF = -1                                # a record's B read: the pile's A read

OPTION_SETS = dict([
    ("def", []), ("plan", ["-d", "20", "-n", "500", "-o", "1000", "-u", "0", "-s", "300"]), ("S", ["-S", "300"]), ("s", ["-s", "300"]),
    ("R63", ["-R", "6", "-R", "3"]), ("R20", ["-R", "2", "-R", "0"]), ("R2", ["-R", "2"]), ("wz", ["-w", "-z", "2"]),
    ("zu", ["-z", "2", "-u", str(U)]), ("b", ["-b", "30"]), ("n", ["-n", "500"]), ("nY", ["-n", "500", "-Y", "300"]),
    ("R6s", ["-s", "300", "-R", "6", "-R", "2"]), ("A", ["-A", "sym.txt"]), ("x", ["-x", "x.txt"]), ("I", ["-I", "i.txt"]), ("f", ["-f", "50"]),
    ("R4", ["-R", "4"]), ("R5", ["-R", "5"]), ("d", ["-d", "20"]), ("o", ["-o", "1000"]), ("u", ["-u", "100"]), ("l", ["-l", "3000"]),
    ("vw", ["-w", "-R", "6"]), ("R6", ["-R", "6"]), ("R46", ["-R", "4", "-R", "6"]), ("so", ["-s", "300", "-o", "1000"]),
    ("sd", ["-s", "300", "-d", "20"])])
SETS_200 = ("def", "b", "R2", "R20")     # what the shapes on two-byte traces are run under
RANDOM_SETS = ("plan", "R6s", "vw", "zu", "R46", "nY")


def P(i):
    assert 0 <= i < NPOOL
    return POOL + i


def R(b, ab, ae, bb=None, be=None, fl=0, df=0, tr=None):
    """a record: B coordinates as A's unless given; tr: its trace values (diffs, B length, ...), or made by trace_of"""
    bb = ab if bb is None else bb
    return (b, ab, ae, bb, bb + (ae - ab) if be is None else be, fl, df, tr)


def trace_of(ab, ae, bb, be, df, ts):
    """B's bases shared out over A's segments, the differences from the first on, at most 40 a segment"""
    cuts = [ab] + list(range((ab // ts + 1) * ts, ae, ts)) + [ae]
    al = np.diff(cuts)
    extra = (be - bb) - (ae - ab)
    bl = al + extra // len(al) + (np.arange(len(al)) < extra % len(al))
    assert np.all(bl >= 0) and bl.sum() == be - bb
    out = []
    for k in range(len(al)):
        out += [min(df, 40), int(bl[k])]
        df -= out[-2]
    assert df == 0
    return out


class Shape:
    def __init__(self, tag, border, alen, recs, trim=None, rep=(), expect=None, over=False, tspace=100):
        self.tag, self.border, self.alen, self.recs, self.trim, self.rep = tag, border, alen, list(recs), trim or (0, alen), list(rep)
        self.expect, self.over, self.tspace, self.aread = expect or {}, over, tspace, None      # over: a run above GROUP, the host's

    def max_run(self):
        return max(len(r) for r in fm.runs([dict(b=r[0]) for r in self.recs]))


def pile(n, runs=None):
    """n records, each a run of its own (record i on pool read i), but for `runs`: {first record: [(ab, ae, ...), ...]}"""
    recs = [R(P(i), 0, 1000) for i in range(n)]
    for i0, rr in (runs or {}).items():
        for j, r in enumerate(rr):
            recs[i0 + j] = R(P(i0), *r)
    return recs


def mark(n, at=None, rest="."):
    """n letters `rest`, but for {first record: letters}"""
    out = [rest] * n
    for i0, s in (at or {}).items():
        out[i0:i0 + len(s)] = list(s)
    assert len(out) == n
    return "".join(out)


def covered(alen, holes, trim=None, partners=4, extra=()):
    """as the planted zu_at: `partners` B reads, each with one record per stretch of the read between the holes; a record
    far from an end of the trim interval ends on that side at its B read's end, so that -u lets it live"""
    tb, te = trim or (0, alen)
    edges = [0] + [x for h in holes for x in h] + [alen]
    recs = []
    for p in range(partners):
        for ab, ae in zip(edges[0::2], edges[1::2]):
            far_b, far_e = ab - tb > U, te - ae > U
            assert not (far_b and far_e) and ab < ae
            recs.append(R(P(p), ab, ae, BLEN - (ae - ab) if far_e else 0))
    return recs + list(extra)


def shapes():
    S = []
    add = lambda *a, **k: S.append(Shape(*a, **k))

    # ---- runs and chunks: runs are met 64 records at a time, the lane of a run's first record walks it alone ----------------
    run2 = [(0, 2000), (100, 900)]                                     # the second inside the first
    run3 = [(0, 1000), (1010, 2000), (100, 900)]                       # the second stitches to the first, the third lies in it
    runk = lambda k: [(0, 2000)] + [(10 * j, 10 * j + 500) for j in range(1, k)]       # all inside the first
    for i0 in (63, 64):
        add("run2_at%d" % i0, "a run of 2 beginning at record %d" % i0, 3000, pile(i0 + 4, {i0: run2}),
            expect=dict(R6=mark(i0 + 4, {i0: ".C"}), vw=mark(i0 + 4, {i0: "DD"}), s=mark(i0 + 4)))
        add("run3_at%d" % i0, "a run of 3 beginning at record %d" % i0, 3000, pile(i0 + 5, {i0: run3}),
            expect=dict(R6=mark(i0 + 5, {i0: "..C"}), vw=mark(i0 + 5, {i0: "DDD"}), s=mark(i0 + 5, {i0: ".T."})))
        add("run64_at%d" % i0, "a run of 64 beginning at record %d" % i0, 3000, pile(i0 + 66, {i0: runk(64)}),
            expect=dict(R6=mark(i0 + 66, {i0: "." + "C" * 63}), vw=mark(i0 + 66, {i0: "D" * 64})))
    add("run64_at1", "a run of 64 beginning at record 1", 3000, pile(66, {1: runk(64)}), expect=dict(R6=mark(66, {1: "." + "C" * 63})))
    add("run65_at63", "a run of 65 beginning at record 63: the host's", 3000, pile(130, {63: runk(65)}), over=True,
        expect=dict(R6=mark(130, {63: "." + "C" * 64})))
    for n in (63, 64, 65, 127, 128, 129):
        add("n%d" % n, "%d runs of one record" % n, 3000, pile(n), expect={"def": mark(n), "R6": mark(n), "vw": mark(n), "s": mark(n)})
    add("pairs_odd_130", "130 records, runs of 2 at the odd records: one lies at 63|64", 3000, pile(130, {i: run2 for i in range(1, 129, 2)}),
        expect=dict(R6="." + ".C" * 64 + ".", vw="." + "DD" * 64 + "."))
    add("chain3_63", "a stitch chain of three whose head is record 63", 3000, pile(67, {63: [(0, 1000), (1010, 2000), (2005, 3000)]}),
        expect=dict(s=mark(67, {63: ".TT"}), S=mark(67, {63: ".TT"})))
    add("two_cand_63", "a stitch partner chosen by length among two candidates in the next chunk", 3000,
        pile(67, {63: [(0, 1000), (1010, 1500), (1020, 2500)]}), expect=dict(s=mark(67, {63: "..T"})))
    add("w_63_65", "a -w containment between record 63 and record 65, the run's last", 3000,
        pile(67, {63: [(0, 2000), (2100, 2500), (500, 1500, 5000)]}), expect=dict(vw=mark(67, {63: "DDD"}), wz=mark(67, rest="D"), R6=mark(67)))
    add("r6_by_63", "a -R 6 containment whose cont_by points from record 64 back to 63, not the run's first", 3000,
        pile(68, {62: [(2500, 2900), (0, 2000), (100, 900), (2100, 2400)]}), expect=dict(R6=mark(68, {62: "..C."})))
    recs = pile(67)
    recs[63] = recs[64] = R(SELF, 0, 1000, 2000)
    add("dup_id_63", "the -R 6 identity duplicate at records 63|64", 3000, recs, expect=dict(R6=mark(67, {63: ".C"})))

    # ---- -R 4: the reference counts the head of every run but the pile's first twice -----------------------------------------
    PR, NP = (0, 3000, 0), (500, 1500, 3000)                           # proper on a read of 3000 bases, and not
    two = dict(head=[PR, NP], second=[NP, PR], both=[PR, PR], none=[NP, NP])
    first = dict(head=".D", second="D.", both="..", none="..")
    for v in two:                                                      # the first run as named; every kind of later run behind it
        add("r4_first_" + v, "-R 4: the pile's first run with %s proper; later runs of every kind, one of one record, one at record 64" % v,
            3000, pile(67, {0: two[v], 2: two["head"], 4: two["second"], 6: two["both"], 8: two["none"], 10: [PR], 64: two["head"]}),
            expect=dict(R4=mark(67, {0: first[v], 2: "..", 4: "D.", 6: "..", 8: "..", 10: ".", 64: ".."})))

    # ---- the order of the steps: what one lane leaves behind a wave_mem_sync for another -----------------------------------------
    add("undiscard_drop", "a head the stitch takes DISCARD | LOCAL off, which filter() then drops under -o", 3000,
        [R(LB, 0, 400, fl=DISCARD | LOCAL), R(LB, 410, 900)], expect={"def": "L.", "s": ".T", "so": "OT"})
    add("stitch_o", "a stitched head whose new aepos alone passes -o", 3000, [R(LB, 0, 600), R(LB, 610, 1200)], expect=dict(o="OO", so=".T"))
    add("stitch_d", "a stitched head whose summed diffs alone fail -d", 3000, [R(LB, 0, 1000, df=150), R(LB, 1010, 2000, df=260)],
        expect=dict(d=".F", sd="FT"))
    add("w_container", "a record -w drops that -R 6 would have used as a container", 3000, [R(LB, 0, 2000), R(LB, 100, 900)],
        expect=dict(vw="DD", R6=".C"))
    add("r2_r0", "-R 2 with -R 0: tlen is zeroed before -R 0 asks for it; the second trace does not add up", 3000,
        [R(LB, 0, 1000), R(LB, 2000, 2500, tr=[0, 100, 0, 100, 0, 100, 0, 100, 0, 101]), R(P(5), 0, 1000)], expect=dict(R20="DDD", R2=".D."))

    # ---- repeats: FL_REPCAP = 1024 values of the A read in LDS, more stay in HBM ----------------------------------------------
    for n in (511, 512, 513):
        end = 2000 + 4 * (n - 1)                                       # n - 1 intervals of 2 bases, 4 apart, and one at the tip
        add("rep_%d" % n, "an A read of %d intervals: the remainder at -n, one under it, and -Y decided by the last interval" % n, 8000,
            [R(P(0), end - 1000, end), R(P(1), end - 1000, end - 2), R(P(2), 7250, 8000)],
            rep=[(2000 + 4 * k, 2002 + 4 * k) for k in range(n - 1)] + [(7800, 8000)], expect=dict(n=".P.", nY=".PP"))
    eb = 2000 + 4 * 513
    add("rep_b513", "a B read of 513 intervals on an A read of none", 8000, [R(BREP, 0, 1000, eb - 1000), R(BREP, 0, 998, eb - 1000)],
        expect=dict(n=".P"))
    add("rep_1", "an A read of one interval, the remainder at -n", 8000, [R(P(0), 0, 1000)], rep=[(0, 500)], expect=dict(n="."))
    add("rep_none", "an A read and a B read without an interval", 8000, [R(P(0), 0, 1000)], expect=dict(n=".", nY="."))

    # ---- coverage, -z 2 -u 32: one bit per base, 32 to a word, the lanes over the words ----------------------------------------------
    def cov(tag, border, alen, holes, letter, **k):
        recs = covered(alen, holes, **k)
        add(tag, border, alen, recs, trim=k.get("trim"), expect=dict(zu=letter * len(recs)))
    cov("zu_word", "a hole of exactly a word", 2048, [(1024, 1056)], ".")
    cov("zu_bit31_32", "a hole of 32 from bit 31 into the next word", 2048, [(1055, 1087)], ".")
    cov("zu_bit31_33", "a hole of 33 from bit 31 into the next word", 2048, [(1055, 1088)], "D")
    cov("zu_bit0_33", "a hole of 33 from bit 0", 2048, [(1024, 1057)], "D")
    cov("zu_inword_32", "a hole within one word and one of 22 before the last ten bases", 2048, [(1030, 1040), (2016, 2038)], ".")
    cov("zu_inword_33", "a hole within one word and one of 23", 2048, [(1030, 1040), (2016, 2039)], "D")
    cov("zu_w63_64_32", "a hole of 32 across the words 63|64, where the lanes wrap round", 2080, [(2032, 2064)], ".")
    cov("zu_w63_64_33", "a hole of 33 across the words 63|64", 2080, [(2032, 2065)], "D")
    cov("zu_len2049", "a read of 2049 bases: over a limit of 2048", 2049, [(1024, 1056)], ".")
    cov("zu_len2047", "a read of 2047 bases, the hole in its last word but one", 2047, [(1984, 2016)], ".")
    cov("zu_trim_0_0_at", "trim [32, 1984): both on word borders, 16 uncovered bases at either end", 2048, [(16, 48), (1968, 2000)], ".", trim=(32, 1984))
    cov("zu_trim_0_0_over", "trim [32, 1984): 16 and 17 uncovered bases", 2048, [(16, 48), (1967, 2000)], "D", trim=(32, 1984))
    cov("zu_trim_31_1_at", "trim [31, 1985): tb % 32 == 31, te % 32 == 1; 16 uncovered bases at either end", 2048, [(15, 47), (1969, 2001)], ".", trim=(31, 1985))
    cov("zu_trim_31_1_over", "trim [31, 1985): 16 and 17 uncovered bases", 2048, [(15, 47), (1968, 2001)], "D", trim=(31, 1985))
    cov("zu_before_tb", "a hole of 40 before tb that must not count, beside one of 32", 2048, [(10, 50), (1024, 1056)], ".", trim=(64, 2048))
    cov("zu_zero_len", "a live record with abpos == aepos beside a hole of 32", 2048, [(1024, 1056)], ".", extra=[R(P(10), 2040, 2040, 0)])
    cov("zu_len33", "a read of 33 bases, all but the first and the last uncovered", 33, [(1, 32)], ".", partners=50)
    cov("zu_len64_at", "a read of 64 bases with a hole of 32", 64, [(16, 48)], ".", partners=8)
    cov("zu_len64_over", "a read of 64 bases with a hole of 33", 64, [(15, 48)], "D", partners=8)
    for k, letter in ((2, "D"), (3, ".")):
        recs = covered(2048, [], partners=k)
        add("z_mean_%d" % k, "-z 2 with bases / length == %d" % k, 2048, recs, expect=dict(wz=letter * k, zu=letter * k))

    # ---- the divisions, in double ---------------------------------------------------------------------------------------------------------
    add("div_d_0", "-d on a record of no bases and no differences: 0.0 / 0", 3000, [R(LB, 1000, 1000)], expect=dict(d="."))
    add("div_d_1", "-d on a record of no bases and one difference: 1.0 / 0", 3000, [R(LB, 1000, 1000, df=1)], expect=dict(d="F"))
    add("div_b", "-b on trace pairs (0, 0) and (3, 0) before the last; 40 in 100 in the last alone", 3000,
        [R(LB, 0, 300, df=10, tr=[0, 0, 5, 150, 5, 150]), R(P(1), 0, 300, df=3, tr=[3, 0, 0, 150, 0, 150]), R(P(2), 0, 300, df=40, tr=[0, 100, 0, 100, 40, 100])],
        expect=dict(b=".F."))

    # ---- the lists of -A, -x and -I at read 0 and at the last read, in records 0 and 64 -------------------------------------------------
    recs = pile(65)
    recs[0], recs[64] = R(0, 0, 1000), R(LAST, 0, 1000)
    add("lists_65", "-A, -x and -I with read 0 in record 0 and the last read in record 64", 3000, recs,
        expect=dict(A=mark(65, {0: "S", 64: "S"}), x=mark(65, {0: "D", 64: "D"}), I=mark(65, {0: ".", 64: "."}, rest="D")))
    return number(S, 1)


def shapes200():
    """on traces of spacing 200, whose values take two bytes: A reads after those of shapes()"""
    S = []
    seg4 = lambda d, bl=200: [0, 200, d, bl, 0, 200, 0, 200]
    S.append(Shape("t2_b", "-b 30 in a middle segment at, over and under the rate, in the last segment alone, and on B lengths of 300", 3000,
                   [R(P(0), 0, 800, df=60, tr=seg4(60)), R(P(1), 0, 800, df=61, tr=seg4(61)), R(P(2), 0, 800, df=59, tr=seg4(59)),
                    R(P(3), 0, 800, df=150, tr=[0, 200, 0, 200, 0, 200, 150, 200]), R(P(4), 0, 800, 0, 900, df=90, tr=seg4(90, 300)),
                    R(P(5), 0, 800, 0, 900, df=91, tr=seg4(91, 300))], expect=dict(b=".F...F"), tspace=200))
    S.append(Shape("t2_r2", "-R 2 on a trace that adds up, one that is off by 256, and a made one", 3000,
                   [R(P(0), 0, 800, 0, 900, tr=seg4(0, 300)), R(P(1), 0, 800, 0, 644, tr=seg4(0, 300)), R(P(2), 100, 2900, df=70)],
                   expect=dict(R2=".D.", R20="DDD"), tspace=200))
    return number(S, 1 + len(shapes()))


def number(S, first):
    assert first + len(S) <= NA + 1 and len({s.tag for s in S}) == len(S)
    for k, s in enumerate(S):
        s.aread = first + k
        recs = []
        for b, ab, ae, bb, be, fl, df, tr in s.recs:
            b = s.aread if b == SELF else b
            blen = s.alen if b == s.aread else BLEN
            assert b == s.aread or b == 0 or POOL <= b < NREADS, s.tag
            assert 0 <= ab <= ae <= s.alen and 0 <= bb <= be <= blen, (s.tag, ab, ae, bb, be)
            tr = trace_of(ab, ae, bb, be, df, s.tspace) if tr is None else list(tr)
            assert len(tr) % 2 == 0 and max(tr) < (256 if s.tspace <= 125 else 65536), s.tag
            recs.append((b, ab, ae, bb, be, fl, df, tr))
        s.recs = recs
        assert all(len(v) == len(recs) for v in s.expect.values()), s.tag
        assert s.over == (s.max_run() > GROUP), s.tag
    return S


def every():
    return shapes() + shapes200()


def read_len(S=None):
    rl = np.full(NREADS, BLEN, dtype=np.int32)
    for s in S or every():
        rl[s.aread] = s.alen
    return rl


def tracks(S=None):
    """(trim anno, trim data, repeat anno, repeat data) over all reads: a trim pair for each, the shapes' intervals and BREP's"""
    S = S or every()
    rl = read_len(S)
    trim = {r: [(0, int(rl[r]))] for r in range(NREADS)}
    rep = {BREP: [(2000 + 4 * k, 2002 + 4 * k) for k in range(513)]}
    for s in S:
        trim[s.aread] = [s.trim]
        if s.rep:
            rep[s.aread] = s.rep
    out = []
    for iv in (trim, rep):
        anno, data = [0], []
        for r in range(NREADS):
            for b, e in iv.get(r, []):
                data += [b, e]
            anno.append(4 * len(data))
        out += [np.array(anno, dtype=np.uint64), np.array(data, dtype=np.int32)]
    return tuple(out)


def files(S=None):
    """the lists of -A, -x and -I"""
    a = next(s.aread for s in S or every() if s.tag == "lists_65")
    return {"sym.txt": "0 %d\n%d %d\n" % (a, a, LAST), "x.txt": "0\n%d\n" % LAST, "i.txt": "%d\n0\n" % LAST}


def params(key, S=None):
    return fc.opts_to_params(OPTION_SETS[key], None, files(S), own=tracks(S))


def arrays(S):
    """the shapes S (of one trace spacing), in that order, as api.pile_filter takes them"""
    ts = S[0].tspace if S else 100
    assert all(s.tspace == ts for s in S)
    return batch_of([(s.aread, s.recs) for s in S], ts)


def batch_of(piles, ts):
    tb = 1 if ts <= 125 else 2
    rows = [r for _, recs in piles for r in recs]
    col = lambda k: np.array([r[k] for r in rows], dtype=np.int32)
    tlen = np.array([len(r[7]) for r in rows], dtype=np.int32)
    trace = np.array([v for r in rows for v in r[7]], dtype="<u2" if tb == 2 else np.uint8).view(np.uint8)
    toff = np.concatenate([[0], np.cumsum(tlen.astype(np.int64) * tb)])[:len(rows)].astype(np.int64)
    off = np.concatenate([[0], np.cumsum([len(recs) for _, recs in piles])]).astype(np.int64)
    return dict(pile_off=off, pile_aread=np.array([a for a, _ in piles], dtype=np.int32), bread=col(0), abpos=col(1), aepos=col(2), bbpos=col(3),
                bepos=col(4), flags=col(5), diffs=col(6), tlen=tlen, trace_off=toff, trace=trace, tbytes=tb, tspace=ts)


def digest():
    """sha256 over the columns and traces of both sets, the read lengths, the tracks and the lists: what ties
    tests/golden/filter/shapes.json to this file"""
    h = hashlib.sha256()
    for S in (shapes(), shapes200()):
        b = arrays(S)
        for k in ("pile_off", "pile_aread", "abpos", "aepos", "bbpos", "bepos", "bread", "flags", "diffs", "tlen", "trace_off", "trace"):
            h.update(np.ascontiguousarray(b[k], dtype=np.int64).tobytes())
    for v in (read_len(),) + tracks():
        h.update(np.ascontiguousarray(v, dtype=np.int64).tobytes())
    h.update(repr(sorted(files().items())).encode())
    return h.hexdigest()


def code(f):
    return ("S" if f & fm.SYM else "C" if f & fm.CONT else "T" if f & fm.STITCH else "P" if f & fm.REPEAT else "L" if f & fm.LOCAL else
            "O" if f & fm.OLEN else "R" if f & fm.RLEN else "F" if f & fm.DIFF else "D" if f & fm.DISCARD else ".")


def check_letters(S, key, flags):
    """every shape of S that states letters under `key` shows them in `flags` (of arrays(S), in that order)"""
    at = 0
    for s in S:
        got = "".join(code(int(f)) for f in flags[at:at + len(s.recs)])
        at += len(s.recs)
        want = s.expect.get(key)
        assert want is None or all(w in ("?", g) for w, g in zip(want, got)), "%s under %s: %s, stated %s" % (s.tag, key, got, want)
    assert at == len(flags)


def on_host(S, key, group=GROUP, maxlen=1 << 30):
    """which piles of S the kernel leaves to the host routine under an option set and the two limits"""
    opts = OPTION_SETS[key]
    cover = "-z" in opts and "-u" in opts
    return [s.max_run() > group or (cover and s.alen > maxlen) for s in S]


def random_piles(seed=20261022):
    """40 seeded piles of 1 to 200 records on the shapes' reads of 2000 bases and more: runs of one B read of 1 to 5 records, one
    in six of up to 70; every kind of flag in the input, traces that add up (and a few that do not), self overlaps, duplicates,
    contained and stitchable records among them -> (batch, read_len)"""
    rl = read_len()
    rng = np.random.default_rng(seed)
    long_reads = np.flatnonzero(rl >= 2000)
    piles = []
    for a in rng.choice(long_reads, size=40, replace=False):
        n, alen, recs = int(rng.integers(1, 201)), int(rl[a]), []
        while n > 0:
            b = int(a) if rng.integers(12) == 0 else int(rng.choice(long_reads))
            run = min(n, int(rng.integers(1, 71)) if rng.integers(6) == 0 else int(rng.integers(1, 6)))
            n -= run
            prev, blen = None, int(rl[b])
            for _ in range(run):
                if prev is not None and rng.integers(3) == 0:
                    kind, (ab, ae, bb, be) = int(rng.integers(3)), prev
                    if kind == 1:
                        ab, ae, bb, be = ab + (ae - ab) // 4, ae - (ae - ab) // 4, bb + (be - bb) // 4, be - (be - bb) // 4
                    elif kind == 2:
                        d = int(rng.integers(0, 60))
                        ab, bb = min(ae + d, alen), min(be + d + int(rng.integers(0, 60)), blen)
                        ae, be = min(ab + 700, alen), min(bb + 700, blen)
                else:
                    ab = 0 if rng.integers(4) == 0 else int(rng.integers(0, alen - 200))
                    ae = int(rng.integers(ab + 100, alen + 1)) if rng.integers(3) else alen
                    if b == a and rng.integers(2):
                        bb, be = ab, ae
                    else:
                        span = min(ae - ab + int(rng.integers(-50, 50)), blen)
                        bb = int(rng.integers(0, blen - span + 1))
                        be = bb + span
                if ae <= ab or be < bb:
                    ab, ae, bb, be = 0, 500, 0, 500
                prev = (ab, ae, bb, be)
                nseg = (ae - 1) // 100 - ab // 100 + 1
                bl = np.full(nseg, (be - bb) // nseg)
                bl[:(be - bb) % nseg] += 1
                tr = np.zeros(2 * nseg, dtype=np.int64)
                tr[1::2] = np.minimum(bl, 255)
                tr[0::2] = rng.integers(0, 45, size=nseg)
                if rng.integers(10) == 0:
                    tr[1] = (int(tr[1]) + 1) % 256
                fl = int(rng.integers(2)) | (int(rng.choice([0, 0x2, 0x12, 0x82, 0x20002, 0x40000, 0x8002, 0x10000])) if rng.integers(5) == 0 else 0)
                recs.append((b, ab, ae, bb, be, fl, int(tr[0::2].sum()), [int(x) for x in tr]))
        piles.append((int(a), recs))
    batch = batch_of(piles, 100)
    assert sum(max(len(r) for r in fm.runs([dict(b=x[0]) for x in recs])) > GROUP for _, recs in piles) > 0
    return batch, rl


def runs_over(batch, group=GROUP):
    """the piles of a batch with a run of one B read above `group` records"""
    out = []
    for p in range(len(batch["pile_aread"])):
        br = batch["bread"][int(batch["pile_off"][p]):int(batch["pile_off"][p + 1])]
        out.append(bool(len(br)) and max(len(r) for r in fm.runs([dict(b=int(x)) for x in br])) > group)
    return out
