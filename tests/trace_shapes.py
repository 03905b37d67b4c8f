"""Planted overlap records at the borders of the trace-point expansion (kernels/trace_pts.hip: Compute_Trace_PTS / _MID).

A family is a list of files; a file is a handful of reads plus planted records over them at one trace spacing.  Everything
is regenerated from fixed seeds: materialize() writes the reads as FASTA, builds the DB with the repository's FA2db and
DBsplit and writes the records in the .las layout that lastrace, oracle_lastrace and ref_lastrace read.

Planting.  A segment with target (M, N, D) is M bases of A against N bases of B with edit distance D + |M - N|:
  light   random 4-letter A; B = A with one block indel of |M - N| bases and D isolated substitutions.  That the distance
          really is D + |del| is checked here with a plain Levenshtein table (edit_distance), another draw is taken if not.
  heavy   (D too large for random sequence) both sides over {a, c}, the shorter one carries D bases of {g, t}: each of them
          costs a substitution or an indel of its own and the length difference costs |del| more, so the distance is
          exactly D + |del| (when A is shorter: subs + dels >= D and ins = dels + |del|, so subs + dels + ins >= D + |del|).
The diffs value of a trace pair is that distance plus a small slack unless a family says otherwise; a complemented record's
B read holds the reverse complement.  Border cases are single-segment records (one trace pair inside one tile), for which
the oracle's answer gives D = diffs - |del| back: check_reach() holds that against what was planted.

Well-formedness.  The reference keeps every wave in rows of tspace + nmax + 3 ints with origin nmax + 1 (align.c:5628-5643),
nmax the record's largest B piece; a segment is planted only if  N - M + D/2 + 1 <= nmax  and  M - N + D/2 <= tspace
(_wellformed; for the pieces between mid points _wellformed_mid).  Beyond that the reference writes across its own rows.
Left out of the definitions for that reason: pieces with M = 0 or N = 0.  In align16 the pairs of lengths more than 18 bases
apart are planted with D = 0: a gap that long absorbs an isolated substitution, so no larger D can be planted exactly there
(and from |del| = 97 on the reference's rows leave no room for one either)."""
import atexit
import os
import shutil
import struct
import subprocess
import tempfile

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
BIN = os.path.join(ROOT, "damar_amd", "bin")
ORACLE = os.path.join(ROOT, "oracle", "oracle_lastrace")
REF = os.path.join(ROOT, "oracle", "_ref", "ref_lastrace")
MODES = (0, 1, -1)

SLOT_MAXB, SLOT_SS, SLOT_ROWS = 240, 40, 64          # the documented limits of trace_waves_slots
ALIGN_LENS = (1, 2, 15, 16, 17, 31, 32, 33, 97, 100)
COUNTS = (1, 63, 64, 65, 128, 129)

# records on which the reference is undefined (found by its sanitizer build): family -> [(file, record)]
REMOVED = {}
REMOVED_CAP = 0.02


def edit_distance(a, b):
    """Levenshtein distance, one numpy row at a time (insertions through a running minimum)"""
    n = len(b)
    idx = np.arange(n + 1)
    prev = idx.copy()
    t = np.empty(n + 1, dtype=np.int64)
    for i in range(len(a)):
        t[0] = i + 1
        np.minimum(prev[1:] + 1, prev[:-1] + (b != a[i]), out=t[1:])
        prev = np.minimum.accumulate(t - idx) + idx
    return int(prev[n])


def revcomp(s):
    return (3 - s[::-1]).astype(np.uint8)


def _spread(n, s, rng, lo=0):
    """s distinct positions spread over [lo, n - lo), no two adjacent"""
    if s == 0:
        return np.zeros(0, dtype=np.int64)
    span = n - 2 * lo
    assert span >= 2 * s - 1, (n, s)
    step = span / s
    pos = [lo + min(int(i * step + rng.integers(0, max(1, int(step) - 1))), span - 1) for i in range(s)]
    assert len(set(pos)) == s
    return np.array(pos)


def derive(src, length, s, rng, where=0.5):
    """a copy of src of `length` bases: one block indel at `where`, s isolated substitutions away from it"""
    n, d = len(src), len(src) - length
    common = min(n, length)
    p = int(common * where)
    if d > 0:
        out = np.concatenate([src[:p], src[p + d:]])
        kept = np.arange(common)
    else:
        out = np.concatenate([src[:p], rng.integers(0, 4, -d).astype(np.uint8), src[p:]])
        kept = np.concatenate([np.arange(p), np.arange(p - d, length)])
    if s:
        gap = min(10, common // 4)              # a substitution next to the block is absorbed by moving the block
        far = kept[(np.abs(kept - p) > gap) & (np.abs(kept - (p - d if d < 0 else p)) > gap)] if d else kept
        far = far[(far > 0) & (far < length - 1)]
        for i in far[_spread(len(far), s, rng)]:
            out[i] = (out[i] + 1 + rng.integers(0, 3)) % 4
    return out.astype(np.uint8)


def plant_light(M, N, s, rng, where=0.5, check=True):
    for _ in range(60):
        a = rng.integers(0, 4, M).astype(np.uint8)
        b = derive(a, N, s, rng, where)
        if not check or edit_distance(a, b) == s + abs(M - N):
            return a, b
    raise AssertionError("no draw of (%d, %d) has distance %d + |del|" % (M, N, s))


def plant_heavy(M, N, s, rng, where=0.5):
    big, d = max(M, N), abs(M - N)
    base = rng.integers(0, 2, big).astype(np.uint8)
    p = int(min(M, N) * where)
    short = np.concatenate([base[:p], base[p + d:]])
    assert s <= len(short)
    at = rng.permutation(len(short))[:s]
    short[at] = 2 + rng.integers(0, 2, s)
    return (base, short) if M >= N else (short, base)


def _wellformed(ts, M, N, D, nmax):
    return 0 < M <= 32000 and 0 < N <= 32000 and N - M + D // 2 + 1 <= nmax and M - N + D // 2 <= ts


def _wellformed_mid(ts, costs, nmax):
    """the pieces between mid points: a piece is the tail of one segment's path (ceil(c/2) edges) and the head of the next
    (floor(c/2) edges), so it costs at most c' = their sum, and |del'| + D'/2 = (c' + |del'|) / 2 <= c'"""
    c = [0] + list(costs) + [0]
    return all((c[i] + 1) // 2 + c[i + 1] // 2 + 1 <= min(ts, nmax) for i in range(len(c) - 1))


class Rec:
    def __init__(self, **kw):
        self.D = None                                   # planted D of a single-segment border record
        self.M = self.N = None
        self.__dict__.update(kw)

    def shape(self):
        strand = "comp" if self.comp else "fwd"
        if self.M is not None:
            return "%s (M, N, D, del, strand) = (%d, %d, %s, %d, %s)" % (self.sub, self.M, self.N, self.D, self.M - self.N, strand)
        return "%s %d segments a[%d, %d) b[%d, %d) %s" % (self.sub, max(1, len(self.pairs)), self.abpos, self.aepos,
                                                          self.bbpos, self.bepos, strand)


class File:
    """reads + records at one spacing; pts / mid: which of Compute_Trace_PTS / _MID it is run with"""

    def __init__(self, name, tspace, seed, pts=True, mid=True):
        self.name, self.tspace, self.pts, self.mid = name, tspace, pts, mid
        self.rng = np.random.default_rng(seed)
        self.reads, self.recs, self.total = [], [], 0
        self.boff = []

    def rnd(self, n):
        return self.rng.integers(0, 4, int(n)).astype(np.uint8)

    def add_read(self, seq, want=None, at=0):
        """-> read index.  want: (block offset of the read + at) & 15, reached with a filler read in front"""
        if want is not None and (self.total + at - want) % 16:
            fill = (want - at - self.total - 1) % 16
            self.add_read(self.rnd(fill if fill else 16))
        assert len(seq) > 0
        self.reads.append(np.asarray(seq, dtype=np.uint8))
        self.boff.append(self.total)
        self.total += len(seq) + 1
        return len(self.reads) - 1

    def single(self, M, N, D, comp, sub, heavy=False, oa=None, ob=None, slack=2, where=0.5, check=True, stated=None):
        """one segment inside the second tile of a read of its own"""
        ts, rng = self.tspace, self.rng
        assert M <= ts and _wellformed(ts, M, N, D, N), (sub, M, N, D)
        a, b = plant_heavy(M, N, D, rng, where) if heavy else plant_light(M, N, D, rng, where, check)
        x = int(rng.integers(0, ts - M + 1))
        aseq = np.concatenate([self.rnd(ts + x), a, self.rnd(rng.integers(0, 20))])
        p = int(rng.integers(0, 30))
        bfwd = np.concatenate([self.rnd(p), b, self.rnd(rng.integers(0, 30))])
        ai = self.add_read(aseq, oa, ts + x)
        bi = self.add_read(revcomp(bfwd) if comp else bfwd, ob, len(bfwd) - 1 - p if comp else p)
        diffs = D + abs(M - N) + slack if stated is None else stated
        self.recs.append(Rec(aread=ai, bread=bi, comp=comp, abpos=ts + x, aepos=ts + x + M, bbpos=p, bepos=p + N,
                             pairs=[(diffs, N)], sub=sub, M=M, N=N, D=D if (check or heavy) else None))
        return self.recs[-1]

    def multi(self, abpos, aepos, spec, comp, sub, tlen0=False):
        """a record over the tiles of a[abpos, aepos); spec(i, M) -> (del, s, heavy, where, stated diffs or None)"""
        ts, rng = self.tspace, self.rng
        cuts = [abpos] + [t * ts for t in range(abpos // ts + 1, (aepos + ts - 1) // ts) if abpos < t * ts < aepos] + [aepos]
        if tlen0:
            cuts = [abpos, aepos]
        sa, sb, pairs, costs, segs = [], [], [], [], []
        for i in range(len(cuts) - 1):
            M = cuts[i + 1] - cuts[i]
            d, s, heavy, where, stated = spec(i, M)
            a, b = plant_heavy(M, M - d, s, rng, where) if heavy else plant_light(M, M - d, s, rng, where, check=False)
            sa.append(a)
            sb.append(b)
            pairs.append((s + abs(d) + 2 if stated is None else stated, M - d))
            costs.append(s + abs(d))
            segs.append((M, M - d, s))
        nmax = max(n for _, n in pairs)
        assert all(_wellformed(ts, M, N, s, nmax) for M, N, s in segs), (sub, segs)
        assert not self.mid or _wellformed_mid(ts, costs, nmax), (sub, costs)
        assert tlen0 or all(0 <= v < (256 if ts <= 125 else 65536) for pr in pairs for v in pr)
        p = int(rng.integers(0, 40))
        aseq = np.concatenate([self.rnd(abpos)] + sa + [self.rnd(rng.integers(0, 30))])
        bfwd = np.concatenate([self.rnd(p)] + sb + [self.rnd(rng.integers(0, 30))])
        ai = self.add_read(aseq)
        bi = self.add_read(revcomp(bfwd) if comp else bfwd)
        self.recs.append(Rec(aread=ai, bread=bi, comp=comp, abpos=abpos, aepos=aepos, bbpos=p, bepos=p + sum(len(b) for b in sb),
                             pairs=[] if tlen0 else pairs, sub=sub, nseg=len(segs)))
        return self.recs[-1]

    def nsegs(self):
        return sum(max(1, len(r.pairs)) for r in self.recs)

    def las_bytes(self):
        out = [struct.pack("<qi", len(self.recs), self.tspace)]
        for r in self.recs:
            out.append(struct.pack("<6iI2i4x", 2 * len(r.pairs), 0, r.abpos, r.bbpos, r.aepos, r.bepos, r.comp, r.aread, r.bread))
            out.append(np.array(r.pairs, dtype=np.uint8 if self.tspace <= 125 else np.uint16).tobytes())
        return b"".join(out)


def light(dels=3, smax=4):
    def spec(rng):
        def f(i, M):
            if M < 20:
                return 0, 0, False, 0.5, None
            return int(rng.integers(-dels, dels + 1)), int(rng.integers(0, smax + 1)), False, 0.5, None
        return f
    return spec


# ---------------------------------------------------------------------------------------------------- the families

def _slot_len():
    files = []
    for ts in (240, 241, 300):
        f = File("s%d" % ts, ts, 1000 + ts)
        for comp in (0, 1):
            for M, N in [(m, n) for m in (239, 240, 241) for n in (239, 240, 241)] + [(240, 201), (201, 240)]:
                if M <= ts:
                    for D in (0, 3):
                        f.single(M, N, D, comp, "len_%d_%d" % (M, N))
        files.append(f)
    return files


def _slot_width():
    by_del = File("del", 100, 2001)
    for comp in (0, 1):
        for ad in (36, 37, 38, 39, 40):
            for sign in (1, -1):
                for D in (0, 1, 2, 3, 4, 6):
                    M, N = (100, 100 - ad) if sign > 0 else (100 - ad, 100)
                    by_del.single(M, N, D, comp, "del%+d" % (sign * ad))
    rows = File("rows", 100, 2002)
    for comp in (0, 1):
        for D in (59, 60, 61, 62, 63, 64, 70):
            for rep in range(2):
                rows.single(100, 100, D, comp, "rows_D%d" % D, heavy=True)
    waves = File("waves", 100, 2003)
    for comp in (0, 1):
        for sign in (1, -1):
            for D in (36, 37, 38, 39, 40):
                M, N = (100, 80) if sign > 0 else (80, 100)
                waves.single(M, N, D, comp, "waves%+d_D%d" % (sign * 20, D), heavy=True)
    return [by_del, rows, waves]


def _align16():
    f = File("a", 100, 3001)
    for comp in (0, 1):
        for oa in range(16):
            for ob in range(16):
                M, N = ALIGN_LENS[(ob + 5 * comp) % 10], ALIGN_LENS[(oa + 5 * comp + 3) % 10]
                D = 1 if min(M, N) >= 15 and abs(M - N) <= 18 else 0      # a longer gap absorbs the substitution
                f.single(M, N, D, comp, "align_%d_%d" % (oa, ob), oa=oa, ob=ob).want = (oa, ob)
    return [f]


def _block_ends():
    files = []
    for ts in (240, 100):
        f = File("e%d" % ts, ts, 4000 + ts)
        rng, n = f.rng, ts
        first = f.rnd(n + 60)                                  # read 0 of the block
        last = f.rnd(2 * ts)                                   # its last read
        f.add_read(first)
        ffwd, todo = revcomp(first), []
        # (sub, given side, the given segment, record fields of the given side)
        cases = [("b0_comp_bepos_blen", "b", ffwd[len(ffwd) - n:], dict(bread=0, comp=1, bbpos=len(ffwd) - n, bepos=len(ffwd))),
                 ("b0_comp_bbpos_0", "b", ffwd[:n], dict(bread=0, comp=1, bbpos=0, bepos=n)),
                 ("b0_fwd_bbpos_0", "b", first[:n], dict(bread=0, comp=0, bbpos=0, bepos=n)),
                 ("alast_aepos_alen", "a", last[ts:], dict(aread=-1, abpos=ts, aepos=2 * ts)),
                 ("blast_fwd_bepos_blen", "b", last[2 * ts - n:], dict(bread=-1, comp=0, bbpos=2 * ts - n, bepos=2 * ts))]
        for sub, side, seg, fields in cases:
            for D in (0, 2, 5):
                for d in (0, 3, -3):
                    for _ in range(60):
                        other = derive(seg, n - d, D, rng)
                        a, b = (other, seg) if side == "b" else (seg, other)
                        if edit_distance(a, b) == D + abs(len(a) - len(b)):
                            break
                    else:
                        raise AssertionError(sub)
                    M, N = len(a), len(b)
                    if M > ts or not _wellformed(ts, M, N, D, N):
                        continue
                    if side == "b":
                        x = int(rng.integers(0, ts - M + 1))
                        ai = f.add_read(np.concatenate([f.rnd(ts + x), a, f.rnd(rng.integers(0, 20))]))
                        rec = Rec(aread=ai, abpos=ts + x, aepos=ts + x + M, **fields)
                    else:
                        for comp in (0, 1):
                            p = int(rng.integers(0, 30))
                            bfwd = np.concatenate([f.rnd(p), b, f.rnd(rng.integers(0, 30))])
                            bi = f.add_read(revcomp(bfwd) if comp else bfwd)
                            todo.append(Rec(bread=bi, comp=comp, bbpos=p, bepos=p + N, pairs=[(D + abs(M - N) + 2, N)],
                                            sub=sub, M=M, N=N, D=D, **fields))
                        continue
                    rec.__dict__.update(pairs=[(D + abs(M - N) + 2, N)], sub=sub, M=M, N=N, D=D)
                    todo.append(rec)
        li = f.add_read(last)
        for r in todo:
            if r.aread == -1:
                r.aread = li
            if r.bread == -1:
                r.bread = li
        f.recs = todo
        files.append(f)
    return files


def _record_walk():
    files = []
    for ts in (40, 100, 125, 126, 300):
        f = File("w%d" % ts, ts, 5000 + ts)
        spec = (light(2, 2) if ts == 40 else light())(f.rng)
        for comp in (0, 1):
            for sa in (0, 1, ts - 1):
                for ea in (0, 1, ts - 1):
                    for nseg in (1, 2, 3) + ((40,) if (sa == ea and comp == 0) or (sa, ea, comp) == (1, ts - 1, 1) else ()):
                        abpos = ts + sa
                        aepos = (1 + nseg - 1) * ts + (ea if ea else ts)
                        if aepos > abpos:
                            f.multi(abpos, aepos, spec, comp, "walk_%d_%d_n%d" % (sa, ea, nseg))
            exact = lambda i, M: (0, 0, False, 0.5, None)
            f.multi(ts + 5, 2 * ts - 5, exact, comp, "tlen0_in_tile", tlen0=True)
            f.multi(ts + 5, 3 * ts + ts // 2, exact, comp, "tlen0_long", tlen0=True)
        if ts == 300:
            for comp in (0, 1):
                for D in (255, 256, 300):                      # `own` is clamped to 255; the differences are really there
                    f.multi(ts, 4 * ts, lambda i, M, D=D: (0, D, True, 0.5, D) if i == 1 else (0, 0, False, 0.5, 2),
                            comp, "own_clamped_D%d" % D)
        files.append(f)
    f = File("dmax1000", 300, 5999)                            # the stripes of what is deferred are sized by `need`
    spec = light()(f.rng)
    f.multi(300, 6 * 300, lambda i, M: (0, 40, True, 0.5, 1000) if i == 2 else spec(i, M), 0, "dmax1000")
    f.multi(300, 3 * 300, spec, 1, "dmax1000_neighbour")
    files.append(f)
    return files


def _mid_drift():
    f = File("drift", 100, 6001, pts=False)
    for comp in (0, 1):
        for ad in (35, 39):
            for where0, where1 in ((0.5, 0.5), (0.05, 0.95), (0.95, 0.05)):
                for first in (1, -1):
                    def spec(i, M, ad=ad, first=first, w=(where0, where1)):
                        return (first * ad if i % 2 == 0 else -first * ad), 3, False, w[i % 2], None
                    f.multi(100, 700, spec, comp, "opposite_%d" % ad)
        for first in (1, -1):
            f.multi(100, 500, lambda i, M, first=first: (first * 20, 3, False, (0.05, 0.95)[i % 2], None), comp, "same_sign_20")
        f.multi(100, 600, lambda i, M: (0, 60, True, 0.5, None) if i in (1, 3) else (0, 0, False, 0.5, None), comp, "heavy_60_by_exact")
        f.multi(150, 450, lambda i, M: (0, 30, True, 0.5, None) if i == 0 else (0, 0, False, 0.5, None), comp, "heavy_first_piece")
    return [f]


def _counts():
    files = []
    for n in COUNTS:
        f = File("n%d" % n, 100, 7000 + n)
        spec = light()(f.rng)
        left, k = n, 0
        while left:
            take = min(left, 20)
            f.multi(100, 100 + take * 100, spec, k & 1, "light_%d" % take)
            left -= take
            k += 1
        files.append(f)
    f = File("mixed", 300, 7999)
    deferred = [lambda c: f.single(139, 100, 2, c, "mixed_del+39", check=False), lambda c: f.single(100, 139, 2, c, "mixed_del-39", check=False),
                lambda c: f.single(241, 241, 1, c, "mixed_M241", check=False), lambda c: f.single(120, 120, 62, c, "mixed_D62", heavy=True)]
    for i in range(350):
        f.single(*_mixed_slot(f.rng), i & 1, "mixed_slot", check=False)
        deferred[i % 4]((i >> 1) & 1)
    files.append(f)
    return files


def _mixed_slot(rng):
    M = int(rng.integers(60, 237))                             # N = M + 4 stays within the 240 staged bases
    return M, M - int(rng.integers(-4, 5)), int(rng.integers(0, 4))


FAMILIES = {"slot_len": _slot_len, "slot_width": _slot_width, "align16": _align16, "block_ends": _block_ends,
            "record_walk": _record_walk, "mid_drift": _mid_drift, "counts": _counts}
SINGLE = ("slot_len", "slot_width", "align16", "block_ends")          # every record one segment with a planted D

_families = {}


def family(name):
    """the files of a family, the records of REMOVED taken out (at most 2 % of it, never a whole sub-shape)"""
    if name not in _families:
        files = FAMILIES[name]()
        gone = REMOVED.get(name, [])
        total = sum(len(f.recs) for f in files)
        assert len(gone) <= REMOVED_CAP * total, "%s: %d of %d records removed, more than 2 %%" % (name, len(gone), total)
        before = {r.sub for f in files for r in f.recs}
        for f in files:
            drop = {i for fn, i in gone if fn == f.name}
            assert all(i < len(f.recs) for i in drop)
            f.recs = [r for i, r in enumerate(f.recs) if i not in drop]
        assert {r.sub for f in files for r in f.recs} == before, "%s: a whole sub-shape was removed" % name
        assert len({f.name for f in files}) == len(files)
        _families[name] = files
    return _families[name]


def jobs(f):
    """(mode, mid) runs of a file"""
    return [(m, k) for k in (0, 1) if (f.mid if k else f.pts) for m in MODES]


# ------------------------------------------------------------------------------------- files on disk, oracle, reference

_tmp = None


def workdir():
    global _tmp
    if _tmp is None:
        _tmp = tempfile.mkdtemp(prefix="trace_shapes_")
        atexit.register(shutil.rmtree, _tmp, True)
    return _tmp


def write_db(d, reads):
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "reads.fasta"), "w") as fa:
        for i, s in enumerate(reads):
            fa.write(">r%d\n" % i)
            t = "".join("acgt"[c] for c in s)
            for o in range(0, len(t), 80):
                fa.write(t[o:o + 80] + "\n")
    subprocess.run([os.path.join(BIN, "FA2db"), "-x1", "G", "reads.fasta"], cwd=d, check=True, stdout=subprocess.DEVNULL)
    subprocess.run([os.path.join(BIN, "DBsplit"), "-s200", "G"], cwd=d, check=True, stdout=subprocess.DEVNULL)


_on_disk = {}


def materialize(fam, f):
    """-> (db root, .las path) of a file, written once per process"""
    key = (fam, f.name)
    if key not in _on_disk:
        d = os.path.join(workdir(), fam, f.name)
        write_db(d, f.reads)
        with open(os.path.join(d, "x.las"), "wb") as o:
            o.write(f.las_bytes())
        _on_disk[key] = (os.path.join(d, "G"), os.path.join(d, "x.las"))
    return _on_disk[key]


def run_tool(exe, db, las, out, mode, mid):
    return subprocess.run([exe, db, las, out, str(mode)] + (["mid"] if mid else []), stderr=subprocess.PIPE, text=True)


_oracle = {}


def oracle(fam):
    """{(file, mode, mid): the oracle's dump}, computed once per process"""
    if fam not in _oracle:
        res = {}
        for f in family(fam):
            db, las = materialize(fam, f)
            for mode, mid in jobs(f):
                out = las + ".o"
                r = run_tool(ORACLE, db, las, out, mode, mid)
                assert r.returncode == 0, (fam, f.name, mode, mid, r.stderr)
                res[(f.name, mode, mid)] = open(out, "rb").read()
        _oracle[fam] = res
    return _oracle[fam]


def parse(dump):
    """-> [(aread, bread, flags, diffs, script)]"""
    ts, mode, n = struct.unpack_from("<iiq", dump, 0)
    pos, out = 16, []
    for _ in range(n):
        a, b, fl, d, tl = struct.unpack_from("<5i", dump, pos)
        pos += 20
        out.append((a, b, fl, d, np.frombuffer(dump, "<i4", tl, pos).tolist()))
        pos += 4 * tl
    assert pos == len(dump)
    return out


FIELDS = ("aread", "bread", "flags", "diffs", "script")


def first_difference(f, got, want):
    """where two dumps of a file's records part: a line naming the record, its planted shape and the field"""
    try:
        g, w = parse(got), parse(want)
    except Exception as e:                                   # noqa: BLE001 - a truncated dump is a difference too
        return "dump of %s cannot be read (%s)" % (f.name, e)
    if len(g) != len(w):
        return "%s: %d records, expected %d" % (f.name, len(g), len(w))
    for i, (x, y) in enumerate(zip(g, w)):
        for k in range(5):
            if x[k] != y[k]:
                what = "%s: %s, expected %s" % (FIELDS[k], x[k], y[k])
                if k == 4:
                    j = next((j for j in range(min(len(x[4]), len(y[4]))) if x[4][j] != y[4][j]), min(len(x[4]), len(y[4])))
                    what = "script of %d values (expected %d), first difference at [%d]" % (len(x[4]), len(y[4]), j)
                return "%s record %d, %s: %s" % (f.name, i, f.recs[i].shape(), what)
    return "%s: headers differ" % f.name


def oracle_D(fam, f):
    """per record of a single-segment file: D = diffs - |del| from the oracle's own answer (PTS, GREEDIEST)"""
    recs = parse(oracle(fam)[(f.name, 0, 0)])
    return [d - abs(r.M - r.N) for (_, _, _, d, _), r in zip(recs, f.recs)]


def slot_defers(M, N, D):
    """what the documented limits of the slot kernel send to the stripe kernel"""
    return not (M <= SLOT_MAXB and N <= SLOT_MAXB and abs(M - N) + D // 2 + 1 < SLOT_SS and D + 2 < SLOT_ROWS)


def check_reach():
    """every family sits where it was planted -- from the definitions and the ORACLE's dumps, never the code under test"""
    for fam in SINGLE:
        for f in family(fam):
            assert all(len(r.pairs) == 1 and r.aepos - r.abpos == r.M and r.bepos - r.bbpos == r.N and
                       r.abpos // f.tspace == (r.aepos - 1) // f.tspace for r in f.recs)
            for i, (r, D) in enumerate(zip(f.recs, oracle_D(fam, f))):
                assert r.D is not None and D == r.D, "%s/%s record %d %s: the oracle finds D = %d" % (fam, f.name, i, r.shape(), D)
                assert _wellformed(f.tspace, r.M, r.N, D, r.N)
    # slot_width: either side of each limit, both signs
    recs = [(r, D) for f in family("slot_width") for r, D in zip(f.recs, oracle_D("slot_width", f))]
    for sign in (1, -1):
        for lim_sub in ("del", "waves"):
            w = [abs(r.M - r.N) + D // 2 + 1 for r, D in recs if r.sub.startswith(lim_sub) and (r.M - r.N) * sign > 0]
            assert ({38, 39, 40, 41} if lim_sub == "del" else {39, 40, 41}) <= set(w), (lim_sub, sign, sorted(set(w)))
        assert all(D + 2 < SLOT_ROWS for r, D in recs if not r.sub.startswith("rows"))
    rows = {D for r, D in recs if r.sub.startswith("rows")}
    assert {61, 62} <= rows and min(rows) < 61 and max(rows) > 62
    for comp in (0, 1):
        assert {slot_defers(r.M, r.N, D) for r, D in recs if r.comp == comp} == {True, False}
    # slot_len: every (M, N) the spacing admits
    for f in family("slot_len"):
        want = {(m, n) for m in (239, 240, 241) for n in (239, 240, 241) if m <= f.tspace} | {(240, 201), (201, 240)}
        for comp in (0, 1):
            assert {(r.M, r.N) for r in f.recs if r.comp == comp} == want
    assert any(r.M == 241 for f in family("slot_len") for r in f.recs)
    # align16: all 16 x 16 alignments on both strands, every length at every alignment of its side
    (f,) = family("align16")
    seen = set()
    for r in f.recs:
        apos = f.boff[r.aread] + r.abpos
        blen = len(f.reads[r.bread])
        bpos = f.boff[r.bread] + (blen - 1 - r.bbpos if r.comp else r.bbpos)
        assert (apos & 15, bpos & 15) == r.want
        seen.add((r.comp, apos & 15, bpos & 15))
    assert len(seen) == 2 * 256
    for comp in (0, 1):
        assert {(f.boff[r.aread] + r.abpos & 15, r.M) for r in f.recs if r.comp == comp} == {(o, m) for o in range(16) for m in ALIGN_LENS}
        assert {(r.want[1], r.N) for r in f.recs if r.comp == comp} == {(o, n) for o in range(16) for n in ALIGN_LENS}
    # block_ends: the segments touch the first and the last base of the block
    for f in family("block_ends"):
        subs = {r.sub for r in f.recs}
        assert subs == {"b0_comp_bepos_blen", "b0_comp_bbpos_0", "b0_fwd_bbpos_0", "alast_aepos_alen", "blast_fwd_bepos_blen"}
        last = len(f.reads) - 1
        for r in f.recs:
            if r.sub == "b0_comp_bepos_blen":
                assert r.bread == 0 and r.comp and r.bepos == len(f.reads[0])
            elif r.sub.startswith("b0"):
                assert r.bread == 0 and r.bbpos == 0
            elif r.sub == "alast_aepos_alen":
                assert r.aread == last and r.aepos == len(f.reads[last])
            else:
                assert r.bread == last and not r.comp and r.bepos == len(f.reads[last])
        assert {r.M for r in f.recs} >= {f.tspace} and f.tspace in (240, 100)
    # counts: exactly the stated numbers of segments; the mixed file alternates inside every run of 64
    files = {f.name: f for f in family("counts")}
    for n in COUNTS:
        assert files["n%d" % n].nsegs() == n
    mixed = files["mixed"]
    D = oracle_D("counts", mixed)
    defer = [slot_defers(r.M, r.N, d) for r, d in zip(mixed.recs, D)]
    assert len(defer) == 700 and all(0 < sum(defer[i:i + 64]) < len(defer[i:i + 64]) for i in range(0, 700, 64))
    assert {r.sub for r, x in zip(mixed.recs, defer) if x} == {"mixed_del+39", "mixed_del-39", "mixed_M241", "mixed_D62"}
    assert not any(x for r, x in zip(mixed.recs, defer) if r.sub == "mixed_slot")
    # record_walk: the starts, ends and segment counts; 16-bit pairs above 255; the record sized by `need`
    for f in family("record_walk"):
        if f.name.startswith("w"):
            ts = f.tspace
            assert {(r.abpos % ts, r.aepos % ts) for r in f.recs if r.pairs} >= {(a, b) for a in (0, 1, ts - 1) for b in (0, 1, ts - 1)}
            assert {len(r.pairs) for r in f.recs} >= {0, 1, 2, 3, 40}
    assert {max(d for d, _ in r.pairs) for f in family("record_walk") for r in f.recs if r.pairs} >= {255, 256, 300, 1000}


# ------------------------------------------------------------------------------------------------ the loud errors

def error_files():
    """{name: file}: a trace pair that pushes be past blen; a record whose dmax is one less than its D; each of them again
    as the last record of a file of good ones"""
    out = {}
    for name, good in (("points", 0), ("align", 0), ("good_then_points", 6), ("good_then_align", 6)):
        f = File(name, 100, 8000 + len(name) + good)
        spec = light()(f.rng)
        for k in range(good):
            f.multi(100, 100 + (k + 1) * 100, spec, k & 1, "good")
        if name.endswith("points"):
            r = f.multi(100, 300, spec, 0, "be_past_blen")
            r.pairs[0] = (r.pairs[0][0], len(f.reads[r.bread]) - r.bbpos + 1)
        else:
            r = f.single(100, 100, 5, 0, "dmax_below_D", stated=4)
        out[name] = f
    return out
