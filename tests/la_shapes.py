"""Local_Alignment tasks at the shapes where the wave kernels (kernels/report_packed.h, kernels/report.hip) can go wrong, for
tests/test_la_host.py (the oracle against the reference) and tests/test_gpu_la_shapes.py (the kernels against the oracle).

A family is a list of groups; a group is one call of the batch entry: two blocks of synthetic reads (the B reads as they are
aligned, i.e. already complemented where comp is set), a task list (aread, bread, diag, anti) and the spec (e, tspace, comp).
A task's seed point is (x, y) = ((anti + diag) / 2, (anti - diag) / 2), 0 <= x <= alen, 0 <= y <= blen; it need not lie on
a match.  Every task carries a tag that names its sub-shape, so that a test can say what it reached.

Everything is made from fixed seeds: family(name) returns the same tasks in every process.

REMOVED lists the tasks taken out of a family because the reference itself is undefined on them (see tests/test_la_host.py);
at most 2 % of a family may be listed and no sub-shape (tag) may lose all its tasks."""
import ctypes as C
import struct

import numpy as np

MAX_MARKS = 16000           # DAMAR_MAX_MARKS (kernels/kernels.h): trace-grid indexes of the packed chain heads
MIXED_SLOTS = 16            # DAMAR_SLOTS the `mixed` family is run under: its largest group has 2 * MIXED_SLOTS + 1 tasks

# family -> {(group name, aread, bread, x, y): reason}
REMOVED = {
}


class Group:
    def __init__(self, name, areads, breads, e=.70, tspace=100, comp=0):
        self.name, self.areads, self.breads = name, areads, breads
        self.e, self.tspace, self.comp = e, tspace, comp
        self.tasks, self.tags = [], []

    def seed(self, ar, br, x, y, tag):
        x, y = int(x), int(y)
        assert 0 <= x <= len(self.areads[ar]) and 0 <= y <= len(self.breads[br]), (self.name, tag, x, y)
        self.tasks.append((ar, br, x - y, x + y))
        self.tags.append(tag)

    def lens(self, t):
        ar, br, _, _ = self.tasks[t]
        return len(self.areads[ar]), len(self.breads[br])

    def point(self, t):
        _, _, dg, anti = self.tasks[t]
        return (anti + dg) // 2, (anti - dg) // 2

    def maxtp(self):
        """values a trace buffer of one path must hold (oracle.h: 2 * (max(alen, blen) / tspace + 2) + 2)"""
        m = max(max(len(r) for r in self.areads), max(len(r) for r in self.breads))
        return 2 * (m // self.tspace + 2) + 2


def _rand(rng, n):
    return rng.randint(0, 4, n).astype(np.uint8)


def _mutate(rng, s, rate):
    """substitutions, insertions and deletions, a third each, at `rate` per base"""
    out = []
    for b in s:
        if rng.rand() >= rate:
            out.append(b)
            continue
        k = rng.randint(0, 3)
        if k == 0:
            out.append((b + 1 + rng.randint(0, 3)) & 3)
        elif k == 1:
            out += [b, rng.randint(0, 4)]
    return np.array(out, dtype=np.uint8)


def _cat(*parts):
    return np.concatenate([np.asarray(p, dtype=np.uint8) for p in parts])


def _noisy_pair():
    rng = np.random.RandomState(101)
    a = _rand(rng, 3000)
    return [a], [_mutate(rng, a, .15), _mutate(rng, a, .30)]


def _seeds_along(g, ar, br, step, tag, offs=(0,)):
    """seeds every `step` bases of A on the line from (0, 0) to (alen, blen), moved off it in B by the offsets in turn (a seed
    need not lie on the alignment it finds: the band has to widen until it reaches it)"""
    al, bl = len(g.areads[ar]), len(g.breads[br])
    for i, x in enumerate(range(step // 2, al, step)):
        g.seed(ar, br, x, max(0, min(bl, x * bl // al + offs[i % len(offs)])), tag)


def _noisy():
    A, B = _noisy_pair()
    out = []
    for comp in (0, 1):
        g = Group("noisy_c%d" % comp, A, B, comp=comp)
        for br, tag in ((0, "15%"), (1, "30%")):
            _seeds_along(g, 0, br, 100, tag, offs=(0, 12, -12, 25, -25))
        out.append(g)
    return out


def _indel():
    rng = np.random.RandomState(102)
    a = _rand(rng, 20000)
    ins = _mutate(rng, _cat(a[:10000], _rand(rng, 25), a[10000:]), .02)
    dele = _mutate(rng, _cat(a[:12000], a[12060:]), .02)
    out = []
    for comp in (0, 1):
        g = Group("indel_c%d" % comp, [a], [ins, dele], comp=comp)
        for br, ev, shift, tag in ((0, 10000, 25, "ins25"), (1, 12000, -60, "del60")):
            bl = len(g.breads[br])
            for x in (2000, 6000, ev - 1000, ev - 100):                    # before the event: on the diagonal of the left part
                g.seed(0, br, x, min(bl, x), tag + "_left")
            for x in (ev + 100 + max(0, -shift), ev + 1000, 16000, 19000):  # behind it: on the diagonal of the right part
                g.seed(0, br, x, min(bl, x + shift), tag + "_right")
            for dx in (-10, -3, 0, 3, 10):                                 # within 10 bases of it, on either diagonal
                g.seed(0, br, ev + dx, min(bl, ev + dx), tag + "_near")
                g.seed(0, br, ev + dx + max(0, -shift), min(bl, ev + dx + max(0, -shift) + shift), tag + "_near")
        out.append(g)
    return out


def _unrelated():
    rng = np.random.RandomState(103)
    g = Group("unrelated", [_rand(rng, 2000), _rand(rng, 5000)], [_rand(rng, 3000), _rand(rng, 14)])
    for ar in (0, 1):
        for br in (0, 1):
            al, bl = len(g.areads[ar]), len(g.breads[br])
            for _ in range(4):
                g.seed(ar, br, rng.randint(1, al), rng.randint(1, bl), "interior")
            g.seed(ar, br, 0, bl // 2, "x=0")
            g.seed(ar, br, al, bl // 3, "x=alen")
            g.seed(ar, br, al // 2, 0, "y=0")
            g.seed(ar, br, al // 3, bl, "y=blen")
            g.seed(ar, br, 0, 0, "corner")
            g.seed(ar, br, al, bl, "corner")
            g.seed(ar, br, 0, bl, "corner")
            g.seed(ar, br, al, 0, "corner")
    return [g]


def _lowcx():
    rng = np.random.RandomState(104)
    unit = np.array([0, 2, 1, 1, 3, 0, 2], dtype=np.uint8)
    u7 = np.tile(unit, 300)
    hom = lambda n: np.zeros(n, dtype=np.uint8)
    ac = np.tile(np.array([0, 1], dtype=np.uint8), 300)
    A = [hom(600), ac, u7]
    B = [hom(600), hom(500), ac, _cat(ac[1:], [0]), u7.copy(), _mutate(rng, u7, .12)]
    g = Group("lowcx", A, B)
    for br, tag in ((0, "homo600"), (1, "homo500")):
        bl = len(B[br])
        for x, y in ((300, 300), (0, 0), (600, bl), (300, 100), (100, 300), (599, bl - 1), (1, 1), (450, 17)):
            g.seed(0, br, x, y, tag)
    for br, tag in ((2, "ac_self"), (3, "ac_shift1")):
        for x, y in ((300, 300), (300, 301), (301, 300), (0, 0), (600, 600), (17, 16), (16, 48), (599, 598), (200, 400)):
            g.seed(1, br, x, y, tag)
    for br, tag in ((4, "u7_clean"), (5, "u7_noisy")):
        bl = len(B[br])
        for off in (0, 7, -7, 14, -14, 21):
            for x in (100, 1050, 2000):
                g.seed(2, br, x, max(0, min(bl, x * bl // 2100 - off)), tag)
    return [g]


SHORT_LENS = [1, 2] + list(range(13, 18)) + [31, 32, 33, 47, 48, 49, 63, 64, 65, 99, 100, 101, 199, 200, 201]


def _short_reads(rng):
    A = [_rand(rng, n) for n in SHORT_LENS]
    one = []
    for a in A:
        b = a.copy()
        b[len(b) // 3] = (b[len(b) // 3] + 1) & 3
        one.append(b)
    return A, [a.copy() for a in A] + one


def _short():
    rng = np.random.RandomState(105)
    A, B = _short_reads(rng)
    g = Group("short", A, B)
    for i, n in enumerate(SHORT_LENS):
        for br, tag in ((i, "same%d" % n), (i + len(SHORT_LENS), "mis%d" % n)):
            for p in (0, n, n // 2, n - 1):
                g.seed(i, br, p, p, tag)
    return [g]


END_DIST = (0, 1, 15, 16, 17)


def _ends():
    rng = np.random.RandomState(106)
    a = _rand(rng, 3000)
    A = [a, a[500:2500].copy()]
    B = [a.copy(), _mutate(rng, a, .10), a[:2000].copy(), a[1000:].copy(), a[500:2500].copy()]
    out = []
    for comp in (0, 1):
        g = Group("ends_c%d" % comp, A, B, comp=comp)
        nl = len(B[1])
        for k in END_DIST:
            g.seed(0, 0, k, k, "same_both_begin")
            g.seed(0, 0, 3000 - k, 3000 - k, "same_both_end")
            g.seed(0, 1, k, k, "noisy_both_begin")
            g.seed(0, 1, 3000 - k, nl - k, "noisy_both_end")
            g.seed(0, 2, k, k, "prefix_both_begin")
            g.seed(0, 2, 2000 - k, 2000 - k, "prefix_B_end")
            g.seed(0, 3, 1000 + k, k, "suffix_B_begin")
            g.seed(0, 3, 3000 - k, 2000 - k, "suffix_both_end")
            g.seed(0, 4, 500 + k, k, "infix_B_begin")
            g.seed(0, 4, 2500 - k, 2000 - k, "infix_B_end")
            g.seed(1, 0, k, 500 + k, "infix_A_begin")
            g.seed(1, 0, 2000 - k, 2500 - k, "infix_A_end")
        out.append(g)
    return out


def _mixed():
    """short and 20 kb reads in one block; neighbouring tasks (the two halves of a wavefront of the two-pair kernel) are a
    short and a long one, the long ones in turn forward-heavy (seed near the begin) and reverse-heavy (seed near the end)"""
    rng = np.random.RandomState(107)
    sa, sb = _short_reads(rng)
    pick = [SHORT_LENS.index(n) for n in (14, 1, 33, 64, 200, 17)]
    A, B, shorts, longs = [], [], [], []
    for j, i in enumerate(pick):
        big = _rand(rng, 20000 - 1000 * j)
        A += [sa[i], big]
        B += [sb[i], _mutate(rng, big, .05)]
        shorts.append(2 * j)
        longs.append(2 * j + 1)
    order = []
    for t in range(2 * MIXED_SLOTS + 1):
        j = (t // 2) % len(pick)
        both = (t // 2) % 3 == 2                       # every third wavefront: two long ones, forward- and reverse-heavy
        if not both and t % 2 == (t // 4) % 2:         # short first in one wavefront, long first in the next
            r = shorts[j]
            n = len(A[r])
            order.append((r, r, n // 2, n // 2, "short"))
        else:
            r = longs[(j + t % 2) % len(pick)] if both else longs[j]
            al, bl = len(A[r]), len(B[r])
            if (t % 2 == 0) if both else ((t // 2) % 2 == 0):
                order.append((r, r, 40, 40, "long_forward"))
            else:
                order.append((r, r, al - 40, bl - 40, "long_reverse"))
    order.append((shorts[0], longs[0], 7, 10000, "short_x_long"))       # a 14-base read against a 20 kb read
    out = []
    for cnt in (1, 2, 3, 2 * MIXED_SLOTS + 1):
        g = Group("mixed_%d" % cnt, A, B)
        take = order[1:2] if cnt == 1 else (order[:cnt - 1] + order[-1:] if cnt > 3 else order[:cnt])
        for ar, br, x, y, tag in take:
            g.seed(ar, br, x, y, tag)
        assert len(g.tasks) == cnt
        out.append(g)
    return out


SPACINGS = (8, 50, 125, 126, 1000, 8192)


def _spacing():
    A, B = _noisy_pair()
    out = []
    for ts in SPACINGS:
        for comp in (0, 1):
            g = Group("spacing_s%d_c%d" % (ts, comp), A, B, tspace=ts, comp=comp)
            for br in (0, 1):
                _seeds_along(g, 0, br, 500, "s%d" % ts)
            out.append(g)
    rng = np.random.RandomState(108)
    a = _rand(rng, 20000)
    b = _mutate(rng, a, .02)
    for comp in (0, 1):                                # 20 000 spacings of one base: beyond the packed chain heads by read length
        g = Group("spacing_marks_c%d" % comp, [a], [b], tspace=1, comp=comp)
        assert len(a) // g.tspace + 8 > MAX_MARKS
        g.seed(0, 0, 10000, min(len(b), 10000), "over_marks")
        out.append(g)
    return out


CORRS = (.65, .75, .85, .95, 1.0)


def _corr():
    A, B = _noisy_pair()
    out = []
    for e in CORRS:
        for comp in (0, 1):
            g = Group("corr_e%g_c%d" % (e, comp), A, B, e=e, comp=comp)
            for br in (0, 1):
                _seeds_along(g, 0, br, 500, "e%g" % e)
            out.append(g)
    return out


FAMILIES = {"noisy": _noisy, "indel": _indel, "unrelated": _unrelated, "lowcx": _lowcx, "short": _short, "ends": _ends,
            "mixed": _mixed, "spacing": _spacing, "corr": _corr}
T8_FAMILIES = ("noisy", "indel", "lowcx", "ends", "spacing")       # run once more with byte traces (groups of tspace <= 125)

_made = {}


def family(name):
    """the groups of a family, the REMOVED tasks taken out"""
    if name not in _made:
        groups = FAMILIES[name]()
        gone = dict(REMOVED.get(name, {}))
        total = sum(len(g.tasks) for g in groups)
        tags = set(t for g in groups for t in g.tags)
        for g in groups:
            keep = [t for t in range(len(g.tasks)) if (g.name, g.tasks[t][0], g.tasks[t][1]) + g.point(t) not in gone]
            for t in range(len(g.tasks)):
                gone.pop((g.name, g.tasks[t][0], g.tasks[t][1]) + g.point(t), None)
            g.tasks, g.tags = [g.tasks[t] for t in keep], [g.tags[t] for t in keep]
        assert not gone, "REMOVED names tasks that %s does not have: %s" % (name, gone)
        left = sum(len(g.tasks) for g in groups)
        assert (total - left) * 50 <= total, "more than 2 %% of %s removed" % name
        assert tags == set(t for g in groups for t in g.tags), "a sub-shape of %s lost all its tasks" % name
        assert left <= 210 and max(len(r) for g in groups for r in g.areads + g.breads) <= 20600
        _made[name] = groups
    return _made[name]


def make_db(reads):
    """A HITS_DB (db/DB.h layout: a 4 in front of the first read and behind every read) of the given reads."""
    from damar_amd import api
    total = sum(len(r) for r in reads) + len(reads)
    buf = np.full(total + 1, 4, dtype=np.uint8)
    recs = (api.HITS_READ * (len(reads) + 1))()
    off = 0
    for i, r in enumerate(reads):
        buf[1 + off:1 + off + len(r)] = r
        recs[i].rlen, recs[i].boff = len(r), off
        off += len(r) + 1
    recs[len(reads)].boff = off
    db = api.HITS_DB()
    db.ureads = db.nreads = len(reads)
    db.maxlen, db.totlen = max(len(r) for r in reads), sum(len(r) for r in reads)
    db.part, db.ufirst, db.loaded = 1, 0, 1
    for i in range(4):
        db.freq[i] = .25
    db.bases = buf.ctypes.data + 1
    db.reads = C.cast(recs, C.POINTER(api.HITS_READ))
    db._keep = (buf, recs)
    return db


def write_family(path, groups):
    """the file oracle/ref_localalign.c reads: int32 ngroups, then per group int32 na, nb, ntasks, tspace, comp, float64 e,
    the A reads and the B reads as (int32 length, bases 0..3), the tasks as 4 int32 each"""
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(groups)))
        for g in groups:
            f.write(struct.pack("<5id", len(g.areads), len(g.breads), len(g.tasks), g.tspace, g.comp, g.e))
            for r in g.areads + g.breads:
                f.write(struct.pack("<i", len(r)))
                f.write(np.asarray(r, dtype=np.uint8).tobytes())
            for t in g.tasks:
                f.write(struct.pack("<4i", *t))


def dump(results):
    """what ref_localalign writes per task: the 12 path integers (A path, then B path: abpos, bbpos, aepos, bepos, diffs,
    tlen), then the A trace and the B trace as uint16"""
    out = []
    for p, at, bt in results:
        out.append(struct.pack("<12i", *p))
        out.append(np.asarray(at, dtype="<u2").tobytes())
        out.append(np.asarray(bt, dtype="<u2").tobytes())
    return b"".join(out)


_oracle = {}


def oracle(name):
    """the oracle's answers for a family, computed once per process: per group a list of (12 path integers, A trace, B trace)
    and a list of the tasks' own OWaveStats"""
    if name not in _oracle:
        import oracle_api as O
        res = []
        for g in family(name):
            adb, bdb = make_db(g.areads), make_db(g.breads)
            spec = O.lib().New_Align_Spec(g.e, g.tspace, adb.freq, 1, 1, 0, 0, 1)
            ans, stats = [], []
            for ar, br, dg, anti in g.tasks:
                st = O.OWaveStats()
                ans.append(O.local_alignment(adb, bdb, ar, br, g.comp, dg, anti, spec, g.maxtp(), st))
                stats.append(st)
            res.append((ans, stats))
        _oracle[name] = res
    return _oracle[name]


def check_reach():
    """What the families are for, asserted on the ORACLE's statistics and answers (never on the code under test): without
    this a family that silently stopped exercising its path would still pass."""
    for name in ("noisy", "indel", "unrelated"):           # the band leaves the 30 lanes of a half, and the 62 of a wavefront
        mb = [st.maxband for _, stats in oracle(name) for st in stats]
        assert sum(m > 30 for m in mb) >= 5 and sum(m > 62 for m in mb) >= 1, (name, sorted(mb)[-5:])
    # a pass of more than 100 wave steps: pass_cells / pass_max of a task's own statistics are those of its LAST pass (the
    # reverse one), so its steps are at least pass_cells / pass_max
    assert any(st.pass_max > 0 and st.pass_cells > 100 * st.pass_max for _, stats in oracle("lowcx") for st in stats)
    g, (ans, _) = family("short")[0], oracle("short")[0]
    for i, n in enumerate(SHORT_LENS):                     # every short length has a path over the whole read
        assert any(g.tasks[t][0] == i and ans[t][0][:4] == [0, 0, n, n] for t in range(len(g.tasks))), n
