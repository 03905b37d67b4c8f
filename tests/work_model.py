"""The reference's rule for which read pairs are aligned at all, in plain Python over unpacked seeds (bread, aread, apos,
diag) -- a model of dalign/filter.c, NOT of the kernels that build the work list (kernels/seed_merge.hip):

  slices   Match_Filter, filter.c:2804-2816: beg_0 = 0; the nominal start p = (nhits * t) >> NSHIFT of slice t moves on while
           bread equals that of seed p - 1; the last slice ends at nhits.
  heads    report_thread, filter.c:2210-2220: minhit = (Hitmin - 1) / Kmer + 1; walking a slice run by run, a run is entered
           when its first seed nidx < end - minhit and seed nidx + minhit - 1 is the same read pair.
  screen   filter.c:2268-2297: per diagonal bucket (diag >> Binshift, a floor shift) score += min(Kmer, apos - lastp), in seed
           order, score and lastp starting at 0; a seed calls Local_Alignment when score[d] + score[d + 1] >= Hitmin or
           score[d] + score[d - 1] >= Hitmin (its A position is beyond lasta[d], which is 0 before the pair's first call, and
           real A positions are at least Kmer - 1 > 0).

A run of at most SCREEN_MAX seeds whose A positions are all at most SCREEN_PANEL is one panel of the reference (filter.c:
2251-2263), so for it "some seed fires" is exactly "report_thread calls Local_Alignment for this pair".  The device may keep
without screening what its kernels document: runs of more than SCREEN_MAX seeds, every run when minhit > SCREEN_MAX, and a
run with an A position above SCREEN_PANEL (sorted seeds: the last seed's; seeds in no order: the largest).  Beside the
reference's rule the device has two of its own, modelled here as documented in include/damar_hip.h: only B reads in
[b_lo, b_hi) are kept, and nshift < 0 means "no slices" (the slice rule was applied before, only seed nidx + minhit - 1 has to
exist)."""
import numpy as np

SCREEN_MAX = 48           # kernels/seed_merge.hip SCREEN_MAX
SCREEN_PANEL = 50000      # kernels/seed_merge.hip SCREEN_PANEL = PANEL_SIZE, filter.c:73
OR_MAX = 2048             # kernels/seed_merge.hip OR_MAX: the longest run that is ordered


def pack(bread, aread, apos, diag, ppos, dbits, abits):
    """-> (keys, vals): ((bread << abits | aread) << ppos | apos) << dbits | bpos with bpos = apos - diag; with dbits == 0 the
    key ends with apos and the diagonal is a u32 in vals (None otherwise)."""
    bread, aread, apos, diag = (np.asarray(x, dtype=np.int64) for x in (bread, aread, apos, diag))
    assert (aread >= 0).all() and (aread < (1 << abits)).all() and (apos >= 0).all() and (apos < (1 << ppos)).all()
    assert (bread >= 0).all() and ppos + dbits + abits < 64 and (bread < (1 << (64 - ppos - dbits - abits))).all()
    pair = (bread.astype(np.uint64) << np.uint64(abits)) | aread.astype(np.uint64)
    keys = (pair << np.uint64(ppos)) | apos.astype(np.uint64)
    if dbits == 0:
        return keys, (diag & 0xffffffff).astype(np.uint32)
    bpos = apos - diag
    assert (bpos >= 0).all() and (bpos < (1 << dbits)).all()
    return (keys << np.uint64(dbits)) | bpos.astype(np.uint64), None


def unpack(keys, vals, ppos, dbits, abits):
    """-> bread, aread, apos, diag (int64 arrays): the inverse of pack"""
    k = np.asarray(keys, dtype=np.uint64)
    bpos = (k & np.uint64((1 << dbits) - 1)).astype(np.int64)
    k = k >> np.uint64(dbits)
    apos = (k & np.uint64((1 << ppos) - 1)).astype(np.int64)
    k = k >> np.uint64(ppos)
    aread = (k & np.uint64((1 << abits) - 1)).astype(np.int64)
    bread = (k >> np.uint64(abits)).astype(np.int64)
    diag = (apos - bpos) if dbits else np.asarray(vals, dtype=np.uint32).astype(np.int32).astype(np.int64)
    return bread, aread, apos, diag


def slices(bread, nshift):
    """filter.c:2804-2816 -> [(beg, end)] of the 1 << nshift thread slices of the whole sorted list"""
    n = len(bread)
    nthreads = 1 << nshift
    beg = [0]
    for t in range(1, nthreads):
        p = (n * t) >> nshift
        if p > 0:
            d = bread[p - 1]
            while p < n and bread[p] == d:               # (the reference stops at its sentinel seed behind the last)
                p += 1
        beg.append(p)
    return [(beg[t], beg[t + 1] if t + 1 < nthreads else n) for t in range(nthreads)]


def minhit_of(kmer, hitmin):
    return (hitmin - 1) // kmer + 1


def run_fires(apos, diag, kmer, hitmin, binshift):
    """filter.c:2268-2297 over one panel: does some seed of the run call Local_Alignment?"""
    score, lastp = {}, {}
    for a, dg in zip(apos, diag):
        d = int(dg) >> binshift
        a = int(a)
        if a - lastp.get(d, 0) >= kmer:
            score[d] = score.get(d, 0) + kmer
        else:
            score[d] = score.get(d, 0) + a - lastp.get(d, 0)
        lastp[d] = a
    for dg in diag:
        d = int(dg) >> binshift
        if score[d] + score.get(d + 1, 0) >= hitmin or score[d] + score.get(d - 1, 0) >= hitmin:
            return True
    return False


def run_fires_brute(apos, diag, kmer, hitmin, binshift):
    """The same statement without the reference's loop: bucket sums, then "any two adjacent buckets reach hitmin"."""
    apos, diag = np.asarray(apos, dtype=np.int64), np.asarray(diag, dtype=np.int64)
    b = diag >> binshift
    total = {}
    for d in np.unique(b):
        a = apos[b == d]                                   # (in seed order)
        total[int(d)] = int(np.minimum(kmer, np.diff(np.concatenate(([0], a)))).sum())
    lo, hi = min(total), max(total)
    return any(total.get(d, 0) + total.get(d + 1, 0) >= hitmin for d in range(lo - 1, hi + 1))


def work_list(bread, aread, apos, diag, kmer, hitmin, binshift, nshift, b_lo=0, b_hi=1 << 32, unsorted=False, off=0, nhits=None):
    """The whole list's seeds in the order the device gets them (sorted; or, unsorted=True, sorted by read pair only).
    -> dict(heads, must, may, flag): sorted seed indices relative to `off`, of the stretch [off, off + nhits) only.
    heads: the runs report_thread enters (B reads in [b_lo, b_hi)); must: those of them that fire; may: must plus those the
    device may keep unscreened; flag: 1 iff some run of `may` has more than OR_MAX seeds."""
    bread, aread, apos, diag = (np.asarray(x, dtype=np.int64) for x in (bread, aread, apos, diag))
    n = len(bread)
    nhits = n - off if nhits is None else nhits
    minhit = minhit_of(kmer, hitmin)
    heads, must, may, flag = [], [], [], 0
    if n == 0:
        return dict(heads=np.zeros(0, np.int64), must=np.zeros(0, np.int64), may=np.zeros(0, np.int64), flag=0)
    pair = list(zip(bread.tolist(), aread.tolist()))
    pair.append(None)                                      # the sentinel behind the last seed (filter.c:2778-2781)
    for beg, end in (slices(bread, nshift) if nshift >= 0 else [(0, n + 1)]):
        eidx = end - minhit
        nidx = beg
        while nidx < eidx:
            cpair = pair[nidx]
            last = nidx + 1
            while pair[last] == cpair:
                last += 1
            if pair[nidx + minhit - 1] == cpair and b_lo <= bread[nidx] < b_hi and off <= nidx < off + nhits:
                heads.append(nidx - off)
                a, d = apos[nidx:last], diag[nidx:last]
                if unsorted:                               # the order the full sort would have left
                    o = np.argsort(a, kind="stable")
                    a, d = a[o], d[o]
                top = int(a.max()) if unsorted else int(a[-1])
                if last - nidx > SCREEN_MAX or minhit > SCREEN_MAX or top > SCREEN_PANEL:
                    may.append(nidx - off)
                    if last - nidx > OR_MAX:
                        flag = 1
                elif run_fires(a, d, kmer, hitmin, binshift):
                    must.append(nidx - off)
                    may.append(nidx - off)
            nidx = last
    return dict(heads=np.array(heads, np.int64), must=np.array(must, np.int64), may=np.array(may, np.int64), flag=flag)
