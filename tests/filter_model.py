"""A model of LAfilter's method on one pile, in plain Python, written from what the reference does and not from host/filter.c:
the steps in the reference's order, every record a dict.  tests/test_filter_host.py holds damar_host_filter_pile to it
field for field.  The names of the options are those api.pile_filter takes."""

COMP, DISCARD, REPEAT, LOCAL, DIFF, STITCH, SYM, OLEN, RLEN = 0x1, 0x2, 0x8, 0x10, 0x20, 0x80, 0x100, 0x200, 0x400
CONT, GAP, TRIM, MODULE = 0x8000, 0x10000, 0x20000, 0x40000
# the method got wrong in one place each: what filter_pile and run_batch take as `mutant`
MUTANTS = ("r4_single_count", "stitch_first", "z_enter_lt", "z_leave_gt", "z_bases_lt", "z_uncovered_ge", "cover_end_bit", "cover_outside_trim",
           "w_skips_last", "cont_by_first", "b_last_segment", "one_byte_trace")
# reason bits and counters, as include/damar_hip.h numbers them
R_SYM, R_OLEN, R_LOCAL, R_DIFF, R_TIPS, R_ALEN, R_AREP, R_BLEN, R_BREP, R_TP, R_MULTI, R_SELF, R_CONT, R_HEAD = (1 << k for k in range(14))
C_DIFFS, C_UNAL, C_CONT, C_LEN, C_REP, C_RLEN, C_LOWCOV, C_SYM, C_MULTI, C_MBASES, C_STITCHED = range(11)


def runs(recs):
    """the runs of consecutive records of one B read, as they lie"""
    out, j = [], 0
    while j < len(recs):
        k = j
        while k + 1 < len(recs) and recs[k + 1]["b"] == recs[j]["b"]:
            k += 1
        out.append(list(range(j, k + 1)))
        j = k + 1
    return out


def overlap(b0, e0, b1, e1):
    return max(0, min(e0, e1) - max(b0, b1))


def inside(b0, e0, b1, e1):
    return b0 >= b1 and e0 <= e1


def repeat_site(o, aread, rl, tab, tae, rep, need, tips):
    """which of filter()'s five repeat tests drops the record, or 0"""
    ra, rb = rep(aread), rep(o["b"])
    lo, hi = tab, tae
    if tips:
        cum = 0
        for b, e in ra:
            if b > tab + tips:
                break
            if e < tab:
                continue
            cum += e - max(b, tab)
            if e > tab + tips:
                break
        if cum > 1 + tips // 3:
            lo = tab + tips
        cum = 0
        for b, e in ra:
            if e < tae - tips:
                continue
            if b > tae:
                break
            cum += min(e, tae) - b
        if cum > 1 + tips // 3:
            hi = tae - tips
    if hi < lo:
        return R_TIPS
    left = min(o["ae"], hi) - max(o["ab"], lo)
    if left < need:
        return R_ALEN
    r = sum(overlap(o["ab"], o["ae"], max(b, lo), min(e, hi)) for b, e in ra if not (e < lo or b > hi))
    if r > 0 and left - r < need:
        return R_AREP
    cut_e, cut_b = max(0, o["ae"] - hi), max(0, lo - o["ab"])
    left = o["be"] - o["bb"] - cut_e - cut_b
    if left < need:
        return R_BLEN
    blen = rl[o["b"]]
    if o["flags"] & COMP:
        b0, e0 = blen - (o["be"] - cut_e), blen - (o["bb"] - cut_b)
    else:
        b0, e0 = o["bb"] + cut_b, o["be"] - cut_e
    r = sum(overlap(b0, e0, b, e) for b, e in rb)
    return R_BREP if r > 0 and left - r < need else 0


def filter_pile(aread, recs, rl, pre=True, main=True, downsample=0, seg_rate=-1, stitch=-1, stitch_aggr=False, min_rlen=-1, min_olen=-1,
                max_unaligned=-1, min_nonrep=-1, max_diffs=-1.0, merge_tips=0, multi=False, lowcov=0, remove=0, trim=None, rep=None,
                sym=None, read_state=None, include=False, mutant=None):
    """recs: dicts of b, ab, ae, bb, be, flags, diffs and trace (the values as they lie: diffs at even, B lengths at odd
    places; None once dropped).  trim(r) -> (b, e) or None without a track; rep(r) -> list of intervals; sym(r) -> the list
    a read's pairs are looked up in.  Changes the records in place, adds `why` and `by`; -> the counters.  mutant: one of
    MUTANTS, the method got wrong in one place, for the tests that hold the shapes of tests/filter_shapes.py to their names."""
    import numpy as np
    cnt = [0] * 11
    for o in recs:
        o["why"], o["by"] = 0, -1
    if pre:
        if downsample:
            top = int(downsample * len(rl) / 100.0)
            for o in recs:
                if aread > top or o["b"] > top:
                    o["flags"] |= DISCARD
        if 0 <= seg_rate <= 100:
            for o in recs:
                t = o["trace"]
                for k in range(0, len(t) - (0 if mutant == "b_last_segment" else 2), 2):
                    with np.errstate(divide="ignore", invalid="ignore"):
                        bad = np.float64(t[k]) * 100.0 / np.float64(t[k + 1]) > seg_rate
                    if bad:
                        o["flags"] |= DISCARD | DIFF
                        cnt[C_DIFFS] += 1
                        break
    if not main or not recs:
        return cnt
    alen = rl[aread]
    tab, tae = (0, alen) if trim is None else trim(aread)

    if stitch >= 0:
        skip = CONT | STITCH | GAP | TRIM
        for run in runs(recs):
            for pos, i in enumerate(run):
                h = recs[i]
                if len(run) < 2 or h["flags"] & skip:
                    continue
                while True:
                    best = None
                    for k in run[pos + 1:]:
                        o = recs[k]
                        if o["flags"] & skip or (o["flags"] ^ h["flags"]) & COMP:
                            continue
                        da, db = abs(h["ae"] - o["ab"]), abs(h["be"] - o["bb"])
                        if da < stitch and db < stitch and (stitch_aggr or abs(da - db) < 40):
                            if o["ae"] - o["ab"] > (recs[best]["ae"] - recs[best]["ab"] if best is not None else 0):
                                best = k
                                if mutant == "stitch_first":
                                    break
                    if best is None:
                        break
                    o = recs[best]
                    h["ae"], h["be"], h["diffs"], h["trace"] = o["ae"], o["be"], h["diffs"] + o["diffs"], None
                    h["flags"] &= ~(DISCARD | LOCAL)
                    h["why"] |= R_HEAD
                    o["flags"] |= DISCARD | STITCH
                    cnt[C_STITCHED] += 1

    for o in recs:
        blen = rl[o["b"]]
        tbb, tbe = (0, blen) if trim is None else trim(o["b"])
        tblen = tbe - tbb
        if o["flags"] & COMP:
            tbb, tbe = blen - tbe, blen - tbb
        n = min(o["ae"] - o["ab"], o["be"] - o["bb"])
        add = 0
        if sym is not None:
            lo, hi = min(aread, o["b"]), max(aread, o["b"])
            if hi in sym(lo):
                add |= DISCARD | SYM
                cnt[C_SYM] += 1
                o["why"] |= R_SYM
        if min_rlen != -1 and (tae - tab < min_rlen or tblen < min_rlen):
            add |= DISCARD | RLEN
            cnt[C_RLEN] += 1
        if min_olen != -1 and n < min_olen:
            add |= DISCARD | OLEN
            cnt[C_LEN] += 1
            o["why"] |= R_OLEN
        if max_unaligned != -1:
            u = max_unaligned
            if (o["ab"] - tab > u and o["bb"] - tbb > u) or (tae - o["ae"] > u and tbe - o["be"] > u):
                add |= DISCARD | LOCAL
                cnt[C_UNAL] += 1
                o["why"] |= R_LOCAL
        if max_diffs > 0:
            with np.errstate(divide="ignore", invalid="ignore"):
                bad = np.float64(o["diffs"]) / np.float64(n) > np.float64(np.float32(max_diffs))
            if bad:
                add |= DISCARD | DIFF
                cnt[C_DIFFS] += 1
                o["why"] |= R_DIFF
        if min_nonrep != -1:
            site = repeat_site(o, aread, rl, tab, tae, rep, min_nonrep, merge_tips)
            if site:
                add |= DISCARD | REPEAT
                cnt[C_REP] += 1
                o["why"] |= site
        if remove & 4 and not o["flags"] & DISCARD:
            t = o["trace"] if o["trace"] is not None else []
            if o["bb"] + sum(int(x) for x in t[1::2]) != o["be"]:
                add |= DISCARD
                o["why"] |= R_TP
        o["flags"] |= add

    if multi:
        for run in runs(recs):
            live = [k for k in (run[:-1] if mutant == "w_skips_last" else run) if not recs[k]["flags"] & (STITCH | DISCARD)]
            hit = any(inside(x["ab"], x["ae"], y["ab"], y["ae"]) or inside(y["ab"], y["ae"], x["ab"], x["ae"]) or
                      inside(x["bb"], x["be"], y["bb"], y["be"]) or inside(y["bb"], y["be"], x["bb"], x["be"])
                      for p, i in enumerate(live) for j in live[p + 1:] for x, y in [(recs[i], recs[j])])
            if hit and len(run) > 1:
                for k in run:
                    recs[k]["flags"] |= DISCARD
                    recs[k]["why"] |= R_MULTI
                    cnt[C_MULTI] += 1
                    cnt[C_MBASES] += recs[k]["ae"] - recs[k]["ab"]

    if lowcov and tae - tab:
        live = [o for o in recs if not o["flags"] & DISCARD]
        enter = sum(o["ab"] < tab if mutant == "z_enter_lt" else o["ab"] <= tab for o in live)
        leave = sum(o["ae"] > tae if mutant == "z_leave_gt" else o["ae"] >= tae for o in live)
        bases = sum(o["ae"] - o["ab"] for o in live)
        mean = int(bases / (tae - tab))
        drop = (mean < lowcov if mutant == "z_bases_lt" else mean <= lowcov) or enter < lowcov or leave < lowcov
        if max_unaligned != -1:
            cov = np.zeros(alen + 1, dtype=bool)
            for o in live:
                cov[max(o["ab"], 0):min(o["ae"], alen) - (1 if mutant == "cover_end_bit" else 0)] = True
            lo, hi = (0, alen) if mutant == "cover_outside_trim" else (tab, tae)
            bare = (hi - lo) - int(cov[lo:hi].sum())
            drop = drop or (bare >= max_unaligned if mutant == "z_uncovered_ge" else bare > max_unaligned)
        if drop:
            for o in live:
                o["flags"] |= DISCARD
                cnt[C_LOWCOV] += 1

    if remove:
        for o in recs:
            if remove & 4:
                o["trace"] = None
            if remove & 2 and o["flags"] & MODULE:
                o["flags"] |= DISCARD
            elif remove & 1 and (o["trace"] is None or len(o["trace"]) == 0):
                o["flags"] |= DISCARD
            elif remove & 8 and o["b"] != aread:
                o["flags"] |= DISCARD
            elif remove & 32 and o["b"] == aread:
                o["flags"] |= DISCARD
        is_proper = lambda o: (o["ab"] == 0 or o["bb"] == 0) and (o["ae"] == alen or o["be"] == rl[o["b"]])
        same = lambda o: o["b"] == aread and o["ab"] == o["bb"] and o["ae"] == o["be"]
        if remove & 16:
            for run in runs(recs):
                # the reference counts the first record of every run but the pile's first twice
                twice = run[0] > 0 and mutant != "r4_single_count"
                n = sum(is_proper(recs[k]) for k in run) + (1 if twice and is_proper(recs[run[0]]) else 0)
                if n == 1 and len(run) > 1:
                    for k in run:
                        if not is_proper(recs[k]):
                            recs[k]["flags"] |= DISCARD
        if remove & 64:
            for run in runs(recs):
                for p, i in enumerate(run):
                    x = recs[i]
                    if len(run) > 1 and x["flags"] & DISCARD:
                        continue
                    if same(x):
                        x["flags"] |= DISCARD | CONT
                        x["why"] |= R_SELF
                        cnt[C_CONT] += 1
                        continue
                    for j in run[p + 1:]:
                        y = recs[j]
                        if y["flags"] & DISCARD:
                            continue
                        if x["b"] != aread:
                            gone = inside(y["ab"], y["ae"], x["ab"], x["ae"]) and inside(y["bb"], y["be"], x["bb"], x["be"])
                        else:
                            gone = (y["ab"], y["ae"], y["bb"], y["be"]) == (x["ab"], x["ae"], x["bb"], x["be"])
                        if gone:
                            y["flags"] |= DISCARD | CONT
                            y["why"] |= R_CONT
                            y["by"] = run[0] if mutant == "cont_by_first" else i
                            cnt[C_CONT] += 1

    if read_state is not None:
        for o in recs:
            sa, sb = int(read_state[aread]), int(read_state[o["b"]])
            if sa & 1 or sb & 1 or (include and not sa & 2 and not sb & 2):
                o["flags"] |= DISCARD
    return cnt


def run_batch(batch, rl, **kw):
    """the model over a batch of the tests' trace_batch form with api.pile_filter's keywords: -> the same dict of arrays"""
    import numpy as np
    trim_arr, reps, sym = kw.pop("trim", None), kw.pop("repeats", None), kw.pop("sym", None)
    steps, mutant = kw.pop("steps", 3), kw.get("mutant")
    trim = None if trim_arr is None else (lambda r: (int(trim_arr[2 * r]), int(trim_arr[2 * r + 1])))
    rep = None
    if reps is not None:
        anno, data = reps
        rep = lambda r: [(int(data[k]), int(data[k + 1])) for k in range(int(anno[r]) // 4, int(anno[r + 1]) // 4, 2)]
    symf = None
    if sym is not None:
        so, sl, sd = sym
        symf = lambda r: [int(x) for x in sd[so[r]:so[r] + sl[r]]]
    n = len(batch["abpos"])
    out = {k: np.zeros(n, dtype=np.int32) for k in ("flags", "aepos", "bepos", "diffs", "tlen", "reason", "cont_by")}
    cnts = []
    tb = batch["tbytes"]
    for p, aread in enumerate(batch["pile_aread"]):
        lo, hi = int(batch["pile_off"][p]), int(batch["pile_off"][p + 1])
        recs = []
        for i in range(lo, hi):
            raw = batch["trace"][int(batch["trace_off"][i]):int(batch["trace_off"][i]) + tb * int(batch["tlen"][i])]
            vals = raw if tb == 1 else raw[0::2] if mutant == "one_byte_trace" else raw.view("<u2")
            recs.append(dict(b=int(batch["bread"][i]), ab=int(batch["abpos"][i]), ae=int(batch["aepos"][i]), bb=int(batch["bbpos"][i]),
                             be=int(batch["bepos"][i]), flags=int(batch["flags"][i]), diffs=int(batch["diffs"][i]), trace=[int(x) for x in vals]))
        cnts.append(filter_pile(int(aread), recs, [int(x) for x in rl], pre=bool(steps & 1), main=bool(steps & 2), trim=trim, rep=rep, sym=symf, **kw))
        for i, o in zip(range(lo, hi), recs):
            out["flags"][i], out["aepos"][i], out["bepos"][i], out["diffs"][i] = o["flags"], o["ae"], o["be"], o["diffs"]
            out["tlen"][i] = 0 if o["trace"] is None else len(o["trace"])
            out["reason"][i], out["cont_by"][i] = o["why"], o["by"]
    out["cnt"] = np.array(cnts, dtype=np.int32).reshape(len(cnts), 11)
    return out
