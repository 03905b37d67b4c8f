"""A model of LAseparate's chain() and of its two verdicts (scrub/LAseparate.c), written from the reference's text and kept
close to it: records are dicts with the reference's field names, the flags are the words of the file, a chain is a list of
records.  It is the yardstick of host/separate.c and kernels/pile_chains.hip where the reference's output cannot show a
field (the number of chains, the members of the best one, the working flags), and tests/golden/make_separate_golden.py
holds it to the reference's files.

    group(recs, alen, blen, twidth, rep, kind) -> dict(flags, nchains, best, proper)
"""
from functools import cmp_to_key

COMP, DISCARD, TEMP, CONT = 0x1, 0x2, 0x800, 0x8000
MIN_LOOK, MAX_LOOK, STRIDE = 5000, 30000, 5000


def intersect(ab, ae, bb, be):
    b, e = max(ab, bb), min(ae, be)
    return e - b if b < e else 0


def contained(ab, ae, bb, be):
    return ab >= bb and ae <= be


def repeat_bases(rep, o, read):
    """getRepeatBases: rep is (anno, data) of the whole database, or None"""
    if rep is None:
        return 0
    anno, data = rep
    blen = o["be"] - o["bb"]
    n = 0
    for t in range(int(anno[read]) // 4, int(anno[read + 1]) // 4, 2):
        rb, re = int(data[t]), int(data[t + 1])
        if o["aread"] == read:
            n += intersect(o["ab"], o["ae"], rb, re)
        elif o["flags"] & COMP:
            n += intersect(blen - o["be"], blen - o["bb"], rb, re)
        else:
            n += intersect(o["bb"], o["be"], rb, re)
    return n


def cmp_abeg(o1, o2):
    c = o1["ab"] - o2["ab"]
    return c if c else (o1["ae"] - o1["ab"]) - (o2["ae"] - o2["ab"])


def chain_len(c):
    n = c[0]["ae"] - c[0]["ab"]
    for i in range(1, len(c)):
        n += c[i]["ae"] - c[i]["ab"]
        if c[i - 1]["ae"] > c[i]["ab"]:
            n -= int(c[i - 1]["ae"] > c[i]["ab"])
    return n


def chain(ovls, alen, blen, twidth, rep):
    """-> the chains in the reference's final order; the flags of ovls are changed as the reference changes them"""
    n = len(ovls)
    chains = []
    if n < 2:
        return chains
    aread, bread = ovls[0]["aread"], ovls[0]["bread"]
    nremain = n
    for i in range(n):
        if ovls[i]["flags"] & CONT:
            continue
        for j in range(i + 1, n):
            if ovls[j]["flags"] & CONT:
                continue
            if contained(ovls[j]["ab"], ovls[j]["ae"], ovls[i]["ab"], ovls[i]["ae"]) and \
                    contained(ovls[j]["bb"], ovls[j]["be"], ovls[i]["bb"], ovls[i]["be"]):
                ovls[j]["flags"] |= CONT
    for o in ovls:
        if o["flags"] & (CONT | DISCARD):
            o["flags"] |= DISCARD
            nremain -= 1
    if nremain < 1:
        return chains

    while nremain > 0:
        uniq_bases = uniq_idx = long_bases = long_idx = -1
        for i, o in enumerate(ovls):
            if o["flags"] & (CONT | DISCARD | TEMP):
                continue
            a_len, b_len = o["ae"] - o["ab"], o["be"] - o["bb"]
            t = max(a_len - repeat_bases(rep, o, o["aread"]), b_len - repeat_bases(rep, o, o["bread"]))
            if t > uniq_bases:
                uniq_bases, uniq_idx = t, i
            t = max(a_len, b_len)
            if t > long_bases:
                long_bases, long_idx = t, i
        if uniq_bases < twidth and long_bases > uniq_bases:
            uniq_bases, uniq_idx = long_bases, long_idx
        assert uniq_idx >= 0, "the reference would index before its array here"
        k = uniq_idx
        ch = [ovls[k]]
        ovls[k]["flags"] |= TEMP
        nremain -= 1

        for side in (+1, -1):
            if not (nremain and (k + 1 < n if side > 0 else k > 0)):
                continue
            ab1, ae1, bb1, be1 = ovls[k]["ab"], ovls[k]["ae"], ovls[k]["bb"], ovls[k]["be"]
            best_uniq_off, best_uniq, best_bases, best_off, best_its = 1, -1, -1, 1, max(alen, blen)
            while True:
                step = MIN_LOOK
                while step <= MAX_LOOK and best_uniq == -1:
                    i = k + side * best_uniq_off
                    while 0 <= i < n:
                        o = ovls[i]
                        i += side
                        ab2, ae2, bb2, be2 = o["ab"], o["ae"], o["bb"], o["be"]
                        if (o["flags"] & COMP) != (ovls[k]["flags"] & COMP):
                            continue
                        if o["flags"] & (CONT | TEMP | DISCARD):
                            continue
                        if contained(ab2, ae2, ab1, ae1) or contained(bb2, be2, bb1, be1):
                            continue
                        if side > 0:
                            if ae2 < ae1 or be2 < be1:
                                continue
                            if max(ab2 - ae1, bb2 - be1) > step:
                                continue
                            if ae1 - ab2 > ae2 - ae1 or be1 - bb2 > be2 - be1:
                                continue
                        else:
                            if ab2 > ab1 or bb2 > bb1:
                                continue
                            if max(ab1 - ae2, bb1 - be2) > step:
                                continue
                            if ae2 - ab1 > ab1 - ab2 or be2 - bb1 > bb1 - bb2:
                                continue
                        ua = (ae2 - ab2) - repeat_bases(rep, o, aread)
                        ub = (be2 - bb2) - repeat_bases(rep, o, bread)
                        its = max(intersect(ab1, ae1, ab2, ae2), intersect(bb1, be1, bb2, be2))
                        here = abs((i - side) - k)
                        if best_its > its and best_bases < min(ae2 - ab2, be2 - bb2):
                            best_bases, best_off, best_its = min(ae2 - ab2, be2 - bb2), here, its
                        if best_uniq < min(ua, ub):
                            best_uniq_off = here
                            best_uniq = min(ua, ub) if side > 0 else ua + ub
                        elif best_uniq == -1 and step + STRIDE > MAX_LOOK:
                            t = ovls[k + side * best_off]
                            if intersect(ab1, ae1, t["ab"], t["ae"]) < ae1 - t["ab"] and intersect(bb1, be1, t["bb"], t["be"]) < be1 - t["bb"]:
                                best_uniq_off, best_uniq = best_off, 1
                    step += STRIDE
                if best_uniq < 0:
                    break
                o = ovls[k + side * best_uniq_off]
                ab1, ae1, bb1, be1 = o["ab"], o["ae"], o["bb"], o["be"]
                ch.append(o)
                o["flags"] |= TEMP
                nremain -= 1
                best_uniq_off += 1
                best_off = best_uniq_off
                best_uniq = best_bases = -1
                best_its = max(alen, blen)
                if not 0 <= k + side * best_uniq_off < n:
                    break
            if side < 0 and len(ch) > 1:
                ch.sort(key=cmp_to_key(cmp_abeg))

        if len(ch) > 1 and nremain > 0:
            ci, last = 0, len(ch) - 1
            for o in ovls:
                if (o["flags"] & (TEMP | CONT | DISCARD)) or (o["flags"] & COMP) != (ch[ci]["flags"] & COMP):
                    continue
                if o["ab"] < ch[ci]["ab"]:
                    continue
                if o["ab"] > ch[last]["ab"]:
                    break
                for j in range(ci, last):
                    if ch[j]["ae"] - 100 < o["ab"] and ch[j + 1]["ab"] + 100 > o["ae"] and ch[j]["be"] - 100 < o["bb"] and ch[j + 1]["bb"] + 100 > o["be"]:
                        la = ch[-1]
                        if intersect(o["ab"], o["ae"], la["ab"], la["ae"]) > 100 or intersect(o["bb"], o["be"], la["bb"], la["be"]) > 100:
                            break
                        o["flags"] |= TEMP
                        ch.append(o)
                        nremain -= 1
                    if o["ab"] > ch[j + 1]["ab"]:
                        ci += 1
            if last < len(ch) - 1:
                ch.sort(key=cmp_to_key(cmp_abeg))

        if nremain:
            ci, last = 0, len(ch) - 1
            for o in ovls:
                if (o["flags"] & (TEMP | CONT | DISCARD)) or (o["flags"] & COMP) != (ch[ci]["flags"] & COMP):
                    continue
                for j in range(ci, last + 1):
                    if intersect(ch[j]["ab"], ch[j]["ae"], o["ab"], o["ae"]) or intersect(ch[j]["bb"], ch[j]["be"], o["bb"], o["be"]):
                        o["flags"] |= DISCARD
                        nremain -= 1
                    if j + 1 < len(ch) and o["ab"] > ch[j + 1]["ab"]:
                        ci += 1

        valid = True
        for old in chains:
            if not valid:
                break
            if (ch[0]["flags"] & COMP) == int(bool(old[0]["flags"]) and bool(COMP)):
                for o in ch:
                    if (o["ab"] > old[0]["ab"] and o["ae"] < old[-1]["ae"]) or (o["bb"] > old[0]["bb"] and o["be"] < old[-1]["be"]):
                        valid = False
                        break
        if valid:
            chains.append(ch)
        else:
            for o in ch:
                o["flags"] |= DISCARD

    if len(chains) > 1:
        chains.sort(key=lambda c: -chain_len(c))           # stable, as glibc's merge sort is
    return chains


def single_proper(o, alen, blen, kind):
    pbeg = min(o["ab"], o["bb"]) < 1000
    pend = o["ae"] + 1000 > alen or o["be"] + 1000 > blen
    if kind == 0:
        return pbeg and pend
    return (pbeg and pend) and not (min(o["ab"], o["bb"]) == 0 and (o["ae"] == alen or o["be"] == blen))


def chain_proper(best, alen, blen, kind):
    pbeg = min(best[0]["ab"], best[0]["bb"]) < 1000
    pend = best[-1]["ae"] + 1000 > alen or best[-1]["be"] + 1000 > blen
    gap_a = gap_b = its_a = its_b = bases = 0
    if pbeg and pend:
        if kind == 1 and len(best) == 1:
            if min(best[0]["ab"], best[0]["bb"]) == 0 and (best[0]["ae"] == alen or best[0]["be"] == blen):
                pbeg = False
        else:
            bases = max(best[0]["ae"] - best[0]["ab"], best[0]["be"] - best[0]["bb"])
            for i in range(1, len(best)):
                xa = xb = 0
                bases += max(best[i]["ae"] - best[i]["ab"], best[i]["be"] - best[i]["bb"])
                if best[i]["ab"] < best[i - 1]["ae"]:
                    xa = best[i - 1]["ae"] - best[i]["ab"]
                    if xa > 1000:
                        its_a = -1
                        break
                    its_a += xa
                else:
                    gap_a += best[i]["ab"] - best[i - 1]["ae"]
                if best[i]["bb"] < best[i - 1]["be"]:
                    xb = best[i - 1]["be"] - best[i]["bb"]
                    if xb > 1000:
                        its_b = -1
                        break
                    its_b += xb
                else:
                    gap_b += best[i]["bb"] - best[i - 1]["be"]
                bases -= max(xa, xb)
    return bool(pbeg and pend and its_a >= 0 and its_b >= 0 and gap_a >= 0 and gap_b >= 0 and bases * 0.3 > max(gap_a, gap_b))


def group(recs, alen, blen, twidth, rep, kind):
    """recs: dicts of aread, bread, ab, ae, bb, be, flags of one group in file order (not changed).  -> the flags the first
    pass leaves (its file holds the records without OVL_DISCARD, the second file the others), the number of chains, the
    members of the best chain as indices into the group, whether it (or the lone record) was found proper, and (kept,
    discarded) as the first pass counts them"""
    ovls = [dict(r, flags=r["flags"] & ~TEMP, idx=i) for i, r in enumerate(recs)]
    chains = chain(ovls, alen, blen, twidth, rep)
    n = len(ovls)
    if not chains:
        proper = single_proper(ovls[0], alen, blen, kind)
        if proper if kind == 0 else not proper:
            ovls[0]["flags"] |= DISCARD
        counts = (0, 1) if (proper if kind == 0 else not proper) else (1, 0)
    elif kind == 0:
        proper = chain_proper(chains[0], alen, blen, 0)
        for o in ovls:
            o["flags"] = (o["flags"] | DISCARD) if proper else (o["flags"] & ~DISCARD)
        counts = (0, n) if proper else (n, 0)
    else:
        proper = len(chains) == 1 and chain_proper(chains[0], alen, blen, 1)
        if not proper:
            for o in ovls:
                o["flags"] |= DISCARD
        nd = sum(1 for o in ovls if o["flags"] & DISCARD)
        counts = (n - nd, nd)
    return dict(flags=[o["flags"] for o in ovls], nchains=len(chains), best=[o["idx"] for o in chains[0]] if chains else [],
                proper=bool(proper), counts=counts)


def all_flagged(recs):
    """the group the reference aborts on: two or more records that all come with OVL_CONT or OVL_DISCARD"""
    return len(recs) >= 2 and all(r["flags"] & (CONT | DISCARD) for r in recs)
