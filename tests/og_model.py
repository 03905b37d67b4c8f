"""A model of OGbuild's two passes (touring/OGbuild.c), written from the reference's text and as literally as Python allows:
the counting pass with its list of symmetric discards, the building pass with the loop over that sorted list, slots that
stay zero where the building pass fills fewer than the counting pass allotted, the stable sort, remove_dupes,
remove_lr_dupes one pair at a time, and the compaction.  It shares nothing with host/graph.c or kernels/graph_edges.hip:
no closed form of the discard loop, no formula for the double count.

    build(cols, rl, trim) -> dict of loff, roff, left, right, status and the counters, as api.og_edges returns them
cols: the ten words of every record in file order (tlen diffs abpos bbpos aepos bepos flags aread bread -), trim: get_trim
of every read as pairs."""
import numpy as np

COMP, DISCARD, SYMDISCARD = 0x1, 0x2, 0x100
CONTAINED, WIDOW, PROPER = 1, 2, 4


def piles_of(cols):
    """the runs of one A read, as lists of mutable records"""
    out, cur = [], []
    for row in cols:
        r = dict(diffs=int(row[1]), ab=int(row[2]), bb=int(row[3]), ae=int(row[4]), be=int(row[5]), flags=int(row[6]), a=int(row[7]), b=int(row[8]))
        if cur and cur[-1]["a"] != r["a"]:
            out.append(cur)
            cur = []
        cur.append(r)
    if cur:
        out.append(cur)
    return out


def drop_parallel_edges(ovls):
    i, n = 0, len(ovls)
    while i < n - 1:
        if ovls[i]["flags"] & DISCARD:
            i += 1
            continue
        j = i + 1
        if ovls[i]["b"] == ovls[j]["b"]:
            dropped = 0
            while j < n and ovls[i]["b"] == ovls[j]["b"]:
                if not ovls[j]["flags"] & DISCARD:
                    ovls[j]["flags"] |= DISCARD
                    dropped += 1
                j += 1
            if dropped > 0:
                ovls[i]["flags"] |= DISCARD
        i = j


def b_trim(o, rl, trim):
    tbb, tbe = trim[2 * o["b"]], trim[2 * o["b"] + 1]
    if o["flags"] & COMP:
        blen = rl[o["b"]]
        tbb, tbe = blen - tbe, blen - tbb
    return int(tbb), int(tbe)


def edge(o, ovh):
    return [o["a"], o["b"], o["ab"], o["ae"], o["bb"], o["be"], o["flags"], ovh, o["diffs"] & 0xffff]


def edge_reversed(o, alen, blen, ovh):
    if o["flags"] & COMP:
        return [o["b"], o["a"], blen - o["be"], blen - o["bb"], alen - o["ae"], alen - o["ab"], o["flags"], ovh, o["diffs"] & 0xffff]
    return [o["b"], o["a"], o["bb"], o["be"], o["ab"], o["ae"], o["flags"], ovh, o["diffs"] & 0xffff]


def build(cols, rl, trim):
    n = len(rl)
    rl = [int(x) for x in rl]
    trim = [int(x) for x in trim]
    # ---- pass 1: handler_count
    nleft, nright, discard, neg_rec, rec0 = [0] * n, [0] * n, [], -1, 0
    for ovls in piles_of(cols):
        a = ovls[0]["a"]
        tab, tae = trim[2 * a], trim[2 * a + 1]
        drop_parallel_edges(ovls)
        for k, o in enumerate(ovls):
            if o["a"] == o["b"]:
                continue
            if o["flags"] & SYMDISCARD:
                discard.append((o["b"], o["a"]))
            if o["flags"] & DISCARD:
                continue
            if o["ab"] == tab and o["ae"] == tae:
                continue
            tbb, tbe = b_trim(o, rl, trim)
            if o["bb"] == tbb and o["be"] == tbe:
                continue
            if o["ab"] == tab:
                ovh = o["bb"] - tbb
                if ovh < 0:
                    neg_rec = rec0 + k if neg_rec < 0 else neg_rec
                elif ovh > 0:
                    nleft[a] += 1
                    if o["ae"] < tae:
                        (nleft if o["flags"] & COMP else nright)[o["b"]] += 1
            if o["ae"] == tae:
                ovh = tbe - o["be"]
                if ovh < 0:
                    neg_rec = rec0 + k if neg_rec < 0 else neg_rec
                elif ovh > 0:
                    nright[a] += 1
                    if o["ab"] > tab:
                        (nright if o["flags"] & COMP else nleft)[o["b"]] += 1
        rec0 += len(ovls)
    # ---- post_count
    discard.sort()
    rflags = [-1] * n
    for i, (first, _) in enumerate(discard):
        rflags[first] = 2 * i
    left = [[[0] * 9 for _ in range(c)] for c in nleft]
    right = [[[0] * 9 for _ in range(c)] for c in nright]
    curleft, curright = [0] * n, [0] * n
    status = [WIDOW] * n
    edges = redges = symdiscard = 0

    def put(lst, cur, r, e):
        lst[r][cur[r]] = e
        cur[r] += 1

    # ---- pass 2: handler_build
    for ovls in piles_of(cols):
        a = ovls[0]["a"]
        alen = rl[a]
        tab, tae = trim[2 * a], trim[2 * a + 1]
        drop_parallel_edges(ovls)
        mine = 0
        for o in ovls:
            if o["a"] == o["b"]:
                continue
            if o["ab"] == tab and o["ae"] == tae:
                status[a] = CONTAINED
                continue
            b, blen = o["b"], rl[o["b"]]
            tbb, tbe = b_trim(o, rl, trim)
            if o["bb"] == tbb and o["be"] == tbe:
                status[b] = CONTAINED
                continue
            if o["flags"] & (DISCARD | SYMDISCARD):
                continue
            if rflags[a] != -1:
                hit = False
                for a_disc, b_disc in discard:
                    if a_disc > a:
                        break
                    if b == b_disc:
                        hit = True
                        break
                if hit:
                    symdiscard += 1
                    continue
            if o["ab"] == tab:
                ovh = o["bb"] - tbb
                if ovh > 0:
                    put(left, curleft, a, edge(o, ovh))
                    edges += 1
                    mine += 1
                    if o["ae"] < tae:
                        if o["flags"] & COMP:
                            put(left, curleft, b, edge_reversed(o, alen, blen, tae - o["ae"]))
                        else:
                            put(right, curright, b, edge_reversed(o, alen, blen, tae - o["ae"]))
                        if status[b] == WIDOW:
                            status[b] = PROPER
                        redges += 1
            if o["ae"] == tae:
                ovh = tbe - o["be"]
                if ovh > 0:
                    put(right, curright, a, edge(o, ovh))
                    edges += 1
                    mine += 1
                    if o["ab"] > tab:
                        if o["flags"] & COMP:
                            put(right, curright, b, edge_reversed(o, alen, blen, o["ab"] - tab))
                        else:
                            put(left, curleft, b, edge_reversed(o, alen, blen, o["ab"] - tab))
                        if status[b] == WIDOW:
                            status[b] = PROPER
                        redges += 1
        if status[a] == WIDOW and mine > 0:
            status[a] = PROPER
    # ---- post_build up to the first compress_graph
    parallel = 0

    def remove_dupes(es):
        dropped = 0
        prev = None
        for cur in es:
            if prev is not None and cur[1] == prev[1]:
                prev[0] = prev[1] = -1
                dropped += 1
            prev = cur
        return dropped

    for r in range(n):
        left[r].sort(key=lambda e: (e[0], e[1]))            # list.sort is stable, as the merge sort behind qsort
        right[r].sort(key=lambda e: (e[0], e[1]))
    for r in range(n):
        if left[r]:
            parallel += remove_dupes(left[r])
        if right[r]:
            parallel += remove_dupes(right[r])
        for le in left[r]:
            for re in right[r]:
                if le[1] == re[1]:
                    re[0] = re[1] = -1
                    parallel += 1
    cnt_left, cnt_right = sum(nleft), sum(nright)
    keep = lambda es: [e for e in es if e[0] != -1 and e[1] != -1]
    left, right = [keep(es) for es in left], [keep(es) for es in right]
    out = dict(status=np.array(status, dtype=np.uint8), cnt_left=cnt_left, cnt_right=cnt_right, edges=edges, redges=redges,
               symdiscard=symdiscard, parallel=parallel, neg_rec=neg_rec)
    for name, lists in (("l", left), ("r", right)):
        out[name + "off"] = np.concatenate([[0], np.cumsum([len(es) for es in lists])]).astype(np.int64)
        flat = [e for es in lists for e in es]
        out["left" if name == "l" else "right"] = np.array(flat, dtype=np.int32).reshape(len(flat), 9)
    out["removed"] = cnt_left + cnt_right - len(out["left"]) - len(out["right"])
    return out
