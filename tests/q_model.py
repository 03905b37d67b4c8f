"""A plain numpy statement of LAq's rules (scrub/LAq.c), the model the fixtures of tests/golden/q/ and the kernels of
kernels/pile_quality.hip are held against.  A batch is the dict of tests/q_common.read_las: the columns of the trace-less
batches plus `trace` (the records' raw trace bytes back to back), `trace_off` (a byte offset per record), `tlen`, `tbytes`
and `tspace`."""
import numpy as np

TRIM_WINDOW = 5


def trace_values(b, i):
    """the trace values of record i as ints: diffs at even, B lengths at odd positions"""
    dt = np.uint8 if b["tbytes"] == 1 else np.dtype("<u2")
    at = int(b["trace_off"][i])
    return np.frombuffer(b["trace"], dtype=dt, count=int(b["tlen"][i]), offset=at).astype(np.int64)


def q_round(s, count):
    """(int)((float)s / count + 0.5) of the reference, in integers"""
    return (2 * s + count) // (2 * count)


def segments(b, read_len, spill=True):
    """-> (tile0 int64[npiles + 1], list of (global tile, value)) after the three inclusion rules and the spill rule"""
    tw = int(b["tspace"])
    np_ = len(b["pile_aread"])
    ntiles = np.array([(int(read_len[a]) + tw - 1) // tw for a in b["pile_aread"]], dtype=np.int64)
    tile0 = np.concatenate([[0], np.cumsum(ntiles)]).astype(np.int64)
    out = []
    for p in range(np_):
        a = int(b["pile_aread"][p])
        alen = int(read_len[a])
        for i in range(int(b["pile_off"][p]), int(b["pile_off"][p + 1])):
            if int(b["bread"][i]) == a:
                continue
            ab, ae, tlen = int(b["abpos"][i]), int(b["aepos"][i]), int(b["tlen"][i])
            v = trace_values(b, i)[0::2]
            nseg = tlen // 2
            for s in range(nseg):
                if s == 0:
                    if ab % tw != 0:
                        continue
                elif s == nseg - 1:
                    if not (ae % tw == 0 or ae == alen):
                        continue
                tile, q = ab // tw + s, int(v[s])
                if spill:
                    tile, q = tile + q // tw, q % tw
                elif q >= tw:
                    continue
                if tile < ntiles[p]:
                    out.append((int(tile0[p]) + tile, q))
    return tile0, out


def tile_q(b, read_len, segmin=1, segmax=20, ccs=False, spill=True):
    """-> (q int32 per tile of the batch, tile0 int64[npiles + 1], depth int64 per tile, segments counted)"""
    tile0, segs = segments(b, read_len, spill)
    nt = int(tile0[-1])
    runs = [[] for _ in range(nt)]
    for t, q in segs:
        runs[t].append(q)
    out = np.zeros(nt, dtype=np.int32)
    depth = np.zeros(nt, dtype=np.int64)
    for t in range(nt):
        r = sorted(runs[t])[:segmax]
        depth[t] = len(runs[t])
        count, s = len(r), sum(r)
        if count < segmin:
            out[t] = 25 if ccs else 0
        else:
            out[t] = q_round(s if s else count, count)
    return out, tile0, depth, len(segs)


class PastEnd(Exception):
    """the walk read the value after the last one of the q data: undefined in the reference"""


def trim_from_q(dataq, ob, oe, rlen, tw, tb, te, trim_q=25, min_len=1000, ccs=False, strict=False):
    """trim_q_offsets: dataq is the q data of ALL reads (the walk looks beyond its own read's values), [ob, oe) this
    read's part of it, (tb, te) the interval to start from (0: the read's end).  -> (tb, te), or None without q data.
    A value past the end of dataq counts as 0; strict: raise PastEnd there."""
    if ob >= oe:
        return None
    base = ob
    nt = (rlen + tw - 1) // tw
    left = tb // tw if tb else 0
    right = te // tw if te else nt
    ob += left
    oe -= nt - right

    def at(k):
        if 0 <= k < len(dataq):
            return int(dataq[k])
        if strict:
            raise PastEnd()
        return 0

    def bad(q):
        return q >= trim_q or (not ccs and q == 0)

    def div(s):
        return -((-s) // TRIM_WINDOW) if s < 0 else s // TRIM_WINDOW

    s, w = 0, ob
    while w - ob <= TRIM_WINDOW and ob < oe:
        q = at(w)
        if bad(q):
            ob, s = w + 1, 0
        else:
            if w - ob == TRIM_WINDOW and div(s) >= trim_q:
                s -= at(ob)
                ob += 1
            s += q
        w += 1
    s, w = 0, oe
    while oe - w <= TRIM_WINDOW and ob < oe:
        q = at(w - 1)
        if bad(q):
            oe, s = w - 1, 0
        else:
            if oe - w == TRIM_WINDOW and div(s) >= trim_q:
                s -= at(oe)
                oe -= 1
            s += q
        w -= 1
    tb = min(rlen, (ob - base) * tw)
    te = min(rlen, (oe - base) * tw)
    if te - tb < min_len:
        tb = te = 0
    return tb, te


def counts_to_anno(counts):
    return np.concatenate([[0], np.cumsum(np.asarray(counts, dtype=np.uint64))]).astype(np.uint64)


def q_track(b, read_len, segmin=1, segmax=20, trim_q=25, min_len=1000, ccs=False, spill=True, strict=False):
    """the annotate pass over one batch holding the whole file -> (q_anno, q_data, trim_anno, trim_data)"""
    tw = int(b["tspace"])
    nreads = len(read_len)
    q, tile0, _, _ = tile_q(b, read_len, segmin, segmax, ccs, spill)
    qc = np.zeros(nreads + 1, dtype=np.uint64)
    for p, a in enumerate(b["pile_aread"]):
        qc[int(a)] += 4 * int(tile0[p + 1] - tile0[p])
    q_anno = counts_to_anno(qc[:nreads])
    tc = np.zeros(nreads, dtype=np.uint64)
    td = []
    for a in range(nreads):
        r = trim_from_q(q, int(q_anno[a]) // 4, int(q_anno[a + 1]) // 4, int(read_len[a]), tw, 0, 0, trim_q, min_len, ccs, strict)
        if r is not None:
            td += list(r)
            tc[a] = 8
    return q_anno, q, counts_to_anno(tc), np.array(td, dtype=np.int32)


def trim_update(b, read_len, q_anno, q_data, trim_anno, trim_data, trim_q=25, min_len=1000, ccs=False, strict=False):
    """the -u pass -> (trim_anno, trim_data, piles tightened, piles emptied)"""
    tw = int(b["tspace"])
    nreads = len(read_len)
    tc = np.zeros(nreads, dtype=np.uint64)
    td, tightened, emptied = [], 0, 0
    for p, a in enumerate(b["pile_aread"]):
        a = int(a)
        lo, hi = int(b["pile_off"][p]), int(b["pile_off"][p + 1])
        keep = [(int(b["abpos"][i]), int(b["aepos"][i])) for i in range(lo, hi)
                if not (int(b["flags"][i]) & 2) and int(b["bread"][i]) != a]
        ab_min = min([k[0] for k in keep], default=None)
        ae_max = max([k[1] for k in keep], default=0)
        at = int(trim_anno[a]) // 4
        assert int(trim_anno[a + 1]) // 4 == at + 2, "read %d has a pile and no trim entry" % a
        tb, te = int(trim_data[at]), int(trim_data[at + 1])
        if ab_min is None:
            if (tb, te) != (0, 0):
                emptied += 1
            tb = te = 0                             # tb < INT_MAX always holds
        elif tb < ab_min or te > ae_max:
            r = trim_from_q(q_data, int(q_anno[a]) // 4, int(q_anno[a + 1]) // 4, int(read_len[a]), tw, ab_min + tw - 1, ae_max,
                            trim_q, min_len, ccs, strict)
            new = r if r is not None else (0, 0)
            if new != (tb, te):
                tightened += 1
            tb, te = new
        td += [tb, te]
        tc[a] += 8
    return counts_to_anno(tc), np.array(td, dtype=np.int32), tightened, emptied
