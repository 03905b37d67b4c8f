"""A literal model of scrub/TKhomogenize.c in Python: the walk over a record's trace as the C is written, with np.float32 and
np.float64 where the C has float and double, a bit array per read set by a line-for-line ba_assign_range, and the read-out
of post_homogenize.  Slow on purpose; tests/hom_shapes.py feeds it small batches, the generator pins it to the reference."""
import numpy as np

MIN_INT_LEN = 500


def assign_range(arr, beg, end):
    """lib.ext/bitarr.c ba_assign_range(arr, beg, end, 1): byte steps and all"""
    assert 0 <= beg < len(arr) and 0 <= end < len(arr), (beg, end, len(arr))
    while True:
        arr[beg] = True
        beg += 1
        if not (beg % 8 and beg <= end):
            break
    while (end + 1) % 8 and end >= beg:
        arr[end] = True
        end -= 1
    while beg < end:
        arr[beg:beg + 8] = True
        beg += 8


def trace_b(batch, i, seg):
    tb = batch["tbytes"]
    at = int(batch["trace_off"][i]) + tb * (2 * seg + 1)
    t = batch["trace"]
    return int(t[at]) if tb == 1 else int(t[at]) | (int(t[at + 1]) << 8)


def new_masks(read_len, res):
    return [np.zeros((int(n) + res - 1) // res + 1 if res > 1 else int(n) + 1, dtype=bool) for n in read_len]


def seed(masks, rep_anno, rep_data, res):
    """pre_homogenize's copy (-m) -> ranges set"""
    n = 0
    for a in range(len(masks)):
        for k in range(int(rep_anno[a]) // 4, int(rep_anno[a + 1]) // 4, 2):
            beg, end = int(rep_data[k]), int(rep_data[k + 1])
            if end - beg < MIN_INT_LEN:
                continue
            assign_range(masks[a], (beg + res - 1) // res, end // res)
            n += 1
    return n


def project(tw, bl, adiff):
    """(int) (adiff / curSegLenRatio) with float curSegLenRatio = 1.0 * twidth / trace[j + 1]"""
    with np.errstate(divide="ignore"):
        ratio = np.float32(np.float64(1.0) * np.float64(tw) / np.float64(bl))
        return int(np.float32(adiff) / ratio)


def add(masks, batch, read_len, rep_anno, rep_data, res=1, ends=-1, pairs=None, seen=None):
    """handler_homogenize over one batch -> ranges set; seen (a dict) counts what the walk met"""
    tw, n = int(batch["tspace"]), 0
    seen = {} if seen is None else seen
    hit = lambda k: seen.__setitem__(k, seen.get(k, 0) + 1)
    for p in range(len(batch["pile_aread"])):
        a = int(batch["pile_aread"][p])
        for i in range(int(batch["pile_off"][p]), int(batch["pile_off"][p + 1])):
            b = int(batch["bread"][i])
            if a == b:
                hit("identity")
                continue
            blen = int(read_len[b])
            trim_b, trim_e = (int(pairs[b][0]), int(pairs[b][1])) if pairs is not None else (0, blen)
            ab, ae, bepos = int(batch["abpos"][i]), int(batch["aepos"][i]), int(batch["bepos"][i])
            tlen = int(batch["tlen"][i])
            ob, oe = int(rep_anno[a]) // 4, int(rep_anno[a + 1]) // 4
            while ob < oe:
                beg, end = int(rep_data[ob]), int(rep_data[ob + 1])
                ob += 2
                if end - beg < MIN_INT_LEN:
                    hit("short")
                    continue
                if beg > ae:
                    hit("stop_before_more" if ob < oe else "stop")
                    break
                iab, iae = max(beg, ab), min(end, ae)
                if iab >= iae:
                    hit("touching" if iab == iae else "apart")
                    continue
                ibb = ibe = -1
                aoff, boff = ab, int(batch["bbpos"][i])
                jb = je = -1
                for j in range(0, tlen, 2):
                    bl = trace_b(batch, i, j // 2)
                    if ibb == -1:
                        if aoff + tw >= iab:
                            ibb = min(boff + project(tw, bl, iab - aoff), bepos)
                            jb = j // 2
                            if bl == 0:
                                hit("zero_under_iab")
                            if aoff + tw == iab:
                                hit("iab_on_segment_end")
                            if j == 0 and ab % tw and iab - ab < tw - ab % tw:
                                hit("iab_in_partial_first")
                        elif j == tlen - 2:
                            ibb = min(boff, bepos)
                    if aoff + tw >= iae and ibe == -1:
                        if ibb == -1:
                            ibb = min(boff, bepos)
                        ibe = min(boff + project(tw, bl, iae - aoff), bepos)
                        je = j // 2
                        if bl == 0:
                            hit("zero_under_iae")
                        break
                    aoff = ((aoff + tw) // tw) * tw
                    boff += bl
                if ibb == -1 or ibe == -1:
                    hit("no_trace" if tlen == 0 else "short_trace")
                    continue
                if jb == je:
                    hit("same_segment")
                if iab > beg:
                    hit("clipped_at_abpos")
                if iae < end:
                    hit("clipped_at_aepos")
                if int(batch["flags"][i]) & 1:
                    ibb, ibe = blen - ibe, blen - ibb
                    hit("comp")
                if int(batch["flags"][i]) & 2:
                    hit("discarded_marks")
                assert ibb <= ibe
                if ends != -1:
                    left, right = ibb < ends + trim_b, ibe > trim_e - ends
                    hit("e_" + ("both" if left and right else "left" if left else "right" if right else "neither"))
                    if left:
                        assign_range(masks[b], (ibb + res - 1) // res, min(ends + trim_b, ibe) // res)
                        n += 1
                    if right:
                        assign_range(masks[b], (max(trim_e - ends, ibb) + res - 1) // res, ibe // res)
                        n += 1
                else:
                    bb, be = (ibb + res - 1) // res, ibe // res
                    if bb > be:
                        hit("single_bit")
                    if be == len(masks[b]) - 1:
                        hit("spare_bit")
                    assign_range(masks[b], bb, be)
                    n += 1
    return n


def read_out(masks, read_len, res, seen=None):
    """post_homogenize -> (anno uint64 byte offsets, data int32, tagged)"""
    seen = {} if seen is None else seen
    hit = lambda k: seen.__setitem__(k, seen.get(k, 0) + 1)
    counts, data = [], []
    for r, m in enumerate(masks):
        rlen, alen = int(read_len[r]), len(m) - 1
        beg, c = -1, 0
        for j in range(alen):
            if m[j] and beg == -1:
                beg = j
            elif not m[j] and beg != -1:
                end = j - 1
                if end * res > rlen:
                    hit("min_bites")
                if end == alen - 2:
                    hit("ends_before_last")
                data += [beg * res, min(end * res, rlen)]
                c += 1
                beg = -1
        if beg != -1:
            hit("reaches_last")
            data += [beg * res, rlen - 1]
            c += 1
        counts.append(8 * c)
    anno = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    data = np.array(data, dtype=np.int32)
    return anno, data, int(np.sum(data[1::2].astype(np.int64) - data[0::2]))


def trim_pairs(trim_anno, trim_data, nreads):
    """get_trim of every read"""
    out = np.zeros((nreads, 2), dtype=np.int32)
    for r in range(nreads):
        ob, oe = int(trim_anno[r]) // 4, int(trim_anno[r + 1]) // 4
        assert oe == ob or oe - ob == 2
        if oe != ob and trim_data[ob] < trim_data[ob + 1]:
            out[r] = trim_data[ob], trim_data[ob + 1]
    return out


def homogenize(batches, read_len, rep_anno, rep_data, merge=False, ends=-1, trim=None, res=1, seen=None):
    """-> (anno, data, tagged, ranges set)"""
    masks = new_masks(read_len, res)
    pairs = trim_pairs(trim[0], trim[1], len(read_len)) if ends != -1 else None
    n = seed(masks, rep_anno, rep_data, res) if merge else 0
    for b in batches:
        n += add(masks, b, read_len, rep_anno, rep_data, res, ends, pairs, seen)
    return read_out(masks, read_len, res, seen) + (n,)
