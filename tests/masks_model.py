"""The two sweeps of the mask tools restated in plain Python, one pile and one event at a time: slow and obvious.  The
expected value of the random tests (tests/test_gpu_masks.py) and checked against the reference-written fixtures
(tests/test_masks_host.py)."""
import numpy as np

DISCARD, DB_BEST = 2, 0x0800


def _piles(p):
    off = p["pile_off"]
    for i in range(len(off) - 1):
        yield i, int(p["pile_aread"][i]), range(int(off[i]), int(off[i + 1]))


def repeats(p, read_len, cov, xcov_enter=2.0, xcov_leave=1.7, merge_dist=-1, min_aln_len=0, inc_identity=0, inccov=0,
            edges=True, first_k=True, **_):
    """-> (count per pile, data, merged, repeat_bases).  edges=False leaves out the extension of regions to a read's ends;
    first_k=False counts its support over all records of the pile, not over the first k, k the number kept, as the
    reference does: both only for the fixture generator, which counts what the fixtures exercise."""
    enter, leave = int(cov * xcov_enter), int(cov * xcov_leave)
    width = 3 if inccov else 2
    counts, data, merged, rbases = [], [], 0, 0
    for _i, a, rng in _piles(p):
        base = len(data)
        ev = []
        for r in rng:
            if p["flags"][r] & DISCARD or (not inc_identity and p["bread"][r] == a) or p["aepos"][r] - p["abpos"][r] < min_aln_len:
                continue
            ev += [int(p["abpos"][r]), -(int(p["aepos"][r]) - 1)]
        k = len(ev) // 2
        ev.sort(key=lambda e: (abs(e), e))
        span = peak = 0
        inside = False
        for e in ev:
            if e < 0:
                span -= 1
            else:
                span += 1
                peak = max(peak, span)
            if inside:
                if span < leave:
                    data.append(-e)
                    rbases += data[-1] - data[-2]
                    if inccov:
                        data.append(peak)
                    inside = False
            elif span > enter:
                if len(data) - base >= width and e - data[len(data) - (width - 1)] < merge_dist:
                    peak = data[-1] if inccov else 0
                    del data[len(data) - (width - 1):]
                    merged += 1
                else:
                    peak = 0
                    data.append(e)
                inside = True
        alen = int(read_len[a])
        first = list(rng)[:k] if first_k else list(rng)
        for j in range(base, len(data) - (1 if inside else 0) if edges else base, width):
            rb, re = data[j], data[j + 1]
            if 0 < rb < 1000 and re < alen - 1000:
                if sum(1 for r in first if re - 200 < p["aepos"][r] < re + 200 and p["abpos"][r] == 0) > 2:
                    data[j] = 0
            if re < alen - 1 and re > alen - 1000 and rb > 1000:
                if sum(1 for r in first if rb - 200 < p["abpos"][r] < rb + 200 and p["aepos"][r] == alen) > 2:
                    data[j + 1] = alen
        counts.append(len(data) - base)
    return np.array(counts, dtype=np.int32), np.array(data, dtype=np.int32), merged, rbases


def coverage(p, read_len, read_flags, max_cov=100, min_aln_len=0, **_):
    """-> (histogram, bases, inactive)"""
    histo, bases, inactive = np.zeros(max_cov, dtype=np.int64), 0, 0
    for _i, a, rng in _piles(p):
        alen = int(read_len[a])
        act = np.zeros(alen + 1, dtype=np.int8)
        total = 0
        for r in rng:
            b = int(p["bread"][r])
            if not (read_flags[b] & DB_BEST) or p["flags"][r] & DISCARD or b == a or p["aepos"][r] - p["abpos"][r] < min_aln_len:
                continue
            total += int(p["aepos"][r] - p["abpos"][r])
            act[p["abpos"][r]:p["aepos"][r]] = 1
        active = int(act[:alen].sum())
        cov = total // active if active > 0 else 0
        if cov < max_cov:
            histo[cov] += 1
        bases += alen
        inactive += alen - active
    return histo, bases, inactive


def tandem(p, min_len=0):
    """-> (count per pile, data)"""
    counts, data = [], []
    for _i, _a, rng in _piles(p):
        base = len(data)
        sel = [r for r in rng if p["abpos"][r] - p["bepos"][r] <= 20 and p["aepos"][r] - p["bbpos"][r] > min_len]
        add = sorted(int(p["bbpos"][r]) for r in sel)
        dele = sorted(int(p["aepos"][r]) for r in sel)
        i = j = x = 0
        while j < len(dele):
            if i < len(add) and add[i] <= dele[j]:
                if x == 0:
                    data.append(add[i])
                x += 1
                i += 1
            else:
                x -= 1
                if x == 0:
                    data.append(dele[j])
                j += 1
        counts.append(len(data) - base)
    return np.array(counts, dtype=np.int32), np.array(data, dtype=np.int32)
