"""A Python model of LAcorrect's method, written from the reference's text (corrector/LAcorrect.c correct_overlaps and
single_tile_consensus, corrector/consensus.c match, v3_align_onp, consensus_add, consensus_sequence) and sharing no code
with the library: the tile layout of a pile, the consensus of a tile, and what of a tile's consensus the kernel's built
limits have to hold (sequence length, profile columns, wave cells).  Waves are dictionaries, so a cell that was never
written cannot be read without an error.  Slow; the tests run it on the planted piles and on the seeded random tiles."""
import os
import struct

import numpy as np

MIN_TWIDTH, MAX_COVERAGE, MAX_TILES = 20, 20, 40
OVL_COMP, OVL_DISCARD = 0x1, 0x2


# ---- consensus.c ------------------------------------------------------------------------------------------------------

def match_base(col):
    """match(): the base a column stands for (first maximum over A C G T), None where the dashes reach that maximum"""
    nmax, cmax = col[0], 0
    for b in (1, 2, 3):
        if col[b] > nmax:
            nmax, cmax = col[b], b
    return None if col[4] >= nmax else cmax


def align_onp(prof, B, events):
    """v3_align_onp of the profile against B: -> (trace as the reference leaves it with Aabs = A, Babs = B: b + 1 for a
    column alone before B[b], -(c + 1) for a base alone before column c; waves used)"""
    M, N = len(prof), len(B)
    code = [match_base(c) for c in prof]
    events["dash_max_columns"] += sum(c is None and sum(col[:4]) > 0 for c, col in zip(code, prof))

    def match(j, col):
        assert 0 <= j < N and 0 <= col < M, (j, col, M, N)
        return code[col] is not None and code[col] == B[j]

    dl = M - N
    low, hgh = (0, dl) if dl >= 0 else (dl, 0)
    PVF, PHF = {-2: {}, -1: {}}, {}
    for d in range(low - 1, hgh + 2):
        PVF[-2][d] = PVF[-1][d] = -2
    PVF[-1][0] = -1
    F1, F0 = PVF[-2], PVF[-1]
    low += 1
    hgh -= 1
    D = 0
    while True:
        F2, F1 = F1, F0
        F0, HF = PVF.setdefault(D, {}), PHF.setdefault(D, {})
        if D % 2 == 0:
            hgh += 1
            low -= 1
        F0[hgh + 1] = F0[low - 1] = -2

        def fs_move(k, am, ap, mdir, pdir, i):
            ac = F1[k] + 1
            if ac < am:
                if ap < am:
                    HF[k], j = mdir, am
                else:
                    HF[k], j = pdir, ap
            elif ap < ac:
                HF[k], j = 0, ac
            else:
                HF[k], j = pdir, ap
            lim = N if N < i else i
            while j < lim and match(j, k + j):
                j += 1
            F0[k] = j
            return j

        j = -2
        for k in range(hgh, dl, -1):
            j = fs_move(k, F2[k - 1], j + 1, -1, 4, M - k)
        j = -2
        for k in range(low, dl):
            j = fs_move(k, j, F2[k + 1] + 1, 2, 1, M - k)
        fs_move(dl, j, F0[dl + 1] + 1, 2, 4, N)
        if F0[dl] >= N:
            break
        D += 1
        assert D <= min(M, N)
    waves = D

    PHF[0][0] = 3
    c, k = N, dl
    e = PHF[D][k]
    PHF[D][k] = 3
    while e != 3:
        h = k + e
        if e > 1:
            h -= 3
        elif e == 0:
            D -= 1
        else:
            D -= 2
        if h < k:
            m = -k if k < 0 else 0
            if PVF[D][h] <= c:
                c = PVF[D][h] - 1
            while c >= m and match(c, k + c):
                c -= 1
            if e < 1:
                if c <= PVF[D + 2][k + 1]:
                    e, h, D = 4, k + 1, D + 2
                elif c == PVF[D + 1][k]:
                    e, h, D = 0, k, D + 1
                else:
                    PVF[D][h] = c + 1
            else:
                m = D if k == dl else D - 2
                if c <= PVF[m][k + 1]:
                    e, h, D = (4 if k == dl else 1), k + 1, m
                elif c == PVF[D - 1][k]:
                    e, h, D = 0, k, D - 1
                else:
                    PVF[D][h] = c + 1
        m = PHF[D][h]
        PHF[D][h] = e
        e, k = m, h

    trace = []
    k = D = 0
    e = PHF[D][k]
    while e != 3:
        h = k - e
        c = PVF[D][k]
        if e > 1:
            h += 3
        elif e == 0:
            D += 1
        else:
            D += 2
        if h > k:
            trace.append(c + 1)
        elif h < k:
            trace.append(-1 - (c + k))
        k = h
        e = PHF[D][h]
    return trace, waves


def consensus_add(prof, B, added, events):
    """consensus_add for a profile that exists: the new profile, and (waves, |M - N|) of the alignment"""
    trace, waves = align_onp(prof, B, events)
    diffs_a = sum(t < 0 for t in trace)
    M = len(prof)
    new = [list(c) for c in prof] + [[0] * 5 for _ in range(diffs_a)]
    n, p, b = M - 1 + diffs_a, M - 1, len(B) - 1
    for c in reversed(trace):
        if c > 0:
            c -= 1
            while c <= b:
                new[n] = list(new[p])
                new[n][B[b]] += 1
                n, b, p = n - 1, b - 1, p - 1
            new[n] = list(new[p])
            new[n][4] += 1
            n, p = n - 1, p - 1
        else:
            c = -c - 1
            while c <= p:
                new[n] = list(new[p])
                new[n][B[b]] += 1
                n, b, p = n - 1, b - 1, p - 1
            new[n] = [0] * 5
            new[n][B[b]] += 1
            new[n][4] = added
            n, b = n - 1, b - 1
    while b >= 0:
        new[n][B[b]] += 1
        n, b, p = n - 1, b - 1, p - 1
    return new, (waves, abs(M - len(B)))


def wave_cells(waves, absdel):
    """cells of the rows -2 .. `waves` as the kernel packs them: |del| + 3 diagonals in the rows -2 .. 0, two more every
    second row (include/damar_hip.h, kernels/tile_consensus.hip)"""
    return 2 * (absdel + 3) + sum(absdel + 3 + 2 * (d // 2) for d in range(waves + 1))


def consensus(tile, limits=None):
    """One tile, its sequences added in order -> (called bases as uint8, sequences added, facts).  facts: `over`, whether
    the kernel at `limits` = (seg, cols, cells) has to leave the tile to the host routine; the events counted on the way."""
    events = dict(dash_max_columns=0, tied_columns=0, dashes_called=0)
    facts = dict(over=False, cols=0, cells=0, seg=max([len(s) for s in tile], default=0))
    if not tile:
        return np.zeros(0, dtype=np.uint8), 0, dict(facts, **events)
    prof = [[0] * 5 for _ in tile[0]]
    for col, b in zip(prof, tile[0]):
        col[int(b)] = 1
    added = 1
    facts["cols"] = len(prof)
    for s in tile[1:]:
        prof, (waves, absdel) = consensus_add(prof, [int(x) for x in s], added, events)
        added += 1
        facts["cols"] = max(facts["cols"], len(prof))
        facts["cells"] = max(facts["cells"], wave_cells(waves, absdel))
    out = []
    for col in prof:
        nmax = cmax = 0
        for b in range(5):
            if col[b] > nmax:
                nmax, cmax = col[b], b
        events["tied_columns"] += sum(x == nmax for x in col[:4]) > 1 and cmax < 4
        ncov = sum(col[:4])
        if added <= 2:
            if added != ncov:
                cmax = 4
        elif ncov < added * 0.5:
            cmax = 4
        if cmax == 4:
            events["dashes_called"] += 1
            continue
        out.append(cmax)
    if limits is not None:
        facts["over"] = bool(facts["seg"] > limits[0] or facts["cols"] > limits[1] or facts["cells"] > limits[2])
    return np.array(out, dtype=np.uint8), added, dict(facts, **events)


# ---- LAcorrect.c ------------------------------------------------------------------------------------------------------

def db_reads(golden_db):
    """the reads of a fixture database, one base per value"""
    idx = open(os.path.join(golden_db, ".G.idx"), "rb").read()
    n = struct.unpack_from("<i", idx, 0)[0]
    recs = np.frombuffer(idx, dtype="<i8", offset=len(idx) - 32 * n).reshape(n, 4)
    bps = np.frombuffer(open(os.path.join(golden_db, ".G.bps"), "rb").read(), dtype=np.uint8)
    out = []
    for r in range(n):
        rlen, boff = int(recs[r, 0] & 0xffffffff), int(recs[r, 1])
        raw = bps[boff:boff + (rlen + 3) // 4]
        out.append(np.stack([(raw >> 6) & 3, (raw >> 4) & 3, (raw >> 2) & 3, raw & 3], axis=1).reshape(-1)[:rlen].astype(np.uint8))
    return out


def trace_of(batch, r):
    n, tb = int(batch["tlen"][r]), batch["tbytes"]
    raw = batch["trace"][batch["trace_off"][r]:batch["trace_off"][r] + n * tb]
    return [int(x) for x in (raw if tb == 1 else raw.view("<u2"))]


def valid_pt_points(batch, r):
    tr, bbpos, bepos = trace_of(batch, r), int(batch["bbpos"][r]), int(batch["bepos"][r])
    be = bbpos + tr[1]
    for t in range(2, len(tr), 2):
        bb = be
        be = bepos + 1 if t == len(tr) - 1 else be + tr[t + 1]
        if bb > be or bb < bbpos or bb > bepos or be < bbpos or be > bepos + 1:
            return False
    return True


def pile_records(batch, pile, first_of_part):
    """the records of a pile that the reference's thread keeps, in its order (by A length, ties in file order)"""
    lo, hi = int(batch["pile_off"][pile]), int(batch["pile_off"][pile + 1])
    gone = lambda r: bool(batch["flags"][r] & OVL_DISCARD) or batch["tlen"][r] == 0
    recs = list(range(lo, hi))
    if first_of_part:
        while recs and gone(recs[0]):
            recs.pop(0)
    recs = [r for i, r in enumerate(recs) if batch["tlen"][r] != 0 and (i == 0 or not gone(r))]
    return sorted(recs, key=lambda r: -(int(batch["aepos"][r]) - int(batch["abpos"][r])))       # sorted() is stable


def layout(batch, recs, alen, q):
    """correct_overlaps up to its sorts: per tile the entries dict(b, comp, bb, be, qv, apos), the A read's own first"""
    tw = int(batch["tspace"])
    ntiles = (alen + tw - 1) // tw
    count = [0] * (ntiles + 1)
    for r in recs:
        tb = int(batch["abpos"][r]) // tw
        for t in range(tb, tb + int(batch["tlen"][r]) // 2):
            if count[t + 1] < MAX_TILES:
                count[t + 1] += 1
    for i in range(ntiles):
        if count[i + 1] < MAX_TILES:
            count[i + 1] += 1
    tiles = [[] for _ in range(ntiles)]
    room = lambda t: len(tiles[t]) < MAX_TILES
    p = None
    for i in range(ntiles):
        p = dict(b=-1, comp=0, bb=tw * i, be=tw * (i + 1), qv=int(q[i]), apos=0)
        tiles[i].append(p)
    p["be"] = alen
    for r in recs:
        tr = trace_of(batch, r)
        abpos, aepos = int(batch["abpos"][r]), int(batch["aepos"][r])
        b, comp = int(batch["bread"][r]), int(batch["flags"][r]) & OVL_COMP
        tile = abpos // tw
        be = int(batch["bbpos"][r]) + tr[1]
        if room(tile):
            p = dict(b=b, comp=comp, bb=int(batch["bbpos"][r]), be=be, qv=tr[0], apos=abpos if abpos % tw else 0)
            tiles[tile].append(p)
        for t in range(2, len(tr), 2):
            tile += 1
            bb, be = be, be + tr[t + 1]
            if room(tile):
                p = dict(b=b, comp=comp, bb=bb, be=be, qv=tr[t], apos=0)
                tiles[tile].append(p)
            else:
                p = -1
        if p != -1 and aepos < alen and aepos % tw:
            p["apos"] = -aepos
    assert [len(t) for t in tiles] == count[1:]
    return [t[:1] + sorted(t[1:], key=lambda x: x["qv"]) for t in tiles]


def taken(entries):
    """single_tile_consensus: the entries whose sequences are added"""
    out = []
    for x in entries:
        if x["apos"] == 0 and x["be"] - x["bb"] >= MIN_TWIDTH:
            out.append(x)
            if len(out) >= MAX_COVERAGE:
                break
    return out


def sequences(entries, aread, reads):
    out = []
    for x in entries:
        rd = reads[aread if x["b"] < 0 else x["b"]]
        rd = (3 - rd[::-1]) if x["comp"] else rd
        out.append(np.ascontiguousarray(rd[x["bb"]:x["be"]]))
    return out


def piles(batch, reads, q_anno, q_data):
    """every pile of a file under -j 1 without -r -> list of dict(aread, bad (the index of a record with bad trace points,
    or None), tiles (the sequences each tile's consensus takes), entries (the layout))"""
    out, first = [], True
    for pile in range(len(batch["pile_aread"])):
        a = int(batch["pile_aread"][pile])
        recs = pile_records(batch, pile, first)
        if not recs:
            continue
        first = False
        bad = next((i for i, r in enumerate(recs) if not valid_pt_points(batch, r)), None)
        if bad is not None:
            out.append(dict(aread=a, bad=bad, bad_bread=int(batch["bread"][recs[bad]]), tiles=[], entries=[]))
            continue
        q0 = int(q_anno[a]) // 4
        ent = layout(batch, recs, len(reads[a]), q_data[q0:])
        out.append(dict(aread=a, bad=None, entries=ent, tiles=[sequences(taken(t), a, reads) for t in ent]))
    return out
