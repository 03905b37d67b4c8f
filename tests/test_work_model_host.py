"""tests/work_model.py -- the model the work-list kernels are held against in test_gpu_work_list.py -- pinned to the reference
on the CPU: over the oracle's sorted seeds of golden comparisons, with the options each fixture was made with, every read
pair that has a record in the reference's .las is in the model's list, and the list is a proper, non-empty part of the run
heads; and the literal two-neighbour rule of filter.c:2289 equals its brute-force statement on random short runs."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

from conftest import read_case, opts_to_plan_kwargs

import work_model as M


def las_pairs(path, comp):
    """(aread, bread) of the records of one orientation (bit 0 of the flags: the B read is complemented)"""
    buf = open(path, "rb").read()
    novl, tspace = struct.unpack_from("<qi", buf, 0)
    tb = 1 if tspace <= 125 else 2
    at, out = 12, set()
    for _ in range(novl):
        tlen, _, _, _, _, _, flags, aread, bread = struct.unpack_from("<9i", buf, at)
        if (flags & 1) == comp:
            out.add((aread, bread))
        at += 40 + tb * tlen
    assert at == len(buf)
    return out


# (fixture, A block, B block, comp)
COMPARISONS = [("tiny2", "2", "1", 0), ("tiny2", "2", "1", 1), ("tandem", "1", "1", 0), ("tandem", "1", "1", 1),
               ("tiny_k12", "1", "1", 0), ("tiny_k12", "1", "1", 1)]


@pytest.mark.parametrize("name,a,b,comp", COMPARISONS, ids=["%s-%s.%s-%s" % (c[0], c[1], c[2], "NC"[c[3]]) for c in COMPARISONS])
def test_model_list_holds_every_pair_of_the_reference_las(built, name, a, b, comp):
    import oracle_api as O
    case = read_case(name)
    kw = opts_to_plan_kwargs(case["opts"])
    k, w, h, j = kw.get("k", 14), kw.get("w", 6), kw.get("h", 35), kw.get("j", 4)
    nshift = j.bit_length() - 1
    assert 1 << nshift == j
    an, bn = os.path.join(case["dbdir"], "G." + a), os.path.join(case["dbdir"], "G." + b)
    self_ = int(a == b)
    oadb, obdb = O.read_block(an), O.read_block(bn)
    if comp:
        O.lib().damar_complement_block(C.byref(obdb), 1)
    prm = O.params(k=k, w=w, h=h, j=j)
    pa, na, _ = O.sort_kmers(oadb, prm)
    pb, nb = (pa, na) if (self_ and not comp) else O.sort_kmers(obdb, prm)[:2]
    s = O.seed_pairs(oadb, obdb, pa, na, pb, nb, self_, comp, prm)
    assert len(s) > 0
    # the oracle's list is in the order the model takes: by (bread, aread, apos), the thread slices over it
    key = (s["bread"].astype(np.int64) << 40) | (s["aread"].astype(np.int64) << 20) | s["apos"]
    assert (np.diff(key) >= 0).all()
    m = M.work_list(s["bread"], s["aread"], s["apos"], s["diag"], k, h, w, nshift)
    kept = set(zip(s["aread"][m["may"]].tolist(), s["bread"][m["may"]].tolist()))
    assert set(m["must"]) <= set(m["may"]) <= set(m["heads"])
    print(name, a, b, "NC"[comp], "seeds", len(s), "heads", len(m["heads"]), "kept", len(m["may"]), "of them fire", len(m["must"]))
    assert 0 < len(m["may"]) < len(m["heads"])
    # the records of the .las carry read numbers of the whole database: ufirst of each block is added
    rec = las_pairs(os.path.join(case["lasdir"], [f for f in case["las"] if f.endswith("G.%s.G.%s.las" % (a, b))][0]), comp)
    assert len(rec) > 0
    missing = []
    for ra, rb in sorted(rec):
        la, lb = ra - oadb.ufirst, rb - obdb.ufirst
        # a comparison of a block with itself holds each pair of reads once: its B-side record is written from the same run
        if (la, lb) not in kept and not (self_ and (lb, la) in kept):
            missing.append((ra, rb))
    assert missing == []


@pytest.mark.parametrize("kmer,hitmin,binshift", [(14, 35, 6), (12, 35, 5), (14, 15, 6), (32, 35, 6), (14, 40, 2)])
def test_two_neighbour_rule_equals_any_two_adjacent_buckets(kmer, hitmin, binshift):
    """filter.c:2289 tests score[d] + score[d + 1] and score[d] + score[d - 1] for the bucket of every seed; that is "some two
    adjacent buckets reach hitmin together" (an empty neighbour counts 0).  1500 random runs of 1 .. 12 seeds per parameter
    set, on a few buckets on both sides of diagonal 0 and with repeated A positions; both answers must occur."""
    rng = np.random.default_rng(kmer * 1000 + hitmin)
    seen = [0, 0]
    for _ in range(1500):
        n = int(rng.integers(1, 13))
        step = rng.integers(0, kmer + 4, n)
        step[0] += kmer - 1
        apos = np.cumsum(step)
        diag = rng.integers(-3 << binshift, 3 << binshift, n)
        f = M.run_fires(apos, diag, kmer, hitmin, binshift)
        assert f == M.run_fires_brute(apos, diag, kmer, hitmin, binshift), (apos.tolist(), diag.tolist())
        seen[int(f)] += 1
    assert min(seen) > 50, seen


def test_pack_and_unpack_are_inverse():
    rng = np.random.default_rng(5)
    n = 1000
    bread, aread = rng.integers(0, 1 << 12, n), rng.integers(0, 1 << 10, n)
    apos = rng.integers(0, 1 << 16, n)
    bpos = rng.integers(0, 1 << 17, n)
    for dbits in (17, 0):
        keys, vals = M.pack(bread, aread, apos, apos - bpos, 16, dbits, 10)
        assert (vals is None) == (dbits != 0)
        got = M.unpack(keys, vals, 16, dbits, 10)
        for g, w in zip(got, (bread, aread, apos, apos - bpos)):
            assert np.array_equal(g, w)
    # the key order is the sort order: bread, aread, apos, bpos
    keys, _ = M.pack([1, 1, 1, 2], [3, 3, 4, 0], [9, 10, 0, 0], [9 - 5, 10 - 0, 0, 0], 16, 17, 10)
    assert (np.diff(keys.astype(np.int64)) > 0).all()


def test_slices_move_to_the_next_change_of_bread():
    """filter.c:2807-2813 on a list of 16 seeds: -j4 puts the nominal starts at 4, 8, 12; each moves on while bread repeats."""
    bread = np.array([0, 0, 0, 0, 0, 0, 1, 1, 2, 3, 3, 3, 3, 3, 4, 5])
    assert M.slices(bread, 2) == [(0, 6), (6, 8), (8, 14), (14, 16)]
    assert M.slices(bread, 0) == [(0, 16)]
    assert M.slices(np.zeros(16, dtype=np.int64), 1) == [(0, 16), (16, 16)]
