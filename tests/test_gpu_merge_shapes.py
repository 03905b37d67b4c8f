"""The merge of two sorted k-mer indexes into seed pairs (kernels/seed_merge.hip) on the planted shapes of
tests/merge_shapes.py: code runs at tile, piece and cap borders that simulated reads reach only by luck.  Every case is one
damar_match with the seed list kept; the list must be the oracle's record for record (diag, apos, aread, bread, in the
reference's order), and a mismatch names the case, the first differing record and the planted run it belongs to.
tests/test_merge_shapes_host.py asserts, without a GPU, that every case sits on the border it is named for.

Four runs of every case: in this process, and in one fresh child process each (the switches are read once per process)
under DAMAR_MERGE_GENERAL=1 (every tile through the general kernel), DAMAR_PACK_POS=0 (position words as block offsets:
the look-up forms of self_hits and pos_decode, self comparisons never in merge_fast) and DAMAR_PACK_SEEDS=0 (the diagonal
in vals).  damar_last_merge_flagged() shows that the fast and the general kernel both ran where a case says so.

Reads shorter than k are not among the shapes: damar_index_build refuses a block that has one, as the reference does
(daligner.c:499-504)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import merge_shapes as M
from test_gpu_slabs import Pair, greedy

pytestmark = pytest.mark.gpu

MODES = {"general": {"DAMAR_MERGE_GENERAL": "1"}, "pack_pos0": {"DAMAR_PACK_POS": "0"}, "pack_seeds0": {"DAMAR_PACK_SEEDS": "0"}}
CHILD_SECONDS = 300


def planted_pair(L, case):
    """Pair (test_gpu_slabs.py) over the blocks of a planted case instead of blocks read from files"""
    adb, bdb = case.dbs()
    return Pair(L, None, None, case.comp, k=case.k, identity=case.identity, blocks=(adb, bdb, not case.self_))


def run_case(L, case):
    """-> flat dict of arrays: the seed list, [counts[0], seeds kept, flagged tiles, cap on mutual matches], and for a slab
    case per figure the slab table and the split run's seed list"""
    from damar_amd import api
    x = M.context(case)
    out = {}
    memvar = C.c_uint64.in_dll(L, "MEM_LIMIT")
    old = memvar.value
    p = planted_pair(L, case)
    try:
        if x.mem is not None:
            memvar.value = x.mem
        r = p.match(seeds=True)
        out["seeds"] = r["seeds"]
        out["meta"] = np.array([r["counts"][0], r["nseeds"], L.damar_last_merge_flagged(), L.damar_last_limit()], dtype=np.int64)
        if case.caps:
            h = np.bincount(x.want["bread"], minlength=x.nrb)
            for i, f in enumerate(case.caps):
                r = p.match(cap=f(h), seeds=True)
                out["cap%d_seeds" % i] = r["seeds"]
                out["cap%d_lo" % i] = np.array(r["slabs"][0], dtype=np.int64)
                out["cap%d_hits" % i] = np.array(r["slabs"][1], dtype=np.int64)
                out["cap%d_meta" % i] = np.array([r["counts"][0], r["nseeds"], r["totals"][0], r["totals"][1]], dtype=np.int64)
    finally:
        memvar.value = old
        p.close()
        api.set_globals()
        L.Set_Filter_Params(14, 6, 0, 35, 4)
    return out


@pytest.fixture(scope="module")
def gpu(built):
    from damar_amd import api
    L = api.lib()
    assert L.damar_hip_init(0) >= 1
    return L


def _child(mode, tmp):
    """every case's results from ONE fresh child process under the mode's switch, with a time limit"""
    out = os.path.join(tmp, mode + ".npz")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], cwd=ROOT, env=dict(os.environ, **MODES[mode]),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=CHILD_SECONDS)
    assert r.returncode == 0, r.stdout[-3000:]
    return np.load(out)


_children = {}


@pytest.fixture(scope="module")
def child(built, tmp_path_factory):
    """mode -> the child's results.  A mode's child is started at most ONCE per session: when it fails (an abort, a fault,
    its time limit) the failure is kept and every later case of the mode fails with it at once, without another process."""
    tmp = str(tmp_path_factory.mktemp("merge_shapes"))

    def get(mode):
        if mode not in _children:
            try:
                _children[mode] = _child(mode, tmp)
            except BaseException as e:
                _children[mode] = e
                raise
        z = _children[mode]
        if isinstance(z, BaseException):
            pytest.fail("the child process of mode %s failed earlier in this session and is not started again: %r" % (mode, z))
        return lambda cid: {k[len(cid) + 2:]: z[k] for k in z.files if k.startswith(cid + "__")}
    return get


def same_seeds(case, x, got, want, what):
    if len(got) == len(want) and np.array_equal(got, want):
        return
    n = min(len(got), len(want))
    d = np.flatnonzero(got[:n] != want[:n])
    i = int(d[0]) if len(d) else n
    rec = got[i] if len(got) > len(want) or i >= len(want) else want[i]        # (more seeds: the one too many; else the one missing)
    pytest.fail("%s (%s): %d seeds, the oracle has %d; first difference at record %d: got %s, want %s -- %s" % (
        case.id, what, len(got), len(want), i, got[i] if i < len(got) else None, want[i] if i < len(want) else None,
        M.describe(case, x, rec)))


def check(case, res, mode):
    x = M.context(case)
    counts0, nseeds, flagged, limit = [int(v) for v in res["meta"]]
    print(case.id, mode, "seeds", nseeds, "tiles", x.ntiles, "flagged", flagged, "limit", limit)
    same_seeds(case, x, res["seeds"], x.want, mode)
    assert counts0 == nseeds == len(x.want)
    assert limit == x.limit                                 # damar_last_limit() is the oracle's LAST_LIMIT
    if mode == "general":
        assert flagged == x.ntiles
    elif mode == "pack_pos0" and case.self_:
        assert flagged == x.ntiles                          # rpbits == 0: a self comparison never takes merge_fast
    else:                                                   # exactly the tiles the rule of merge_fast hands on
        want = M.flagged_tiles(x)
        assert flagged == len(want), (flagged, sorted(want))
        if case.flagged == ">0":
            assert 0 < flagged < x.ntiles                   # both kernels ran
        elif case.flagged is not None:
            assert flagged == case.flagged
    if case.caps:
        h = np.bincount(x.want["bread"], minlength=x.nrb)
        for i, f in enumerate(case.caps):
            lo, sums = greedy(h, f(h))
            assert len(sums) >= 3
            assert (list(res["cap%d_lo" % i]), list(res["cap%d_hits" % i])) == (lo, sums)
            c0, ns, stages, split = [int(v) for v in res["cap%d_meta" % i]]
            assert (c0, ns, split) == (len(x.want), len(x.want), 1) and stages == sum(1 for s in sums if s > 0)
            same_seeds(case, x, res["cap%d_seeds" % i], x.want, "%s, in %d slabs" % (mode, len(sums)))


@pytest.mark.parametrize("cid", M.IDS)
def test_gpu_planted_merge_equals_oracle(gpu, cid):
    case = M.BY_ID[cid]
    check(case, run_case(gpu, case), "default")


@pytest.mark.parametrize("cid", M.IDS)
@pytest.mark.parametrize("mode", sorted(MODES))
def test_gpu_planted_merge_equals_oracle_under_switch(child, mode, cid):
    case = M.BY_ID[cid]
    check(case, child(mode)(cid), mode)


def test_every_case_is_run():
    assert [c.id for c in M.CASES] == M.IDS and len(M.IDS) == len(set(M.IDS))


if __name__ == "__main__":                                 # the child: every case under the switch the environment holds
    from damar_amd import api
    L = api.lib()
    assert L.damar_hip_init(0) >= 1
    res = {}
    for case in M.CASES:
        for k, v in run_case(L, case).items():
            res[case.id + "__" + k] = v
    np.savez(sys.argv[1], **res)
