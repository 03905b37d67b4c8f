"""LArepeat and TANmask on the GPU (kernels/pile_sweep.hip): every fixture of tests/golden/masks_*/ through the commands and
the Python calls, random piles at the shapes that can break the kernels against the plain model (tests/masks_model.py), the
host path as second opinion, batching, and the mask chain datander -> TANmask -> daligner -mtan with our tools alone."""
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import masks_model
from conftest import GOLDEN
from masks_common import (BIN, REP, REP_CASES, TAN, TAN_CASES, case_las, check_repeat_arrays, opts_to_kwargs, run_larepeat,
                          run_tanmask)

pytestmark = pytest.mark.gpu
TILE = 4096                 # DAMAR_SCAN_TILE (kernels/kernels.h); the sweep's own chunk is 256 events


@pytest.fixture(autouse=True)
def device_path(monkeypatch, built):
    monkeypatch.delenv("DAMAR_PILES", raising=False)


@pytest.mark.parametrize("case", REP_CASES, ids=[c["name"] for c in REP_CASES])
def test_larepeat_command_on_device(case, tmp_path):
    run_larepeat(case, str(tmp_path), {}, timeout_s=120)


@pytest.mark.parametrize("case", TAN_CASES, ids=[c["name"] for c in TAN_CASES])
def test_tanmask_command_on_device(case, tmp_path):
    run_tanmask(case, str(tmp_path), {}, timeout_s=120)


def test_python_calls_on_device_equal_reference_and_host(monkeypatch):
    from damar_amd import api
    db = os.path.join(REP, "G")
    for case in REP_CASES:
        las = os.path.join(REP, case_las(case))
        exp = np.load(os.path.join(REP, "expected_%s.npz" % case["name"]))
        kw = opts_to_kwargs(case["opts"])
        anno, data, stats = api.repeat_track(db, las, **kw)
        check_repeat_arrays(case, anno, data, exp)
        assert stats["merged"] == int(exp["MERGED"]) and stats["bases_repeat"] == int(exp["BASES_REPEAT"])
        if "histo" in exp.files:
            assert np.array_equal(stats["histo"], exp["histo"]) and stats["cov_max"] == int(exp["MAX"])
        monkeypatch.setenv("DAMAR_PILE_BATCH", "1000")               # the same file in many batches
        anno2, data2, stats2 = api.repeat_track(db, las, **kw)
        monkeypatch.setenv("DAMAR_PILES", "host")                    # ... and on the host path
        anno3, data3, stats3 = api.repeat_track(db, las, **kw)
        monkeypatch.delenv("DAMAR_PILES")
        monkeypatch.delenv("DAMAR_PILE_BATCH")
        assert np.array_equal(anno, anno2) and np.array_equal(data, data2) and stats2["merged"] == stats["merged"]
        assert np.array_equal(anno, anno3) and np.array_equal(data, data3) and stats3["bases_repeat"] == stats["bases_repeat"]
    for case in TAN_CASES:
        e = np.load(os.path.join(TAN, "expected_%s.npz" % case["name"]))
        offs, data = api.tan_track(os.path.join(GOLDEN, case["db"], "G"), os.path.join(GOLDEN, case["las"]), 0, 0 if case["whole"] else 1)
        assert offs.astype("<i8").tobytes() == e["anno"].tobytes()[8:] and data.astype("<i4").tobytes() == e["data"].tobytes()
    ms, events, regions = api.pile_last()
    assert events > 0 and regions > 0 and all(v >= 0 for v in ms.values())


def _random_batch(rng, sizes, nreads, rlen, dense=False, discard=0.1):
    """piles of the given record counts over reads of length rlen; dense: few distinct coordinates, many ties"""
    n = int(sum(sizes))
    step = 500 if dense else 1
    ab = (rng.integers(0, (rlen - 2) // step, n) * step).astype(np.int32)
    ab[rng.random(n) < 0.1] = 0
    ln = (rng.integers(1, max(2, (rlen // 2) // step), n) * step).astype(np.int32)
    ae = np.minimum(ab + ln, rlen).astype(np.int32)
    ae[rng.random(n) < 0.1] = rlen
    bb = np.maximum(ab - rng.integers(0, 60, n), 0).astype(np.int32)          # tandem-like: bepos close to abpos
    be = np.maximum(ab - rng.integers(-30, 30, n), 1).astype(np.int32)
    aread = rng.choice(nreads, len(sizes), replace=False).astype(np.int32)
    aread.sort()
    bread = rng.integers(0, nreads, n).astype(np.int32)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    for i in range(len(sizes)):                                                # some identity overlaps
        if sizes[i] and rng.random() < 0.3:
            bread[off[i]] = aread[i]
    flags = np.where(rng.random(n) < discard, 2, 0).astype(np.int32) | (rng.random(n) < 0.5).astype(np.int32)
    return dict(pile_off=off, pile_aread=aread, abpos=ab, aepos=ae, bbpos=bb, bepos=be, bread=bread, flags=flags)


SHAPES = [                      # (pile sizes in records, read length, dense)
    ([0, 1, 2, 0], 5000, False),
    ([31, 32, 33], 5000, True),                     # 62..66 events before the filters
    ([32], 3000, False),
    ([127, 128, 129, 1], 8000, True),               # around the sweep's 256-event chunk
    ([128, 128, 128], 8000, False),                 # pile boundaries on chunk boundaries (no record dropped: see below)
    ([TILE // 2 - 1, TILE // 2, TILE // 2 + 1], 20000, True),      # one below / at / above the scan tile, in events
    ([3 * TILE // 2 + 7], 30000, False),            # one pile over three tiles
    ([5] * 5000, 6000, True),                       # 5000 piles
    ([40, 0, 0, 700, 3], (1 << 17) - 1, False),     # the longest read 17 position bits allow
]


@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_random_piles_equal_model(shape):
    from damar_amd import api
    sizes, rlen, dense = SHAPES[shape]
    rng = np.random.default_rng(1000 + shape)
    nreads = max(len(sizes) + 3, 50)
    rl = np.full(nreads, rlen, dtype=np.int32)
    rl[0] = max(rlen // 2, 10)
    rf = np.where(rng.random(nreads) < 0.8, 0x0800, 0).astype(np.int32)
    p = _random_batch(rng, sizes, nreads, rlen, dense, discard=0.0 if shape == 4 else 0.1)
    for a, i in zip(p["pile_aread"], range(len(sizes))):             # coordinates inside the pile's own read
        s = slice(int(p["pile_off"][i]), int(p["pile_off"][i + 1]))
        p["aepos"][s] = np.minimum(p["aepos"][s], rl[a])
        p["abpos"][s] = np.minimum(p["abpos"][s], p["aepos"][s] - 1)
    for kw in (dict(cov=2), dict(cov=2, inccov=1, merge_dist=600), dict(cov=1, xcov_leave=0.5, merge_dist=600),
               dict(cov=3, xcov_enter=2.0, xcov_leave=2.0, inccov=1), dict(cov=2, merge_dist=2000, inc_identity=1, min_aln_len=700)):
        count, data, merged, rbases = api.pile_repeats(p, rl, rf, api.repeat_params(**kw))
        ecount, edata, emerged, erbases = masks_model.repeats(p, rl, **kw)
        assert np.array_equal(count, ecount) and np.array_equal(data, edata), kw
        assert (merged, rbases) == (emerged, erbases), kw
    histo, bases, inactive = api.pile_coverage(p, rl, rf, api.repeat_params(min_aln_len=300))
    eh, eb, ei = masks_model.coverage(p, rl, rf, min_aln_len=300)
    assert np.array_equal(histo, eh) and (bases, inactive) == (eb, ei)
    for min_len in (0, 900):
        count, data = api.pile_tandem(p, rl, rf, min_len)
        ecount, edata = masks_model.tandem(p, min_len)
        assert np.array_equal(count, ecount) and np.array_equal(data, edata)


def _kept_batch(rng, sizes, nreads, rlen):
    """like _random_batch, but every record passes every filter of the three sweeps, so the event counts are exact: nothing
    discarded, no identity overlap, every B read DB_BEST (the caller's read_flags), tandem-like coordinates"""
    p = _random_batch(rng, sizes, nreads, rlen, dense=True, discard=0.0)
    p["flags"][:] &= 1
    for i in range(len(sizes)):
        s = slice(int(p["pile_off"][i]), int(p["pile_off"][i + 1]))
        p["bread"][s] = (p["pile_aread"][i] + 1 + rng.integers(0, nreads - 1, int(sizes[i]))) % nreads        # never the A read
    p["aepos"][:] = np.maximum(p["aepos"], p["abpos"] + 1)
    p["bbpos"][:] = p["abpos"]
    p["bepos"][:] = p["abpos"]
    return p


EXACT = [                       # pile sizes in records; a record is two events, so a pile's event count is even
    [31, 32, 33],                                   # 62 / 64 / 66 events
    [127, 128, 129],                                # 254 / 256 / 258: one pair below, at and above the sweep's 256-event chunk
    [255, 256, 257],                                # 510 / 512 / 514: two chunks; and 255 / 256 / 257 kept records
    [128, 256, 128, 384],                           # every pile boundary on a chunk boundary, in the sorted keys too
    [1] * 4095, [1] * 4096, [1] * 4097,             # piles one below / at / above the scan tile of the per-pile offsets
    [2, 0, 1] * 1365 + [1],                         # 4096 piles, a third of them empty
]


@pytest.mark.parametrize("shape", range(len(EXACT)))
def test_exact_shapes_equal_model(shape):
    from damar_amd import api
    sizes = EXACT[shape]
    rng = np.random.default_rng(2000 + shape)
    nreads, rlen = len(sizes) + 7, 9000
    rl = np.full(nreads, rlen, dtype=np.int32)
    rf = np.full(nreads, 0x0800, dtype=np.int32)
    p = _kept_batch(rng, sizes, nreads, rlen)
    for kw in (dict(cov=2), dict(cov=1, inccov=1, merge_dist=600), dict(cov=3, xcov_enter=2.0, xcov_leave=2.0, inc_identity=1)):
        count, data, merged, rbases = api.pile_repeats(p, rl, rf, api.repeat_params(**kw))
        _ms, events, regions = api.pile_last()
        assert events == 2 * sum(sizes)                                # every record kept: the counts above are the kernel's
        ecount, edata, emerged, erbases = masks_model.repeats(p, rl, **kw)
        assert np.array_equal(count, ecount) and np.array_equal(data, edata), kw
        assert (merged, rbases) == (emerged, erbases), kw
        width = 3 if kw.get("inccov") else 2
        assert regions == sum((int(c) + width - 1) // width for c in ecount)
    histo, bases, inactive = api.pile_coverage(p, rl, rf, api.repeat_params())
    assert api.pile_last()[1] == 2 * sum(sizes)
    eh, eb, ei = masks_model.coverage(p, rl, rf)
    assert np.array_equal(histo, eh) and (bases, inactive) == (eb, ei)
    count, data = api.pile_tandem(p, rl, rf, 0)
    _ms, events, intervals = api.pile_last()
    assert events == 2 * sum(sizes) and intervals == len(data) // 2
    ecount, edata = masks_model.tandem(p, 0)
    assert np.array_equal(count, ecount) and np.array_equal(data, edata)


def test_planted_shapes():
    """chains of three merges, a region that opens and never closes, equal coordinates, abpos == 0, all records dropped"""
    from damar_amd import api
    rl = np.full(8, 20000, dtype=np.int32)
    rf = np.full(8, 0x0800, dtype=np.int32)
    iv = []
    for s in (1000, 3000, 5000, 9000):                               # four stacks of 4; gaps 1000, 1000, 3000
        iv += [(s, s + 1001)] * 4
    iv += [(0, 20000), (0, 20000), (12000, 12000 + 1)]
    one = dict(pile_off=np.array([0, len(iv), len(iv) + 2], dtype=np.int64), pile_aread=np.array([1, 4], dtype=np.int32),
               abpos=np.array([a for a, _ in iv] + [5, 6], dtype=np.int32), aepos=np.array([e for _, e in iv] + [900, 800], dtype=np.int32),
               bbpos=np.zeros(len(iv) + 2, dtype=np.int32), bepos=np.ones(len(iv) + 2, dtype=np.int32),
               bread=np.array([2] * len(iv) + [4, 4], dtype=np.int32), flags=np.array([0] * len(iv) + [0, 2], dtype=np.int32))
    for kw in (dict(cov=2, merge_dist=1500), dict(cov=2, merge_dist=1500, inccov=1), dict(cov=1, xcov_enter=1.0, xcov_leave=0.4),
               dict(cov=1, xcov_enter=1.0, xcov_leave=0.4, merge_dist=5000, inccov=1)):
        count, data, merged, rbases = api.pile_repeats(one, rl, rf, api.repeat_params(**kw))
        ecount, edata, emerged, erbases = masks_model.repeats(one, rl, **kw)
        assert np.array_equal(count, ecount) and np.array_equal(data, edata) and (merged, rbases) == (emerged, erbases), kw
        assert count[1] == 0                                         # identity and discarded: nothing kept
    c, d, m, _ = api.pile_repeats(one, rl, rf, api.repeat_params(cov=2, merge_dist=1500))
    assert m == 2                                                    # the first three stacks are one chain
    c, d, m, _ = api.pile_repeats(one, rl, rf, api.repeat_params(cov=1, xcov_enter=1.0, xcov_leave=0.4))
    assert c[0] == 1                                                 # leave threshold 0: opens once, never closes


def test_mask_chain_with_our_tools(tmp_path):
    d = str(tmp_path)
    for f in ("G.db", ".G.idx", ".G.bps"):
        shutil.copy(os.path.join(GOLDEN, "tandem", f), os.path.join(d, f))
    t = ["timeout", "-k", "10", "120"]
    subprocess.run(t + [os.path.join(BIN, "datander"), "-j4", "G.1"], cwd=d, check=True, stdout=subprocess.DEVNULL)
    subprocess.run(t + [os.path.join(BIN, "TANmask"), "G", "tan/G.1.G.1.las"], cwd=d, check=True)
    subprocess.run(t + [os.path.join(BIN, "daligner"), "-k14", "-j4", "-mtan", "G.1", "G.1"], cwd=d, check=True, stdout=subprocess.DEVNULL)
    for ln in open(os.path.join(TAN, "chain_md5.txt")):
        md5, rel = ln.split()
        assert hashlib.md5(open(os.path.join(d, rel), "rb").read()).hexdigest() == md5, rel
