"""LAq on the GPU (kernels/pile_quality.hip): every fixture of tests/golden/q/ through the command and the Python calls,
equal to the reference's tracks and to the host path; the same file in many batches; random batches against the plain model
(tests/q_model.py) at the shapes that can break the kernels (tests/q_shapes.py); the counts damar_q_last reports."""
import os

import numpy as np
import pytest

import q_common
import q_model
import q_shapes
from q_common import GOLDEN, INPUTS

pytestmark = pytest.mark.gpu
CASES = q_common.load_cases()
IDS = [c["name"] for c in CASES]


@pytest.fixture(autouse=True)
def device_path(monkeypatch, built):
    monkeypatch.delenv("DAMAR_PILES", raising=False)
    monkeypatch.delenv("DAMAR_PILE_BATCH", raising=False)
    monkeypatch.delenv("DAMAR_PILE_TRACE_BYTES", raising=False)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_laq_command_on_device(case, tmp_path):
    q_common.run_case(case, str(tmp_path), {}, timeout_s=120)


def _tracks(case, tmp):
    from damar_amd import api
    db = os.path.join(GOLDEN, INPUTS[case["input"]][0], "G")
    las = q_common.input_path(case["input"], tmp)
    kw = q_common.opts_to_kwargs(case["opts"])
    if "-u" in case["opts"]:
        plain = api.q_track(db, q_common.input_path("tiny2", tmp))
        return plain[:2] + api.trim_update(db, las, plain[:2], plain[2:], **{k: v for k, v in kw.items() if k != "segmin" and k != "segmax"})
    return api.q_track(db, las, **kw)


def _same(got, want):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_python_calls_on_device_equal_reference_and_host(case, tmp_path, monkeypatch):
    from damar_amd import api
    exp = q_common.expected(case["name"])
    got = _tracks(case, str(tmp_path))
    _same(got, [exp[k] for k in ("q_anno", "q_data", "trim_anno", "trim_data")])
    ms, segs, tiles = api.q_last()
    assert tiles > 0 and all(v >= 0 for v in ms.values())
    monkeypatch.setenv("DAMAR_PILES", "host")
    _same(_tracks(case, str(tmp_path)), got)


@pytest.mark.parametrize("name", ["def_tiny2", "def_tiny_s", "def_synth"])
def test_many_batches_on_device(name, tmp_path, monkeypatch):
    from damar_amd import api
    case = [c for c in CASES if c["name"] == name][0]
    exp = q_common.expected(name)
    want = [exp[k] for k in ("q_anno", "q_data", "trim_anno", "trim_data")]
    monkeypatch.setenv("DAMAR_PILE_BATCH", "1000")
    _same(_tracks(case, str(tmp_path)), want)
    monkeypatch.setenv("DAMAR_PILE_BATCH", "10")                     # fewer records than any of the files holds
    _same(_tracks(case, str(tmp_path)), want)
    assert api.q_last()[2] < len(exp["q_data"])                      # the last call held a part of the file only
    monkeypatch.delenv("DAMAR_PILE_BATCH")
    monkeypatch.setenv("DAMAR_PILE_TRACE_BYTES", "3000")
    _same(_tracks(case, str(tmp_path)), want)


@pytest.mark.parametrize("shape", range(len(q_shapes.SHAPES)))
def test_random_batches_equal_model(shape):
    from damar_amd import api
    b, rl, kw = q_shapes.make(shape)
    q, tile0, depth, nseg = q_model.tile_q(b, rl, **kw)
    got = api.pile_quality(b, rl, **kw)
    ms, segs, tiles = api.q_last()
    print("shape %d: %d records, %d tiles, %d segments, depths %d..%d, ms %s" % (shape, len(b["abpos"]), len(q), nseg, depth.min(), depth.max(), ms))
    assert (segs, tiles) == (nseg, len(q))                           # exact: what the walk counted and what was laid out
    bad = np.flatnonzero(got != q)
    assert len(bad) == 0, "tiles %s: device %s, model %s, depth %s" % (bad[:8], got[bad[:8]], q[bad[:8]], depth[bad[:8]])
    if shape == 0:                                                   # the shapes are what they are meant to be
        assert set([0, 1, 19, 20, 21]) <= set(depth.tolist())
        spilled = q_model.tile_q(b, rl, spill=False, **kw)[0]
        assert np.any(spilled != q)
    if shape == 2:
        assert set([255, 256, 257, 5000]) <= set(depth.tolist())
    if shape >= len(q_shapes.SHAPES) - 4:
        assert len(q) == q_shapes.SHAPES[shape][2]


def test_other_options_on_one_batch():
    """segmax 1, 20, 64 and 1000, segmin and ccs over one batch with deep and shallow tiles"""
    from damar_amd import api
    b, rl, _ = q_shapes.make(2)
    for kw in (dict(segmax=1), dict(segmax=20), dict(segmax=64, segmin=64), dict(segmax=1000, segmin=300, ccs=True),
               dict(segmax=0x7fffffff)):
        assert np.array_equal(api.pile_quality(b, rl, **kw), q_model.tile_q(b, rl, **kw)[0]), kw
