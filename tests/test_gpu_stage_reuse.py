"""The stage record of the shim (damar_amd/csrc/stage.h, struct DevStage) under release and reuse: every call family is
called on the first two piles (boxes, tiles) of its smallest input, released, and called on the whole input, so that every
buffer grows from nothing and the events are made anew.  The result must be the host routine's, the counters of
damar_*_last those of a call on a fresh stage, and every device phase must have taken time."""
import os

import numpy as np
import pytest

import q_common

pytestmark = pytest.mark.gpu
DROP = ("DAMAR_PILES", "DAMAR_TRIM", "DAMAR_STITCH", "DAMAR_PILE_BATCH", "DAMAR_TEST_GAP_BINS", "DAMAR_TEST_FIX_SEGS",
        "DAMAR_TEST_FILTER_LEN", "DAMAR_TEST_FILTER_GROUP", "DAMAR_TEST_CORRECT_COLS", "DAMAR_TEST_BOX_LIMIT", "DAMAR_POSTRACE",
        "DAMAR_TEST_READ_DIFFS", "DAMAR_TEST_READ_GRID", "DAMAR_TEST_FILTER_GRID")
RECORD_COLS = ("abpos", "aepos", "bbpos", "bepos", "bread", "flags", "diffs", "tlen", "trace_off")
PHASES = ("upload", "kernel", "download")


@pytest.fixture(autouse=True)
def device_path(monkeypatch):
    for k in DROP:
        monkeypatch.delenv(k, raising=False)


def smallest(common, names):
    """the input of a common module whose .las file is the smallest"""
    return min(names, key=lambda n: os.path.getsize(os.path.join(q_common.GOLDEN, common.INPUTS[n][1])))


def head(batch, k=2):
    """the first k piles of a batch of the read_piles / read_trace_piles form"""
    n = int(batch["pile_off"][k])
    out = dict(batch, pile_off=batch["pile_off"][:k + 1], pile_aread=batch["pile_aread"][:k])
    for c in RECORD_COLS:
        if c in batch:
            out[c] = batch[c][:n]
    if "trace" in batch:
        out["trace"] = batch["trace"][:int(batch["trace_off"][n - 1]) + int(batch["tlen"][n - 1]) * int(batch["tbytes"])]
    return out


def same(got, want):
    if isinstance(want, dict):
        assert sorted(got) == sorted(want)
        for k in want:
            same(got[k], want[k])
    elif isinstance(want, (tuple, list)):
        assert len(got) == len(want)
        for g, w in zip(got, want):
            same(g, w)
    elif isinstance(want, np.ndarray):
        assert np.array_equal(got, want)
    else:
        assert got == want


# every stage: -> (call(part) with part "head" or "whole", api's *_last, the name api.release takes or None, the variable
# that sends the call to the host routine, the names of the device phases)

def pile_stage():
    import masks_common as mc
    from damar_amd import api
    las = min((os.path.join(mc.REP, f) for f in ("G.1.las", "G.1f.las")), key=os.path.getsize)
    whole, = api.read_piles(las)
    rl, rf, _ = api.db_info(os.path.join(mc.REP, "G"))
    parts = dict(head=head(whole), whole=whole)
    return (lambda part: api.pile_repeats(parts[part], rl, rf, api.repeat_params(cov=8)), api.pile_last, "pile", "DAMAR_PILES",
            ("upload", "sort", "sweep", "download"))


def q_stage():
    from damar_amd import api
    inp = smallest(q_common, [n for n, v in q_common.INPUTS.items() if v[1]])
    whole, rl = q_common.read_las(q_common.input_path(inp, None)), q_common.db_read_len(q_common.INPUTS[inp][0])
    parts = dict(head=head(whole), whole=whole)
    return lambda part: api.pile_quality(parts[part], rl), api.q_last, "q", "DAMAR_PILES", ("upload", "count", "select", "download")


def homog_stage():
    import hom_checks
    from damar_amd import api
    p, _ = hom_checks.plan()
    ra, rd = p.track()
    parts = dict(head=p.batch(p.piles()[:2]), whole=p.batch())
    return (lambda part: api.pile_homogenize([parts[part]], p.rl, ra, rd), api.homog_last, None, "DAMAR_PILES",
            ("upload", "mark", "readout", "download"))


def box_stage():
    import trim_common as tc
    from damar_amd import api
    z = tc.boxes()                                                           # fewer bases than boxes_wide()
    a, b = tc.box_seqs({k: z[k] for k in ("m", "n", "aoff", "boff", "bases")})
    parts = dict(head=(a[:2], b[:2]), whole=(a, b))
    return lambda part: api.align_boxes(*parts[part]), api.box_last, "box", "DAMAR_TRIM", PHASES


def tbox_stage():
    import stitch_common as sc
    from damar_amd import api
    bx = sc.tboxes()
    a, b, at = sc.run_seqs(bx, np.arange(len(bx["run_box"])))
    parts = dict(head=(a[:2], b[:2], at[:2]), whole=(a, b, at))
    return lambda part: api.trace_boxes(*parts[part], sc.TW), api.tbox_last, "tbox", "DAMAR_STITCH", PHASES


def gap_stage():
    import gap_common as gc
    from damar_amd import api
    inp = smallest(gc, gc.REAL + ("gsynth",))
    names = ("pile_off", "pile_aread", "abpos", "aepos", "bbpos", "bepos", "bread", "flags")
    whole = dict(zip(names, gc.pile_arrays(os.path.join(gc.GOLDEN, gc.INPUTS[inp][1]))))
    rl = q_common.db_read_len(gc.INPUTS[inp][0])
    parts = dict(head=head(whole), whole=whole)
    return lambda part: api.pile_gaps(parts[part], rl, stitch=100), api.gap_last, "gap", "DAMAR_PILES", PHASES


def fix_stage():
    import fix_common as fc
    from damar_amd import api
    inp = smallest(fc, fc.REAL + ("fsynth",))
    whole, rl = fc.batch_of(inp)
    tr = fc.tracks(inp)
    trims = fc.trims_of(whole, rl, tr["trim"])
    parts = dict(head=(head(whole), trims[:2]), whole=(whole, trims))
    return (lambda part: api.pile_patches(parts[part][0], rl, parts[part][1], tr["q"], repeats=tr["rep"]), api.fix_last, "fix",
            "DAMAR_PILES", PHASES)


def filter_stage():
    import filter_common as fc
    from damar_amd import api
    inp = smallest(fc, fc.REAL + ("fsynth",))
    whole, rl = fc.trace_batch(os.path.join(fc.GOLDEN, fc.INPUTS[inp][1])), q_common.db_read_len(fc.INPUTS[inp][0])
    parts = dict(head=head(whole), whole=whole)
    return lambda part: api.pile_filter(parts[part], rl, stitch=300, min_olen=500), api.filter_last, "filter", "DAMAR_PILES", PHASES


def correct_stage():
    import correct_common as cc
    from damar_amd import api
    planted = [t for p in cc.planted_piles() for t in p["tiles"]]
    size = lambda tiles: sum(len(s) for t in tiles for s in t)
    whole = min((cc.random_tiles(), planted), key=size)
    parts = dict(head=whole[:2], whole=whole)
    return lambda part: api.tile_consensus(parts[part]), api.correct_last, "correct", "DAMAR_PILES", PHASES


def read_stage():
    import read_align_common as rc
    from damar_amd import api
    bx = rc.boxes()
    a, b = rc.box_seqs(bx, rc.family_rows(bx, "many"))                       # forty short boxes
    parts = dict(head=(a[:2], b[:2]), whole=(a, b))
    return lambda part: api.align_reads(*parts[part]), api.read_last, "read", "DAMAR_POSTRACE", PHASES


STAGES = dict(pile=pile_stage, q=q_stage, homog=homog_stage, box=box_stage, tbox=tbox_stage, gap=gap_stage, fix=fix_stage,
              filter=filter_stage, correct=correct_stage, read=read_stage)


@pytest.mark.parametrize("stage", sorted(STAGES))
def test_release_then_whole_input(stage, monkeypatch):
    from damar_amd import api
    call, last, name, host_var, phases = STAGES[stage]()
    release = (lambda: api.release(name)) if name else (lambda: None)       # a homogenize session ends inside its call
    release()
    call("whole")
    fresh = last()[1:]                                                       # the counters of a call on a fresh stage
    call("head")
    release()
    got = call("whole")
    ms, counters = last()[0], last()[1:]
    monkeypatch.setenv(host_var, "host")
    want = call("whole")
    monkeypatch.delenv(host_var)
    same(got, want)
    assert counters == fresh
    for k in phases:
        assert ms[k] > 0, (k, ms)
