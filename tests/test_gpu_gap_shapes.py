"""kernels/pile_gaps.hip against the plain model (tests/gap_model.py) on the shapes of tests/gap_shapes.py, which sit on the
kernel's borders of 64 lanes and 64 bins, and on seeded random piles: flags, events and the count of piles left to the host
routine, exactly; whole, in slices, with few workgroups (DAMAR_TEST_GAP_GRID) and with a low bin limit."""
import json
import os

import numpy as np
import pytest

import gap_common as gc
import gap_model as gm
import gap_shapes as gs

pytestmark = pytest.mark.gpu
DROP = ("DAMAR_PILES", "DAMAR_TEST_GAP_BINS", "DAMAR_TEST_GAP_GRID", "DAMAR_PILE_BATCH")
KW = dict(gs.OPTION_SETS)


@pytest.fixture(autouse=True)
def device_path(monkeypatch):
    for k in DROP:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def shapes():
    every = gs.shapes()
    rl = gs.read_len(every)
    js = json.load(open(os.path.join(gc.GDIR, "shapes.json")))
    assert gs.digest(gs.arrays(every, rl)[0], rl) == js["sha256"], "tests/gap_shapes.py changed: run tests/golden/make_gap_shapes_golden.py"
    return [s for s in every if not s.refused], rl


@pytest.fixture(scope="module")
def random_piles():
    return gs.random_piles()


def device_against_model(piles, rl, ex, kw, what, limits=None):
    """one call on the device path: flags, events and the three counts of gap_last against the model -> (model, on_host)"""
    from damar_amd import api
    limits = limits or api.gap_limits()
    flags, events = api.pile_gaps(piles, rl, stitch=kw.get("stitch", 0), exclude=ex if kw.get("exclude") else None)
    ms, npiles, host_piles, nev = api.gap_last()
    res = gm.run(piles, rl, stitch=kw.get("stitch", 0), exclude=ex if kw.get("exclude") else None)
    print("%s: %d piles, %d records, kernel %.3f ms" % (what, npiles, len(flags), ms["kernel"]))
    bad = np.flatnonzero(flags != res.flags_array())
    assert len(bad) == 0, "%s: flags differ in records %s" % (what, bad[:8])
    assert len(events) == len(res.events)
    for p, (d, m) in enumerate(zip(events, res.events)):
        assert d == m, "%s: pile %d (read %d): %s against %s" % (what, p, piles["pile_aread"][p], d, m)
    assert (npiles, host_piles, nev) == (len(res.events), res.host_piles(limits), sum(len(e) for e in res.events)), what
    return res, res.on_host(limits)


def test_limits_are_the_shapes():
    from damar_amd import api
    assert api.gap_limits() == (4096, 16)              # what events_16 / events_17 and the nb_* reads are placed at
    assert (gs.BIN, gs.MIN_LR, gs.WAVE) == (gm.BIN, gm.MIN_LR, gm.WAVE) == (100, 450, 64)
    assert api.GAP_KINDS == ("masked", "stitchable", "drop_L", "drop_R", "drop_none") and api.GAP_TRAILING == gm.TRAILING
    assert (gm.MASKED, gm.STITCHABLE, gm.DROP_L, gm.DROP_R, gm.DROP_NONE) == (0, 1, 2, 3, 4)


@pytest.mark.parametrize("key", list(KW))
def test_shapes_match_the_model(shapes, key):
    S, rl = shapes
    piles, _, ex = gs.arrays(S, rl)
    _, on_host = device_against_model(piles, rl, ex, KW[key], "shapes " + key)
    # the host routine does the pile of 17 events and the one whose B reads descend: no other, not the pile of 16 events
    assert sorted(s.tag for s, h in zip(S, on_host) if h) == ["descending", "events_17"]


@pytest.mark.parametrize("key", ["def", "s300", "e", "es"])
def test_random_piles_match_the_model(random_piles, key):
    piles, rl, ex = random_piles
    device_against_model(piles, rl, ex, KW[key], "random piles " + key)


@pytest.mark.parametrize("grid", [1, 3, 7])
def test_a_workgroup_takes_several_piles(shapes, grid, monkeypatch):
    """the bins in LDS reused from pile to pile: the read of 129 bins alternating with reads of 63, and with the piles a
    workgroup passes over (no records, marked for the host, over the event limit)"""
    S, rl = shapes
    by = {s.tag: s for s in S}
    special = [by[t] for t in ("nb_129", "nb_63", "empty", "nb_129", "descending", "nb_63", "events_17", "nb_129", "all_discarded")]
    order = []
    for i, s in enumerate(S):
        order += [s, special[i % len(special)]]
    piles, _, ex = gs.arrays(order, rl)
    monkeypatch.setenv("DAMAR_TEST_GAP_GRID", str(grid))
    for key in ("def", "es"):
        _, on_host = device_against_model(piles, rl, ex, KW[key], "grid %d, %s" % (grid, key))
        assert {s.tag for s, h in zip(order, on_host) if h} == {"descending", "events_17"}


def test_bin_limit_of_64(shapes, monkeypatch):
    S, rl = shapes
    piles, _, ex = gs.arrays(S, rl)
    monkeypatch.setenv("DAMAR_TEST_GAP_BINS", "64")
    _, on_host = device_against_model(piles, rl, ex, KW["def"], "64 bins", limits=(64, 16))
    gone = {s.tag for s, h in zip(S, on_host) if h}
    assert gone == {s.tag for s in S if (s.alen + 100) // 100 > 64} | {"descending", "events_17"}
    assert "nb_64" not in gone and "nb_63" not in gone and "nb_65" in gone
    # who does which pile, pile by pile: what the count of one call cannot show
    from damar_amd import api
    for p, s in enumerate(S):
        one, _, ex1 = gs.arrays([s], rl)
        api.pile_gaps(one, rl)
        assert api.gap_last()[2] == int(on_host[p]), s.tag


@pytest.mark.parametrize("step", [1, 2, 50])
def test_slices_give_the_same_as_the_whole(shapes, step):
    S, rl = shapes
    whole = gm.run(gs.arrays(S, rl)[0], rl, stitch=300, exclude=gs.arrays(S, rl)[2])
    flags, events, hosts = [], [], 0
    for at in range(0, len(S), step):
        piles, _, ex = gs.arrays(S[at:at + step], rl)
        res, on_host = device_against_model(piles, rl, ex, KW["es"], "piles %d..%d" % (at, at + step - 1))
        flags += res.flags
        events += res.events
        hosts += sum(on_host)
        if step == 1:
            assert on_host[0] == (S[at].tag in ("descending", "events_17")), S[at].tag
    assert flags == whole.flags and events == whole.events and hosts == 2
