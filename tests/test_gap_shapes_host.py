"""The plain model of LAgap's per-pile routine (tests/gap_model.py) against the reference's fixtures, old and new, and against
the host routine (host/gap.c, DAMAR_PILES=host) on the shapes of tests/gap_shapes.py, the random piles and the planted file;
and the shapes against the model's mutants: every border of kernels/pile_gaps.hip got wrong shows on a named shape."""
import json
import os

import numpy as np
import pytest

import gap_common as gc
import gap_model as gm
import gap_shapes as gs
import q_common

HEAD = "\x1b[32mPASS gaps\x1b[0m"
OLD = [c for c in gc.load_cases() if "-t" not in c["opts"] and "-p" not in c["opts"]]
KW = dict(gs.OPTION_SETS)


@pytest.fixture(scope="module")
def fixture():
    """the shapes rebuilt, held against the sha256 the generator left: fixture and code cannot part company"""
    every = gs.shapes()
    js = json.load(open(os.path.join(gc.GDIR, "shapes.json")))
    rl = gs.read_len(every)
    assert gs.digest(gs.arrays(every, rl)[0], rl) == js["sha256"], "tests/gap_shapes.py changed: run tests/golden/make_gap_shapes_golden.py"
    return every, rl, js, np.load(os.path.join(gc.GDIR, "shapes_expected.npz"))


def model_stdout(areads, res):
    cont, dropped, breaks = gm.counts(res)
    out = [HEAD] + [ln for a, ev in zip(areads, res.events) for ln in gm.lines(int(a), ev)]
    return "\n".join(out + ["dropped %d containments" % cont, "dropped %d overlaps in %d break/gaps" % (dropped, breaks)]) + "\n"


def run_model(piles, rl, ex, kw, mutant=None):
    return gm.run(piles, rl, stitch=kw.get("stitch", 0), exclude=ex if kw.get("exclude") else None, mutant=mutant)


def as_piles(path):
    off, aread, ab, ae, bb, be, br, fl = gc.pile_arrays(path)
    return dict(pile_off=off, pile_aread=aread, abpos=ab, aepos=ae, bbpos=bb, bepos=be, bread=br, flags=fl)


@pytest.mark.parametrize("case", OLD, ids=[c["name"] for c in OLD])
def test_model_gives_the_existing_fixtures(case):
    """the file keeps every bit of the pile call's flags but OVL_TEMP (host/gap.c damar_gap_las; lib/pass.c takes it off)"""
    db, las = gc.INPUTS[case["input"]]
    piles = as_piles(os.path.join(gc.GOLDEN, las))
    kw = gc.opts_to_kwargs(case["opts"])
    ex = gc.tracks(case["input"])[2:] if "exclude" in kw else None
    res = gm.run(piles, q_common.db_read_len(db), stitch=kw.get("stitch", 0), exclude=ex)
    exp = gc.expected(case["name"])["cols"][:, 6]
    bad = np.flatnonzero((res.flags_array() & ~gm.TEMP) != exp)
    assert len(bad) == 0, "flags differ in records %s" % bad[:8]
    assert model_stdout(piles["pile_aread"], res) == case["stdout"]


@pytest.mark.parametrize("key", list(KW))
def test_model_gives_the_reference_on_the_shapes(fixture, key):
    every, rl, js, exp = fixture
    S = [s for s in every if not s.api_only]
    assert [(s.tag, s.aread, len(s.recs)) for s in S] == [(d["tag"], d["aread"], d["nrec"]) for d in js["shapes"]]
    piles, _, ex = gs.arrays(S, rl)
    res = run_model(piles, rl, ex, KW[key])
    bad = np.flatnonzero((res.flags_array() & ~gm.TEMP) != exp["flags_" + key])
    assert len(bad) == 0, "flags differ in records %s" % bad[:8]
    assert model_stdout(piles["pile_aread"], res) == js["stdout"][key]
    for d, ev in zip(js["shapes"], res.events):
        assert gm.lines(d["aread"], ev) == d["lines"][key], d["tag"]


def test_shapes_sit_on_their_borders(fixture):
    every, rl, _, _ = fixture
    S = [s for s in every if not s.refused]
    gs.hold_to_borders(S, gs.model_runs(S, rl))
    nb = lambda s: (s.alen + 100) // 100
    assert {nb(s) for s in S} >= {63, 64, 65, 127, 128, 129}
    assert {len(s.ex) for s in S} >= {0, 1, 64, 65, 130}


def host_against_model(piles, rl, ex, monkeypatch, what):
    from damar_amd import api
    monkeypatch.setenv("DAMAR_PILES", "host")
    for key, kw in gs.OPTION_SETS:
        flags, events = api.pile_gaps(piles, rl, stitch=kw.get("stitch", 0), exclude=ex if kw.get("exclude") else None)
        res = run_model(piles, rl, ex, kw)
        bad = np.flatnonzero(flags != res.flags_array())
        assert len(bad) == 0, "%s, %s: flags differ in records %s" % (what, key, bad[:8])
        for p, (h, m) in enumerate(zip(events, res.events)):
            assert h == m, "%s, %s: pile %d (read %d): %s against %s" % (what, key, p, piles["pile_aread"][p], h, m)
        assert len(events) == len(res.events)


def test_host_routine_gives_the_model_on_the_shapes(fixture, monkeypatch):
    every, rl, _, _ = fixture
    piles, _, ex = gs.arrays([s for s in every if not s.refused], rl)
    host_against_model(piles, rl, ex, monkeypatch, "shapes")


def test_host_routine_gives_the_model_on_random_piles(monkeypatch):
    piles, rl, ex = gs.random_piles()
    n = np.diff(piles["pile_off"])
    assert 120 <= len(n) <= 180 and n.min() >= 1 and n.max() <= 300 and 200 < n.max()
    assert len(piles["abpos"]) + sum(len(s.recs) for s in gs.shapes()) < 20000
    assert all(np.any(piles["flags"] & bit) for bit in (gm.COMP, gm.DISCARD, gm.STITCH, gm.TEMP, gm.CONT, gm.GAP, gm.TRIM))
    host_against_model(piles, rl, ex, monkeypatch, "random piles")


def test_host_routine_gives_the_model_on_the_planted_file(monkeypatch):
    piles = as_piles(os.path.join(gc.GDIR, "synth.las"))
    host_against_model(piles, q_common.db_read_len("tiny2"), gc.tracks("gsynth")[2:], monkeypatch, "synth.las")


def test_a_live_record_past_its_read_is_refused(fixture, monkeypatch):
    """e and e0 are held to nb by the kernel; no input damar_gap_inputs_valid admits reaches that (e <= (len - 450) / 100 <
    nb), so the shape that shows an e left free is one the call refuses: the check is what the kernel's bins rely on"""
    from damar_amd import api
    every, rl, _, _ = fixture
    piles, _, _ = gs.arrays([s for s in every if s.refused], rl)
    monkeypatch.setenv("DAMAR_PILES", "host")
    with pytest.raises(RuntimeError):
        api.pile_gaps(piles, rl)


def test_every_mutant_is_caught_by_a_named_shape(fixture):
    """Each mutant is the model with one border of the kernel got wrong.  It must differ from the model in flags, events or
    in who does the pile on at least one deterministic shape: a mutant that none catches means a shape is missing."""
    every, rl, _, _ = fixture
    piles, _, ex = gs.arrays(every, rl)
    off, limits = piles["pile_off"], (4096, 16)
    base = {key: run_model(piles, rl, ex, kw) for key, kw in gs.OPTION_SETS}
    missed = []
    for m in gm.MUTANTS:
        caught = []
        for key, kw in gs.OPTION_SETS:
            r, b = run_model(piles, rl, ex, kw, mutant=m), base[key]
            rh, bh = r.on_host(limits, m), b.on_host(limits)
            for p, s in enumerate(every):
                if (r.flags[off[p]:off[p + 1]] != b.flags[off[p]:off[p + 1]] or r.events[p] != b.events[p] or rh[p] != bh[p]) \
                        and s.tag not in caught:
                    caught.append(s.tag)
        print("%-16s caught by %s" % (m, ", ".join(caught) if caught else "no shape"))
        if not caught:
            missed.append(m)
    assert not missed, "no shape tells the model from: %s" % ", ".join(missed)
