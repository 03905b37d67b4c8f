"""The model of LAfilter's method (tests/filter_model.py) against what the reference made of the shapes of
tests/filter_shapes.py (tests/golden/filter/shapes_expected.npz), the host routine (host/filter.c, DAMAR_PILES=host) against the
model on the shapes and on seeded random piles, all eight outputs, and the shapes against the model's mutants: every border of
kernels/pile_filter.hip got wrong shows on the shape named for it."""
import json
import os

import numpy as np
import pytest

import filter_common as fc
import filter_model as fm
import filter_shapes as fs

NAMES = ("flags", "aepos", "bepos", "diffs", "tlen", "reason", "cont_by", "cnt")
WORDS = dict(tlen=0, diffs=1, aepos=4, bepos=5, flags=6)
SETS = [("t100", k) for k in fs.OPTION_SETS] + [("t200", k) for k in fs.SETS_200]
# the shapes that must tell each mutant of the model from the model
CAUGHT_BY = dict(r4_single_count="r4_first_none", stitch_first="two_cand_63", z_enter_lt="zu_word", z_leave_gt="zu_word", z_bases_lt="z_mean_2",
                 z_uncovered_ge="zu_bit31_32", cover_end_bit="zu_w63_64_32", cover_outside_trim="zu_before_tb", w_skips_last="w_63_65",
                 cont_by_first="r6_by_63", b_last_segment="t2_b", one_byte_trace="t2_r2")


@pytest.fixture(scope="module")
def fixture():
    """the shapes rebuilt, held against the sha256 the generator left: fixture and code cannot part company"""
    js = json.load(open(os.path.join(fc.FDIR, "shapes.json")))
    assert fs.digest() == js["sha256"], "tests/filter_shapes.py changed: run tests/golden/make_filter_shapes_golden.py"
    sets = dict(t100=fs.shapes(), t200=fs.shapes200())
    return sets, {k: fs.arrays(S) for k, S in sets.items()}, fs.read_len(), js, np.load(os.path.join(fc.FDIR, "shapes_expected.npz"))


def differ(got, want, what):
    for k in NAMES:
        bad = np.flatnonzero(np.any(got[k] != want[k], axis=1) if k == "cnt" else got[k] != want[k])
        assert len(bad) == 0, "%s: %s differs in %d places, the first %d: %s against %s" % (what, k, len(bad), bad[0], got[k][bad[0]], want[k][bad[0]])


def test_the_fixture_lists_the_shapes(fixture):
    sets, _, _, js, _ = fixture
    every = sets["t100"] + sets["t200"]
    assert [(s.tag, s.aread, len(s.recs), s.tspace, s.over, s.expect) for s in every] == \
        [(d["tag"], d["aread"], d["nrec"], d["tspace"], d["over"], d["letters"]) for d in js["shapes"]]
    assert [s.tag for s in every if s.over] == ["run65_at63"]
    assert {s.alen for s in every} >= {33, 64, 2047, 2048, 2049, 2080}
    assert {len(s.rep) for s in every} >= {0, 511, 512, 513}
    assert sum(len(s.recs) for s in every) < 5000


@pytest.mark.parametrize("name,key", SETS, ids=["%s_%s" % s for s in SETS])
def test_model_gives_the_reference_on_the_shapes(fixture, name, key):
    sets, batches, rl, _, exp = fixture
    b = batches[name]
    cols = {0: b["tlen"].copy(), 1: b["diffs"].copy(), 4: b["aepos"].copy(), 5: b["bepos"].copy(), 6: b["flags"].copy()}
    for k in fc.LOOSE:
        cols[k][exp["%s:%s:i%d" % (name, key, k)]] = exp["%s:%s:v%d" % (name, key, k)]
    fs.check_letters(sets[name], key, cols[6])
    model = fm.run_batch(b, rl, **fs.params(key))
    for w, k in WORDS.items():
        bad = np.flatnonzero(model[w] != cols[k])
        assert len(bad) == 0, "%s differs in records %s" % (w, bad[:8])


@pytest.mark.parametrize("name,key", SETS, ids=["%s_%s" % s for s in SETS])
def test_host_routine_gives_the_model_on_the_shapes(fixture, name, key, monkeypatch):
    from damar_amd import api
    _, batches, rl, _, _ = fixture
    monkeypatch.setenv("DAMAR_PILES", "host")
    kw = fs.params(key)
    differ(api.pile_filter(batches[name], rl, **kw), fm.run_batch(batches[name], rl, **kw), "%s %s" % (name, key))


@pytest.fixture(scope="module")
def random_piles():
    return fs.random_piles()


def test_random_piles_are_what_they_say(random_piles):
    batch, _ = random_piles
    n = np.diff(batch["pile_off"])
    runs = [len(r) for p in range(len(n)) for r in fm.runs([dict(b=int(x)) for x in batch["bread"][batch["pile_off"][p]:batch["pile_off"][p + 1]]])]
    assert len(n) == 40 and 1 <= n.min() and 150 < n.max() <= 200
    assert max(runs) > fs.GROUP and min(runs) == 1 and max(runs) <= 70
    assert 0 < sum(fs.runs_over(batch)) < len(n)
    assert all(np.any(batch["flags"] & bit) for bit in (fm.COMP, fm.DISCARD, fm.STITCH, fm.CONT, fm.GAP, fm.TRIM, fm.MODULE, fm.LOCAL))


@pytest.mark.parametrize("key", fs.RANDOM_SETS + ("S", "R63", "R20", "wz", "b", "sd"))
def test_host_routine_gives_the_model_on_random_piles(random_piles, key, monkeypatch):
    from damar_amd import api
    batch, rl = random_piles
    monkeypatch.setenv("DAMAR_PILES", "host")
    kw = fs.params(key)
    differ(api.pile_filter(batch, rl, **kw), fm.run_batch(batch, rl, **kw), "random piles, " + key)


def test_every_mutant_is_caught_by_the_shape_named_for_it(fixture):
    """Each mutant is the model with one border of the method got wrong.  It must differ from the model, in one of the eight
    outputs under one of the option sets, on the deterministic shape named for it in CAUGHT_BY."""
    sets, batches, rl, _, _ = fixture
    assert set(CAUGHT_BY) == set(fm.MUTANTS)
    base = {s: fm.run_batch(batches[s[0]], rl, **fs.params(s[1])) for s in SETS}
    missed = []
    for m in fm.MUTANTS:
        caught = []
        for name, key in SETS:
            r, b = fm.run_batch(batches[name], rl, mutant=m, **fs.params(key)), base[(name, key)]
            off = batches[name]["pile_off"]
            for p, s in enumerate(sets[name]):
                lo, hi = int(off[p]), int(off[p + 1])
                if s.tag not in caught and any(np.any(r[k][p] != b[k][p]) if k == "cnt" else np.any(r[k][lo:hi] != b[k][lo:hi]) for k in NAMES):
                    caught.append(s.tag)
        print("%-20s caught by %s" % (m, ", ".join(caught) if caught else "no shape"))
        if CAUGHT_BY[m] not in caught:
            missed.append(m)
    assert not missed, "the shape named does not tell the model from: %s" % ", ".join(missed)
