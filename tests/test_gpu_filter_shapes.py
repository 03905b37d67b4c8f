"""kernels/pile_filter.hip against the model of the method (tests/filter_model.py) on the shapes of tests/filter_shapes.py, which
sit on the kernel's borders (64 lanes, 64 records of a run, 1024 repeat values, words of 32 coverage bits, two-byte traces), and
on seeded random piles: all eight outputs and the count of piles left to the host routine, exactly; whole, in slices, with few
workgroups (DAMAR_TEST_FILTER_GRID) and with the two limits lowered."""
import json
import os

import numpy as np
import pytest

import filter_common as fc
import filter_model as fm
import filter_shapes as fs

pytestmark = pytest.mark.gpu
DROP = ("DAMAR_PILES", "DAMAR_TEST_FILTER_LEN", "DAMAR_TEST_FILTER_GROUP", "DAMAR_TEST_FILTER_GRID", "DAMAR_PILE_BATCH")
NAMES = ("flags", "aepos", "bepos", "diffs", "tlen", "reason", "cont_by", "cnt")


@pytest.fixture(autouse=True)
def device_path(monkeypatch):
    for k in DROP:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def shapes():
    js = json.load(open(os.path.join(fc.FDIR, "shapes.json")))
    assert fs.digest() == js["sha256"], "tests/filter_shapes.py changed: run tests/golden/make_filter_shapes_golden.py"
    return fs.shapes(), fs.shapes200(), fs.read_len()


@pytest.fixture(scope="module")
def random_piles():
    return fs.random_piles()


def device_against_model(batch, rl, key, what, host_piles, model=None):
    """one call on the device path: the eight outputs against the model, the count of host piles against `host_piles`"""
    from damar_amd import api
    kw = fs.params(key)
    dev = api.pile_filter(batch, rl, **kw)
    ms, npiles, on_host, _ = api.filter_last()
    model = fm.run_batch(batch, rl, **kw) if model is None else model
    print("%s, %s: %d piles, %d records, kernel %.3f ms" % (what, key, npiles, len(dev["flags"]), ms["kernel"]))
    for k in NAMES:
        bad = np.flatnonzero(np.any(dev[k] != model[k], axis=1) if k == "cnt" else dev[k] != model[k])
        assert len(bad) == 0, "%s, %s: %s differs in %d places, the first %d: %s against the model's %s" % (
            what, key, k, len(bad), bad[0], dev[k][bad[0]], model[k][bad[0]])
    assert (npiles, on_host) == (len(batch["pile_aread"]), host_piles), (what, key)
    return model


def test_limits_are_the_shapes():
    from damar_amd import api
    assert api.filter_limits() == (fs.GROUP, 400000) and fs.WAVE == 64


@pytest.mark.parametrize("key", list(fs.OPTION_SETS))
def test_shapes_match_the_model(shapes, key):
    S, _, rl = shapes
    gone = fs.on_host(S, key)
    assert [s.tag for s, h in zip(S, gone) if h] == ["run65_at63"]         # the host routine does the run of 65 and no other pile
    model = device_against_model(fs.arrays(S), rl, key, "shapes", 1)
    fs.check_letters(S, key, model["flags"])


@pytest.mark.parametrize("key", list(fs.SETS_200))
def test_two_byte_traces_match_the_model(shapes, key):
    _, S, rl = shapes
    batch = fs.arrays(S)
    assert batch["tbytes"] == 2 and batch["trace"].view("<u2").max() > 255
    model = device_against_model(batch, rl, key, "spacing 200", 0)
    fs.check_letters(S, key, model["flags"])


@pytest.mark.parametrize("key", list(fs.RANDOM_SETS))
def test_random_piles_match_the_model(random_piles, key):
    batch, rl = random_piles
    over = sum(fs.runs_over(batch))
    assert over > 0
    device_against_model(batch, rl, key, "random piles", over)


@pytest.mark.parametrize("grid", [1, 3, 7])
def test_a_workgroup_takes_several_piles(shapes, grid, monkeypatch):
    """s_rep, s_mask and the counters reused from pile to pile: every shape followed by, in turn, the read of 513 intervals
    (its values stay in HBM), one of a single interval, the coverage pile of 2048 bases, the one of 33, the run of 65 a
    workgroup passes over, and a pile of one record"""
    S, _, rl = shapes
    by = {s.tag: s for s in S}
    special = [by[t] for t in ("rep_513", "rep_1", "zu_word", "zu_len33", "run65_at63", "div_d_0")]
    order = []
    for i, s in enumerate(S):
        order += [s, special[i % len(special)]]
    batch = fs.arrays(order)
    monkeypatch.setenv("DAMAR_TEST_FILTER_GRID", str(grid))
    for key in ("plan", "nY", "zu", "R46"):
        gone = fs.on_host(order, key)
        assert {s.tag for s, h in zip(order, gone) if h} == {"run65_at63"}
        device_against_model(batch, rl, key, "grid %d" % grid, sum(gone))


@pytest.mark.parametrize("step", [1, 2, 50])
def test_slices_give_the_same_as_the_whole(shapes, step):
    S, _, rl = shapes
    for key in ("R6s", "zu"):
        whole = fm.run_batch(fs.arrays(S), rl, **fs.params(key))
        parts = []
        for at in range(0, len(S), step):
            part = S[at:at + step]
            parts.append(device_against_model(fs.arrays(part), rl, key, "piles %d..%d" % (at, at + len(part) - 1), sum(fs.on_host(part, key))))
        for k in NAMES:
            assert np.array_equal(np.concatenate([m[k] for m in parts]), whole[k]), (key, k)


def test_lowered_limits_move_the_named_shapes(shapes, monkeypatch):
    """DAMAR_TEST_FILTER_GROUP=63 sends the runs of 64 to the host routine as well; DAMAR_TEST_FILTER_LEN=2048 the reads of
    2049 and 2080 bases, not those of 2048, and only under -z with -u, which alone needs the coverage bits.  Pile by pile, in
    calls of one pile each: what the count of one call cannot show."""
    from damar_amd import api
    S, _, rl = shapes
    longer = {s.tag for s in S if s.alen > 2048}                       # the coverage shapes among them, and every pile on 3000 or 8000 bases
    assert longer >= {"zu_w63_64_32", "zu_w63_64_33", "zu_len2049"} and not longer & {"zu_word", "zu_len2047", "zu_trim_0_0_at", "zu_len33"}
    for env, value, key, limits, want in (
            ("DAMAR_TEST_FILTER_GROUP", "63", "s", dict(group=63), {"run64_at63", "run64_at64", "run64_at1", "run65_at63"}),
            ("DAMAR_TEST_FILTER_LEN", "2048", "zu", dict(maxlen=2048), longer | {"run65_at63"}),
            ("DAMAR_TEST_FILTER_LEN", "2048", "wz", dict(maxlen=2048), {"run65_at63"})):
        monkeypatch.setenv(env, value)
        gone = fs.on_host(S, key, **limits)
        assert {s.tag for s, h in zip(S, gone) if h} == want
        device_against_model(fs.arrays(S), rl, key, "%s=%s" % (env, value), len(want))
        kw = fs.params(key)
        for s, h in zip(S, gone):
            api.pile_filter(fs.arrays([s]), rl, **kw)
            assert api.filter_last()[2] == int(h), (env, s.tag)
        monkeypatch.delenv(env)
