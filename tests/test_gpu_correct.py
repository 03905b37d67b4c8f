"""LAcorrect on the GPU: the command on the device path against the fixture cases of tests/golden/correct/ (made by the
reference), whole and in small batches of piles; api.tile_consensus against the host routine tile for tile, at the built
limits and at lowered ones; the tiles the host routine does beside the kernel, counted."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import correct_common as cc                            # noqa: E402

pytestmark = pytest.mark.gpu
CASES = cc.load_cases()
DROP = ("DAMAR_PILES",)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_command_matches_reference(case, tmp_path):
    cc.run_case(case, str(tmp_path), timeout_s=120, drop=DROP)


@pytest.mark.parametrize("case", [c for c in CASES if c["name"] in ("plain_synth", "j3_synth", "plain_tiny_s")], ids=lambda c: c["name"])
def test_command_in_small_batches(case, tmp_path):
    cc.run_case(case, str(tmp_path), dict(DAMAR_PILE_BATCH="40"), timeout_s=120, drop=DROP)


def same_calls(got, calls):
    cons, added = got
    assert list(added) == [c[1] for c in calls]
    bad = [i for i, c in enumerate(calls) if not np.array_equal(cons[i], c[0])]
    assert not bad, "tiles %s differ" % bad[:8]


def host_count(calls, limits):
    return sum(cc.over(c[2], limits) for c in calls if c[1] > 0)


@pytest.mark.parametrize("which", ["random", "planted"])
def test_kernel_equals_host_routine_and_model(which, monkeypatch):
    """tile for tile, and the host routine does exactly the tiles that the model finds beyond the built limits"""
    from damar_amd import api
    monkeypatch.delenv("DAMAR_PILES", raising=False)
    tiles, calls = cc.model_calls(which)
    got = api.tile_consensus(tiles)
    _, ntiles, nhost, nbases = api.correct_last()
    monkeypatch.setenv("DAMAR_PILES", "host")
    want = api.tile_consensus(tiles)
    assert list(got[1]) == list(want[1]) and all(np.array_equal(x, y) for x, y in zip(got[0], want[0]))
    same_calls(got, calls)
    assert (ntiles, nbases) == (len(tiles), sum(len(c[0]) for c in calls))
    assert nhost == host_count(calls, api.correct_limits())
    if which == "planted":
        assert nhost == next(c for c in CASES if c["name"] == "plain_synth")["host_tiles"] > 0
    else:
        assert nhost == 0


def test_tiles_beyond_the_limits_go_to_the_host(monkeypatch):
    """every sequence holds 20 bases at the least: with room for 18 columns no tile fits; with room for 120 or for
    cc.LOW_COLS exactly the tiles whose profile the model sees grow beyond that; a sequence one base over the limit"""
    from damar_amd import api
    monkeypatch.delenv("DAMAR_PILES", raising=False)
    seg, cols, cells = api.correct_limits()
    for which, low in (("random", 18), ("random", 120), ("planted", cc.LOW_COLS)):
        tiles, calls = cc.model_calls(which)
        monkeypatch.setenv("DAMAR_TEST_CORRECT_COLS", str(low))
        same_calls(api.tile_consensus(tiles), calls)
        assert api.correct_last()[2] == host_count(calls, (seg, low, cells)) > 0
        if low == 18:
            assert api.correct_last()[2] == sum(c[1] > 0 for c in calls)
    monkeypatch.delenv("DAMAR_TEST_CORRECT_COLS")
    rng = np.random.default_rng(3)
    long_one = [[rng.integers(0, 4, size=seg + 1).astype(np.uint8)] * 3, [rng.integers(0, 4, size=seg).astype(np.uint8)] * 3, []]
    cons, added = api.tile_consensus(long_one)
    assert api.correct_last()[2] == 1 and list(added) == [3, 3, 0]
    assert np.array_equal(cons[0], long_one[0][0]) and np.array_equal(cons[1], long_one[1][0]) and len(cons[2]) == 0


@pytest.mark.parametrize("low", [None, cc.LOW_COLS])
def test_planted_file_counts_its_host_tiles(low, tmp_path, monkeypatch):
    """the pass over the planted file: the reference's FASTA, and the host routine did exactly the planted tiles beyond the
    limits, as the generator counted them with the model (at the built column limit, and at the lowered one)"""
    import fix_common as fc
    from damar_amd import api
    monkeypatch.delenv("DAMAR_PILES", raising=False)
    if low is not None:
        monkeypatch.setenv("DAMAR_TEST_CORRECT_COLS", str(low))
    case = next(c for c in CASES if c["name"] == "plain_synth")
    tmp = cc.workdir(str(tmp_path), case["input"])
    st = api.correct_las(os.path.join(tmp, "G"), os.path.join(tmp, cc.LAS), os.path.join(tmp, cc.OUT))
    assert st["host_tiles"] == case["host_tiles" if low is None else "host_tiles_low_cols"]
    assert fc.md5(os.path.join(tmp, cc.OUT + ".00.fasta")) == case["md5"][cc.OUT + ".00.fasta"]
