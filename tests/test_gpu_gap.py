"""LAgap on the device path (kernels/pile_gaps.hip, and kernels/box_align.hip under -t) against the fixtures the reference's
LAgap left in tests/golden/gap/, and damar_pile_gaps on the planted piles against the plain routine of host/gap.c."""
import os

import numpy as np
import pytest

import gap_common as gc
import q_common

pytestmark = pytest.mark.gpu
CASES = gc.load_cases()
DROP = ("DAMAR_PILES", "DAMAR_TRIM", "DAMAR_TEST_GAP_BINS", "DAMAR_TEST_GAP_GRID", "DAMAR_TEST_BOX_LIMIT", "DAMAR_PILE_BATCH")


@pytest.fixture(autouse=True)
def device_path(monkeypatch):
    for k in DROP:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def planted():
    off, aread, ab, ae, bb, be, br, fl = gc.pile_arrays(os.path.join(gc.GDIR, "synth.las"))
    piles = dict(pile_off=off, pile_aread=aread, abpos=ab, aepos=ae, bbpos=bb, bepos=be, bread=br, flags=fl)
    _, _, ea, ed = gc.tracks("gsynth")
    return piles, q_common.db_read_len("tiny2"), (ea, ed)


def both_paths(piles, rl, monkeypatch, **kw):
    from damar_amd import api
    dev = api.pile_gaps(piles, rl, **kw)
    last = api.gap_last()
    monkeypatch.setenv("DAMAR_PILES", "host")
    host = api.pile_gaps(piles, rl, **kw)
    monkeypatch.delenv("DAMAR_PILES")
    assert np.array_equal(dev[0], host[0]), "flags differ in records %s" % np.flatnonzero(dev[0] != host[0])[:8]
    assert len(dev[1]) == len(host[1])
    for i, (d, h) in enumerate(zip(dev[1], host[1])):
        assert d == h, "pile %d (read %d): %s against %s" % (i, piles["pile_aread"][i], d, h)
    return host, last


@pytest.mark.parametrize("kw", [dict(), dict(stitch=100), dict(stitch=300), dict(exclude=True), dict(stitch=300, exclude=True)],
                         ids=["def", "s100", "s300", "e", "es"])
def test_planted_piles_match_the_host_routine(planted, kw, monkeypatch):
    piles, rl, ex = planted
    kw = dict(kw, exclude=ex) if kw.get("exclude") else kw
    host, (ms, npiles, host_piles, nev) = both_paths(piles, rl, monkeypatch, **kw)
    events = host[1]
    # the kernel leaves exactly the piles with more events than its slot holds: the one planted for that
    from damar_amd import api
    over = [i for i, e in enumerate(events) if len(e) > api.gap_limits()[1]]
    many = gc.load_cases("plants")["many_events"]["aread"]
    assert [int(piles["pile_aread"][i]) for i in over] == [many]
    assert (npiles, host_piles, nev) == (len(events), 1, sum(len(e) for e in events))
    assert ms["kernel"] > 0


@pytest.mark.parametrize("kw", [dict(), dict(stitch=300), dict(exclude=True), dict(stitch=300, exclude=True)], ids=["def", "s300", "e", "es"])
def test_random_piles_match_the_host_routine(kw, monkeypatch):
    import gap_shapes
    piles, rl, ex = gap_shapes.random_piles()
    kw = dict(kw, exclude=ex) if kw.get("exclude") else kw
    host, (ms, npiles, host_piles, nev) = both_paths(piles, rl, monkeypatch, **kw)
    assert (npiles, nev) == (len(host[1]), sum(len(e) for e in host[1]))


def test_bin_limit_leaves_only_the_longest_read(planted, monkeypatch):
    piles, rl, _ = planted
    nbins = (rl[piles["pile_aread"]] + 100) // 100
    limit = int(np.sort(nbins)[-2])                    # what every planted read but the longest needs
    assert int(np.sum(nbins > limit)) == 1 and int(piles["pile_aread"][np.argmax(nbins)]) == gc.load_cases("plants")["longest"]["aread"]
    monkeypatch.setenv("DAMAR_TEST_GAP_BINS", str(limit))
    _, (_, npiles, host_piles, _) = both_paths(piles, rl, monkeypatch)
    assert host_piles == 2                             # that one, and the one with too many events


def test_b_reads_out_of_order_go_to_the_host(monkeypatch):
    """The reference's containment loop skips a discarded record before it looks at its B read, so it pairs the two records
    of read 50 here across the discarded one of read 60.  The kernel takes a run of one B read for a group and would not:
    such a pile is marked and done by the host routine, and counted."""
    rl = q_common.db_read_len("tiny2")
    piles = dict(pile_off=[0, 3, 5], pile_aread=[1, 2], abpos=[0, 300, 100, 0, 100], aepos=[800, 700, 500, 800, 500],
                 bbpos=[0, 300, 100, 0, 100], bepos=[800, 700, 500, 800, 500], bread=[50, 60, 50, 50, 50], flags=[0, 2, 0, 0, 0])
    (flags, events), (_, npiles, host_piles, _) = both_paths(piles, rl, monkeypatch)
    assert [int(f) & 0x8002 for f in flags] == [0, 2, 0x8002, 0, 0x8002]       # both inner records contained, in either pile
    assert (npiles, host_piles) == (2, 1)                                      # the sorted pile stays on the device


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_tool_case_small_batches_and_host_count(case, tmp_path, monkeypatch):
    """the command on the device path, whole and in small batches, against the fixture; then the same two runs through
    api.gap_las, which shows the count the command does not: the host routine does the planted pile with too many events
    and no other pile of any case"""
    from damar_amd import api
    dev, small = os.path.join(str(tmp_path), "dev"), os.path.join(str(tmp_path), "small")
    os.makedirs(dev)
    os.makedirs(small)
    gc.run_case(case, dev, timeout_s=120, drop=DROP)
    gc.run_case(case, small, {"DAMAR_PILE_BATCH": "40"}, timeout_s=120, drop=DROP)
    r = gc.lacheck(dev)
    assert r.returncode == 0, r.stdout + r.stderr
    p = lambda f: os.path.join(dev, f)
    for batch in (None, "40"):
        if batch:
            monkeypatch.setenv("DAMAR_PILE_BATCH", batch)
        st = api.gap_las(p("G"), p(gc.LAS), p("api.las"), **gc.opts_to_kwargs(case["opts"]))
        assert gc.tc.md5(p("api.las")) == case["md5"], (case["name"], batch)
        assert st["host_piles"] == gc.host_piles_of(case["input"]), (case["name"], batch, st)
