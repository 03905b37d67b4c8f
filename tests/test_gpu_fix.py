"""LAfix on the device path (kernels/pile_patch.hip) against the fixtures the reference's LAfix left in tests/golden/fix/,
and damar_pile_patches on every input against the plain routine of host/fix.c, repair for repair."""
import os

import numpy as np
import pytest

import fix_common as fc

pytestmark = pytest.mark.gpu
CASES = fc.load_cases()
DROP = ("DAMAR_PILES", "DAMAR_TEST_FIX_SEGS", "DAMAR_PILE_BATCH")


@pytest.fixture(autouse=True)
def device_path(monkeypatch):
    for k in DROP:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def inputs():
    out = {}
    for inp in fc.REAL + ("fsynth",):
        batch, rl = fc.batch_of(inp)
        tr = fc.tracks(inp)
        out[inp] = (batch, rl, tr, fc.trims_of(batch, rl, tr["trim"]))
    return out


def both_paths(inp, inputs, monkeypatch, **kw):
    from damar_amd import api
    batch, rl, tr, trims = inputs[inp]
    dev = api.pile_patches(batch, rl, trims, tr["q"], **kw)
    last = api.fix_last()
    monkeypatch.setenv("DAMAR_PILES", "host")
    host = api.pile_patches(batch, rl, trims, tr["q"], **kw)
    monkeypatch.delenv("DAMAR_PILES")
    assert len(dev) == len(host)
    for i, (d, h) in enumerate(zip(dev, host)):
        assert d == h, "pile %d (read %d): %s against %s" % (i, batch["pile_aread"][i], d[:3], h[:3])
    return host, last


def host_piles_of(inp):
    """the piles damar_pile_patches may leave to the host routine: the one pile the planted file holds with more
    candidates than the kernel's list, and none anywhere else"""
    return 1 if inp == "fsynth" else 0


@pytest.mark.parametrize("inp", fc.REAL + ("fsynth",))
@pytest.mark.parametrize("kw", [dict(), dict(low_q=fc.load_cases("q_picked")), dict(low_coverage=True), dict(rep=True)],
                         ids=["def", "Q", "l", "r"])
def test_patches_match_the_host_routine(inp, kw, inputs, monkeypatch):
    kw = dict(kw)
    if kw.pop("rep", False):
        kw["repeats"] = inputs[inp][2]["rep"]
    host, (ms, npiles, host_piles, ngaps) = both_paths(inp, inputs, monkeypatch, **kw)
    assert (npiles, host_piles, ngaps) == (len(host), host_piles_of(inp), sum(len(g) for g in host))
    assert ms["kernel"] > 0


def test_segment_limit_leaves_only_the_longest_read(inputs, monkeypatch):
    batch, rl, _, _ = inputs["fsynth"]
    nsegs = (rl[batch["pile_aread"]] + fc.TW - 1) // fc.TW
    limit = int(np.sort(nsegs)[-2])
    plants = fc.load_cases("plants")
    assert int(np.sum(nsegs > limit)) == 1 and int(batch["pile_aread"][np.argmax(nsegs)]) == plants["longest"]["aread"]
    monkeypatch.setenv("DAMAR_TEST_FIX_SEGS", str(limit))
    host, (_, _, host_piles, _) = both_paths("fsynth", inputs, monkeypatch)
    assert host_piles == 2              # that one, and the one with too many candidates
    assert [x["b"] for x in host[int(np.argmax(nsegs))]] == [plants["longest"]["winner"]]


def test_lane_stride_plants(inputs):
    """piles of 64, 65 and 129 records with the winner in the last stride, and two equal winners in different strides"""
    from damar_amd import api
    batch, rl, tr, trims = inputs["fsynth"]
    got = api.pile_patches(batch, rl, trims, tr["q"])
    plants = fc.load_cases("plants")
    by_read = {int(a): g for a, g in zip(batch["pile_aread"], got)}
    for tag in ("n64", "n65", "n129", "tie_strides", "border_exact", "partial_start", "comp_winner", "border_edges", "longest"):
        pl = plants[tag]
        assert [x["b"] for x in by_read[pl["aread"]]] == [pl["winner"]], tag
    assert by_read[plants["border_short"]["aread"]] == []
    edge = by_read[plants["border_edges"]["aread"]]
    assert [x["support"] for x in edge] == [plants["border_edges"]["support"]]
    assert api.fix_last()[2] == 1


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_tool_case_and_host_count(case, tmp_path):
    """the command on the device path against the fixture, then the same run through api.fix_las, which shows the count the
    command does not: the host routine does the planted pile with too many candidates and no other pile of any case"""
    from damar_amd import api
    tmp = str(tmp_path)
    fc.run_case(case, tmp, timeout_s=120, drop=DROP)
    p = lambda f: os.path.join(tmp, f)
    kw = fc.opts_to_kwargs(case["opts"])
    kw.pop("trim_out", None)
    st = api.fix_las(p("G"), p(fc.LAS), p("api.fasta"), **kw)
    assert fc.md5(p("api.fasta")) == case["md5"], case["name"]
    assert st["host_piles"] == host_piles_of(case["input"]), (case["name"], st)


@pytest.mark.parametrize("case", [c for c in CASES if c["input"] in ("fsynth", "tiny2")], ids=lambda c: c["name"])
def test_small_batches_give_the_same(case, tmp_path):
    """the device path with batches of 40 records: a slot offset per pile of every batch"""
    fc.run_case(case, str(tmp_path), {"DAMAR_PILE_BATCH": "40"}, timeout_s=120, drop=DROP)


@pytest.mark.parametrize("batch", [None, "40"])
def test_sanity_exits(batch, tmp_path):
    """a read that fails one of the reference's two checks ends the run after the reads before it are written, whole and in
    small batches (the batch is cut short at the read)"""
    tmp = fc.workdir(str(tmp_path), "tiny2")
    for e in fc.load_cases("errors"):
        if e["md5"] is None:
            continue
        r = fc.run_tool([], tmp, {"DAMAR_PILE_BATCH": batch} if batch else None, timeout_s=120, args=e["args"], drop=DROP)
        assert (r.returncode, r.stdout, r.stderr) == (e["rc"], e["stdout"], e["stderr"]), e["name"]
        assert fc.md5(os.path.join(tmp, fc.OUT)) == e["md5"], e["name"]
