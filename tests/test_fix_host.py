"""LAfix on the plain host path (DAMAR_PILES=host: host/fix.c) against the fixtures the reference's LAfix left in
tests/golden/fix/: FASTA, -T file, stdout, stderr and exit status of every case, and the error runs."""
import os

import numpy as np
import pytest

import fix_common as fc

CASES = fc.load_cases()
HOST = {"DAMAR_PILES": "host"}
SMALL = dict(HOST, DAMAR_PILE_BATCH="40")


@pytest.fixture(autouse=True)
def host_path(monkeypatch):
    monkeypatch.setenv("DAMAR_PILES", "host")


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_tool_case(case, tmp_path):
    fc.run_case(case, str(tmp_path), HOST)


@pytest.mark.parametrize("case", [c for c in CASES if c["input"] in ("fsynth", "tiny2")], ids=lambda c: c["name"])
def test_small_batches_give_the_same(case, tmp_path):
    fc.run_case(case, str(tmp_path), SMALL)


def test_error_runs(tmp_path):
    tmp = fc.workdir(str(tmp_path), "tiny2")
    for e in fc.load_cases("errors"):
        r = fc.run_tool([], tmp, HOST, args=e["args"])
        assert (r.returncode, r.stdout, r.stderr) == (e["rc"], e["stdout"], e["stderr"]), e["name"]
        if e["md5"] is not None:               # the sanity exits: the reads before the one that fails are written
            assert fc.md5(os.path.join(tmp, fc.OUT)) == e["md5"], e["name"]
    r = fc.run_tool(["-X"], tmp, HOST)
    assert (r.returncode, r.stdout, r.stderr) == fc.NO_CHIMER
    r = fc.run_tool(["-f", "x.quiva"], tmp, HOST)
    assert (r.returncode, r.stdout, r.stderr) == fc.NO_QUIVA
    assert not os.path.exists(os.path.join(tmp, "x.quiva"))


def test_fixtures_do_not_lean_on_the_out_of_range_rules():
    """the generator counts, with tests/fix_model.py over every input, the q values read beyond the track's data and the
    scans that reach a read's border, asserts that there are none and says so in cases.json"""
    assert fc.load_cases("rules_seen") == dict(q_beyond_data=0, scan_hit_border=0)
    assert "no fixture's result depends" in fc.load_cases("rules_note")


PARAMS = [dict(), dict(low_q=fc.load_cases("q_picked")), dict(low_coverage=True), dict(max_gap=300), dict(max_gap=-1), dict(rep=True)]


@pytest.mark.parametrize("inp", ["fsynth", "tiny2"])
@pytest.mark.parametrize("kw", PARAMS, ids=["def", "Q", "l", "g300", "g0", "r"])
def test_pile_patches_equal_the_model(inp, kw):
    """api.pile_patches on the host path against the Python model of steps 4 to 6, repair for repair and field for field"""
    import fix_model
    from damar_amd import api
    batch, rl = fc.batch_of(inp)
    tr = fc.tracks(inp)
    kw = dict(kw)
    if kw.pop("rep", False):
        kw["repeats"] = tr["rep"]
    trims = fc.trims_of(batch, rl, tr["trim"])
    got = api.pile_patches(batch, rl, trims, tr["q"], **kw)
    want, _ = fix_model.patches(batch, rl, trims, tr["q"], **kw)
    assert len(got) == len(want)
    for a, g, w in zip(batch["pile_aread"], got, want):
        assert g == w, "read %d: %s against the model's %s" % (a, g[:3], w[:3])
    if inp == "fsynth" and not kw:
        plants = fc.load_cases("plants")
        edge = got[list(batch["pile_aread"]).index(plants["border_edges"]["aread"])]
        assert [x["support"] for x in edge] == [plants["border_edges"]["support"]]       # both inclusive edges, and no further


@pytest.mark.parametrize("name", ["c_synth", "r_synth", "Q_tiny2"])
def test_api_agrees_with_the_command(name, tmp_path, capfd):
    from damar_amd import api
    case = next(c for c in CASES if c["name"] == name)
    tmp = fc.workdir(str(tmp_path), case["input"])
    p = lambda f: os.path.join(tmp, f)
    kw = fc.opts_to_kwargs(case["opts"])
    if "trim_out" in kw:
        kw["trim_out"] = p(kw["trim_out"])
    st = api.fix_las(p("G"), p(fc.LAS), p(fc.OUT), **kw)
    assert fc.md5(p(fc.OUT)) == case["md5"]
    exp = fc.expected(name)
    assert st["reads_fixed"] + st["reads_trimmed"] == len(exp["heads"]) and st["host_piles"] == 0
    assert capfd.readouterr().out == case["stdout"]


def test_pile_patches_on_the_planted_file():
    """api.pile_patches on the host path: every plant's repairs as the fixtures' FASTA shows them (how many bases go and
    come), the winner planted for it, and nothing for a pile without a trim"""
    from damar_amd import api
    batch, rl = fc.batch_of("fsynth")
    tr = fc.tracks("fsynth")
    trims = fc.trims_of(batch, rl, tr["trim"])
    got = api.pile_patches(batch, rl, trims, tr["q"])
    plants = fc.load_cases("plants")
    by_read = {int(a): g for a, g in zip(batch["pile_aread"], got)}
    for tag, pl in plants.items():
        g = by_read[pl["aread"]]
        if "winner" in pl:
            assert [x["b"] for x in g] == [pl["winner"]], tag
        if pl["head"] == "trimmed" and "flips" not in pl:
            assert g == [], tag
    assert [x["b"] for x in by_read[plants["break_sup4"]["aread"]]] == [40]          # the sort tie: the first in the file
    assert by_read[plants["comp_winner"]["aread"]][0]["comp"] == 1
    none = api.pile_patches(batch, rl, np.zeros_like(trims), tr["q"])
    assert all(g == [] for g in none)


def test_reads_the_database_does_not_have(tmp_path):
    tmp = fc.workdir(str(tmp_path), "tiny2")
    fc.tc.foreign_aread(os.path.join(tmp, fc.LAS), fc.tc.nreads_of("tiny2"))
    r = fc.run_tool(["-t", "trim"], tmp, HOST)
    assert (r.returncode, r.stdout, r.stderr) == (1, "\x1b[32mPASS fix\x1b[0m\n", fc.tc.FOREIGN)
