"""DBdust without a GPU (DAMAR_DUST=host): the command and the routine of host/dust.c against the reference's recorded
tracks (tests/golden/dust/, made by tests/golden/make_dust_golden.py), the routine run in pieces against itself run over
whole reads, and against the plain model of tests/dust_model.py."""
import numpy as np
import pytest

import dust_common as dc
import dust_model

HOST = {"DAMAR_DUST": "host"}


@pytest.fixture(scope="module")
def planted(built):
    return dc.db_reads(dc.DUST, "P")


@pytest.fixture(scope="module")
def synthetic():
    return dc.synthetic_reads()


@pytest.mark.parametrize("name", list(dc.OPTION_SETS))
def test_command_equals_reference(name, built, tmp_path):
    dc.check_option_set(name, str(tmp_path), HOST)


def test_command_equals_reference_on_mask_dust_blocks(built, tmp_path):
    dc.check_mask_dust(str(tmp_path), HOST)


def test_command_appends_as_reference(built, tmp_path):
    st = dc.check_append(str(tmp_path), HOST)
    assert st["reads"] == 2                     # only the reads beyond the track


@pytest.mark.parametrize("name", list(dc.ERROR_RUNS))
def test_error_runs_are_the_references(name, built, tmp_path):
    dc.planted_workdir(str(tmp_path))
    r = dc.run_dbdust(dc.ERROR_RUNS[name], str(tmp_path), HOST)
    assert ("%s\nrc %d\n" % (r.stderr, r.returncode)).encode() == dc.expected("errors")[name]
    assert dc.dust_files(str(tmp_path)) == {}


def test_dam_is_refused(built, tmp_path):
    open(str(tmp_path / "D.dam"), "w").write("files = 0\n")
    for arg in ("D", "D.dam"):
        r = dc.run_dbdust([arg], str(tmp_path), HOST)
        assert r.returncode == 1 and len(r.stderr.strip().split("\n")) == 1 and ".dam" in r.stderr


@pytest.mark.parametrize("name", [k for k in dc.OPTION_SETS if k not in dc.ERROR_SETS])
def test_routine_equals_reference(name, planted, built):
    from damar_amd import api
    reads, freq = planted
    kw = dc.kwargs_of(dc.OPTION_SETS[name])
    if kw.get("biased"):
        kw["freq"] = freq
    exp = dc.expected(name)
    want = dc.track_intervals(exp[".P.dust.anno"], exp[".P.dust.data"])
    for r, w in zip(reads, want):
        assert np.array_equal(api.dust_host_read(r, **kw)[0], w)


def _pieces_equal_whole(reads, w, t):
    from damar_amd import api
    for r in reads:
        whole = api.dust_host_read(r, window=w, thresh=t, minlen=2)[0]
        for piece in (w, 333, api.dust_limits()[0]):
            cut = api.dust_host_read(r, window=w, thresh=t, minlen=2, piece=piece, halo=2 * w)[0]
            assert np.array_equal(whole, cut), (len(r), w, t, piece)


@pytest.mark.parametrize("w", [16, 32, 64])
@pytest.mark.parametrize("t", [1.5, 2.0, 3.5])
def test_pieces_equal_whole_reads_synthetic(w, t, synthetic, built):
    _pieces_equal_whole(synthetic, w, t)


@pytest.mark.parametrize("w", [16, 32, 64])
def test_pieces_equal_whole_reads_fixtures(w, planted, built):
    _pieces_equal_whole(planted[0] + dc.db_reads(dc.MASK_DUST, "G")[0], w, 2.0)


def test_pieces_without_halo_differ(synthetic, built):
    """the check above can fail: with nothing run in front of a piece some reads come out different"""
    from damar_amd import api
    differ = sum(not np.array_equal(api.dust_host_read(r, minlen=2)[0], api.dust_host_read(r, minlen=2, piece=64, halo=0)[0])
                 for r in synthetic[:100])
    assert differ > 0


def test_model_equals_routine_on_planted_reads(planted, built):
    from damar_amd import api
    longest = 0
    for r in planted[0]:
        seq = [int(x) for x in r]
        cands, n = dust_model.candidates(seq)
        got, m = api.dust_host_candidates(r)
        assert [tuple(x) for x in got.tolist()] == cands and n == m
        assert [tuple(x) for x in api.dust_host_read(r)[0].tolist()] == dust_model.join(cands)
        longest = max(longest, n)
    assert longest == dc.cases()["longest_candidate_list"]
