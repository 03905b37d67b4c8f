"""LAcorrect without a GPU (DAMAR_PILES=host): the command against every fixture case of tests/golden/correct/ (made by the
reference, see make_correct_golden.py) and its error runs; the host routine on seeded random tiles against what any
consensus of these tiles has to satisfy."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import correct_common as cc                            # noqa: E402

HOST = dict(DAMAR_PILES="host")
CASES = cc.load_cases()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_command_matches_reference(case, tmp_path):
    cc.run_case(case, str(tmp_path), HOST, timeout_s=120)


@pytest.mark.parametrize("case", [c for c in CASES if c["name"] in ("plain_synth", "j3_synth", "plain_tiny_s")], ids=lambda c: c["name"])
def test_command_in_small_batches(case, tmp_path):
    cc.run_case(case, str(tmp_path), dict(HOST, DAMAR_PILE_BATCH="40", DAMAR_CORRECT_THREADS="3"), timeout_s=120)


@pytest.mark.parametrize("err", cc.load_cases("errors"), ids=lambda e: e["name"])
def test_error_runs(err, tmp_path):
    cc.workdir(str(tmp_path), "tiny_s")
    r = cc.run_tool([], str(tmp_path), HOST, timeout_s=60, args=err["args"])
    assert (r.returncode, r.stdout, r.stderr) == (err["rc"], err["stdout"], err["stderr"])


def test_partition_past_its_offsets_is_refused(tmp_path):
    """-j 7 on 3004 records: the reference's partition_overlaps writes a ninth offset into eight; here a message and 1"""
    cc.workdir(str(tmp_path), "tiny_s")
    import q_common
    novl = len(q_common.read_las(os.path.join(str(tmp_path), cc.LAS))["tlen"])
    parts = next(p for p in range(2, 64) if -(-novl // (novl // p)) > p + 1)
    r = cc.run_tool(["-j", str(parts)], str(tmp_path), HOST, timeout_s=60)
    assert r.returncode == 1 and r.stdout == "" and r.stderr.count("\n") == 1 and "partition" in r.stderr


def same_calls(got, calls):
    cons, added = got
    assert list(added) == [c[1] for c in calls]
    bad = [i for i, c in enumerate(calls) if not np.array_equal(cons[i], c[0])]
    assert not bad, "tiles %s differ from the model" % bad[:8]


@pytest.mark.parametrize("which", ["random", "planted"])
def test_host_routine_equals_model(which, monkeypatch):
    """consensus and `added` per tile, on the 200 seeded random tiles and on every tile of the planted piles"""
    from damar_amd import api
    monkeypatch.setenv("DAMAR_PILES", "host")
    tiles, calls = cc.model_calls(which)
    same_calls(api.tile_consensus(tiles), calls)
    assert api.correct_last()[1:3] == (len(tiles), 0)


def test_model_equals_reference_on_planted_piles():
    """the model's layout and consensus against the reference's FASTA of the planted file: correctionq and the bases of
    every corrected read, the bad trace points, the plants' `added` values"""
    case = next(c for c in CASES if c["name"] == "plain_synth")
    fasta = bytes(cc.expected("plain_synth")["fasta_out.00.fasta"])
    recs = {b.split(b" ")[0].decode(): (b.partition(b"\n")[0].decode(), b.partition(b"\n")[2].replace(b"\n", b"")) for b in fasta.split(b">")[1:]}
    _, calls = cc.model_calls("planted")
    at, serial = 0, 0
    for p in cc.planted_piles():
        if p["bad"] is not None:
            assert "ERROR: bad pt points ovl %d aread %d bread %d\n" % (p["bad"], p["aread"], p["bad_bread"]) in case["stdout"]
            assert "copy.%d" % p["aread"] in recs
            continue
        mine = calls[at:at + len(p["tiles"])]
        at += len(p["tiles"])
        head, bases = recs["%d.%d" % (p["aread"], serial)]
        serial += 1
        assert "correctionq=" + ",".join("%d,%d" % (len(c[0]), c[1]) for c in mine) in head.split(" postrace=")[0] + " "
        assert bases == b"".join(bytes(b"acgt"[x] for x in c[0]) for c in mine), p["aread"]
    added = {p["aread"]: p for p in cc.planted_piles()}
    for tag, pl in cc.load_cases("plants").items():
        for tile, n in pl.get("added", {}).items():
            assert len(added[pl["aread"]]["tiles"][int(tile)]) == n, (tag, tile)


def test_reads_the_database_does_not_have(tmp_path):
    tmp = cc.workdir(str(tmp_path), "tiny2")
    cc.tc.foreign_aread(os.path.join(tmp, cc.LAS), cc.tc.nreads_of("tiny2"))
    r = cc.run_tool([], tmp, HOST)
    assert (r.returncode, r.stdout, r.stderr) == (1, "", cc.tc.FOREIGN)
