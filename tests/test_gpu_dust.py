"""DBdust on the GPU (kernels/dust.hip): damar_dust_reads against the routine of host/dust.c interval for interval, the
command on the device path against the reference's recorded tracks, what the host routine is left with, and batch sizes."""
import numpy as np
import pytest

import dust_common as dc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def reads(built):
    planted, freq = dc.db_reads(dc.DUST, "P")
    return planted, dc.synthetic_reads(), freq


@pytest.fixture(scope="module")
def host_results(reads):
    """the host routine's intervals per integer option set, made once"""
    from damar_amd import api
    planted, synthetic, _ = reads
    return {name: [api.dust_host_read(r, **dc.kwargs_of(dc.OPTION_SETS[name]))[0] for r in planted + synthetic]
            for name in dc.INTEGER_SETS if name not in dc.HOST_SETS}


@pytest.mark.parametrize("name", [k for k in dc.INTEGER_SETS if k not in dc.HOST_SETS])
def test_kernel_equals_host_routine(name, reads, host_results):
    from damar_amd import api
    planted, synthetic, _ = reads
    got = api.dust_reads(planted + synthetic, **dc.kwargs_of(dc.OPTION_SETS[name]))
    _ms, n, host, nint, steps, walks = api.dust_last()
    assert (n, host) == (len(got), 0) and nint == sum(len(g) for g in got) and 0 < walks <= steps
    for i, (g, h) in enumerate(zip(got, host_results[name])):
        assert np.array_equal(g, h), (name, i)


@pytest.mark.parametrize("name", list(dc.OPTION_SETS))
def test_command_on_device(name, built, tmp_path):
    stats = dc.check_option_set(name, str(tmp_path), {}, timeout_s=120)
    for st in stats:
        assert st["host_reads"] == (st["reads"] if name in dc.HOST_SETS else 0), (name, st)


def test_command_on_device_mask_dust_blocks(built, tmp_path):
    dc.check_mask_dust(str(tmp_path), {}, timeout_s=120)


def test_command_appends_on_device(built, tmp_path):
    st = dc.check_append(str(tmp_path), {}, timeout_s=120)
    assert (st["reads"], st["host_reads"]) == (2, 0)


def test_host_routine_does_exactly_its_reads(reads, host_results, monkeypatch):
    from damar_amd import api
    planted, _synthetic, freq = reads
    exp = dc.expected("b")
    got = api.dust_reads(planted, biased=True, freq=freq)
    assert api.dust_last()[1:3] == (len(planted), len(planted))
    assert all(np.array_equal(g, w) for g, w in zip(got, dc.track_intervals(exp[".P.dust.anno"], exp[".P.dust.data"])))
    exp = dc.expected("w80")
    got = api.dust_reads(planted, window=80)
    assert api.dust_last()[1:3] == (len(planted), len(planted))
    assert all(np.array_equal(g, w) for g, w in zip(got, dc.track_intervals(exp[".P.dust.anno"], exp[".P.dust.data"])))
    # a stripe of 8 candidates: the reads with a piece that retires more are the host routine's, and no other
    piece = api.dust_limits()[0]
    over = 0
    for r in planted:
        c = api.dust_host_candidates(r)[0]
        over += bool(len(c)) and int(np.bincount(c[:, 0] // piece).max()) > 8
    assert 0 < over < len(planted)
    monkeypatch.setenv("DAMAR_TEST_DUST_STRIPE", "8")
    got = api.dust_reads(planted)
    assert api.dust_last()[1:3] == (len(planted), over)
    assert all(np.array_equal(g, h) for g, h in zip(got, host_results["default"]))
    monkeypatch.delenv("DAMAR_TEST_DUST_STRIPE")
    api.dust_reads(planted)
    assert api.dust_last()[1:3] == (len(planted), 0)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_batch_sizes(n, reads, host_results):
    from damar_amd import api
    planted, synthetic, _ = reads
    at = len(planted)
    got = api.dust_reads(synthetic[:n])
    assert len(got) == n and all(np.array_equal(g, h) for g, h in zip(got, host_results["default"][at:at + n]))


def test_no_reads_and_short_reads():
    from damar_amd import api
    assert api.dust_reads([]) == []
    got = api.dust_reads([np.zeros(k, dtype=np.uint8) for k in (0, 1, 2, 3)])
    assert [len(g) for g in got] == [0, 0, 0, 0]


def test_daligner_takes_the_blocks_tracks_made_here(built, tmp_path):
    """the head of the pipeline with this project's tools alone: DBdust G.1, DBdust G.2, then the mask_dust case's
    `daligner -mdust` lines -> the reference's recorded .las files"""
    import os
    import subprocess
    from conftest import read_case, compare_las
    from damar_amd import api
    case = read_case("mask_dust")
    work = str(tmp_path)
    dc.planted_workdir(work, ("G.db", ".G.idx", ".G.bps"), dc.MASK_DUST)
    for blk in ("G.1", "G.2"):
        assert dc.run_dbdust([blk], work, {}, timeout_s=120).returncode == 0
    assert sorted(dc.dust_files(work)) == [".G.1.dust.anno", ".G.1.dust.data", ".G.2.dust.anno", ".G.2.dust.data"]
    with open(os.path.join(work, "plan.txt"), "w") as f:
        for a, bs in case["lines"]:
            f.write("daligner %s G.%s %s\n" % (" ".join(case["opts"]), a, " ".join("G." + b for b in bs)))
    subprocess.run(["timeout", "-k", "10", "120", api.daligner_binary(), "-P", "plan.txt"], cwd=work, check=True, stdout=subprocess.DEVNULL)
    assert compare_las(case, work) == []
