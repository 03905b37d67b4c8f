"""`daligner -C`: every .las file checked by the thread that writes it (csrc/host/las.c on the routine of lascheck.c).
Clean runs stay clean and byte-identical, the counts of DAMAR_PLAN_STATS equal what the files hold, files that
DAMAR_LAS_KEEP discards are checked all the same, and without -C nothing changes.  That the check FIRES is shown on the
CPU (tests/test_lacheck_host.py drives the same routine, with the writer's options, on damaged record arrays): nothing
here makes the GPU write a wrong record.  Every command runs under a time limit of its own; nothing is run twice."""
import json
import os
import subprocess

import pytest

from conftest import ROOT, GOLDEN, read_case, link_db, compare_las, opts_to_plan_kwargs

pytestmark = pytest.mark.gpu

LIMIT = 300          # seconds for one daligner command on a golden (they take about a second)
KINDS = ["tiny2", "mask_two", "tandem2"]          # plain, with mask tracks, through bridging


@pytest.fixture(scope="module")
def gpu(built):
    from damar_amd import api
    L = api.lib()
    assert L.damar_hip_init(0) >= 1
    return L


def daligner(args, cwd, env=None):
    from damar_amd import api
    r = subprocess.run([api.daligner_binary()] + args, cwd=cwd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True,
                       timeout=LIMIT, env=dict(os.environ, **(env or {})))
    return r.returncode, r.stderr


def write_plan(case, work, extra=()):
    link_db(case["dbdir"], work)
    with open(os.path.join(work, "plan.txt"), "w") as f:
        for a, bs in case["lines"]:
            f.write("daligner %s G.%s %s\n" % (" ".join(list(case["opts"]) + list(extra)), a, " ".join("G." + b for b in bs)))


def stats_line(err):
    """the DAMAR_PLAN_STATS=- line of a command's stderr"""
    lines = [ln for ln in err.splitlines() if ln.startswith('{"tool"')]
    assert len(lines) == 1, err
    return json.loads(lines[0])


def files_of(case):
    return sorted(set(case["las"]) | set(case["las_md5"]))


def record_total(work, rels):
    from damar_amd import driver
    return sum(driver.las_stats(os.path.join(work, rel))[0] for rel in rels)


@pytest.mark.parametrize("name", KINDS)
def test_gpu_cli_with_C_is_clean_identical_and_counts_every_record(gpu, tmp_path, name):
    case = read_case(name)
    # the single command, once per line of the case
    one = str(tmp_path / "single")
    link_db(case["dbdir"], one)
    for a, bs in case["lines"]:
        st, err = daligner(list(case["opts"]) + ["-C", "G." + a] + ["G." + b for b in bs], one)
        assert st == 0 and "CHECK" not in err, err
    assert compare_las(case, one) == []
    # the plan, with the counts
    work = str(tmp_path / "plan")
    write_plan(case, work)
    st, err = daligner(["-C", "-P", "plan.txt"], work, {"DAMAR_PLAN_STATS": "-"})
    assert st == 0 and "CHECK" not in err, err
    assert compare_las(case, work) == []
    s = stats_line(err)
    rels = files_of(case)
    print(name, {k: s[k] for k in s if k.startswith("check")}, "records", s["records"])
    assert s["check_violations"] == 0 and s["checked_discarded_files"] == 0
    assert s["checked_files"] == len(rels) == s["las_files"]
    assert s["checked_records"] == record_total(work, rels) == s["records"]


@pytest.mark.parametrize("name", KINDS)
def test_gpu_cli_without_C_is_what_it_was(gpu, tmp_path, name):
    """No -C: the files are the goldens (bytes or md5), the stats line has no field of the check, no CHECK text."""
    case = read_case(name)
    work = str(tmp_path)
    write_plan(case, work)
    st, err = daligner(["-P", "plan.txt"], work, {"DAMAR_PLAN_STATS": "-"})
    assert st == 0 and "CHECK" not in err
    assert compare_las(case, work) == []
    s = stats_line(err)
    assert not [k for k in s if k.startswith("check")]


def test_gpu_plan_checks_the_files_that_are_discarded(gpu, tmp_path):
    """A plan of three block pairs (four files) with a DAMAR_LAS_KEEP list of one: all four are checked, three of them
    on their way to /dev/null, and the kept one is the golden."""
    case = read_case("tiny2")
    work = str(tmp_path)
    write_plan(case, work)
    rels = files_of(case)
    assert len(rels) >= 3
    keep = rels[-1]
    with open(os.path.join(work, "keep.txt"), "w") as f:
        f.write(keep + "\n")
    st, err = daligner(["-C", "-P", "plan.txt"], work, {"DAMAR_PLAN_STATS": "-", "DAMAR_LAS_KEEP": os.path.join(work, "keep.txt")})
    assert st == 0 and "CHECK" not in err, err
    s = stats_line(err)
    print({k: s[k] for k in s if k.startswith("check")})
    assert s["checked_files"] == len(rels)
    assert s["checked_discarded_files"] == len(rels) - 1
    assert s["check_violations"] == 0
    assert s["checked_records"] == record_total(case["lasdir"], rels)
    assert open(os.path.join(work, keep), "rb").read() == open(os.path.join(case["lasdir"], keep), "rb").read()
    assert [r for r in rels if os.path.exists(os.path.join(work, r))] == [keep]


def test_gpu_slab_path_with_C(gpu, tmp_path):
    """The comparisons cut into slabs of B reads (DAMAR_TEST_SEED_CAP, as tests/test_gpu_slabs.py lowers the figure):
    the files are the goldens, every record was checked, nothing found."""
    from test_gpu_slabs import case_cap, HOOK
    case = read_case("tiny2")
    cap = case_cap(gpu, case)
    os.environ.pop(HOOK, None)
    work = str(tmp_path)
    write_plan(case, work)
    st, err = daligner(["-C", "-P", "plan.txt"], work, {"DAMAR_PLAN_STATS": "-", HOOK: str(cap)})
    assert st == 0 and "CHECK" not in err, err
    s = stats_line(err)
    print("cap", cap, "seed_slabs", s["seed_slabs"], "split", s["split_comparisons"], {k: s[k] for k in s if k.startswith("check")})
    assert s["seed_slabs"] > s["split_comparisons"] > 0
    assert compare_las(case, work) == []
    rels = files_of(case)
    assert (s["checked_files"], s["check_violations"]) == (len(rels), 0)
    assert s["checked_records"] == record_total(work, rels)


def test_gpu_datander_with_C(gpu, tmp_path):
    """datander writes through the same las.c: -C there too."""
    from damar_amd import api
    case = read_case("tan_tandem")
    work = str(tmp_path)
    link_db(case["dbdir"], work)
    exe = api.daligner_binary().replace("daligner", "datander")
    for a, bs in case["lines"]:
        r = subprocess.run([exe] + list(case["opts"]) + ["-C", "G." + a], cwd=work, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE,
                           text=True, timeout=LIMIT)
        assert r.returncode == 0 and "CHECK" not in r.stderr, r.stderr
    assert compare_las(case, work) == []


def test_gpu_in_process_driver_with_check(gpu, tmp_path):
    from damar_amd import api, driver
    case = read_case("mask_two")
    work = str(tmp_path)
    link_db(case["dbdir"], work)
    before = api.check_totals()
    plan = driver.Plan(check=True, **opts_to_plan_kwargs(case["opts"]))
    try:
        blocks = {}
        for a, bs in case["lines"]:
            for x in [a] + bs:
                if x not in blocks:
                    blocks[x] = driver.Block(os.path.join(work, "G." + x))
            plan.run_line(blocks[a], [blocks[b] for b in bs], work)
        plan.finish()
    finally:
        api.set_check(False)
    after = api.check_totals()
    got = [y - x for x, y in zip(before, after)]
    rels = files_of(case)
    print("check totals", got)
    assert compare_las(case, work) == []
    assert got == [len(rels), record_total(work, rels), 0, 0]
    # and the tool on what was written: -p -s -d and the strict set
    for rel in rels:
        assert api.las_check(os.path.join(work, "G"), os.path.join(work, rel), strict=True) == (0, [])
