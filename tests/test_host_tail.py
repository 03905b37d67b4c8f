"""The product's whole host tail (damar_amd/csrc/host/tail.cpp: the item/seq ordering, the job filter, the wide map, the
two views of a record, the thread pool with direct and private buffers, the two-stage pipeline) on the CPU: behind the
oracle's front (oracle/hosttail.cpp, the *_hosttail programs), with the records handed over the ways a launch delivers
them, against the .las files the reference wrote.  Then the same programs built under the thread sanitizer and under
the address and undefined-behaviour sanitizers, as processes of their own."""
import os
import subprocess

import pytest

from conftest import ROOT, read_case, run_cli, compare_las

EXE = os.path.join(ROOT, "oracle", "oracle_daligner_hosttail")
# multi-record pairs, fusions, bridges, -e.75; tiny_s is the case whose spacing (-s126) lies above TRACE_XOVR (125): its
# pool stays 16-bit under the bytes knob and its records are written with two-byte trace values
CASES = ["tandem", "fusion", "fusion2", "indel", "tiny_s"]

THREADS7 = {"DAMAR_TAIL_MIN": "1", "DAMAR_TAIL_THREADS": "7"}
THREADS1 = {"DAMAR_TAIL_MIN": "1", "DAMAR_TAIL_THREADS": "1"}
DIRECT = {"ORACLE_HT_SPEC_THREADS": "8"}           # at least as many overlap buffers as tail threads: filled directly
PRIVATE = {"ORACLE_HT_SPEC_THREADS": "2"}          # fewer: private buffers, appended in order
KNOBS = {
    "shuffle": {"ORACLE_HT_SHUFFLE": "11"},
    "shuffle_bytes": {"ORACLE_HT_SHUFFLE": "12", "ORACLE_HT_BYTES": "1"},
    "shuffle_jobs": {"ORACLE_HT_SHUFFLE": "13", "ORACLE_HT_JOBS": "2"},
    "shuffle_wide": {"ORACLE_HT_SHUFFLE": "14", "ORACLE_HT_WIDE": "3"},
    # one thread takes the unthreaded path whatever the Align_Spec holds: run with one buffer and with eight
    "1thread_direct": dict(THREADS1, **DIRECT),
    "1thread_private": dict(THREADS1, ORACLE_HT_SPEC_THREADS="1"),
    "7threads_direct": dict(THREADS7, **DIRECT),
    "7threads_private": dict(THREADS7, **PRIVATE),
    "pipeline": dict(THREADS7, ORACLE_HT_PIPELINE="1", ORACLE_HT_SHUFFLE="15", **PRIVATE),
}


def run_case(exe, name, workdir, knobs):
    case = read_case(name)
    env = dict(os.environ)
    env.update(knobs)
    from conftest import link_db
    link_db(case["dbdir"], workdir)
    if case["tool"] == "datander":
        exe = exe.replace("daligner", "datander")
    err = ""
    for a, bs in case["lines"]:
        r = subprocess.run([exe] + case["opts"] + ["G." + a] + ["G." + b for b in bs], cwd=workdir, env=env,
                           stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0, r.stderr
        err += r.stderr
    return case, err


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("knob", sorted(KNOBS))
def test_records_delivered_like_a_launch_give_the_reference_las(built, tmp_path, name, knob):
    case, _ = run_case(EXE, name, str(tmp_path), KNOBS[knob])
    assert compare_las(case, str(tmp_path)) == []


@pytest.mark.parametrize("name", ["tan_plain", "tan_tandem"])
def test_datander_front_through_the_tail_matches_reference_las(built, tmp_path, name):
    """datander's rule (no bridge context, A records only) through the same tail function: plain, and cut over seven
    threads with the records shuffled"""
    case = read_case(name)
    assert case["tool"] == "datander"
    run_cli(EXE, case, str(tmp_path))
    assert compare_las(case, str(tmp_path)) == []
    d2 = os.path.join(str(tmp_path), "threads")
    case, _ = run_case(EXE, name, d2, dict(THREADS7, ORACLE_HT_SHUFFLE="16", **DIRECT))
    assert compare_las(case, d2) == []


SANITIZERS = {"thread": ["-fsanitize=thread"],
              "address": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}


@pytest.fixture(scope="module", params=sorted(SANITIZERS))
def sanitized(request, tmp_path_factory):
    """the hosttail program built at -O1 -g under one sanitizer, where an empty program built that way links and starts.
    The tail, its driver and the product's host sources behind it are instrumented; the oracle's front, which is most
    of a run's time and none of what is under test, is built plain."""
    flags = SANITIZERS[request.param]
    tmp = str(tmp_path_factory.mktemp("ht_" + request.param))
    open(os.path.join(tmp, "empty.cpp"), "w").write("int main(void) { return 0; }\n")
    trial = subprocess.run(["g++"] + flags + ["-o", os.path.join(tmp, "empty"), os.path.join(tmp, "empty.cpp")],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if trial.returncode == 0:
        trial = subprocess.run([os.path.join(tmp, "empty")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if trial.returncode != 0:
        pytest.skip("no -fsanitize=%s program links and starts here" % request.param)
    exe = os.path.join(tmp, "oracle_daligner_hosttail")
    b = subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "HTOUT=" + tmp + "/", "HTFRONT=-O3 -g",
                        "HTFLAGS=-O1 -g " + " ".join(flags), exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, b.stdout
    return exe


@pytest.mark.parametrize("name", ["fusion", "indel"])
@pytest.mark.parametrize("knob", ["pipeline", "7threads_direct"])
def test_tail_threads_under_a_sanitizer(built, sanitized, tmp_path, name, knob):
    """a process of its own: exit 0, nothing from the sanitizer, the reference's files"""
    # (no leak report at exit: the driver ends like the reference's daligner, holding its Align_Spec, block and index,
    # and the writers' scratch of host/las.c lives as long as its thread; none of it is the tail's)
    case, err = run_case(sanitized, name, str(tmp_path), dict(KNOBS[knob], ASAN_OPTIONS="detect_leaks=0"))
    assert "Sanitizer" not in err and "runtime error" not in err, err
    assert compare_las(case, str(tmp_path)) == []
