"""The record writer of host/laspass.c on its own: tests/las_out_check.c, a program with its own main built here from
laspass.c alone (with the address and undefined-behaviour sanitizers where an empty program built with them links and
starts), writes a handful of small files; they are read back with the reader of the LAtrim tests and held against what was
offered."""
import os
import subprocess

import numpy as np
import pytest

import trim_common as tc

HOSTDIR = os.path.join(tc.ROOT, "damar_amd", "csrc", "host")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
DISCARD, TEMP = 0x2, 0x800

# (flags, trace values) as tests/las_out_check.c offers them
MIXED = [(0x0, [3, 90, 2, 70]), (0x2, [1, 50]), (0x801, [0, 255]), (0x0, []), (0x802, [9, 99, 8, 88]), (0x1, [255, 255])]
WIDE = [(0x0, [3, 256, 2, 1000]), (0x800, [65535, 0]), (0x0, [])]
BIG = [(0x0, [1, 100]), (0x0, [1, 256]), (0x0, [2, 255, 3, 50])]
TOO_BIG = "%s: Compression of trace to bytes fails, value too big\n"


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """the program built and run once: (its lines by file name, its stderr, the directory of its files)"""
    tmp = str(tmp_path_factory.mktemp("las_out"))
    open(os.path.join(tmp, "empty.c"), "w").write("int main(void) { return 0; }\n")
    trial = subprocess.run(["gcc"] + SANITIZE + ["-o", os.path.join(tmp, "empty"), os.path.join(tmp, "empty.c")], stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE)
    if trial.returncode == 0:                                       # linked: does a program built that way start here?
        trial = subprocess.run([os.path.join(tmp, "empty")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    flags = SANITIZE if trial.returncode == 0 else []
    exe = os.path.join(tmp, "las_out_check")
    cmd = ["gcc", "-O1", "-g", "-Wall", "-Werror"] + flags + ["-I" + os.path.join(tc.ROOT, "include"), "-I" + HOSTDIR, "-o", exe,
                                                               os.path.join(tc.ROOT, "tests", "las_out_check.c"), os.path.join(HOSTDIR, "laspass.c")]
    b = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, b.stdout
    r = subprocess.run([exe, tmp], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return {l.split()[0]: l.split()[1:] for l in r.stdout.splitlines()}, r.stderr, tmp


def said(words, puts, written, discarded):
    """a line of the program: begin 0, the outcome of every put, the count before and after the close, close 0"""
    n = str(written)
    return words == ["begin", "0", "put"] + [str(p) for p in puts] + ["written-so-far", n, "close", "0", "written", n, "discarded", str(discarded)]


def check_file(path, tspace, offered):
    """the file holds exactly the offered records, OVL_TEMP gone, and its header counts them"""
    buf = open(path, "rb").read()
    offs, end = tc.record_offsets(buf)
    assert end == len(buf) and len(offs) == len(offered)
    cols, trace, novl, ts = tc.read_records(path)
    assert (novl, ts) == (len(offered), tspace)
    assert list(cols[:, 6]) == [f & ~TEMP for f, _ in offered] and list(cols[:, 0]) == [len(v) for _, v in offered]
    wide = np.array([x for _, v in offered for x in v], dtype="<u2" if tspace > 125 else np.uint8)
    assert trace.tobytes() == wide.tobytes()
    return cols


def test_purge_off_keeps_every_record(run):
    lines, _, tmp = run
    assert said(lines["keep"], [0] * 6, 6, 2)
    cols = check_file(os.path.join(tmp, "keep.las"), 100, MIXED)
    assert list(cols[:, 1]) == [10, 11, 12, 13, 14, 15] and list(cols[:, 8]) == [5, 6, 7, 8, 9, 10]      # in the order offered


def test_purge_on_skips_discarded_records_and_counts_the_rest(run):
    lines, _, tmp = run
    assert said(lines["purge"], [0] * 6, 4, 2)                      # the header's count: records written, not offered
    check_file(os.path.join(tmp, "purge.las"), 100, [r for r in MIXED if not r[0] & DISCARD])


def test_temp_flag_does_not_reach_the_file(run):
    _, _, tmp = run
    assert any(f & TEMP for f, _ in MIXED)
    assert not np.any(tc.read_records(os.path.join(tmp, "keep.las"))[0][:, 6] & TEMP)


def test_bytes_and_values_give_the_same_file(run):
    lines, _, tmp = run
    assert said(lines["bytes1"], [0] * 6, 6, 2) and said(lines["vals2"], [0] * 3, 3, 0) and said(lines["bytes2"], [0] * 3, 3, 0)
    assert tc.md5(os.path.join(tmp, "bytes1.las")) == tc.md5(os.path.join(tmp, "keep.las"))
    assert tc.md5(os.path.join(tmp, "bytes2.las")) == tc.md5(os.path.join(tmp, "vals2.las"))
    check_file(os.path.join(tmp, "vals2.las"), 200, WIDE)           # two bytes a value: 256 and above are written


def test_a_value_above_255_is_refused_in_byte_mode(run):
    lines, err, tmp = run
    assert err == TOO_BIG % "(null)" + TOO_BIG % "LAtrim"           # once per tool string, nothing else on stderr
    for name in ("refused_null", "refused_latrim"):
        assert said(lines[name], [0, 2, 0], 2, 0)
        check_file(os.path.join(tmp, name + ".las"), 100, [BIG[0], BIG[2]])       # 255 is written; the count matches what the file holds


def test_no_record_at_all(run):
    lines, _, tmp = run
    assert said(lines["empty"], [], 0, 0)
    check_file(os.path.join(tmp, "empty.las"), 100, [])
