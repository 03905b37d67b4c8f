#!/usr/bin/env python3
"""Fixtures of OGbuild (tests/golden/og/) from the REFERENCE.

Runs only where the reference sources lie (REF_SRC, default /root/reference): OGbuild and LAfilter are compiled with plain
gcc lines into a temporary directory outside the repository.  The inputs are .las files of this repository filtered by the
reference's LAfilter under the plan's options of the LAfilter fixtures (tiny2.las, fusion.las), one planted file with two
planted trim tracks (synth.las, synth_tracks.npz), a file that yields no edge (noedge.las) and one whose only fault is a
negative overhang (neg.las).  Only data is kept: the inputs, cases.json (options, exit status, stdout, stderr, md5 of every
file written; the error runs; what synth.las plants) and expected_<case>.txt, the graph of the small cases.  Nothing
compiled is kept.  The asserts at the end hold the plants to what the reference's output shows of them.

    python tests/golden/make_og_golden.py
"""
import json
import os
import shutil
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
SRC = os.environ.get("REF_SRC", "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import q_common                                        # noqa: E402
import filter_common as fc                             # noqa: E402
import og_common as oc                                 # noqa: E402

OUT = oc.ODIR
MAX_FILE = 1 << 20
KEEP_TEXT = 24 << 10                    # a graph up to this size is kept as it is
COMP, DISCARD, SYM = 0x1, 0x2, 0x100
LIBS = [("lib", "read_loader.c"), ("lib", "utils.c"), ("lib", "tracks.c"), ("lib", "pass.c"), ("lib", "oflags.c"), ("lib", "compression.c"),
        ("lib", "trim.c"), ("db", "QV.c"), ("db", "DB.c"), ("dalign", "align.c")]


def build_tools(tmp):
    s = lambda *p: os.path.join(SRC, *p)
    for name, src in (("OGbuild", s("touring", "OGbuild.c")), ("LAfilter", s("scrub", "LAfilter.c"))):
        subprocess.run(["gcc", "-O3", "-w", "-fno-strict-aliasing", "-I" + SRC, "-o", os.path.join(tmp, name), src] + [s(*l) for l in LIBS] +
                       ["-lm", "-lz", "-lpthread"], cwd=tmp, check=True)
    return os.path.join(tmp, "OGbuild"), os.path.join(tmp, "LAfilter")


def rec(a, b, ab, ae, bb, be, flags=0, diffs=7):
    return struct.pack("<10i", 0, diffs, ab, bb, ae, be, flags, a, b, 0)


def synth(rl):
    """-> (file body, record count, plants, trim, trim2).  Trim is (100, length - 100) but for read 60 (200, length - 100) and
    read 90, which has no interval; trim2 is (0, length).  A plant names the reads it uses."""
    n = len(rl)
    trim = {r: (100, int(rl[r]) - 100) for r in range(n)}
    trim[60] = (200, int(rl[60]) - 100)
    del trim[90]
    piles, plants = {}, {}

    def te(r):
        return trim[r][1]

    def add(a, b, ab, ae, bb, be, flags=0):
        ae, be, bb = min(ae, int(rl[a])), min(be, int(rl[b])), max(bb, 0)        # held to the reads; no plant depends on the far end of B
        piles.setdefault(a, []).append((b, len(piles.get(a, [])), rec(a, b, ab, ae, bb, be, flags)))

    def left(a, b, ovh=50, flags=0, length=1500):       # a record at A's trim begin that ends inside A; B plain or complemented
        add(a, b, 100, 100 + length, 100 + ovh, 100 + ovh + length, flags)

    def right(a, b, ovh=50, flags=0, length=1500):      # a record at A's trim end that begins inside A
        add(a, b, te(a) - length, te(a), max(te(b) - ovh - length, 150), te(b) - ovh, flags)

    def inner(a, b, flags=0):
        add(a, b, 500, 1500, 500, 1500, flags)

    # pile sizes: 1, 63, 64, 65, 129 records; every second record is discarded already, so no run holds two live ones.  Four of
    # the live records are edges, to reads that stay PROPER (so the graph shows them): the others lie inside A
    to = {0: 9, 62: 77, 64: 78, 128: 79}
    for a, size in ((0, 1), (1, 63), (2, 64), (3, 65), (4, 129)):
        for k in range(size):
            b = 10 + k // 2
            if k % 2 == 1:
                inner(a, b, DISCARD)
            elif k in to:
                left(a, to[k], ovh=10 + k)
            else:
                inner(a, b)
    plants["sizes"] = dict(areads=[0, 1, 2, 3, 4])
    # a run of one B read across the 64-record border: 62 records inside A, then four live records of read 80
    for k in range(62):
        inner(5, 10 + k)
    for k in range(4):
        add(5, 80, 100 + 0 * k, 1600 + k, 150, 1650 + k)
    plants["run_border"] = dict(aread=5, bread=80)
    left(6, 20);  left(6, 20, ovh=60)                                   # a run of two live records: both go
    left(7, 20);  inner(7, 20, DISCARD);  left(7, 20, ovh=60)           # three with a discarded middle: both live ones go
    inner(8, 20, DISCARD);  left(8, 20)                                 # a run that starts with a discarded record: the live one stays
    inner(8, 21, DISCARD);  left(8, 21);  left(8, 21, ovh=60)           # ... and with two live ones behind it: both go
    plants["runs"] = dict(gone=[6, 7], stays=(8, 20), gone_b=(8, 21))
    add(9, 9, 100, 1600, 300, 1800)                                     # a self overlap
    left(9, 22)
    # containment: A contained; B contained plain and complemented (read 60's interval is not symmetric); by a discarded record
    add(10, 23, 100, te(10), 200, 1200)
    add(11, 24, 300, 1300, 100, te(24))
    add(12, 60, 300, 1300, 100, int(rl[60]) - 200, COMP)
    add(13, 24, 300, 1300, 100, te(24) - 100, COMP)                     # read 24's interval is symmetric: contained again
    add(14, 25, 100, te(14), 200, 1200, DISCARD)
    plants["contained"] = dict(reads=[10, 24, 60, 14])
    add(15, 26, 100, 1600, 100, 1700)                                   # overhang exactly 0
    left(16, 27)                                                        # the mirrored edge lands in B's right list
    left(17, 27, flags=COMP)                                            # ... in B's left list
    right(18, 28)
    right(19, 28, flags=COMP)
    plants["mirror"] = dict(b_right=(27, 16), b_left=(27, 17), b_left2=(28, 18), b_right2=(28, 19))
    # symmetric discards.  The pairs are (B, A) of the flagged records: (31, 30) and (33, 32) and (29, 34)
    add(30, 31, 500, 1500, 500, 1500, SYM)
    left(31, 30)                                                        # found: 31 is a first member, and 30 a second one of (31, 30)
    add(32, 33, 500, 1500, 500, 1500, SYM)
    left(32, 35)                                                        # 32 is no first member: the loop does not run
    left(33, 36)                                                        # 33 is one, 36 is no second member
    add(34, 29, 500, 1500, 500, 1500, SYM)
    left(33, 34)                                                        # matched through (29, 34): 29 <= 33, and 34 is its second member
    left(31, 32)                                                        # missed: (33, 32) lies behind the entries of 31
    plants["sym"] = dict(found=(31, 30), through=(33, 34), missed=(31, 32), not_run=(32, 35))
    # equal b in the left and the right list of one read: 40's own left edge to 41, and 41's left edge mirrored into 40's right list
    left(40, 41)
    left(41, 40)
    # the double count: 42's left list holds its own edge to 43 and the mirror of 43's complemented left edge (one is dropped),
    # its right list two edges to 44 the same way
    left(42, 43);  left(43, 42, flags=COMP)
    right(42, 44);  right(44, 42, flags=COMP)
    plants["dupes"] = dict(lr=(40, 41), double=42)
    # three edges with equal b in one list.  Edges of records cannot do that (a live run of one B read is dropped whole, so a
    # list holds one own and one mirrored edge per b at most): the three are slots the building pass leaves as zeros, b = 0.
    # Piles 51..53 each flag a record to read 50, so (50, 51), (50, 52), (50, 53) are pairs and all three of 50's edges go
    for b in (51, 52, 53):
        add(b, 50, 500, 1500, 500, 1500, SYM)
        left(50, b)
    plants["three_equal_b"] = dict(aread=50, breads=[51, 52, 53])
    left(45, 90)                                                        # a read with no interval in the trim track
    # degrees: 46 has MAXDEG_TEST left edges, 47 one more
    for k in range(oc.MAXDEG_TEST):
        left(46, 61 + k, ovh=20 + k, length=te(46) - 100 - 50)
    for k in range(oc.MAXDEG_TEST + 1):
        left(47, 61 + k, ovh=20 + k, length=te(47) - 100 - 50)
    plants["degree"] = dict(at=46, over=47)
    inner(48, 70)                                                       # a widow
    plants["widow"] = 48
    body, nrec = [], 0
    for a in sorted(piles):
        recs = sorted(piles[a], key=lambda x: (x[0], x[1]))
        for b, _, raw in recs:
            f = struct.unpack("<10i", raw)
            assert 0 <= f[2] < f[4] <= rl[a] and 0 <= f[3] < f[5] <= rl[b], (a, b, f)
        body += [x[2] for x in recs]
        nrec += len(recs)
    trim2 = {r: (0, int(rl[r])) for r in range(n)}
    return b"".join(body), nrec, plants, trim, trim2


def track_arrays(iv, n):
    anno, data = [0], []
    for r in range(n):
        if r in iv:
            data += list(iv[r])
        anno.append(4 * len(data))
    return np.array(anno, dtype=np.uint64), np.array(data, dtype=np.int32)


def edges_of(text):
    """the (source, target, end) of a graphml file"""
    import re
    return set((int(a), int(b), e) for a, b, e in re.findall(r'<edge source="(\d+)" target="(\d+)">.*?<data key="end">(.)</data>', text, re.S))


def main():
    tmp = tempfile.mkdtemp(prefix="og_golden_")
    try:
        ogbuild, lafilter = build_tools(tmp)
        shutil.rmtree(OUT, ignore_errors=True)
        os.makedirs(OUT)
        plan = next(c for c in fc.load_cases() if c["name"] == "plan_tiny2")["opts"]
        for inp in oc.REAL:
            work = tempfile.mkdtemp(dir=tmp)
            fc.workdir(work, inp)
            r = subprocess.run([lafilter] + plan + ["G", fc.LAS, fc.OUT], cwd=work, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            assert r.returncode == 0, (inp, r.stderr)
            shutil.copy(os.path.join(work, fc.OUT), os.path.join(OUT, inp + ".las"))
        rl = q_common.db_read_len("tiny2")
        body, nrec, plants, trim, trim2 = synth(rl)
        open(os.path.join(OUT, "synth.las"), "wb").write(struct.pack("<qi", nrec, 100) + body)
        ta, td = track_arrays(trim, len(rl))
        ua, ud = track_arrays(trim2, len(rl))
        np.savez_compressed(os.path.join(OUT, "synth_tracks.npz"), trim_anno=ta, trim_data=td, trim2_anno=ua, trim2_data=ud)
        inner = [rec(a, a + 1, 500, 1500, 500, 1500) for a in range(0, 40, 2)]
        open(os.path.join(OUT, "noedge.las"), "wb").write(struct.pack("<qi", len(inner), 100) + b"".join(inner))
        neg = [rec(0, 1, 500, 1500, 500, 1500), rec(2, 3, 100, 1600, 50, 1550), rec(4, 5, 500, 1500, 500, 1500)]
        open(os.path.join(OUT, "neg.las"), "wb").write(struct.pack("<qi", len(neg), 100) + b"".join(neg))
        for f in os.listdir(OUT):
            assert os.path.getsize(os.path.join(OUT, f)) < MAX_FILE, f
        cases, text, kept = [], {}, set()
        for name, inp, opts in oc.CASES:
            work = tempfile.mkdtemp(dir=tmp)
            oc.workdir(work, inp)
            r = oc.run_tool(opts + ["G", oc.LAS, oc.OUT], work, tool=ogbuild)
            assert r.returncode == (1 if inp == "neg" else 0), (name, r.returncode, r.stderr)
            case = dict(name=name, input=inp, opts=opts, rc=r.returncode, stdout=r.stdout, stderr=r.stderr, md5=oc.outputs(work))
            cases.append(case)
            whole = os.path.join(work, oc.OUT)
            if os.path.exists(whole):
                text[name] = open(whole).read()
                if os.path.getsize(whole) <= KEEP_TEXT and case["md5"][oc.OUT] not in kept:      # one copy of a graph that several cases give
                    kept.add(case["md5"][oc.OUT])
                    shutil.copy(whole, os.path.join(OUT, "expected_%s.txt" % name))
            print("%-14s rc %d, %2d files, %s" % (name, r.returncode, len(case["md5"]), " | ".join(l.strip() for l in r.stdout.splitlines() if "edges" in l)))
        work = tempfile.mkdtemp(dir=tmp)
        oc.workdir(work, "synth")
        errors = []
        for name, args in oc.ERRORS:
            r = oc.run_tool(args, work, tool=ogbuild)
            errors.append(dict(name=name, args=args, rc=r.returncode, stdout=r.stdout, stderr=r.stderr))
            assert r.returncode == 1, (name, r.returncode, r.stderr)

        # the plants, where the reference's output shows them
        E = edges_of(text["def_synth"])
        out = next(c for c in cases if c["name"] == "def_synth")["stdout"]
        shown = dict(sizes=[(0, 9, "l") in E, (1, 9, "l") in E, (1, 77, "l") in E, (2, 77, "l") in E, (3, 78, "l") in E, (4, 79, "l") in E],
                     border_run_gone=not any(a == 5 and b == 80 for a, b, _ in E),
                     runs_gone=not any(a in (6, 7) for a, _, _ in E), run_stays=(8, 20, "l") in E, run_b_gone=(8, 21, "l") not in E,
                     no_self=(9, 9, "l") not in E, self_pile_edge=(9, 22, "l") in E,
                     contained_gone=not any(r in (a, b) for r in plants["contained"]["reads"] for a, b, _ in E),
                     ovh0=not any(a == 15 and b == 26 for a, b, _ in E), mirrors=[(27, 16, "r") in E, (27, 17, "l") in E, (28, 18, "l") in E, (28, 19, "r") in E],
                     sym=[(31, 30, "l") not in E, (33, 34, "l") not in E, (31, 32, "l") in E, (32, 35, "l") in E, (33, 36, "l") in E],
                     lr=[(40, 41, "l") in E, (40, 41, "r") not in E], double=[(42, 43, "l") in E, (42, 44, "r") in E],
                     three=not any(a == 50 for a, _, _ in E), no_interval=(45, 90, "l") in E,
                     degree=[sum(1 for a, _, e in E if a == 46 and e == "l") == oc.MAXDEG_TEST, sum(1 for a, _, e in E if a == 47 and e == "l") == oc.MAXDEG_TEST + 1],
                     widow=not any(48 in (a, b) for a, b, _ in E))
        plants["shown"] = shown
        print("plants shown:", shown)
        for k, v in shown.items():
            assert all(v) if isinstance(v, list) else v, "the reference's graph does not show plant %s: %s" % (k, v)
        # read 50's three edges of zeros: two are dropped as neighbours with one b, the third is written from 50's list as 0 -> 0
        assert text["def_synth"].count('<edge source="0" target="0">') >= 1
        assert "  5 symmetric discards" in out
        no = next(c for c in cases if c["name"] == "def_noedge")
        assert "0 left edges\n0 right edges" in no["stdout"] and "<edge" not in text["def_noedge"]
        ng = next(c for c in cases if c["name"] == "def_neg")
        assert ng["stderr"].count("error: ovh   -50 <= 0       2 ->       3") == 2
        json.dump(dict(cases=cases, errors=errors, plants=plants, plan=plan), open(os.path.join(OUT, "cases.json"), "w"), indent=1)
        for f in os.listdir(OUT):
            assert os.path.getsize(os.path.join(OUT, f)) < MAX_FILE, (f, os.path.getsize(os.path.join(OUT, f)))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
