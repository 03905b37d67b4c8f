#!/usr/bin/env python3
"""Fixtures of LAgap (tests/golden/gap/) from the REFERENCE.

Runs only where the reference sources lie (REF_SRC, default /root/reference): LAgap is compiled with a plain gcc line into
a temporary directory outside the repository, run on .las files this repository already holds (with the trim tracks of the
LAtrim fixtures) and on one synthetic file written here, and only data is kept: synth.las, its two tracks
(synth_tracks.npz), cases.json (options, exit status, stdout, stderr, md5 of the output; the error runs; what synth.las
plants) and expected_<case>.npz (the ten words of every expected record, and the trace bytes where -t changes them).
Nothing compiled is kept.  The asserts at the end hold every plant of the synthetic file to the branch it was made for.

    python tests/golden/make_gap_golden.py
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
import gap_common as gc                                # noqa: E402
import trim_common as tc                               # noqa: E402

OUT = gc.GDIR
TW = gc.TW
MAX_FILE = 1 << 20
DISCARD, COMP, CONT, GAP, TRIM = 0x2, 0x1, 0x8000, 0x10000, 0x20000


def build_tool(tmp):
    s = lambda *p: os.path.join(SRC, *p)
    subprocess.run(["gcc", "-O3", "-w", "-fno-strict-aliasing", "-I" + SRC, "-o", os.path.join(tmp, "LAgap"), s("scrub", "LAgap.c"),
                    s("lib", "read_loader.c"), s("lib", "utils.c"), s("lib", "tracks.c"), s("lib", "pass.c"), s("lib", "oflags.c"),
                    s("lib", "compression.c"), s("lib", "trim.c"), s("db", "QV.c"), s("db", "DB.c"), s("dalign", "align.c"),
                    "-lm", "-lz", "-lpthread"], cwd=tmp, check=True)
    return os.path.join(tmp, "LAgap")


# ---- the synthetic file ----------------------------------------------------------------------------------------------

def rec(a, b, ab, ae, bb, be=None, flags=0):
    """one record with a trace of its own: no differences, B's bases shared out over A's intervals"""
    be = bb + (ae - ab) if be is None else be
    cuts = [ab] + list(range((ab // TW + 1) * TW, ae, TW)) + [ae]
    al = np.diff(cuts)
    extra = (be - bb) - (ae - ab)
    bl = al + extra // len(al) + (np.arange(len(al)) < extra % len(al))
    assert np.all(bl >= 0) and np.all(bl <= 255) and bl.sum() == be - bb
    tr = np.zeros(2 * len(al), dtype=np.uint8)
    tr[1::2] = bl
    return (b, ab), struct.pack("<10i", len(tr), 0, ab, bb, ae, be, flags, a, b, 0) + tr.tobytes()


def synth(rl):
    """-> (file body, record count, plants, trim pairs, exclude intervals).  A plant is one pile on an A read of its own;
    `expect` says per kind of case what becomes of each of its records, in file order: '.' kept, 'C' dropped as contained,
    'G' dropped at a gap, 'D' discarded in the input and left at that, '?' whatever the reference makes of it."""
    plants, piles, ex = {}, [], {}
    trim = {r: (0, int(rl[r])) for r in range(len(rl))}

    def plant(tag, recs, lines=(), **expect):
        a = len(piles)
        made = sorted((rec(a, *r) for r in recs), key=lambda x: x[0])
        assert all(int(rl[r[0]]) >= max(r[3] if len(r) > 4 and r[4] is not None else r[3] + r[2] - r[1], 0) for r in recs), tag
        assert all(r[2] <= rl[a] for r in recs), tag
        piles.append(b"".join(m[1] for m in made))
        plants[tag] = dict(aread=a, nrec=len(recs), expect=expect, lines=list(lines))
        return a

    two = lambda ab, ae, b0: [(b0, ab, ae, 100), (b0 + 1, ab, ae, 100)]
    # with -t: a cut on B inside a trace interval (a box to align), and a containment that only the cut on A makes
    plant("t_box", [(105, 0, 2000, 300)], **{"def": "G", "t": "?"})
    trim[105] = (550, int(rl[105]))
    a = plant("t_cont", [(106, 1000, 3000, 1000), (106, 800, 2500, 900)], **{"def": ".G", "t": "CG"})
    trim[a] = (1000, int(rl[a]))
    # a middle break dropped on either side, and a tie in length (the first record wins: the left one)
    plant("drop_L", two(0, 2000, 50) + two(2300, 4500, 52), ["BREAK  15.. 27 \nDROP L @  1400.. 2800"], **{"def": "GG.."})
    plant("drop_R", two(0, 2500, 50) + two(2800, 4500, 52), ["BREAK  20.. 32 \nDROP R @  1900.. 3300"], **{"def": "..GG"})
    plant("tie", two(0, 2000, 50) + two(2300, 4300, 52), ["DROP R @  1400.. 2800"], **{"def": "..GG"})
    # two breaks: the first drop takes the pile's longest record away, the second is decided by what is left
    plant("two_breaks", [(50, 0, 4400, 100)] + two(0, 1600, 51) + two(1900, 4400, 53) + two(4700, 6400, 55),
          ["BREAK  11.. 23 \nDROP R @  1000.. 2400", "BREAK  39.. 51 \nDROP R @  3800.. 5200"], **{"def": "G..GGGG"})
    # a run still open at the end: dropped whatever -e and -s say (the pair on B read 51 is within 300, the interval contains it)
    a = plant("trailing", two(0, 2500, 50) + [(51, 2600, 5000, 2700)], ["DROP R @  1900.. 4600"], **{"def": "..G"})
    ex[a] = [(1000, 6000)]
    # -e: strictly inside an interval (the first of two that contain it is printed), and sharing an edge with one
    a = plant("masked", two(0, 2000, 50) + two(2300, 4500, 52), **{"def": "GG..", "e": "...."})
    ex[a] = [(100, 200), (1350, 2850), (1300, 2900)]
    plants["masked"]["lines_e"] = ["BREAK  15.. 27  MASKED  1350.. 2850"]
    a = plant("edge", two(0, 2000, 50) + two(2300, 4500, 52), **{"def": "GG..", "e": "GG.."})
    ex[a] = [(1400, 2900)]
    # -s: a pair on B read 54 across the break, its deltas 99 (under -s 100), 100 (equal to it), 50 with one complemented,
    # and 50 with the left record contained (the longer record over it is OVL_TEMP against the right one)
    base = two(0, 2000, 50) + two(2300, 4500, 52)
    plant("s_under", base + [(54, 0, 2000, 100), (54, 2099, 4500, 2199)], **{"def": "GG..G.", "s100": "......", "s300": "......"})
    plants["s_under"]["lines_s100"] = ["BREAK  15.. 27  STITCHABLE using 1"]
    plant("s_equal", base + [(54, 0, 2000, 100), (54, 2100, 4500, 2200)], **{"def": "GG..G.", "s100": "GG..G.", "s300": "......"})
    plant("s_mixed", base + [(54, 0, 2000, 100), (54, 2050, 4500, 2150, None, COMP)], **{"def": "GG..G.", "s100": "GG..G.", "s300": "GG..G."})
    plant("s_cont", base + [(54, 0, 2200, 3000), (54, 500, 2000, 3500), (54, 2050, 4500, 5050)],
          **{"def": "GG..GC.", "s100": "GG..GC.", "s300": "GG..GC."})
    # containments, all under 900 bases so that no bin is counted
    plant("cont1", [(50, 100, 500, 100), (50, 0, 800, 0)], **{"def": ".C"})             # (file order is by abpos: the outer one first)
    plant("cont1_i", [(50, 100, 500, 100), (50, 100, 800, 0, 700)], **{"def": "C."})    # i inside k: i goes, the inner loop ends
    plant("equal", [(50, 0, 800, 0), (50, 0, 800, 0)], **{"def": "C."})
    plant("b_other_way", [(50, 100, 500, 0, 600), (50, 100, 800, 100, 500)], **{"def": "C."})
    plant("comp_pair", [(50, 100, 500, 100, None, COMP), (50, 100, 800, 0, 700, COMP)], **{"def": "C."})
    plant("comp_mixed", [(50, 100, 500, 100, None, COMP), (50, 100, 800, 0, 700)], **{"def": ".."})
    plant("three", [(50, 100, 500, 100), (50, 100, 800, 0, 700), (50, 150, 450, 150)], **{"def": "C.C"})
    plant("mid_discarded_k", [(50, 0, 800, 0), (50, 100, 500, 100, None, DISCARD), (50, 150, 450, 150)], **{"def": ".DC"})
    # OVL_TEMP: equal lengths (the later record is marked, so the earlier one sets the covered range), and three in a row
    plant("temp_equal", [(50, 0, 2000, 0), (50, 1000, 3000, 3000)], **{"def": "GG"})
    plant("temp_three", [(50, 0, 1500, 0), (50, 1000, 3000, 2000), (50, 2500, 3700, 4500)], **{"def": ".GG"})
    a = len(piles)
    plant("self", [(a, 0, 2000, 0)], **{"def": "."})
    plant("one_record", [(50, 0, 3000, 100)], **{"def": "G"})
    plant("short_only", [(50, 0, 800, 100), (51, 100, 850, 100)], **{"def": ".."})
    plant("all_gone", [(50, 0, 3000, 100), (51, 200, 2800, 100)], ["BREAK   4..  6 \nDROP R @   300..  700"], **{"def": "GG"})
    a = len(piles)
    assert a < 30
    plant("many_b", [(b, 0, 2000, 100) for b in range(30, 100)] + [(99, 100, 1900, 200)], **{"def": "." * 70 + "C"})
    # more breaks than the kernel's event slot holds: 20 pairs of records, a thin run between each two
    a = len(piles)
    assert rl[a] >= 6800
    plant("many_events", [r for k in range(20) for r in two(300 * k, 300 * k + 1000, 50 + 2 * k)], **{"def": "G" * 40})
    while len(piles) < 104:                                              # the longest read of the database
        piles.append(b"")
    assert rl[104] == rl.max()
    plant("longest", [(50, 0, 9000, 0, 6000), (51, 0, 9000, 0, 6000), (52, 9500, 19975, 0, 6000), (53, 9500, 19975, 0, 6000)],
          ["BREAK  85.. 99 \nDROP L @  8400..10000"], **{"def": "GG.."})
    nrec = sum(p["nrec"] for p in plants.values())
    return b"".join(piles), nrec, plants, trim, ex


def want(plant, key):
    e = plant["expect"]
    chain = {"s100": ("s100",), "s300": ("s300",), "e": ("e",), "t": ("t",), "tL": ("t",), "es": ("e", "s300"), "R": ()}[key] if key != "def" else ()
    for k in chain:
        if k in e:
            return e[k]
    return e["def"]


def check_plants(name, key, cols, stdout, plants):
    """the reference's output against every plant's expectation: -> what it made of each plant"""
    seen = {}
    for tag, pl in plants.items():
        rows = np.flatnonzero(cols[:, 7] == pl["aread"])
        assert len(rows) == pl["nrec"], (name, tag)
        got = "".join("C" if f & CONT else "G" if f & GAP else "D" if f & DISCARD else "." for f in cols[rows, 6])
        exp = want(pl, key)
        assert all(e in ("?", g) or (e == "D" and g == "D") for e, g in zip(exp, got)) and len(exp) == len(got), \
            "%s: plant %s came out as %s, planted %s" % (name, tag, got, exp)
        for line in pl["lines"] + pl.get("lines_" + key, []):
            head, _, rest = line.partition("\n")
            full = "READ %7d %s" % (pl["aread"], head) + ("\n" + rest if rest else "")
            assert full in stdout or (not rest and head in stdout), (name, tag, full)
        seen[tag] = got
    return seen


def main():
    tmp = tempfile.mkdtemp(prefix="gap_golden_")
    try:
        lagap = build_tool(tmp)
        shutil.rmtree(OUT, ignore_errors=True)
        os.makedirs(OUT)
        rl = q_common.db_read_len("tiny2")
        body, nrec, plants, trim, ex = synth(rl)
        open(os.path.join(OUT, "synth.las"), "wb").write(struct.pack("<qi", nrec, TW) + body)
        assert os.path.getsize(os.path.join(OUT, "synth.las")) < MAX_FILE
        tracks = {}
        for nm, iv in (("trim", {r: [v] for r, v in trim.items()}), ("ex", ex)):
            anno, data = [0], []
            for r in range(len(rl)):
                for b, e in iv.get(r, []):
                    data += [b, e]
                anno.append(4 * len(data))
            tracks[nm + "_anno"], tracks[nm + "_data"] = np.array(anno, dtype=np.uint64), np.array(data, dtype=np.int32)
        np.savez_compressed(os.path.join(OUT, "synth_tracks.npz"), **tracks)
        cases, md5s, own_L = [], {}, {}
        for name, inp, opts in gc.CASES:
            work = tempfile.mkdtemp(dir=tmp)
            gc.workdir(work, inp)
            if "-L" in opts:                                             # the reference's own -L run is only compared, not kept
                r = subprocess.run([lagap] + opts + ["G", gc.LAS, gc.OUT], cwd=work, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
                assert r.returncode == 0, (name, r.stderr)
                own_L[inp] = tc.md5(os.path.join(work, gc.OUT))
            ref_opts = [o for o in opts if o != "-L"]                    # -L changes nothing here: the yardstick is the run without it
            r = subprocess.run([lagap] + ref_opts + ["G", gc.LAS, gc.OUT], cwd=work, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            assert r.returncode == 0, (name, r.stderr)
            out = os.path.join(work, gc.OUT)
            cols, trace, novl, tspace = tc.read_records(out)
            case = dict(name=name, input=inp, opts=opts, rc=r.returncode, stdout=r.stdout, stderr=r.stderr, md5=tc.md5(out))
            cases.append(case)
            md5s[name] = case["md5"]
            dst = os.path.join(OUT, "expected_%s.npz" % name)
            if inp == "gsynth" and "-t" in opts:
                np.savez_compressed(dst, novl=novl, tspace=tspace, cols=cols, trace=trace)
            else:                                                        # the md5 holds the trace bytes
                np.savez_compressed(dst, novl=novl, tspace=tspace, cols=cols)
            assert os.path.getsize(dst) < MAX_FILE, (name, os.path.getsize(dst))
            gone = lambda bit: int(np.sum((cols[:, 6] & bit) != 0))
            print("%-12s %6d records out, %5d contained, %5d at gaps, %4d breaks printed" % (name, novl, gone(CONT), gone(GAP), r.stdout.count("BREAK")))
            if inp == "gsynth" and "-p" not in opts:
                key = name.split("_")[0]
                seen = check_plants(name, key, cols, r.stdout, plants)
                for tag, got in seen.items():
                    plants[tag].setdefault("seen", {})[key] = got
        # whether the reference's own -t -L run gives the bytes of its -t run: recorded, not required
        same_L = {inp: own_L[inp] == md5s["t_" + inp.replace("gsynth", "synth")] for inp in own_L}
        assert all(md5s["tL_" + inp.replace("gsynth", "synth")] == md5s["t_" + inp.replace("gsynth", "synth")] for inp in own_L)
        print("-t -L equals -t:", same_L)
        # the plants of -t reached their branches: a cut inside a trace interval, and a containment made by the cut
        tcols = gc.expected("t_synth")["cols"]
        row = tcols[tcols[:, 7] == plants["t_box"]["aread"]][0]
        assert row[3] == 550 and row[2] % TW != 0 and not (row[6] & TRIM), row
        assert plants["t_cont"]["seen"]["t"][0] == "C" and plants["t_cont"]["seen"]["def"][0] == "."
        # the trailing run drops under -e and -s as well, nothing but the containing interval masks, only deltas under the fuzz stitch
        for key in ("def", "e", "s300", "es"):
            assert plants["trailing"]["seen"][key] == "..G", key
        assert plants["many_events"]["seen"]["def"] == "G" * 40
        work = tempfile.mkdtemp(dir=tmp)
        gc.workdir(work, "tiny2")
        errors = []
        for name, args in gc.ERRORS:
            r = subprocess.run([lagap] + args, cwd=work, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            errors.append(dict(name=name, args=args, rc=r.returncode, stdout=r.stdout, stderr=r.stderr))
            assert r.returncode == 1, (name, r.returncode, r.stderr)
        json.dump(dict(cases=cases, errors=errors, plants=plants, same_L=same_L), open(os.path.join(OUT, "cases.json"), "w"), indent=1)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
