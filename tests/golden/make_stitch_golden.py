#!/usr/bin/env python3
"""Fixtures of LAstitch and of the exact box alignment into trace pairs under it (tests/golden/stitch/) from the REFERENCE.

Runs only where the reference sources lie (REF_SRC, default /root/reference): LAstitch and a small driver around
Compute_Alignment(DIFF_TRACE) are compiled with plain gcc lines into a temporary directory outside the repository, run on
.las files this repository already holds and on one synthetic file written here, and only data is kept: synth.las, the
track of the -t cases (lc_track.npz), cases.json (options, exit status, stdout, stderr, md5 of the output; the error runs;
what synth.las plants), expected_<case>.npz (the ten words of every expected record and their trace bytes) and tboxes.npz.
Nothing compiled is kept.  The asserts at the end hold the synthetic file to the branches it plants.

    python tests/golden/make_stitch_golden.py
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
import stitch_common as sc                             # noqa: E402
import trim_common as tc                               # noqa: E402
from make_trim_golden import box_list, mutate          # noqa: E402

OUT = sc.SDIR
TW = sc.TW
MAX_FILE = 1 << 20

# our own driver: boxes in, what Compute_Alignment(DIFF_TRACE) makes of them out
DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "db/DB.h"
#include "dalign/align.h"

int main(int argc, char *argv[])
{ FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
  Work_Data *work = New_Work_Data();
  Alignment  al;
  Path       path;
  int        nbox, i, m, n, at;
  if (in == NULL || out == NULL || fread(&nbox, sizeof(int), 1, in) != 1)
    return 1;
  for (i = 0; i < nbox; i++)
    { char *a, *b;
      if (fread(&m, sizeof(int), 1, in) != 1 || fread(&n, sizeof(int), 1, in) != 1 || fread(&at, sizeof(int), 1, in) != 1)
        return 1;
      a = malloc(at + m + 2);
      b = malloc(n + 2);
      memset(a, 4, at + 1);
      b[0] = 4;
      if (fread(a + 1 + at, 1, m, in) != (size_t) m || fread(b + 1, 1, n, in) != (size_t) n)
        return 1;
      a[at + m + 1] = b[n + 1] = 4;
      memset(&al, 0, sizeof(al));
      al.path = &path;  al.aseq = a + 1;  al.bseq = b + 1;
      path.abpos = at;  path.bbpos = 0;  path.aepos = at + m;  path.bepos = n;
      path.diffs = 0;
      if (Compute_Alignment(&al, work, DIFF_TRACE, 100))
        return 1;
      fwrite(&path.diffs, sizeof(int), 1, out);
      fwrite(&path.tlen, sizeof(int), 1, out);
      fwrite(path.trace, sizeof(uint16), path.tlen, out);
      free(a);
      free(b);
    }
  fclose(out);
  return 0;
}
"""


def build_tools(tmp):
    s = lambda *p: os.path.join(SRC, *p)
    common = ["gcc", "-O3", "-w", "-fno-strict-aliasing", "-I" + SRC]
    subprocess.run(common + ["-o", os.path.join(tmp, "LAstitch"), s("scrub", "LAstitch.c"), s("lib", "read_loader.c"), s("lib", "utils.c"),
                             s("lib", "tracks.c"), s("lib", "pass.c"), s("lib", "oflags.c"), s("lib", "compression.c"), s("db", "QV.c"),
                             s("db", "DB.c"), s("dalign", "align.c"), "-lm", "-lz", "-lpthread"], cwd=tmp, check=True)
    open(os.path.join(tmp, "tboxdriver.c"), "w").write(DRIVER)
    subprocess.run(common + ["-o", os.path.join(tmp, "tboxdriver"), os.path.join(tmp, "tboxdriver.c"), s("dalign", "align.c"),
                             s("db", "DB.c"), s("db", "QV.c"), "-lm", "-lpthread"], cwd=tmp, check=True)
    return os.path.join(tmp, "LAstitch"), os.path.join(tmp, "tboxdriver")


# ---- the box cases ---------------------------------------------------------------------------------------------------

def tbox_list():
    """(A, B, family, the offsets it runs at) -- the families of the trim generator and the ones trace pairs add"""
    rng = np.random.default_rng(20261020)
    rnd = lambda n: rng.integers(0, 4, n).astype(np.uint8)
    old, small = box_list()
    bx = [(a, b, "small" if i < small else "old_big" if max(len(a), len(b)) > 1000 else "random", sc.OFFSETS)
          for i, (a, b) in enumerate(old)]
    for m in (1, 20, 40):                                                # inside one interval (but where it begins at 99)
        a = rnd(m)
        bx.append((a, mutate(rng, a, .2, 200), "inside", sc.OFFSETS))
    for off in sc.OFFSETS:                                               # ending exactly on a boundary
        for k in (1, 2, 3):
            a = rnd(k * TW - off)
            bx.append((a, mutate(rng, a, .15, 10000), "boundary", (off,)))
            bx.append((a, np.concatenate([a, rnd(7)]), "fold", (off,)))  # insertions sitting exactly on the last boundary
            bx.append((a, np.concatenate([mutate(rng, a, .15, 10000), 3 - a[-1:], 3 - a[-1:]]), "fold", (off,)))
    for n in (1, 50, 130):                                               # one base of A against B alone, and the reverse
        bx.append((rnd(1), rnd(n), "lone_a", sc.OFFSETS))
        bx.append((rnd(n), rnd(1), "lone_b", sc.OFFSETS))
    for rate in (.15, .30):
        for _ in range(150):
            a = rnd(int(rng.integers(400, 701)))
            bx.append((a, mutate(rng, a, rate, 10000), "stitch", sc.OFFSETS))
    for _ in range(40):
        bx.append((rnd(int(rng.integers(400, 701))), rnd(int(rng.integers(400, 701))), "unrelated", sc.OFFSETS))
    for m, rate in ((2000, .15), (2600, .30), (3300, .15), (4000, .15), (4096, .05)):
        a = rnd(m)
        bx.append((a, mutate(rng, a, rate, 4096), "large", sc.OFFSETS))
    bx.append((rnd(2100), rnd(2300), "large_unrelated", (0, 50)))
    bx.append((rnd(4096), rnd(3000), "large_unrelated", (99,)))
    for m, n in ((4097, 4097), (4500, 4400), (5000, 300), (200, 4200)):  # beyond what the kernel keeps: the host routine's
        a = rnd(m)
        b = mutate(rng, a, .1, n)
        bx.append((a, np.concatenate([b, rnd(n)])[:n], "beyond", (0, 99)))
    return bx


def make_tboxes(driver, tmp):
    bx = tbox_list()
    runs = [(i, off) for i, (_, _, _, offs) in enumerate(bx) for off in offs]
    inp, outp = os.path.join(tmp, "tboxes.in"), os.path.join(tmp, "tboxes.out")
    with open(inp, "wb") as f:
        f.write(struct.pack("<i", len(runs)))
        for i, off in runs:
            a, b = bx[i][0], bx[i][1]
            at = off + TW * (i % 3)                                      # not only in A's first interval
            f.write(struct.pack("<iii", len(a), len(b), at) + a.tobytes() + b.tobytes())
    subprocess.run([driver, inp, outp], check=True)
    buf, at = open(outp, "rb").read(), 0
    diffs, toff, trace = [], [0], []
    for _ in runs:
        d, n = struct.unpack_from("<ii", buf, at)
        trace.append(np.frombuffer(buf, dtype="<u2", count=n, offset=at + 8))
        at += 8 + 2 * n
        diffs.append(d)
        toff.append(toff[-1] + n)
    assert at == len(buf)
    m = np.array([len(x[0]) for x in bx], dtype=np.int32)
    n = np.array([len(x[1]) for x in bx], dtype=np.int32)
    aoff = np.concatenate([[0], np.cumsum(m + n)[:-1]]).astype(np.int64)
    bases = np.concatenate([np.concatenate(p[:2]) for p in bx]).astype(np.uint8)
    fams = sorted(set(x[2] for x in bx))
    family = np.array([fams.index(x[2]) for x in bx], dtype=np.int32)
    run_box = np.array([r[0] for r in runs], dtype=np.int32)
    run_abpos = np.array([r[1] + TW * (r[0] % 3) for r in runs], dtype=np.int32)
    diffs = np.array(diffs, dtype=np.int32)
    dst = os.path.join(OUT, "tboxes.npz")
    np.savez_compressed(dst, m=m, n=n, aoff=aoff, boff=aoff + m, bases=bases, family=family, families=np.array(fams), run_box=run_box,
                        run_abpos=run_abpos, diffs=diffs, toff=np.array(toff, dtype=np.int64), trace=np.concatenate(trace).astype(np.uint16))
    assert os.path.getsize(dst) < MAX_FILE, os.path.getsize(dst)
    for k, fam in enumerate(fams):                                       # every family is in the result
        assert np.any(family[run_box] == k), fam
    big = np.maximum(m, n)[run_box]
    assert np.any(big > 4096) and np.any((big > 1024) & (big <= 4096)) and np.any(diffs > big // 2)
    tl = np.diff(np.array(toff))
    assert np.all(tl == 2 * ((run_abpos + m[run_box] + TW - 1) // TW - run_abpos // TW))
    print("tboxes: %d boxes, %d runs, %d values, the largest difference count %d, %d bytes" % (len(bx), len(runs), toff[-1], diffs.max(),
                                                                                          os.path.getsize(dst)))


# ---- the synthetic file ----------------------------------------------------------------------------------------------

def write_synth(path):
    """true records of tiny2's file cut at trace points, so that the traces on both sides are real alignments, and what
    every group of pieces plants: -> (track anno, track data, plants)"""
    src = q_common.read_las(os.path.join(tc.GOLDEN, q_common.INPUTS["tiny2"][1]))
    buf = open(os.path.join(tc.GOLDEN, q_common.INPUTS["tiny2"][1]), "rb").read()
    novl = len(src["tlen"])
    rl = q_common.db_read_len("tiny2")
    at, words = 12, []
    for i in range(novl):
        words.append(np.frombuffer(buf, dtype="<i4", count=10, offset=at).copy())
        at += 40 + int(words[-1][0])
    tr = lambda i: src["trace"][src["trace_off"][i]:src["trace_off"][i] + src["tlen"][i]]

    def piece(i, s0, s1, flags=None, bshift=0):
        """segments [s0, s1) of record i as a record of its own"""
        w, t = words[i], tr(i)
        ab, ae = int(w[2]), int(w[4])
        first = ab // TW
        a0 = ab if s0 == 0 else (first + s0) * TW
        a1 = ae if s1 == len(t) // 2 else (first + s1) * TW
        b0 = int(w[3]) + int(t[1:2 * s0:2].sum())
        b1 = b0 + int(t[2 * s0 + 1:2 * s1:2].sum())
        tt = t[2 * s0:2 * s1]
        out = np.array([len(tt), int(tt[0::2].sum()), a0, b0 + bshift, a1, b1 + bshift, w[6] if flags is None else flags, w[7], w[8], 0],
                       dtype="<i4")
        return out.tobytes() + tt.tobytes()

    seen, normal, comp = set(), [], []
    for i in range(novl):                                                # one long record per pair of reads, so groups stay apart
        w = words[i]
        key = (int(w[7]), int(w[8]))
        if key in seen or w[7] == w[8] or (w[4] - w[2]) < 3600 or (w[6] & 2):
            continue
        if sum(1 for j in range(novl) if (int(words[j][7]), int(words[j][8])) == key) != 1:
            continue
        seen.add(key)
        (comp if w[6] & 1 else normal).append(i)
    assert len(normal) >= 18 and len(comp) >= 6, (len(normal), len(comp))
    groups, plants, lc = [], {}, {}
    KEYS = ("def", "f150", "f0", "t", "td", "wide", "far")

    def plant(tag, i, pieces, refused=(), **expect):
        """expect: records of the group stitched away per kind of case (sc.PLANT_KEY); a kind not named: as under the
        defaults, -f 0: none.  refused: the kinds in which the group's one candidate gets its box and Check_Bridge turns
        it down."""
        groups.append((int(words[i][7]), int(words[i][8]), len(groups), b"".join(pieces)))
        exp = {k: expect.get(k, 0 if k == "f0" else expect["def"]) for k in KEYS}
        plants[tag] = dict(aread=int(words[i][7]), bread=int(words[i][8]), pieces=len(pieces), expect=exp, refused=list(refused))

    nseg = lambda i: int(src["tlen"][i]) // 2
    blen = lambda i, s0, s1: int(tr(i)[2 * s0 + 1:2 * s1:2].sum())
    cut_of = lambda i, h: (int(words[i][2]) // TW + h) * TW
    it = iter(normal)
    i = next(it); h = nseg(i) // 2
    plant("gap0", i, [piece(i, 0, h), piece(i, h, nseg(i))], **{"def": 1})
    i = next(it); h = nseg(i) // 2                                       # |ae1 - ab2| = 100: past the default fuzz
    plant("overlap1", i, [piece(i, 0, h + 1), piece(i, h, nseg(i))], **{"def": 0, "f150": 1, "wide": 1, "far": 1})
    i = next(it); h = nseg(i) // 2
    plant("gap1", i, [piece(i, 0, h), piece(i, h + 1, nseg(i))], **{"def": 0, "f150": 1, "wide": 1, "far": 1})
    i = next(it); h = nseg(i) // 3
    plant("chain3", i, [piece(i, 0, h), piece(i, h, 2 * h), piece(i, 2 * h, nseg(i))], **{"def": 2})
    # the four ordering tests, each failed alone where it can be
    i = next(it); h = nseg(i) // 2
    plant("order_a", i, [piece(i, h, nseg(i)), piece(i, 0, h)], **{"def": 0})                # ab1 > ab2 (and bb1 > bb2)
    i = next(it); h = nseg(i) // 2
    plant("order_ae", i, [piece(i, 0, nseg(i)), piece(i, h, nseg(i) - 6)], **{"def": 0})     # ae1 > ae2
    i = next(it); h = nseg(i) // 3
    sh = blen(i, 0, h) + 50                                              # bb1 = bb2 + 50, the other three in order
    assert int(words[i][3]) + blen(i, 0, h) + sh <= int(words[i][5])
    plant("order_bb", i, [piece(i, 0, h, bshift=sh), piece(i, h, nseg(i))], **{"def": 0})
    i = next(it); h = nseg(i) // 2
    sh = -(blen(i, 0, h) - 100)                                          # bb2 = bb1 + 100, be2 some 1 100 below be1
    assert blen(i, h, h + 6) + 100 < blen(i, 0, h)
    plant("order_be", i, [piece(i, 0, h), piece(i, h, h + 6, bshift=sh)], **{"def": 0})
    i = next(it)
    plant("short", i, [piece(i, 0, 4), piece(i, 4, nseg(i))], **{"def": 0, "wide": 1})       # under 500 bases of A: no anchor but with -a 100
    i = next(it); h = nseg(i) // 2
    plant("strands", i, [piece(i, 0, h), piece(i, h, nseg(i), flags=1)], **{"def": 0})
    # the joint aligns badly: B of the second piece begins 140 (120) bases early, so the box holds that many bases of A
    # with nothing opposite around the cut: shared by the two intervals next to it they leave each 60 to 70 differences
    # over 30 to 40 bases of B, all in one a hundred over none: past 0.57 either way.  (39 early, under the default fuzz,
    # is shared out as 20 and 19 and passes: the reference stitches that.)
    for tag, sh in (("shifted", -140), ("shifted2", -120)):
        i = next(it); h = nseg(i) // 2
        plant(tag, i, [piece(i, 0, h), piece(i, h, nseg(i), bshift=sh)], refused=("f150", "wide", "far"), **{"def": 0})
        plants[tag]["widened"] = ["f150", "wide", "far"]                 # path 1 at the cut is past bb2 here too: two steps
    i = next(it); h = nseg(i) // 2
    plant("discarded_first", i, [piece(i, 0, h, flags=2), piece(i, h, nseg(i))], **{"def": 0})
    i = next(it); h = nseg(i) // 2
    w = words[i].copy()
    ident = [bytearray(piece(i, 0, h)), bytearray(piece(i, h, nseg(i)))]
    for p in ident:
        struct.pack_into("<i", p, 32, int(w[7]))
    groups.append((int(w[7]), int(w[7]), len(groups), b"".join(bytes(p) for p in ident)))
    plants["identity"] = dict(aread=int(w[7]), bread=int(w[7]), pieces=2, expect={k: 0 for k in KEYS}, refused=[])
    # an A overlap of one interval with B of the second piece 20 early: path 1 is past bb2 at ab2 (bin > bbpos), one
    # widening step; 20 bases of A alone in a box of 700 do not make a bad segment
    i = next(it); h = nseg(i) // 2
    plant("widen", i, [piece(i, 0, h + 1), piece(i, h, nseg(i), bshift=-20)], **{"def": 0, "f150": 1, "wide": 1, "far": 1})
    plants["widen"]["widened"] = ["f150", "wide", "far"]
    # the same at the very start of a record: the widening step runs off record 1 (it begins inside an interval): no box
    i = next(i for i in it if int(words[i][2]) % TW != 0 and int(tr(i)[1]) >= 12)
    plant("widen_off", i, [piece(i, 0, 3), piece(i, 1, nseg(i), bshift=-10)], **{"def": 0})
    plants["widen_off"]["no_box"] = ["wide"]
    # breaks in a low-complexity stretch (-t): three intervals gone, the track astride them
    for tag, anchor_ok in (("lc_break", True), ("lc_no_anchor", False), ("lc_250", True)):
        i = next(it)
        h = nseg(i) // 2 if anchor_ok else 6
        a, cut = int(words[i][7]), cut_of(i, h)
        if tag == "lc_break":                                            # a gap of 300 in both reads: -t, or a fuzz beyond it
            plant(tag, i, [piece(i, 0, h), piece(i, h + 3, nseg(i))], **{"def": 0, "t": 1, "td": 1, "far": 1})
        elif tag == "lc_no_anchor":                                      # 600 bases of A, 160 of them in the track: 440 anchor bases
            plant(tag, i, [piece(i, 0, h), piece(i, h + 3, nseg(i))], **{"def": 0, "far": 1})
        else:                                                            # 260 bases more of B in the gap: -d 0.6 lets it through,
            assert blen(i, nseg(i) - 4, nseg(i)) >= 260                   # an interval of the box then holds more than 250
            plant(tag, i, [piece(i, 0, h), piece(i, h + 3, nseg(i) - 4, bshift=260)], refused=("td", "far"), **{"def": 0})
        lc.setdefault(a, []).extend([(cut - 160, cut + 120), (cut + 125, cut + 135), (cut + 129, cut + 460)])
    # ten widening steps that stay inside both records and still leave path 1 past bb2: bout < bin
    far = [i for i in it if nseg(i) >= 48]
    if far:
        i = far[0]; h = nseg(i) // 2
        sh = -(blen(i, h - 10, h + 11) + 30)                             # B of piece 2 at cut + 1 100 lies below B of piece 1 at cut - 1 000
        assert blen(i, 0, h) >= -sh and blen(i, h, nseg(i)) + sh >= blen(i, h, h + 1) and blen(i, h, h + 1) - sh < 2400
        plant("far10", i, [piece(i, 0, h + 1), piece(i, h, nseg(i), bshift=sh)], **{"def": 0})
        plants["far10"]["no_box"] = ["far"]
    for n, i in enumerate(comp[:6]):                                     # what becomes of a complement joint is the reference's to say
        h = nseg(i) // 2
        groups.append((int(words[i][7]), int(words[i][8]), len(groups), piece(i, 0, h) + piece(i, h, nseg(i))))
        plants["comp%d" % n] = dict(aread=int(words[i][7]), bread=int(words[i][8]), pieces=2, expect=None, refused=None)

    groups.sort(key=lambda g: (g[0], g[2]))
    body = b"".join(g[3] for g in groups)
    nrec = sum(p["pieces"] for p in plants.values())
    open(path, "wb").write(struct.pack("<qi", nrec, TW) + body)
    anno, data = [0], []
    for r in range(len(rl)):
        for b, e in sorted(lc.get(r, [])):
            data += [max(b, 0), min(e, int(rl[r]))]
        anno.append(4 * len(data))
    return np.array(anno, dtype=np.uint64), np.array(data, dtype=np.int32), plants


def group_result(cols, plant):
    """(records of the plant's group that came out flagged as stitched away, the group's rows)"""
    rows = np.flatnonzero((cols[:, 7] == plant["aread"]) & (cols[:, 8] == plant["bread"]))
    return int(np.sum((cols[rows, 6] & 0x82) == 0x82)), rows


def main():
    tmp = tempfile.mkdtemp(prefix="stitch_golden_")
    try:
        lastitch, driver = build_tools(tmp)
        shutil.rmtree(OUT, ignore_errors=True)
        os.makedirs(OUT)
        make_tboxes(driver, tmp)
        anno, data, plants = write_synth(os.path.join(OUT, "synth.las"))
        np.savez_compressed(os.path.join(OUT, "lc_track.npz"), anno=anno, data=data)
        cases, md5s, total, chain, refused = [], {}, 0, 0, set()
        for name, inp, opts in sc.CASES:
            work = tempfile.mkdtemp(dir=tmp)
            sc.workdir(work, inp)
            r = subprocess.run([lastitch] + opts + ["G", sc.LAS, sc.OUT], cwd=work, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            assert r.returncode == 0, (name, r.stderr)
            out = os.path.join(work, sc.OUT)
            cols, trace, novl, tspace = tc.read_records(out)
            case = dict(name=name, input=inp, opts=opts, rc=r.returncode, stdout=r.stdout, stderr=r.stderr, md5=tc.md5(out))
            cases.append(case)
            md5s[name] = case["md5"]
            dst = os.path.join(OUT, "expected_%s.npz" % name)
            if inp == "ssynth":
                np.savez_compressed(dst, novl=novl, tspace=tspace, cols=cols, trace=trace)
            else:                                                        # the real files: the md5 holds the trace bytes
                np.savez_compressed(dst, novl=novl, tspace=tspace, cols=cols)
            assert os.path.getsize(dst) < MAX_FILE
            gone = int(np.sum((cols[:, 6] & 0x80) != 0))
            total += gone
            print("%-12s %6d records out, %4d flagged as stitched\n%s" % (name, novl, gone, r.stdout.replace("\x1b", "^")), end="")
            key = sc.PLANT_KEY.get(name)
            if key is not None:                                          # each planted group ends up as its plant says
                for tag, pl in plants.items():
                    got, rows = group_result(cols, pl)
                    pl.setdefault("seen", {})[name] = got
                    if pl["expect"] is None:
                        continue
                    want = pl["expect"][key]
                    assert got == want, "%s: plant %s has %d records stitched away, planted %d" % (name, tag, got, want)
                    if key in pl["refused"]:
                        refused.add((tag, key))
                    if tag == "chain3" and got == 2:
                        chain += 1
                        assert cols[rows[0], 4] == cols[rows[2], 4] and cols[rows[0], 5] == cols[rows[2], 5]
        # -L only caches reads: the same bytes as without it
        assert md5s["L_tiny2"] == md5s["def_tiny2"] and md5s["synth_L"] == md5s["synth"]
        # complement joints: the reference stitches some and refuses some (no test but Check_Bridge stands between a
        # two-piece complement group cut at a trace point and its stitch: the candidate tests pass as for gap0)
        for tag, pl in plants.items():
            if pl["expect"] is None:
                assert all(v == pl["seen"]["synth"] for k, v in pl["seen"].items() if k != "synth_f0") and pl["seen"]["synth_f0"] == 0, tag
                pl["expect"] = {k: 0 if k == "f0" else pl["seen"]["synth"] for k in ("def", "f150", "f0", "t", "td", "wide", "far")}
                pl["refused"] = [] if pl["seen"]["synth"] else ["def", "f150", "t", "td", "wide", "far"]
                refused.update((tag, k) for k in pl["refused"])
        comp_seen = [pl["seen"]["synth"] for t, pl in plants.items() if t.startswith("comp")]
        print("complement plants stitched:", comp_seen, " stitched away over all cases:", total, " refused:", len(refused),
              "of", len(set(t for t, _ in refused)), "plants")
        assert 0 in comp_seen and 1 in comp_seen
        assert total >= 20 and chain >= 1 and len(set(t for t, _ in refused)) >= 5
        assert plants["lc_break"]["seen"]["synth_t"] == 1
        assert "far10" in plants, "no record of tiny2 is long enough for ten widening steps"
        # the error paths
        work = tempfile.mkdtemp(dir=tmp)
        sc.workdir(work, "tiny2")
        errors = []
        for name, args in sc.ERRORS:
            r = subprocess.run([lastitch] + args, cwd=work, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            errors.append(dict(name=name, args=args, rc=r.returncode, stdout=r.stdout, stderr=r.stderr))
            assert r.returncode == 1, (name, r.returncode, r.stderr)
        json.dump(dict(cases=cases, errors=errors, plants=plants), open(os.path.join(OUT, "cases.json"), "w"), indent=1)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
