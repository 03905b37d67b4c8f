#!/usr/bin/env python3
"""Fixtures of LAtrim and of the exact box alignment under it (tests/golden/trim/) from the REFERENCE.

Runs only where the reference sources lie (REF_SRC, default /root/reference): LAq, LAtrim and a small driver around
Compute_Alignment(DIFF_ALIGN) are compiled with plain gcc lines into a temporary directory outside the repository, run on
.las files this repository already holds and on one synthetic file written here, and only data is kept: synth.las,
cases.json (options, exit status, stdout, stderr, md5 of the output), expected_<case>.npz (the trim track the case runs on,
the ten words of every expected record and their trace bytes) and boxes.npz.  Nothing compiled is kept.  The asserts at the
end hold the synthetic file to the branches it plants.

    python tests/golden/make_trim_golden.py
"""
import itertools
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
import trim_common as tc                               # noqa: E402
from make_q_golden import build_tool as build_laq, read_a2      # noqa: E402

OUT = tc.TDIR
TW = 100
MAX_FILE = 1 << 20

# our own driver: boxes in, what Compute_Alignment(DIFF_ALIGN) makes of them out
DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include "db/DB.h"
#include "dalign/align.h"

int main(int argc, char *argv[])
{ FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
  Work_Data *work = New_Work_Data();
  Alignment  al;
  Path       path;
  int        nbox, i, m, n;
  if (in == NULL || out == NULL || fread(&nbox, sizeof(int), 1, in) != 1)
    return 1;
  for (i = 0; i < nbox; i++)
    { char *a, *b;
      if (fread(&m, sizeof(int), 1, in) != 1 || fread(&n, sizeof(int), 1, in) != 1)
        return 1;
      a = malloc(m + 2);
      b = malloc(n + 2);
      a[0] = b[0] = 4;
      if (fread(a + 1, 1, m, in) != (size_t) m || fread(b + 1, 1, n, in) != (size_t) n)
        return 1;
      a[m + 1] = b[n + 1] = 4;
      al.path = &path;  al.flags = 0;  al.aseq = a + 1;  al.bseq = b + 1;  al.alen = m;  al.blen = n;
      path.abpos = path.bbpos = 0;  path.aepos = m;  path.bepos = n;
      path.diffs = (m + n > 30) ? m + n : 30;
      if (Compute_Alignment(&al, work, DIFF_ALIGN, 100))
        return 1;
      fwrite(&path.diffs, sizeof(int), 1, out);
      fwrite(&path.tlen, sizeof(int), 1, out);
      fwrite(path.trace, sizeof(int), path.tlen, out);
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
    subprocess.run(common + ["-o", os.path.join(tmp, "LAtrim"), s("scrub", "LAtrim.c"), s("lib", "trim.c"), s("lib", "read_loader.c"),
                             s("lib", "utils.c"), s("lib", "tracks.c"), s("lib", "pass.c"), s("lib", "compression.c"), s("db", "QV.c"),
                             s("db", "DB.c"), s("dalign", "align.c"), "-lm", "-lz", "-lpthread"], cwd=tmp, check=True)
    open(os.path.join(tmp, "boxdriver.c"), "w").write(DRIVER)
    subprocess.run(common + ["-o", os.path.join(tmp, "boxdriver"), os.path.join(tmp, "boxdriver.c"), s("dalign", "align.c"),
                             s("db", "DB.c"), s("db", "QV.c"), "-lm", "-lpthread"], cwd=tmp, check=True)
    return build_laq(tmp), os.path.join(tmp, "LAtrim"), os.path.join(tmp, "boxdriver")


# ---- the box cases ---------------------------------------------------------------------------------------------------

def mutate(rng, a, rate, n_max):
    out = []
    for x in a:
        u = rng.random()
        if u < rate / 3:
            continue
        if u < 2 * rate / 3:
            out.append(int(rng.integers(0, 4)))
        if u < rate:
            out.append(int((x + 1 + rng.integers(0, 3)) % 4))
        else:
            out.append(int(x))
    out = out[:n_max] or [0]
    return np.array(out, dtype=np.uint8)


def box_list():
    rng = np.random.default_rng(20261019)
    rnd = lambda n: rng.integers(0, 4, n).astype(np.uint8)
    bx = []
    for m, n in itertools.product((1, 2, 3), repeat=2):                  # every pair over a two-letter alphabet
        for bits in range(1 << (m + n)):
            s = [(bits >> k) & 1 for k in range(m + n)]
            bx.append((np.array(s[:m], dtype=np.uint8), np.array(s[m:], dtype=np.uint8)))
    for n in (1, 5, 64, 100, 125):                                       # no difference
        a = rnd(n)
        bx.append((a, a.copy()))
    for n in (2, 7, 65, 100):                                            # one difference: A longer, B longer, square
        a = rnd(n)
        for at in (0, n // 2, n - 1):
            bx.append((a, np.delete(a, at)))
            bx.append((np.delete(a, at), a))
            b = a.copy()
            b[at] = (b[at] + 1) % 4
            bx.append((a, b))
    for m, n in ((40, 40), (100, 120), (125, 255), (3, 200), (90, 2)):   # unrelated
        bx.append((rnd(m), rnd(n)))
    for n in (1, 60, 100, 140, 255):
        a = rnd(100)
        bx.append((a, mutate(rng, a, .2, n) if n > 1 else rnd(1)))
        if n > 1 and len(bx[-1][1]) < n:
            bx[-1] = (a, np.concatenate([bx[-1][1], rnd(n - len(bx[-1][1]))]))
    a = rnd(125)
    bx.append((a, np.concatenate([mutate(rng, a, .3, 255), rnd(255)])[:255]))
    for m, n in ((30, 30), (30, 37), (37, 30), (100, 131), (64, 65)):    # many optimal paths tie
        bx.append((np.zeros(m, dtype=np.uint8), np.zeros(n, dtype=np.uint8)))
        bx.append((np.arange(m, dtype=np.uint8) % 2, np.arange(n, dtype=np.uint8) % 2))
        bx.append((np.arange(m, dtype=np.uint8) % 2, (np.arange(n, dtype=np.uint8) + 1) % 2))
        bx.append((np.zeros(m, dtype=np.uint8), np.arange(n, dtype=np.uint8) % 2))
    small = len(bx)
    for rate in (.15, .30):
        for _ in range(1000):
            a = rnd(int(rng.integers(1, 126)))
            bx.append((a, mutate(rng, a, rate, 255)))
    for m, n in ((100, 1200), (900, 2000), (1500, 1400), (1001, 3)):     # beyond what the kernel keeps: the host routine's
        a = rnd(m)
        b = mutate(rng, a, .15, n)
        bx.append((a, b if m > 1000 and n < 10 else np.concatenate([b, rnd(n)])[:n]))
    return bx, small


def run_boxes(driver, tmp, bx):
    inp, outp = os.path.join(tmp, "boxes.in"), os.path.join(tmp, "boxes.out")
    with open(inp, "wb") as f:
        f.write(struct.pack("<i", len(bx)))
        for a, b in bx:
            f.write(struct.pack("<ii", len(a), len(b)) + a.tobytes() + b.tobytes())
    subprocess.run([driver, inp, outp], check=True)
    buf, at = open(outp, "rb").read(), 0
    diffs, soff, script = [], [0], []
    for _ in bx:
        d, n = struct.unpack_from("<ii", buf, at)
        script.append(np.frombuffer(buf, dtype="<i4", count=n, offset=at + 8))
        at += 8 + 4 * n
        diffs.append(d)
        soff.append(soff[-1] + n)
    assert at == len(buf)
    return np.array(diffs, dtype=np.int32), np.array(soff, dtype=np.int64), np.concatenate(script).astype(np.int32)


def make_boxes(driver, tmp):
    bx, small = box_list()
    diffs, soff, script = run_boxes(driver, tmp, bx)
    m = np.array([len(a) for a, _ in bx], dtype=np.int32)
    n = np.array([len(b) for _, b in bx], dtype=np.int32)
    aoff = np.concatenate([[0], np.cumsum(m + n)[:-1]]).astype(np.int64)
    bases = np.concatenate([np.concatenate(p) for p in bx]).astype(np.uint8)
    np.savez_compressed(os.path.join(OUT, "boxes.npz"), m=m, n=n, aoff=aoff, boff=aoff + m, bases=bases, diffs=diffs, soff=soff,
                        script=script, small=small)
    sq = (m == n)
    assert np.any(diffs == 0) and np.any((diffs == 1) & (m > n)) and np.any((diffs == 1) & (m < n)) and np.any((diffs == 1) & sq)
    assert np.any(diffs > (m + n) // 3) and np.any(np.maximum(m, n) > 1000)
    print("boxes: %d, %d script values, the largest difference count %d" % (len(bx), len(script), diffs.max()))


# ---- the synthetic file ----------------------------------------------------------------------------------------------

def read_bases(db, r):
    """read r of a fixture database, one value per base"""
    idx = open(os.path.join(tc.GOLDEN, db, ".G.idx"), "rb").read()
    n = struct.unpack_from("<i", idx, 0)[0]
    recs = np.frombuffer(idx, dtype="<i4", offset=len(idx) - 32 * n).reshape(n, 8)
    rlen, boff = int(recs[r, 0]), int(np.frombuffer(recs[r, 2:4].tobytes(), dtype="<i8")[0])
    raw = np.frombuffer(open(os.path.join(tc.GOLDEN, db, ".G.bps"), "rb").read(), dtype=np.uint8, count=(rlen + 3) // 4, offset=boff)
    return np.stack([(raw >> 6) & 3, (raw >> 4) & 3, (raw >> 2) & 3, raw & 3], axis=1).reshape(-1)[:rlen]


def is_subsequence(a, b):
    at = 0
    for x in b:
        if at < len(a) and x == a[at]:
            at += 1
    return at == len(a)


def write_synth(path):
    """records on tiny2's reads, spacing 100, and the trim track they meet: -> (anno, data, what each planted record must
    look like afterwards)"""
    rl = q_common.db_read_len("tiny2")
    nreads = len(rl)
    long_enough = [r for r in range(nreads) if rl[r] >= 7000]
    assert len(long_enough) >= 12
    A0, A4, A6 = long_enough[0], long_enough[1], long_enough[2]
    B = long_enough[3:12]
    trim = {r: (0, int(rl[r])) for r in range(nreads)}
    recs, plant = [], {}

    def rec(tag, a, b, ab, ae, bb, blens, flags=0):
        nseg = (ae + TW - 1) // TW - ab // TW
        assert len(blens) == nseg
        tr = bytes(int(x) for bl in blens for x in (7, bl))
        recs.append((a, len(recs), tag, struct.pack("<10i", 2 * nseg, 7 * nseg, ab, bb, ae, bb + sum(blens), flags, a, b, 0) + tr))

    # both cuts inside one trace segment
    trim[B[0]] = (2210, 2260)
    rec("same", A0, B[0], 1000, 1500, 2000, [100] * 5)
    plant["same"] = dict(tlen=2, bbpos=2210, bepos=2260)
    # cuts exactly on a segment's B boundaries: nothing is aligned
    trim[B[1]] = (2200, 2400)
    rec("edge", A0, B[1], 1000, 1500, 2000, [100] * 5)
    plant["edge"] = dict(tlen=4, abpos=1200, aepos=1400, bbpos=2200, bepos=2400)
    # the cut's A coordinate is the segment's end: five bases of A against 250 of B, all five matched before the cut
    a_tail = read_bases("tiny2", A0)[1095:1100]
    bseq = read_bases("tiny2", B[2])
    bb = next(x for x in range(3000, 4000) if is_subsequence(a_tail, bseq[x:x + 249]) and bseq[x + 249] != a_tail[4])
    trim[B[2]] = (bb + 249, int(rl[B[2]]))
    rec("dec", A0, B[2], 1095, 1500, bb, [250, 100, 100, 100, 100])
    plant["dec"] = dict(abpos=1099, bbpos=bb + 249, tlen=10)
    # a complement record cut on both sides, each inside a segment
    blen = int(rl[B[3]])
    trim[B[3]] = (blen - 2440, blen - 2130)
    rec("comp", A0, B[3], 1000, 1500, 2000, [100] * 5, flags=1)
    plant["comp"] = dict(bbpos=2130, bepos=2440, tlen=8)
    # the B read keeps nothing: an empty interval, an inverted one, and no entry at all
    trim[B[4]] = (500, 500)
    trim[B[5]] = (600, 400)
    trim[B[6]] = None
    for b in B[4:7]:
        rec("none", A0, b, 1000, 1500, 2000, [100] * 5)
    plant["none"] = dict(flags=2 | (1 << 17), abpos=1000, tlen=10)
    # untouched
    rec("asis", A0, B[7], 1000, 1500, 2000, [100] * 5)
    plant["asis"] = dict(flags=0, abpos=1000, aepos=1500, tlen=10)
    # cut on A only: whole segments go, B follows
    trim[A4] = (1250, 1730)
    rec("aonly", A4, B[7], 1000, 2000, 3000, [90, 110] * 5)
    plant["aonly"] = dict(abpos=1250, aepos=1730, bbpos=3200, bepos=3800, tlen=12, flags=0)
    # what the cut on A leaves of B lies outside what B keeps: the final test discards it
    trim[A6] = (1000, 1300)
    trim[B[8]] = (5500, int(rl[B[8]]))
    rec("final", A6, B[8], 1000, 2000, 5000, [100] * 10)
    plant["final"] = dict(flags=2 | (1 << 17), aepos=1300, bepos=5300, tlen=6)

    recs.sort(key=lambda x: (x[0], x[1]))
    open(path, "wb").write(struct.pack("<qi", len(recs), TW) + b"".join(r[3] for r in recs))
    anno, data = [0], []
    for r in range(nreads):
        if trim[r] is not None:
            data += list(trim[r])
        anno.append(4 * len(data))
    return np.array(anno, dtype=np.uint64), np.array(data, dtype=np.int32), [r[2] for r in recs], plant


COLS = dict(tlen=0, diffs=1, abpos=2, bbpos=3, aepos=4, bepos=5, flags=6, aread=7, bread=8)


def main():
    tmp = tempfile.mkdtemp(prefix="trim_golden_")
    try:
        laq, latrim, driver = build_tools(tmp)
        shutil.rmtree(OUT, ignore_errors=True)
        os.makedirs(OUT)
        make_boxes(driver, tmp)
        s_anno, s_data, s_tags, s_plant = write_synth(os.path.join(OUT, "synth.las"))
        cases = []
        for name, inp, src, opts in tc.CASES:
            work = tempfile.mkdtemp(dir=tmp)
            db = tc.INPUTS[inp][0]
            for f in ("G.db", ".G.idx", ".G.bps"):
                shutil.copy(os.path.join(tc.GOLDEN, db, f), os.path.join(work, f))
            shutil.copy(os.path.join(tc.GOLDEN, tc.INPUTS[inp][1]), os.path.join(work, tc.LAS))
            tname = tc.track_name(opts)
            if src == "synth":
                anno, data = s_anno, s_data
                tc.write_track_a2(os.path.join(work, ".G." + tname), len(anno) - 1, anno, data)
            else:
                r = q_common.run_tool(laq, src, work)
                assert r.returncode == 0, (name, r.stderr)
                _, anno, data = read_a2(os.path.join(work, ".G." + tname))
            r = subprocess.run([latrim] + opts + ["G", tc.LAS, tc.OUT], cwd=work, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            assert r.returncode == 0, (name, r.stderr)
            out = os.path.join(work, tc.OUT)
            cols, trace, novl, tspace = tc.read_records(out)
            case = dict(name=name, input=inp, opts=opts, rc=r.returncode, stdout=r.stdout, stderr=r.stderr, md5=tc.md5(out))
            cases.append(case)
            dst = os.path.join(OUT, "expected_%s.npz" % name)
            np.savez_compressed(dst, trim_anno=anno, trim_data=data, novl=novl, tspace=tspace, cols=cols, trace=trace)
            if os.path.getsize(dst) >= MAX_FILE:
                np.savez_compressed(dst, trim_anno=anno, trim_data=data, novl=novl, tspace=tspace, cols=cols)
            assert os.path.getsize(dst) < MAX_FILE
            nin = q_common.read_las(os.path.join(work, tc.LAS))["tlen"].shape[0]
            gone = int(np.sum((cols[:, 6] & 2) != 0))
            print("%-14s %6d records in, %6d out, %6d flagged\n%s" % (name, nin, novl, gone, r.stdout.replace("\x1b", "^")), end="")
            if name == "d20_tandem":
                assert gone == novl == nin, "every record of the -d20 track's case is discarded"
            if name == "d20_tandem_p":
                assert novl == 0 and os.path.getsize(out) == 12
            if name == "synth":                                          # each planted record looks as its coordinates say
                assert novl == len(s_tags)
                for i, tag in enumerate(s_tags):
                    for k, v in s_plant[tag].items():
                        assert cols[i, COLS[k]] == v, "synth record %d (%s): %s is %d, planted %d" % (i, tag, k, cols[i, COLS[k]], v)
        # the error paths
        work = tempfile.mkdtemp(dir=tmp)
        for f in ("G.db", ".G.idx", ".G.bps"):
            shutil.copy(os.path.join(tc.GOLDEN, "tiny2", f), os.path.join(work, f))
        shutil.copy(os.path.join(tc.GOLDEN, tc.INPUTS["tiny2"][1]), os.path.join(work, tc.LAS))
        errors = []
        for name, args in (("no_track", ["-t", "nosuch", "G", tc.LAS, tc.OUT]), ("no_las", ["G", "nosuch.las", tc.OUT]),
                           ("no_args", ["G", tc.LAS]), ("bad_option", ["-x", "G", tc.LAS, tc.OUT])):
            r = subprocess.run([latrim] + args, cwd=work, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            errors.append(dict(name=name, args=args, rc=r.returncode, stdout=r.stdout, stderr=r.stderr))
            assert r.returncode == 1, (name, r.returncode, r.stderr)
        json.dump(dict(cases=cases, errors=errors), open(os.path.join(OUT, "cases.json"), "w"), indent=1)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
