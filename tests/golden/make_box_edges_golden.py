#!/usr/bin/env python3
"""Fixtures that hold the box kernels to every size they admit (tests/golden/trim/boxes_wide.npz for kernels/box_align.hip,
tests/golden/stitch/tboxes_wide.npz for kernels/box_trace.hip) from the REFERENCE.

Runs only where the reference sources lie (REF_SRC, default /root/reference): two small drivers, one around
Compute_Alignment(DIFF_ALIGN) and one around Compute_Alignment(DIFF_TRACE, spacing) that takes the spacing per run, are
compiled with plain gcc lines into a temporary directory outside the repository, and only data is kept.  The two files have
the layout of boxes.npz and tboxes.npz (trim_common.box_seqs / check_boxes and stitch_common.run_seqs / check_runs read
them), and beside it: family / families (what a box was planted for), planted (boxes_wide: the substitutions planted into a
ladder box, -1 elsewhere) and run_tspace (tboxes_wide: the spacing of a run).  No other fixture is touched.

What the families are for is said where they are made; the asserts at the end of make_boxes_wide and make_tboxes_wide hold
every family to the property it was planted for.  The reference's routine took every spacing asked of it (16, 64, 126, 255,
1000): none is left out.

    python tests/golden/make_box_edges_golden.py
"""
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
import stitch_common as sc                             # noqa: E402
import trim_common as tc                               # noqa: E402
from make_trim_golden import DRIVER as ALIGN_DRIVER, mutate, run_boxes        # noqa: E402

MAX_FILE = 1 << 20
BOX_MAX = 1000                                         # DAMAR_BOX_MAXLEN
TBOX_MAX = 4096                                        # DAMAR_TBOX_MAXLEN
TB_SMALL = 1024                                        # the largest box of box_trace's first build
WAVE = 64

# our own driver: runs in, what Compute_Alignment(DIFF_TRACE) at the run's spacing makes of them out
TRACE_DRIVER = r"""
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
  int        nrun, i, m, n, at, ts;
  if (in == NULL || out == NULL || fread(&nrun, sizeof(int), 1, in) != 1)
    return 1;
  for (i = 0; i < nrun; i++)
    { char *a, *b;
      if (fread(&m, sizeof(int), 1, in) != 1 || fread(&n, sizeof(int), 1, in) != 1 || fread(&at, sizeof(int), 1, in) != 1 ||
          fread(&ts, sizeof(int), 1, in) != 1)
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
      if (Compute_Alignment(&al, work, DIFF_TRACE, ts))
        return 2;
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


def build_drivers(tmp):
    s = lambda *p: os.path.join(SRC, *p)
    out = []
    for name, text in (("boxdriver", ALIGN_DRIVER), ("tboxdriver", TRACE_DRIVER)):
        open(os.path.join(tmp, name + ".c"), "w").write(text)
        subprocess.run(["gcc", "-O3", "-w", "-fno-strict-aliasing", "-I" + SRC, "-o", os.path.join(tmp, name), os.path.join(tmp, name + ".c"),
                        s("dalign", "align.c"), s("db", "DB.c"), s("db", "QV.c"), "-lm", "-lpthread"], cwd=tmp, check=True)
        out.append(os.path.join(tmp, name))
    return out


def meeting_lane(a, b):
    """the search of kernels/box_search.h (host/bridge.c middle) on the whole box, with the diagonals of a frontier numbered
    from the top as the kernel deals them to its lanes: -> (differences, the number of the diagonal the searches meet on)"""
    a, b = [int(x) for x in a], [int(x) for x in b]
    M, N = len(a), len(b)
    dl = M - N

    def fwd(k, r):
        end = min(N, M - k)
        while r < end and k + r >= 0 and b[r] == a[k + r]:
            r += 1
        return r

    def bwd(k, r):
        top = max(-k, 0)
        while r >= top and r < N and k + r < M and b[r] == a[k + r]:
            r -= 1
        return r

    r0 = fwd(0, 0)
    if r0 >= M and N == M:
        return 0, 0
    F, G = {0: r0}, {dl: bwd(dl, N - 1)}
    flo = fhi = 0
    glo = ghi = dl
    d = 0
    while True:
        d += 1
        nf = {}
        for i, k in enumerate(range(fhi + 1, flo - 2, -1)):
            right = (F[k + 1] if k + 1 <= fhi else -3 if k + 1 > fhi + 1 else -2) + 1
            diag = (F[k] if flo <= k <= fhi else -3 if k > fhi + 1 else -2) + 1
            down = F[k - 1] if k - 1 >= flo else -2
            r = max(right, diag, down)
            if glo <= k <= ghi and r > G[k]:
                return 2 * d - 1, i
            nf[k] = fwd(k, r)
        F, flo, fhi = nf, flo - 1, fhi + 1
        ng = {}
        for i, k in enumerate(range(ghi + 1, glo - 2, -1)):
            left = (G[k + 1] if k + 1 <= ghi else N + 1) + 1
            diag = G[k] if glo <= k <= ghi else N + 1
            up = G[k - 1] if k - 1 >= glo else N + 1
            r = min(left, diag, up)
            if flo <= k <= fhi and r <= F[k]:
                return 2 * d, i
            ng[k] = bwd(k, r - 1)
        G, glo, ghi = ng, glo - 1, ghi + 1


def tie_makers(m, n):
    """the four of make_trim_golden.box_list: many optimal paths tie"""
    return [(np.zeros(m, dtype=np.uint8), np.zeros(n, dtype=np.uint8)),
            (np.arange(m, dtype=np.uint8) % 2, np.arange(n, dtype=np.uint8) % 2),
            (np.arange(m, dtype=np.uint8) % 2, (np.arange(n, dtype=np.uint8) + 1) % 2),
            (np.zeros(m, dtype=np.uint8), np.arange(n, dtype=np.uint8) % 2)]


def pack(bx):
    m = np.array([len(x[0]) for x in bx], dtype=np.int32)
    n = np.array([len(x[1]) for x in bx], dtype=np.int32)
    aoff = np.concatenate([[0], np.cumsum(m + n)[:-1]]).astype(np.int64)
    bases = np.concatenate([np.concatenate(p[:2]) for p in bx]).astype(np.uint8)
    fams = sorted(set(x[2] for x in bx))
    family = np.array([fams.index(x[2]) for x in bx], dtype=np.int32)
    return dict(m=m, n=n, aoff=aoff, boff=aoff + m, bases=bases, family=family, families=np.array(fams))


# ---- DIFF_ALIGN: kernels/box_align.hip, every box up to 1000 ---------------------------------------------------------

def wide_box_list():
    """(A, B, family, substitutions planted or -1)"""
    rng = np.random.default_rng(20261021)
    rnd = lambda n: rng.integers(0, 4, n).astype(np.uint8)
    fit = lambda b, n: np.concatenate([b, rnd(n)])[:n]
    bx = []
    # limit: the last sizes the kernel takes, related and unrelated, and the first ones it leaves to the host routine
    for m, n in ((1000, 1000), (999, 1000), (1000, 999), (1000, 1), (1, 1000), (1000, 500), (500, 1000)):
        a = rnd(m)
        bx.append((a, fit(mutate(rng, a, .15, n), n), "limit", -1))
        bx.append((rnd(m), rnd(n), "limit", -1))
    for m, n in ((1001, 1000), (1000, 1001), (1001, 1)):
        a = rnd(m)
        bx.append((a, fit(mutate(rng, a, .15, n), n), "limit", -1))
    # worst: as many differences as the longer side has bases, the most a frontier has to hold
    for m, n in ((1000, 1000), (999, 999), (1000, 700), (700, 1000)):
        bx.append((np.zeros(m, dtype=np.uint8), np.ones(n, dtype=np.uint8), "worst", -1))
    bx.append((np.arange(1000, dtype=np.uint8) % 2, 2 + np.arange(1000, dtype=np.uint8) % 2, "worst", -1))
    # ladder: difference counts around 64, 128 and 256, where a frontier takes another chunk of 64 diagonals; odd counts
    # meet in the forward step, even ones in the backward step.  A is random over the values 0, 1, 2 and a substitution
    # writes a 3: a base of B that is like none of A costs a difference wherever it goes, so D of them cost exactly D (over
    # four values, 253 and more substitutions in 600 bases leave a cheaper path with indels: 293 for 300)
    for D in list(range(61, 68)) + list(range(125, 132)) + list(range(253, 260)) + [300]:
        a = rng.integers(0, 3, 600).astype(np.uint8)
        at = (np.arange(D) * 600) // D
        b = a.copy()
        b[at] = 3
        bx.append((a, b, "ladder", D))
        b = a.copy()
        b[at[0::2]] = 3
        bx.append((a, np.delete(b, at[1::2]), "ladder", -1))
    # skew: |M - N| large, the meeting diagonal far from the top of the frontier
    for rate in (.05, .15):
        for m, n in ((400, 470), (600, 730), (300, 500), (550, 1000), (250, 950)):
            for mm, nn in ((m, n), (n, m)):
                a = rnd(mm)
                bx.append((a, fit(mutate(rng, a, rate, nn), nn), "skew", -1))
        a = rnd(1000)
        bx.append((a, fit(mutate(rng, a, rate, 300), 300), "skew", -1))
    for m, n in ((500, 500), (500, 563), (563, 500), (1000, 937), (256, 257)):
        bx += [(a, b, "ties", -1) for a, b in tie_makers(m, n)]
    for i in range(200):
        a = rnd(int(rng.integers(256, 1001)))
        bx.append((a, mutate(rng, a, (.05, .15, .30)[i % 3], 1000), "random", -1))
    return bx


def make_boxes_wide(driver, tmp):
    bx = wide_box_list()
    diffs, soff, script = run_boxes(driver, tmp, [p[:2] for p in bx])
    z = pack(bx)
    planted = np.array([p[3] for p in bx], dtype=np.int32)
    dst = os.path.join(tc.TDIR, "boxes_wide.npz")
    np.savez_compressed(dst, diffs=diffs, soff=soff, script=script, planted=planted, **z)
    assert os.path.getsize(dst) < MAX_FILE, os.path.getsize(dst)
    m, n, big = z["m"], z["n"], np.maximum(z["m"], z["n"])
    fam = lambda name: np.flatnonzero(z["family"] == list(z["families"]).index(name))
    sizes = lambda rows: set(zip(m[rows].tolist(), n[rows].tolist()))
    assert np.sum(big[fam("limit")] > BOX_MAX) == 3 and np.sum(big[fam("limit")] == BOX_MAX) == 14
    assert np.all(big[np.concatenate([fam(f) for f in z["families"] if f != "limit"])] <= BOX_MAX)
    assert len(fam("worst")) == 5 and np.all(diffs[fam("worst")] == big[fam("worst")])
    lad = fam("ladder")
    pure = lad[planted[lad] >= 0]
    assert len(lad) == 44 and len(pure) == 22 and np.all(diffs[pure] == planted[pure]), (diffs[pure], planted[pure])
    assert np.all(diffs[np.setdiff1d(lad, pure)] <= planted[pure])        # D/2 substitutions and D/2 deletions: D at the most
    assert set(abs(int(x)) for x in (m - n)[fam("skew")]) == {70, 130, 200, 450, 700} and len(fam("skew")) == 22
    assert np.any((m - n)[fam("skew")] == 700) and np.any((m - n)[fam("skew")] == -700)
    lanes = {f: [meeting_lane(*bx[i][:2]) for i in fam(f)] for f in ("skew", "ladder")}
    for f in lanes:
        assert [d for d, _ in lanes[f]] == diffs[fam(f)].tolist(), f       # the model of the search is the search
    # a box whose surplus is a random tail has many optimal paths, and the sweep from the top takes the highest diagonal that
    # meets: about half the skew boxes meet in the first chunk for that reason; the others must be far from it, on both sides
    skew = [(int((m - n)[i]), lane) for i, (_, lane) in zip(fam("skew"), lanes["skew"])]
    assert any(dl > 0 and lane >= WAVE for dl, lane in skew) and any(dl < 0 and lane >= WAVE for dl, lane in skew), skew
    assert sum(lane >= WAVE for _, lane in skew) >= 8 and max(lane for _, lane in skew) >= 8 * WAVE, skew
    chunks = sorted(set(lane // WAVE for f in lanes for _, lane in lanes[f]))
    # substitutions alone meet on diagonal 0, lane d of a frontier of d differences: 63 and 64, 127 and 128 are the borders
    assert {63, 64, 127, 128} <= set(lane for _, lane in lanes["ladder"]) and set(chunks) >= {0, 1, 2, 3}, chunks
    assert sizes(fam("ties")) == {(500, 500), (500, 563), (563, 500), (1000, 937), (256, 257)} and len(fam("ties")) == 20
    assert len(fam("random")) == 200 and m[fam("random")].min() >= 256 and big[fam("random")].max() <= BOX_MAX
    print("boxes_wide: %d boxes (%s), %d script values, the largest difference count %d, meetings in chunks %s, %d bytes"
          % (len(bx), ", ".join("%s %d" % (f, len(fam(f))) for f in z["families"]), len(script), diffs.max(), chunks, os.path.getsize(dst)))


# ---- DIFF_TRACE: kernels/box_trace.hip, both builds, other spacings, the ledger's bound -------------------------------

def wide_tbox_list():
    """(A, B, family, the (spacing, offset) pairs it runs at)"""
    rng = np.random.default_rng(20261022)
    rnd = lambda n: rng.integers(0, 4, n).astype(np.uint8)
    fit = lambda b, n: np.concatenate([b, rnd(n)])[:n]
    at100 = tuple((sc.TW, off) for off in sc.OFFSETS)
    bx = []
    # build_border: the last sizes of box_trace<1032> and the first of box_trace<4104>
    for big in (1023, 1024, 1025, 1026):
        for m, n in ((big, big - 60), (big - 60, big)):
            a = rnd(m)
            bx.append((a, fit(mutate(rng, a, .15, n), n), "build_border", at100))
            bx.append((rnd(m), rnd(n), "build_border", at100))
    for i in range(40):
        a = rnd(int(rng.integers(701, 2001)))
        bx.append((a, mutate(rng, a, (.15, .30)[i % 2], TBOX_MAX), "middle", at100))
    for _ in range(6):
        bx.append((rnd(int(rng.integers(701, 2001))), rnd(int(rng.integers(701, 2001))), "middle", at100))
    # worst: as many differences as the longer side has bases; the last frontier step of either build
    for m, n in ((1024, 1024), (1024, 600), (4096, 4096), (4096, 2000)):
        bx.append((np.zeros(m, dtype=np.uint8), np.ones(n, dtype=np.uint8), "worst", ((sc.TW, 0), (sc.TW, 99))))
    # spacing: the arithmetic of intervals, room and ledger cells at other spacings than 100
    spacings = {ts: (0, 1, ts - 1, 2 * ts + 7) for ts in (16, 64, 126, 255, 1000)}
    everywhere = tuple((ts, off) for ts, offs in spacings.items() for off in offs)
    for i in range(30):
        a = rnd(int(rng.integers(50, 901)))
        bx.append((a, mutate(rng, a, (.15, .30)[i % 2], TBOX_MAX), "spacing", everywhere))
    for ts, offs in spacings.items():                                    # the boundary and fold makers of tbox_list
        for off in offs:
            for k in (1, 2, 3):
                a = rnd(k * ts - off % ts)
                bx.append((a, mutate(rng, a, .15, TBOX_MAX), "spacing", ((ts, off),)))
                bx.append((a, np.concatenate([a, rnd(7)]), "spacing", ((ts, off),)))
                bx.append((a, np.concatenate([mutate(rng, a, .15, TBOX_MAX - 2), 3 - a[-1:], 3 - a[-1:]]), "spacing", ((ts, off),)))
    # ledger: 512 cells are the last the kernel takes
    a = rnd(4080)
    bx.append((a, mutate(rng, a, .05, TBOX_MAX), "ledger", ((16, 0), (16, 1))))
    a = rnd(4081)
    bx.append((a, mutate(rng, a, .05, TBOX_MAX), "ledger", ((16, 0),)))
    return bx


def ncell(m, abpos, ts):
    """the ledger cells kernels/box_trace.hip needs for a run"""
    return 2 * ((abpos % ts + m + ts - 1) // ts + 1)


def make_tboxes_wide(driver, tmp):
    bx = wide_tbox_list()
    runs = [(i, off + ts * (i % 3), ts) for i, p in enumerate(bx) for ts, off in p[3]]      # not only in A's first interval
    inp, outp = os.path.join(tmp, "tboxes.in"), os.path.join(tmp, "tboxes.out")
    with open(inp, "wb") as f:
        f.write(struct.pack("<i", len(runs)))
        for i, at, ts in runs:
            a, b = bx[i][0], bx[i][1]
            f.write(struct.pack("<iiii", len(a), len(b), at, ts) + a.tobytes() + b.tobytes())
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
    z = pack(bx)
    run_box = np.array([r[0] for r in runs], dtype=np.int32)
    run_abpos = np.array([r[1] for r in runs], dtype=np.int32)
    run_tspace = np.array([r[2] for r in runs], dtype=np.int32)
    diffs = np.array(diffs, dtype=np.int32)
    dst = os.path.join(sc.SDIR, "tboxes_wide.npz")
    np.savez_compressed(dst, run_box=run_box, run_abpos=run_abpos, run_tspace=run_tspace, diffs=diffs, toff=np.array(toff, dtype=np.int64),
                        trace=np.concatenate(trace).astype(np.uint16), **z)
    assert os.path.getsize(dst) < MAX_FILE, os.path.getsize(dst)
    m, n = z["m"][run_box], z["n"][run_box]
    big = np.maximum(m, n)
    fam = lambda name: np.flatnonzero(z["family"][run_box] == list(z["families"]).index(name))
    assert np.all(big <= TBOX_MAX)
    assert np.all(np.diff(np.array(toff)) == 2 * ((run_abpos + m + run_tspace - 1) // run_tspace - run_abpos // run_tspace))
    rows = fam("build_border")
    for size in (1023, 1024, 1025, 1026):                                # either side the larger one, related and not
        for side in (m, n):
            at_size = rows[(side[rows] == size) & (big[rows] == size)]
            assert np.any(diffs[at_size] < size // 3) and np.any(diffs[at_size] > size // 3), size
    rows = fam("middle")
    assert len(set(run_box[rows])) == 46 and np.all((m[rows] > 700) & (m[rows] <= 2000))
    assert np.any(big[rows] <= TB_SMALL) and np.any(big[rows] > TB_SMALL)
    rows = fam("worst")
    assert len(rows) == 8 and np.all(diffs[rows] == big[rows]) and set(run_abpos[rows] % sc.TW) == {0, 99}
    assert sorted(set(zip(m[rows].tolist(), n[rows].tolist()))) == [(1024, 600), (1024, 1024), (4096, 2000), (4096, 4096)]
    assert np.all(run_tspace[np.concatenate([fam(f) for f in ("build_border", "middle", "worst")])] == sc.TW)
    rows = fam("spacing")
    for ts in (16, 64, 126, 255, 1000):
        orgs = (run_abpos % run_tspace)[rows[run_tspace[rows] == ts]]
        assert set(orgs.tolist()) == {0, 1, ts - 1, 7}, (ts, set(orgs.tolist()))
    assert np.all(ncell(m[rows], run_abpos[rows], run_tspace[rows]) <= 512)
    rows = fam("ledger")
    assert sorted(ncell(m[rows], run_abpos[rows], run_tspace[rows]).tolist()) == [512, 514, 514] and np.all(run_tspace[rows] == 16)
    print("tboxes_wide: %d boxes, %d runs (%s), %d values, the largest difference count %d, %d bytes"
          % (len(bx), len(runs), ", ".join("%s %d" % (f, len(fam(f))) for f in z["families"]), toff[-1], diffs.max(), os.path.getsize(dst)))


def main():
    tmp = tempfile.mkdtemp(prefix="box_edges_golden_")
    try:
        align_driver, trace_driver = build_drivers(tmp)
        make_boxes_wide(align_driver, tmp)
        make_tboxes_wide(trace_driver, tmp)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
