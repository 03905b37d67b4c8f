#!/usr/bin/env python3
"""Fixtures of LAq (tests/golden/q/) from the REFERENCE's LAq.

Runs only where the reference sources lie (REF_SRC, default /root/reference): the tool is compiled with a plain gcc line
(source set of scrub/Makefile.in) into a temporary directory outside the repository, run on .las files this repository
already holds (tests/q_common.py INPUTS) and on one small synthetic file written here, and only data is kept: synth.las,
cases.json (options, exit status, stdout, stderr) and expected_<case>.npz with the inflated q / trim anno and data.
Nothing compiled is kept.  The asserts at the end hold the set to the branches the tests are meant to reach.

    python tests/golden/make_q_golden.py
"""
import json
import os
import shutil
import struct
import sys
import tempfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
SRC = os.environ.get("REF_SRC", "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import q_common                                        # noqa: E402
import q_model                                         # noqa: E402

OUT = q_common.QDIR


def build_tool(tmp):
    s = lambda *p: os.path.join(SRC, *p)
    q_common.subprocess.run(["gcc", "-O3", "-w", "-fno-strict-aliasing", "-I" + SRC, "-o", os.path.join(tmp, "LAq"),
                             s("scrub", "LAq.c"), s("lib", "utils.c"), s("lib", "tracks.c"), s("lib", "pass.c"), s("db", "QV.c"),
                             s("dalign", "align.c"), s("db", "DB.c"), s("lib", "compression.c"), "-lm", "-lz", "-lpthread"],
                            cwd=tmp, check=True)
    return os.path.join(tmp, "LAq")


def inflate(buf):
    out, at = b"", 0
    while at < len(buf):
        n = struct.unpack_from("<Q", buf, at)[0]
        out += zlib.decompress(buf[at + 8:at + 8 + n])
        at += 8 + n
    return out


def read_a2(prefix):
    a = open(prefix + ".a2", "rb").read()
    version, size, _pad, length, clen, cdlen = struct.unpack_from("<HHIQQQ", a, 0)
    assert (version, size) == (2, 8)
    return length, np.frombuffer(inflate(a[64:64 + clen]), dtype="<u8"), np.frombuffer(inflate(open(prefix + ".d2", "rb").read()), dtype="<i4")


def write_synth(path):
    """a few piles on tiny2's reads, spacing 100, with the rare branches planted: a spill that changes a tile's value, a
    spill past the last tile, a tile of zeros only, aepos == alen off a spacing boundary, and a read (18) whose length is a
    multiple of the spacing"""
    rl = q_common.db_read_len("tiny2")
    rng = np.random.default_rng(4)
    tw, recs = 100, []

    def rec(a, b, ab, ae, vals=None, flags=0):
        nseg = (ae + tw - 1) // tw - ab // tw
        v = list(rng.integers(1, 14, nseg)) if vals is None else list(vals)
        assert len(v) == nseg and nseg >= 2
        bl = [min(ae, (ab // tw + k + 1) * tw) - max(ab, (ab // tw + k) * tw) for k in range(nseg)]
        tr = bytes(int(x) for pair in zip(v, bl) for x in pair)
        recs.append((a, struct.pack("<10i", 2 * nseg, int(sum(v)), ab, ab, ae, ae, flags, a, b, 0) + tr))

    assert rl[18] % tw == 0 and rl[0] % tw != 0 and rl[40] % tw != 0
    for a in (0, 18, 40, 77, 111):
        alen = int(rl[a])
        for k in range(7):                                           # body: aligned and unaligned ends, a few to the read's end
            ab = int(rng.integers(0, alen // 3))
            ab -= ab % tw if k % 2 else 0
            ae = alen if k % 3 == 0 else int(rng.integers(2 * alen // 3, alen))
            ae -= ae % tw if k % 3 == 1 else 0
            rec(a, (a + 1 + k) % len(rl), ab, ae, flags=k & 1)
    alen = int(rl[0])
    v = [3] * 12
    v[2] = 130                                                       # tile 2 -> tile 3 at 30: changes tile 3's mean
    rec(0, 5, 0, 1200, v)
    n = (alen + tw - 1) // tw - (alen - 1000) // tw
    rec(0, 6, alen - 1000, alen, [4] * (n - 1) + [150])              # the last tile's value goes past the read: dropped
    v = [2] * ((alen - 700 + tw - 1) // tw - (alen - 2000) // tw)
    v[3] = 230                                                       # two tiles on, at 30
    rec(0, 7, alen - 2000, alen - 700, v)
    keep = []
    for a, r in recs:                                                # zero every value of read 40's tiles 30..33
        if a == 40:
            head, tr = bytearray(r[:40]), bytearray(r[40:])
            ab = struct.unpack_from("<i", head, 8)[0]
            for t in range(30, 34):
                s = t - ab // tw
                if 0 <= s < len(tr) // 2:
                    tr[2 * s] = 0
            r = bytes(head) + bytes(tr)
        keep.append((a, r))
    keep.sort(key=lambda x: x[0])
    body = b"".join(r for _, r in keep)
    open(path, "wb").write(struct.pack("<qi", len(keep), tw) + body)
    assert len(body) < 200 * 1000


def main():
    tmp = tempfile.mkdtemp(prefix="q_golden_")
    try:
        exe = build_tool(tmp)
        shutil.rmtree(OUT, ignore_errors=True)
        os.makedirs(OUT)
        write_synth(os.path.join(OUT, "synth.las"))
        cases, seen = [], dict(low=0, capped=0, spill_alters=0, sum0=0, no_pile=0, left=0, right=0, zeroed=0, tight=0, emptied=0)
        for name, opts, inp in q_common.CASES:
            work = tempfile.mkdtemp(dir=tmp)
            q_common.workdir(work, inp)
            if "-u" in opts:
                q_common.prepare_update(exe, work)
                before = read_a2(os.path.join(work, ".G.trim"))
            r = q_common.run_tool(exe, opts, work)
            assert r.returncode == 0, (name, r.stderr)
            block, qn, tn = q_common.track_names(opts)
            pre = os.path.join(work, ".G.%s" % ("%d." % block if block else ""))
            if "-u" in opts:                                         # -u reads the q track of the whole database
                nreads, q_anno, q_data = read_a2(os.path.join(work, ".G.q"))
            else:
                nreads, q_anno, q_data = read_a2(pre + qn)
            _, t_anno, t_data = read_a2(pre + tn)
            case = dict(name=name, opts=opts, input=inp, rc=r.returncode, stdout=r.stdout, stderr=r.stderr)
            if "-L" in opts:
                case["qlog"] = open(os.path.join(work, "qlog.txt")).read()
            cases.append(case)
            np.savez_compressed(os.path.join(OUT, "expected_%s.npz" % name), nreads=nreads, q_anno=q_anno, q_data=q_data,
                                trim_anno=t_anno, trim_data=t_data)

            # the model agrees, and which branches the case reaches
            b = q_common.read_las(os.path.join(work, q_common.LAS))
            rl = q_common.db_read_len(q_common.INPUTS[inp][0])
            kw = q_common.opts_to_kwargs(opts)
            assert np.all(b["tlen"] >= 4), "%s holds a record with tlen < 4" % name
            if "-u" in opts:
                ta, td, tight, emptied = q_model.trim_update(b, rl, q_anno, q_data, before[1], before[2], strict=True, **kw)
                assert np.array_equal(ta, t_anno) and np.array_equal(td, t_data), "%s: the model and the reference part ways (-u)" % name
                seen["tight"] += tight
                seen["emptied"] += emptied
                print("%-12s -u: %d piles tightened, %d emptied" % (name, tight, emptied))
                continue
            mq = q_model.q_track(b, rl, strict=True, **kw)
            for got, want, what in zip(mq, (q_anno, q_data, t_anno, t_data), ("q anno", "q data", "trim anno", "trim data")):
                assert np.array_equal(got, want), "%s: the model and the reference part ways (%s)" % (name, what)
            qk = {k: v for k, v in kw.items() if k in ("segmin", "segmax", "ccs")}
            _, _, depth, _ = q_model.tile_q(b, rl, **qk)
            bare = q_model.tile_q(b, rl, spill=False, **qk)[0]
            low = int(np.sum(depth < kw.get("segmin", 1)))
            capped = int(np.sum(depth > kw.get("segmax", 20)))
            alters = int(np.sum(bare != q_data))
            tile0, segs = q_model.segments(b, rl)
            sums = np.zeros(int(tile0[-1]), dtype=np.int64)
            for t, v in segs:
                sums[t] += v
            sum0 = int(np.sum((sums == 0) & (depth > 0)))
            no_pile = int(np.sum(np.diff(q_anno.astype(np.int64)) == 0))
            tr = t_data.reshape(-1, 2)
            has = np.flatnonzero(np.diff(t_anno.astype(np.int64)) > 0)
            left = int(np.sum(tr[:, 0] > 0))
            right = int(np.sum((tr[:, 1] > 0) & (tr[:, 1] < rl[has])))
            big = q_model.q_track(b, rl, **dict(kw, min_len=-(1 << 30)))[3].reshape(-1, 2)
            zeroed = int(np.sum((tr[:, 0] == 0) & (tr[:, 1] == 0) & (big[:, 1] - big[:, 0] > 0)))
            print("%-12s low-count %5d capped %5d spill alters %3d sum==0 %3d reads without pile %3d trims left %3d right %3d zeroed by -o %3d"
                  % (name, low, capped, alters, sum0, no_pile, left, right, zeroed))
            for k, v in (("low", low), ("capped", capped), ("spill_alters", alters), ("sum0", sum0), ("no_pile", no_pile),
                         ("left", left), ("right", right), ("zeroed", zeroed)):
                seen[k] += v
        for k, v in seen.items():
            assert v >= 1, "no fixture reaches the branch %r" % k
        json.dump(cases, open(os.path.join(OUT, "cases.json"), "w"), indent=1)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
