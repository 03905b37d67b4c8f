#!/usr/bin/env python3
"""What the REFERENCE's LAgap makes of the shapes of tests/gap_shapes.py (tests/golden/gap/shapes_expected.npz, shapes.json).

Runs only where the reference sources lie (REF_SRC, default /root/reference), like make_gap_golden.py, whose build_tool and
rec it uses: the shapes that are not api_only are written as one .las into a temporary directory, beside a database of the
shapes' read lengths with random bases and the exclude track, and LAgap is run under the option sets def, -s 100, -s 300,
-e ex and -e ex -s 300.  Only data is kept: the flags word of every record per option set (shapes_expected.npz), and in
shapes.json the stdout per option set, tag and A read of every shape, the lines each shape must produce, and a sha256 over
the shapes' columns and read lengths, which the tests assert first.  Nothing compiled, no .las and no database is kept.  The
asserts at the end hold every shape to the border it names (gap_shapes.hold_to_borders) and the model to the reference.

    python tests/golden/make_gap_shapes_golden.py
"""
import io
import json
import os
import shutil
import struct
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..")))
import make_gap_golden as mg                           # noqa: E402
import gap_common as gc                                # noqa: E402
import gap_model as gm                                 # noqa: E402
import gap_shapes as gs                                # noqa: E402
import trim_common as tc                               # noqa: E402

OPTS = dict([("def", []), ("s100", ["-s", "100"]), ("s300", ["-s", "300"]), ("e", ["-e", gc.EX_TRACK]),
             ("es", ["-e", gc.EX_TRACK, "-s", "300"])])
HEAD = "\x1b[32mPASS gaps\x1b[0m"


def write_db(directory, root, rl, seed=1):
    """a one-block database of reads of the lengths rl with random bases (.db stub, .idx, .bps in the layout of db/DB.h)"""
    from damar_amd import api
    rng = np.random.default_rng(seed)
    hdr = api.HITS_DB()
    hdr.ureads = len(rl)
    for c in range(4):
        hdr.freq[c] = 0.25
    hdr.maxlen = int(max(rl))
    hdr.totlen = int(sum(int(x) for x in rl))
    with open(os.path.join(directory, ".%s.idx" % root), "wb") as idx, open(os.path.join(directory, ".%s.bps" % root), "wb") as bps:
        idx.write(bytes(hdr))
        off = 0
        for n in rl:
            r = api.HITS_READ()
            r.rlen, r.boff, r.coff, r.flags = int(n), off, -1, 0x800
            idx.write(bytes(r))
            packed = rng.integers(0, 256, size=(int(n) + 3) // 4, dtype=np.uint8)
            bps.write(packed.tobytes())
            off += len(packed)
    with open(os.path.join(directory, "%s.db" % root), "w") as f:
        f.write("files = %9d\n  %9d %s %s\n" % (1, len(rl), "syn", "Syn"))
        f.write("blocks = %9d\nsize = %9d\n %9d\n %9d\n" % (1, 200, 0, len(rl)))


def model_stdout(S, res):
    cont, dropped, breaks = gm.counts(res)
    out = [HEAD] + [ln for s, ev in zip(S, res.events) for ln in gm.lines(s.aread, ev)]
    return "\n".join(out + ["dropped %d containments" % cont, "dropped %d overlaps in %d break/gaps" % (dropped, breaks)]) + "\n"


def main():
    tmp = tempfile.mkdtemp(prefix="gap_shapes_")
    try:
        lagap = mg.build_tool(tmp)
        every = gs.shapes()
        S = [s for s in every if not s.api_only]
        rl = gs.read_len(every)
        piles, _, (ea, ed) = gs.arrays(S, rl)
        body = b"".join(mg.rec(s.aread, b, ab, ae, bb, be, fl)[1] for s in S for b, ab, ae, bb, be, fl in s.recs)
        nrec = sum(len(s.recs) for s in S)
        work = os.path.join(tmp, "work")
        os.makedirs(work)
        open(os.path.join(work, gc.LAS), "wb").write(struct.pack("<qi", nrec, gc.TW) + body)
        write_db(work, "G", rl)
        tc.write_track_a2(os.path.join(work, ".G." + gc.EX_TRACK), len(rl), ea, ed)
        runs = gs.model_runs(S, rl)
        gs.hold_to_borders(S, runs)
        flags, stdout, lines = {}, {}, {s.tag: {} for s in S}
        for key, opts in OPTS.items():
            r = subprocess.run([lagap] + opts + ["G", gc.LAS, gc.OUT], cwd=work, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            assert r.returncode == 0 and r.stderr == "", (key, r.stderr)
            cols = tc.read_records(os.path.join(work, gc.OUT))[0]
            assert len(cols) == nrec and np.array_equal(cols[:, 7], np.repeat(piles["pile_aread"], np.diff(piles["pile_off"])))
            flags[key], stdout[key] = cols[:, 6].astype(np.int32), r.stdout
            # the model against the reference: a difference is the model's fault
            bad = np.flatnonzero((runs[key].flags_array() & ~gm.TEMP) != flags[key])
            assert len(bad) == 0, (key, bad[:8])
            assert model_stdout(S, runs[key]) == r.stdout, key
            for s, ev in zip(S, runs[key].events):
                lines[s.tag][key] = gm.lines(s.aread, ev)
                assert "\n".join(lines[s.tag][key]) in r.stdout, (key, s.tag)
            print("%-5s %5d records, %4d contained, %4d at gaps, %3d breaks printed" %
                  (key, nrec, int(np.sum((flags[key] & gm.CONT) != 0)), int(np.sum((flags[key] & gm.GAP) != 0)), r.stdout.count("BREAK")))
        dst = os.path.join(gc.GDIR, "shapes_expected.npz")
        with zipfile.ZipFile(dst, "w", zipfile.ZIP_DEFLATED) as z:           # an .npz with fixed dates: the same bytes from the same data
            for k, v in flags.items():
                buf = io.BytesIO()
                np.lib.format.write_array(buf, v, allow_pickle=False)
                z.writestr(zipfile.ZipInfo("flags_%s.npy" % k, date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)
        shapes = [dict(tag=s.tag, aread=s.aread, nrec=len(s.recs), border=s.border, lines=lines[s.tag]) for s in S]
        js = os.path.join(gc.GDIR, "shapes.json")
        json.dump(dict(sha256=gs.digest(gs.arrays(every, rl)[0], rl), stdout=stdout, shapes=shapes), open(js, "w"), indent=1, sort_keys=True)
        for f in (dst, js):
            assert os.path.getsize(f) < mg.MAX_FILE, (f, os.path.getsize(f))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
