#!/usr/bin/env python3
"""What the REFERENCE's LAfilter makes of the shapes of tests/filter_shapes.py (tests/golden/filter/shapes_expected.npz,
shapes.json).

Runs only where the reference sources lie (REF_SRC, default /root/reference), like make_filter_golden.py, whose build_tool and
rec it uses, with the write_db of make_gap_shapes_golden.py: the shapes are written as one .las per trace spacing into a
temporary directory, beside a database of the shapes' read lengths with random bases, the trim and the repeat track and the
read lists, and LAfilter is run without -p under every option set of filter_shapes.OPTION_SETS (the shapes on two-byte traces
under SETS_200).  Only data is kept: per option set the five words of a record that LAfilter may change, as (index, value)
where they differ from the input (shapes_expected.npz), and in shapes.json tag, A read, record count and stated letters of
every shape and a sha256 over the shapes, which the tests assert first.  Nothing compiled, no .las and no database is kept.
The asserts hold every shape to the letters it states, the -R 4 shapes to the reference's double count, and the model
(tests/filter_model.py) to the reference on flags, aepos, bepos, diffs and tlen.

    python tests/golden/make_filter_shapes_golden.py
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
import make_filter_golden as mf                        # noqa: E402
import make_gap_shapes_golden as mg                    # noqa: E402
import filter_common as fc                             # noqa: E402
import filter_model as fm                              # noqa: E402
import filter_shapes as fs                             # noqa: E402
import trim_common as tc                               # noqa: E402

WORDS = dict(tlen=0, diffs=1, aepos=4, bepos=5, flags=6)


def las_bytes(S):
    """the shapes S as a .las body, and the ten words of every record"""
    ts = S[0].tspace
    body, cols = [], []
    for s in S:
        for b, ab, ae, bb, be, fl, df, tr in s.recs:
            words = (len(tr), df, ab, bb, ae, be, fl, s.aread, b, 0)
            one = struct.pack("<10i", *words) + np.array(tr, dtype=np.uint8 if ts <= 125 else "<u2").tobytes()
            if ts == fc.TW and tr == fs.trace_of(ab, ae, bb, be, df, ts):
                assert one == mf.rec(s.aread, b, ab, ae, bb, be, fl, df), s.tag      # a made trace is make_filter_golden's
            body.append(one)
            cols.append(words)
    return b"".join(body), np.array(cols, dtype=np.int32)


def main():
    tmp = tempfile.mkdtemp(prefix="filter_shapes_")
    try:
        tool = mf.build_tool(tmp)
        rl = fs.read_len()
        ta, td, ra, rd = fs.tracks()
        keep, letters = {}, {}
        for name, S, keys in (("t100", fs.shapes(), list(fs.OPTION_SETS)), ("t200", fs.shapes200(), list(fs.SETS_200))):
            work = os.path.join(tmp, name)
            os.makedirs(work)
            body, cols_in = las_bytes(S)
            open(os.path.join(work, fc.LAS), "wb").write(struct.pack("<qi", len(cols_in), S[0].tspace) + body)
            mg.write_db(work, "G", rl)
            tc.write_track_a2(os.path.join(work, ".G.trim"), len(rl), ta, td)
            tc.write_track_a2(os.path.join(work, ".G.repeats"), len(rl), ra, rd)
            for f, text in fs.files().items():
                open(os.path.join(work, f), "w").write(text)
            batch = fs.arrays(S)
            for key in keys:
                r = subprocess.run([tool] + fs.OPTION_SETS[key] + ["G", fc.LAS, fc.OUT], cwd=work, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
                assert r.returncode == 0, (key, r.stderr)
                cols, _, novl, tspace = tc.read_records(os.path.join(work, fc.OUT))
                assert novl == len(cols_in) and tspace == S[0].tspace and np.array_equal(cols[:, fc.FIXED], cols_in[:, fc.FIXED]), (name, key)
                for k in fc.LOOSE:
                    at = np.flatnonzero(cols[:, k] != cols_in[:, k]).astype(np.int32)
                    keep["%s:%s:i%d" % (name, key, k)], keep["%s:%s:v%d" % (name, key, k)] = at, cols[at, k].astype(np.int32)
                # every shape shows the letters it states, and the model is the reference
                fs.check_letters(S, key, cols[:, 6])
                model = fm.run_batch(batch, rl, **fs.params(key))
                for w, k in WORDS.items():
                    bad = np.flatnonzero(model[w] != cols[:, k])
                    assert len(bad) == 0, "%s %s: the model's %s differs in records %s: %s against %s" % (name, key, w, bad[:8], model[w][bad[:8]], cols[bad[:8], k])
                at = 0
                for s in S:
                    letters.setdefault(s.tag, {})[key] = "".join(fs.code(int(f)) for f in cols[at:at + len(s.recs), 6])
                    at += len(s.recs)
                print("%s %-5s %5d records, %5d discarded" % (name, key, novl, int(np.sum((cols[:, 6] & fm.DISCARD) != 0))))
        # -R 4: a first run whose head alone is proper loses its other record, a later such run does not
        assert letters["r4_first_head"]["R4"][0:4] == ".D.." and letters["r4_first_head"]["R4"][64:66] == ".."
        every = fs.every()
        assert not any(s.expect.keys() - letters[s.tag].keys() for s in every), "a shape states letters under an option set it is not run under"
        dst = os.path.join(fc.FDIR, "shapes_expected.npz")
        with zipfile.ZipFile(dst, "w", zipfile.ZIP_DEFLATED) as z:           # an .npz with fixed dates: the same bytes from the same data
            for k in sorted(keep):
                buf = io.BytesIO()
                np.lib.format.write_array(buf, keep[k], allow_pickle=False)
                z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)
        js = os.path.join(fc.FDIR, "shapes.json")
        shapes = [dict(tag=s.tag, aread=s.aread, nrec=len(s.recs), tspace=s.tspace, border=s.border, over=s.over, letters=s.expect) for s in every]
        json.dump(dict(sha256=fs.digest(), shapes=shapes), open(js, "w"), indent=1, sort_keys=True)
        for f in (dst, js):
            assert os.path.getsize(f) < mf.MAX_FILE, (f, os.path.getsize(f))
            print(os.path.basename(f), os.path.getsize(f), "bytes")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
