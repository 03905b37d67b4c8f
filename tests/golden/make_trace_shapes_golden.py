"""tests/golden/trace_shapes_ref_md5.txt: per (family, file, mode, pts|mid) of tests/trace_shapes.py the md5 of what the REAL
reference's Compute_Trace_PTS / Compute_Trace_MID leaves in every record (oracle/_ref/ref_lastrace, built by
oracle/Makefile.ref).  Run it where the reference build is present:

    python tests/golden/make_trace_shapes_golden.py [<ref_lastrace built with -fsanitize=address,undefined>]

With the argument, every run is first made with that stand-alone sanitizer build; a run it objects to is reported and nothing
is written: the record goes into trace_shapes.REMOVED (within its cap) or the family's definition is corrected."""
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))

import trace_shapes as S  # noqa: E402


def main():
    san = sys.argv[1] if len(sys.argv) > 1 else None
    lines, bad = [], []
    for fam in S.FAMILIES:
        for f in S.family(fam):
            db, las = S.materialize(fam, f)
            for mode, mid in S.jobs(f):
                out = las + ".r"
                if san is not None:
                    r = S.run_tool(san, db, las, out, mode, mid)
                    if r.returncode != 0 or "ERROR" in r.stderr or "runtime error" in r.stderr:
                        bad.append((fam, f.name, mode, mid, r.stderr[-2000:]))
                        continue
                    checked = open(out, "rb").read()
                r = S.run_tool(S.REF, db, las, out, mode, mid)
                assert r.returncode == 0, (fam, f.name, mode, mid, r.stderr)
                dump = open(out, "rb").read()
                assert san is None or dump == checked
                lines.append("%s %s %s %d %s\n" % (hashlib.md5(dump).hexdigest(), fam, f.name, mode, "mid" if mid else "pts"))
    for b in bad:
        print("the sanitizer build objects: %s/%s mode %d mid %d\n%s" % b)
    if bad:
        sys.exit(1)
    with open(os.path.join(HERE, "trace_shapes_ref_md5.txt"), "w") as o:
        o.writelines(lines)
    print("%d runs recorded%s" % (len(lines), ", every one clean under the sanitizer build" if san else ""))


if __name__ == "__main__":
    main()
