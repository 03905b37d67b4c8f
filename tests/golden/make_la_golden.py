"""Records what the REAL reference's Local_Alignment (align.c:1904, driven by oracle/ref_localalign.c, built into oracle/_ref/
by oracle/Makefile.ref) answers on the task families of tests/la_shapes.py: one line `md5 family tasks` per family in
tests/golden/la_ref_md5.txt -- results only.  tests/test_la_host.py holds the oracle's answers against these.

    python tests/golden/make_la_golden.py          (after build(), with the reference present)"""
import hashlib
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import la_shapes as S  # noqa: E402


def main():
    tool = os.path.join(ROOT, "oracle", "_ref", "ref_localalign")
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        for name in S.FAMILIES:
            fam, out = os.path.join(tmp, name + ".fam"), os.path.join(tmp, name + ".bin")
            S.write_family(fam, S.family(name))
            subprocess.run([tool, fam, out], check=True)
            md5 = hashlib.md5(open(out, "rb").read()).hexdigest()
            lines.append("%s %s %d\n" % (md5, name, sum(len(g.tasks) for g in S.family(name))))
    with open(os.path.join(HERE, "la_ref_md5.txt"), "w") as f:
        f.writelines(lines)
    sys.stdout.writelines(lines)


if __name__ == "__main__":
    main()
