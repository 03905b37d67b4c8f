#!/usr/bin/env python3
"""Fixtures of LAcorrect (tests/golden/correct/) from the REFERENCE.

Runs only where the reference sources lie (REF_SRC, default /root/reference): LAcorrect is compiled with a plain gcc line
into a temporary directory outside the repository, run on .las files this repository already holds (with the q tracks of
the LAq fixtures) and on one synthetic file written here, and only data is kept: synth.las, its q track (synth_q.npz),
cases.json (options, exit status, stdout, stderr, md5 per output file; the error runs; what synth.las plants) and
expected_<case>.npz (header lines and crc32 of the bases per record; the planted file's FASTA whole).  Nothing compiled is
kept.  The asserts at the end hold the plants to the branch they were made for, wherever the reference's output shows it.

    python tests/golden/make_correct_golden.py
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
import fix_common as fc                                # noqa: E402
import correct_common as cc                            # noqa: E402
import correct_model as cm                             # noqa: E402

OUT = cc.CDIR
TW = cc.TW
MAX_FILE = 1 << 20
COMP, DISCARD = 0x1, 0x2


def build_tool(tmp):
    s = lambda *p: os.path.join(SRC, *p)
    subprocess.run(["gcc", "-O3", "-w", "-fno-strict-aliasing", "-I" + SRC, "-o", os.path.join(tmp, "LAcorrect"),
                    s("corrector", "LAcorrect.c"), s("corrector", "consensus.c"), s("lib", "utils.c"), s("lib", "tracks.c"),
                    s("lib", "pass.c"), s("lib", "oflags.c"), s("lib", "compression.c"), s("db", "QV.c"), s("db", "DB.c"),
                    s("dalign", "align.c"), "-lm", "-lz", "-lpthread"], cwd=tmp, check=True)
    return os.path.join(tmp, "LAcorrect")


def rec(a, b, ab, ae, bb, be=None, flags=0, qv=0, bepos=None):
    """one record with a trace of its own: `qv` differences per segment, B's bases shared out over A's intervals"""
    be = bb + (ae - ab) if be is None else be
    cuts = [ab] + list(range((ab // TW + 1) * TW, ae, TW)) + [ae]
    al = np.diff(cuts)
    extra = (be - bb) - (ae - ab)
    bl = al + extra // len(al) + (np.arange(len(al)) < extra % len(al))
    assert np.all(bl >= 0) and np.all(bl <= 255) and bl.sum() == be - bb, (ab, ae, bb, be)
    tr = np.zeros(2 * len(al), dtype=np.uint8)
    tr[0::2] = qv
    tr[1::2] = bl
    return struct.pack("<10i", len(tr), 0, ab, bb, ae, be if bepos is None else bepos, flags, a, b, 0) + tr.tobytes()


def synth(rl):
    """-> (file body, record count, plants).  A plant is one pile on an A read of its own (reads 0 .. 29, all of 6100
    bases and more); `added` says what the reference's correctionq has to show: {tile: sequences taken}."""
    plants, piles = {}, []

    def plant(tag, recs, a=None, **more):
        a = len(piles) if a is None else a
        while len(piles) < a:
            piles.append(b"")
        assert rl[a] >= 6100, (tag, a, rl[a])
        made = sorted(((r[1], i, rec(a, *r)) for i, r in enumerate(recs)), key=lambda x: x[:2])     # records of one B read lie in the order of abpos
        piles.append(b"".join(m[2] for m in made))
        plants[tag] = dict(aread=a, nrec=len(recs), **more)
        return a

    me = lambda ab, ae, shift=0, **kw: (len(piles), ab, ae, ab + shift) + ((None, kw.get("flags", 0), kw.get("qv", 0)) if kw else ())
    # coverage 1, 2 and 3 on both sides of the `added <= 2` rule
    plant("coverage", [me(0, 3000), me(1000, 2000, 3)], added={0: 2, 10: 3, 25: 2, 40: 1})
    # 20 and 21 eligible entries (A and 19, A and 21), 19 beside them
    plant("eligible", [me(0, 1000, k % 3) for k in range(19)] + [me(2000, 3000, k % 4) for k in range(21)] +
          [me(4000, 5000, k % 2) for k in range(18)], added={5: 20, 25: 20, 45: 19})
    # 40 entries of a tile, the 41st refused; the refused record ends off a trace point, so its mark lands on the slot
    # written last, the one record that was eligible: tile 5 is left with the A read alone.  38 records begin off a trace
    # point in tile 5 (not eligible there) and go on into tile 6
    plant("carried_p", [me(510, 700) for _ in range(38)] + [me(500, 600), me(500, 580)], added={5: 1, 6: 20})
    # the same without the refused record: the eligible one counts
    plant("not_carried", [me(510, 700) for _ in range(38)] + [me(500, 600)], added={5: 2, 6: 20})
    # B tiles of 19 and of 20 bases
    a = len(piles)
    plant("b19_b20", [(a, 1000, 1100, 1000, 1019), (a, 2000, 2100, 2000, 2020)], added={10: 1, 20: 2})
    # partial first and last tiles
    plant("partial", [me(150, 2950)], added={1: 1, 2: 2, 28: 2, 29: 1})
    # an overlap ending exactly at alen, off a trace point: its last tile counts.  With a last A tile under 20 bases the B
    # tile founds the profile
    a = len(piles)
    assert rl[a] % TW != 0
    last = int(rl[a]) // TW
    plant("ends_at_alen", [(a, int(rl[a]) - 250, int(rl[a]), int(rl[a]) - 250)], added={last: 2 if rl[a] % TW >= 20 else 1, last - 1: 2})
    short = [r for r in range(len(piles) + 1, 30) if 0 < rl[r] % TW < 20 and rl[r] >= 6100]
    if short:
        a = short[0]
        plant("short_last", [(a, int(rl[a]) - 250, int(rl[a]), 1000, 1350)], a=a, added={int(rl[a]) // TW: 1})
    # equal qv values: two unrelated B reads with the same differences; the file order decides which is added first
    a = len(piles)
    plant("equal_qv", [(a + 40, 0, 1000, 500, None, 0, 7), (a + 41, 0, 1000, 700, None, 0, 7)], added={3: 3})
    # a complemented B read, unrelated to A: columns tied between two bases, columns whose dashes reach the maximum
    a = len(piles)
    plant("comp", [(a + 40, 0, 1000, 200, None, COMP), (a + 41, 0, 1000, 300, None, 0), (a, 2000, 3000, 2001)], added={3: 3, 25: 2})
    # a discarded record mid-pile is dropped, one at the head of a pile (not the file's first) is used
    a = len(piles)
    plant("discard_mid", [(a, 0, 1000, 0), (a, 2000, 3000, 2000, None, DISCARD)], added={5: 2, 25: 1})
    a = len(piles)
    plant("discard_head", [(a, 0, 1000, 0, None, DISCARD), (a + 1, 2000, 3000, 2000)], added={5: 2, 25: 2})
    # a record whose trace runs past its bepos: the read stays uncorrected and is copied
    a = len(piles)
    plant("bad_points", [(a, 0, 1000, 0, None, 0, 0, 500)], bad=True)
    # B tiles of 250 bases from other reads: the waves outgrow the kernel's cells (and the profile a lowered column limit)
    a = len(piles)
    plant("over_cols", [(a + 40 + k, 0, 1000, 100 + 300 * k, 100 + 300 * k + 2500) for k in range(6)], added={3: 7})
    # the carried slot again.  Tile 5 holds the A read, 38 records that begin off a trace point and one eligible record E
    # (40 entries), tile 6 the A read, the 38 and Z, a longer record (40).  X lies over both and is refused in both: its last tile refused,
    # the slot is forgotten (p = -1), and the refused record R after it, which ends off a trace point, marks nothing: E
    # counts.  Without X, R's mark lands on E, the slot written last
    plant("carried_none", [me(510, 700) for _ in range(38)] + [me(600, 750), me(500, 600), me(540, 620), me(500, 570)], added={5: 2, 6: 20})
    plant("carried_last", [me(510, 700) for _ in range(38)] + [me(600, 750), me(500, 600), me(500, 570)], added={5: 1, 6: 20})
    # a last A tile under 20 bases with nothing over it: an empty tile, 0,0 in correctionq
    a = next(r for r in range(len(piles), len(rl)) if 0 < rl[r] % TW < 20 and rl[r] >= 6100)
    plant("empty_last", [(a, 0, 1000, 0)], a=a, added={int(rl[a]) // TW: 0}, empty=int(rl[a]) // TW)
    # B tiles of 120 bases: profiles of 120 columns and more, on waves that fit
    a = len(piles)
    plant("more_cols", [(a, 3000, 4000, 3000, 4200)], added={35: 2})
    nrec = sum(p["nrec"] for p in plants.values())
    return b"".join(piles), nrec, plants


def limits():
    """DAMAR_CORRECT_MAXSEG, _MAXCOLS, _CELLS as include/damar_hip.h sets them"""
    text = open(os.path.join(ROOT, "include", "damar_hip.h")).read()
    return tuple(int(text.split("#define DAMAR_CORRECT_" + k)[1].split()[0]) for k in ("MAXSEG", "MAXCOLS", "CELLS"))


def run(exe, opts, work):
    return subprocess.run([exe] + opts + ["G", cc.LAS, cc.OUT], cwd=work, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def main():
    tmp = tempfile.mkdtemp(prefix="correct_golden_")
    try:
        exe = build_tool(tmp)
        shutil.rmtree(OUT, ignore_errors=True)
        os.makedirs(OUT)
        rl = q_common.db_read_len("tiny2")
        body, nrec, plants = synth(rl)
        open(os.path.join(OUT, "synth.las"), "wb").write(struct.pack("<qi", nrec, TW) + body)
        assert os.path.getsize(os.path.join(OUT, "synth.las")) < MAX_FILE
        rng = np.random.default_rng(7)
        q = [rng.integers(1, 30, size=(int(n) + TW - 1) // TW) for n in rl]
        anno = np.zeros(len(rl) + 1, dtype=np.uint64)
        anno[1:] = 4 * np.cumsum([len(x) for x in q])
        np.savez_compressed(os.path.join(OUT, "synth_q.npz"), q_anno=anno, q_data=np.concatenate(q).astype(np.int32))

        cases, by_name = [], {}
        for inp in fc.REAL + ("csynth",):
            for v, opts in cc.VARIANTS:
                whole = not any(o == "-r" for o in opts)
                if (whole and inp not in cc.WHOLE) or (inp == "long") or (v == "b2" and cc.INPUTS[inp][0] != "tiny2"):
                    continue
                name = "%s_%s" % (v, inp.replace("csynth", "synth"))
                work = cc.workdir(tempfile.mkdtemp(dir=tmp), inp)
                r = run(exe, opts, work)
                assert r.returncode == 0, (name, r.stderr)
                files = cc.out_files(work)
                case = dict(name=name, input=inp, opts=opts, rc=r.returncode, stdout=r.stdout, stderr=r.stderr,
                            md5={f: fc.md5(os.path.join(work, f)) for f in files})
                cases.append(case)
                keep, fasta = {}, {}
                for f in files:
                    buf = open(os.path.join(work, f), "rb").read()
                    heads, lens, crcs = fc.digest(buf)
                    keep["heads_" + f], keep["crcs_" + f] = np.array(heads), crcs
                    fasta["fasta_" + f] = np.frombuffer(buf, dtype=np.uint8)
                by_name[name] = (case, keep)
                dst = os.path.join(OUT, "expected_%s.npz" % name)
                np.savez_compressed(dst, **keep, **(fasta if inp == "csynth" else {}))
                if os.path.getsize(dst) >= MAX_FILE:
                    np.savez_compressed(dst, **keep)
                assert os.path.getsize(dst) < MAX_FILE, (name, os.path.getsize(dst))
                print("%-14s %d files, %4d reads" % (name, len(files), sum(len(keep["heads_" + f]) for f in files)))

        # the plants against what the reference made of them
        heads = {h.split()[0]: h for h in by_name["plain_synth"][1]["heads_out.00.fasta"]}
        stdout = by_name["plain_synth"][0]["stdout"]
        serial = 0
        for tag, pl in plants.items():
            a = pl["aread"]
            if pl.get("bad"):
                assert "ERROR: bad pt points ovl 0 aread %d bread %d\n" % (a, a) in stdout, tag
                assert "copy.%d" % a in heads, tag
                continue
            h = heads["%d.%d" % (a, serial)]
            serial += 1
            cq = [int(x) for x in h.split("correctionq=")[1].split()[0].split(",")]
            for tile, n in pl["added"].items():
                assert cq[2 * int(tile) + 1] == n, (tag, tile, cq[2 * int(tile) + 1], n)
            if "empty" in pl:
                assert cq[2 * pl["empty"]:2 * pl["empty"] + 2] == [0, 0], tag

        # the model of tests/correct_model.py against the reference on every planted pile: the bases called and correctionq
        # per read; then what only the model can say of the plants
        fasta = bytes(np.load(os.path.join(OUT, "expected_plain_synth.npz"))["fasta_out.00.fasta"])
        body = {b.split(b" ")[0].decode(): b.partition(b"\n")[2].replace(b"\n", b"") for b in fasta.split(b">")[1:]}
        batch = q_common.read_las(os.path.join(OUT, "synth.las"))
        reads = cm.db_reads(os.path.join(q_common.GOLDEN, "tiny2"))
        qt = cc.q_track("csynth")
        model = cm.piles(batch, reads, qt[0], qt[1])
        lim, over, serial, facts_of = limits(), 0, 0, {}
        for pl in model:
            if pl["bad"] is not None:
                continue
            calls = [cm.consensus(t, lim) for t in pl["tiles"]]
            facts_of[pl["aread"]] = calls
            over += sum(c[2]["over"] for c in calls)
            name = "%d.%d" % (pl["aread"], serial)
            serial += 1
            cq = ",".join("%d,%d" % (len(c[0]), c[1]) for c in calls)
            assert "correctionq=%s" % cq in heads[name] + " ", pl["aread"]
            assert body[name] == b"".join(bytes(b"acgt"[x] for x in c[0]) for c in calls), pl["aread"]
        assert over >= 1, "no planted tile lies beyond the kernel's limits"
        oc = facts_of[plants["over_cols"]["aread"]]
        assert sum(c[2]["over"] for c in oc) == over and all(c[2]["cells"] > lim[2] for c in oc if c[2]["over"])
        # the column limit: no plant passes it at its built value before the waves outgrow their cells, so it is counted
        # at the lowered value the tests set (DAMAR_TEST_CORRECT_COLS)
        low = [c[2] for calls in facts_of.values() for c in calls]
        over_low = sum(f["seg"] > lim[0] or f["cols"] > cc.LOW_COLS or f["cells"] > lim[2] for f in low)
        assert sum(f["cols"] > cc.LOW_COLS and f["cells"] <= lim[2] for f in low) > 0 and over_low > over
        comp = facts_of[plants["comp"]["aread"]]
        assert sum(c[2]["tied_columns"] for c in comp) > 0 and sum(c[2]["dash_max_columns"] for c in comp) > 0
        # equal qv: with the two entries of qv 7 the other way round the model calls another sequence for some tile
        eq = next(m for m in model if m["aread"] == plants["equal_qv"]["aread"])
        differs = 0
        for t in range(10):
            ent = cm.taken(eq["entries"][t])
            assert [x["qv"] for x in ent[1:]] == [7, 7], ent
            swapped = cm.sequences([ent[0], ent[2], ent[1]], eq["aread"], reads)
            differs += not np.array_equal(cm.consensus(swapped)[0], cm.consensus(eq["tiles"][t])[0])
        assert differs > 0, "the order of the equal qv values does not show in any tile"
        next(c for c in cases if c["name"] == "plain_synth").update(host_tiles=int(over), host_tiles_low_cols=int(over_low))
        print("planted tiles beyond the limits %s: %d" % (lim, over))

        assert "copy.50" in heads and "copy.50" not in {h.split()[0] for h in by_name["r_synth"][1]["heads_out.00.fasta"]}
        assert len(by_name["j3_synth"][0]["md5"]) == 3 and len(by_name["rj_synth"][0]["md5"]) == 2
        assert "T0 READ" in by_name["v_synth"][0]["stdout"]

        work = cc.workdir(tempfile.mkdtemp(dir=tmp), "tiny_s")
        errors = []
        for name, args in cc.ERRORS:
            r = subprocess.run([exe] + args, cwd=work, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            errors.append(dict(name=name, args=args, rc=r.returncode, stdout=r.stdout, stderr=r.stderr))
            assert r.returncode == 1, (name, r.returncode, r.stderr)
        json.dump(dict(cases=cases, errors=errors, plants=plants), open(os.path.join(OUT, "cases.json"), "w"), indent=1)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
