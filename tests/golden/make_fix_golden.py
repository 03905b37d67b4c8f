#!/usr/bin/env python3
"""Fixtures of LAfix (tests/golden/fix/) from the REFERENCE.

Runs only where the reference sources lie (REF_SRC, default /root/reference): LAfix is compiled with a plain gcc line into
a temporary directory outside the repository, run on .las files this repository already holds (with the q and trim tracks
of the LAq fixtures) and on one synthetic file written here, and only data is kept: synth.las, its tracks
(synth_tracks.npz), cases.json (options, exit status, stdout, stderr, md5 of the FASTA and of the -T file; the error runs;
what synth.las plants; the -Q value picked) and expected_<case>.npz (header lines, bases and crc32 per read; the planted
file's FASTA whole).  Nothing compiled is kept.  The asserts at the end hold the plants to the branch they were made for.

    python tests/golden/make_fix_golden.py
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
import fix_model                                       # noqa: E402

OUT = fc.FDIR
TW = fc.TW
MAX_FILE = 1 << 20
COMP = 0x1
GOOD, BEST, BAD = 10, 5, 40             # q of an ordinary segment, of the reads planted to win, of a weak segment
BEST_READS, WEAK_READ = (30, 99), 97


def build_tool(tmp):
    s = lambda *p: os.path.join(SRC, *p)
    subprocess.run(["gcc", "-O3", "-w", "-fno-strict-aliasing", "-I" + SRC, "-o", os.path.join(tmp, "LAfix"), s("scrub", "LAfix.c"),
                    s("lib", "read_loader.c"), s("lib", "utils.c"), s("lib", "tracks.c"), s("lib", "pass.c"), s("lib", "oflags.c"),
                    s("lib", "compression.c"), s("lib", "trim.c"), s("db", "QV.c"), s("db", "DB.c"), s("dalign", "align.c"),
                    "-lm", "-lz", "-lpthread"], cwd=tmp, check=True)
    return os.path.join(tmp, "LAfix")


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
    """-> (file body, record count, plants, q per read, trim pairs, repeat intervals, -c intervals).  A plant is one pile
    on an A read of its own; `head` says how the reference has to name the read under the default options."""
    plants, piles = {}, []
    q = {r: np.full((int(rl[r]) + TW - 1) // TW, GOOD, dtype=np.int32) for r in range(len(rl))}
    for r in BEST_READS:
        q[r][:] = BEST
    q[WEAK_READ][5] = 0
    trim = {r: (0, int(rl[r])) for r in range(len(rl))}
    rep, cv = {}, {}

    def plant(tag, recs, head, bad=(20,), at=None, **more):
        upto = at if at is not None else 100 if len(piles) == 30 else 0       # A reads: 0..29 and 100 on, B reads: 30..99
        while len(piles) < upto:
            piles.append(b"")
        a = len(piles)
        assert (a < 30 or a > 99) and rl[a] >= 6100 and (a != 104 or at == 104), (tag, a, rl[a])
        made = sorted((rec(a, *r) for r in recs), key=lambda x: x[0])
        piles.append(b"".join(m[1] for m in made))
        for s in bad:
            q[a][s] = BAD
        plants[tag] = dict(aread=a, nrec=len(recs), head=head, **more)
        return a

    others = [b for b in range(31, 97)]
    span = lambda b, ab=500, ae=3500: (b, ab, ae, 200)
    # more candidates than the kernel keeps: 45 holes each in seven B reads (three of each lost where B's offsets wrap)
    assert rl[len(piles)] >= 9400
    plant("many_cand", [(b, 200 * k, 200 * k + 100, (200 * k) % 3000) for b in range(40, 47) for k in range(46)], "trimmed", bad=())
    # missed adapters: a complement overlap of the read with itself across the anti-diagonal, and two with a gap between
    a = len(piles)
    m = int(rl[a]) // 2
    plant("flip_cross", [(a, m - 1000, m + 1000, m - 1000, None, COMP), (a + 40, 0, 1000, 0)], "trimmed", bad=(), flips="CROSS")
    a = len(piles)
    m = int(rl[a]) // 2
    plant("flip_gap", [(a, m - 1500, m - 100, m - 1500, None, COMP), (a, m + 100, m + 1500, m + 100, None, COMP), (a + 40, 0, 1000, 0)],
          "trimmed", bad=(), flips="GAP  ")
    plant("one_record", [span(50)], "trimmed", bad=())
    for n in (64, 65, 129):                                              # the winner (read 99) is the last record
        plant("n%d" % n, [span(others[k % len(others)], 500 + k % 7) for k in range(n - 1)] + [span(99)], "fixed", winner=99)
    plant("tie_strides", [span(30)] + [span(b) for b in others[:64]] + [span(99)], "fixed", winner=30)
    plant("border_exact", [(99, 1900, 3500, 200)], "fixed", winner=99)
    plant("border_short", [(99, 1901, 3500, 200)], "trimmed")
    plant("partial_start", [(99, 1850, 3500, 200), span(50)], "fixed", winner=99)
    plant("comp_winner", [(99, 500, 3500, 200, None, COMP), span(50)], "fixed", winner=99)
    plant("weak_b", [(WEAK_READ, 1500, 3500, 0)], "trimmed")               # the stretch lies in B's segment 5
    a = plant("zero_ends", [span(50, 0, 4600)], "fixed", bad=(20,), zero=(0, 1, 2, 43, 44, 45))
    q[a][[0, 1, 2, 43, 44, 45]] = 0
    trim[a] = (0, 4600)
    # a break: two records of one B read with a gap on A over segment 20, the B stretch `extra` longer than the hole
    brk = lambda b, extra=7, ae1=2000, ab2=2100: [(b, 0, ae1, 100), (b, ab2, 4000, 100 + ab2 + extra)]
    four = lambda *e: [r for k, x in enumerate(e) for r in brk(40 + k, x)]
    plant("break_sup4", four(7, 7, 7, 7), "fixed", length=+7)
    plant("break_sup3", four(7, 7, 7), "trimmed")
    # the fourth stretch 49 and 50 longer than the others: its quality sorts it first.  At 49 it takes the three in and fills
    # the hole; at 50 it stands alone, the three merge without it and take it in as an intersecting break
    plant("break_49", four(7, 7, 7, 56), "fixed", length=+56)
    plant("break_50", four(7, 7, 7, 57), "fixed", length=+7)
    plant("span_7", four(7, 7, 7, 7) + [span(60 + k, 0, 4000) for k in range(7)], "fixed", length=+7)
    plant("span_8", four(7, 7, 7, 7) + [span(60 + k, 0, 4000) for k in range(8)], "fixed", length=0)
    a = plant("span_8_r", four(7, 7, 7, 7) + [span(60 + k, 1300, 2800) for k in range(8)], "fixed", length=0)
    rep[a] = [(1800, 2300)]                                              # under -r the eight do not reach 800 bases out
    plants["span_8_r"]["length_r"] = +7
    plant("gap_300", four(7, 7, 7, 7), "fixed", length=+7)                 # -g 300 cuts an A interval of 300
    plant("gap_200", [r for k in range(4) for r in brk(40 + k, 7, 2000, 2050)], "fixed", length=+7)
    # the B stretch against ten times the A interval of 300: 3400 is dropped whatever -g says, 2700 only by the -g cut
    plant("ten_times", [r for k in range(4) for r in brk(40 + k, 3300)], "trimmed")
    plant("nine_times", [r for k in range(4) for r in brk(40 + k, 2600)], "trimmed")
    # -g 300 against the B stretch: 299 bases stay, 300 are cut (no record spans the weak segment then)
    plant("gap_b299", [r for k in range(4) for r in brk(40 + k, 99, 2000, 2050)], "fixed", length=+99)
    plant("gap_b300", [r for k in range(4) for r in brk(40 + k, 100, 2000, 2050)], "fixed", length=+100)
    # two breaks that intersect, the first in the order with the larger support: it takes the other in (+7, not +17)
    plant("merge_first_wins", four(7, 7, 7, 7) + brk(44, 17, 2100, 2200), "fixed", bad=(20, 21), length=+7)
    # a B stretch 100 bases short of its hole on a read kept to 6050 bases: 5950 after the splice, under -x 6000
    a = plant("short_after", [r for k in range(4) for r in brk(40 + k, -100)], "fixed", length_abs=5950)
    trim[a] = (0, 6050)
    # the weak segment 2000..2100 and records that end at 2000 and 1999 and begin at 2100 and 2101: support 2
    plant("border_edges", [span(99), (50, 0, 2000, 0), (51, 0, 1999, 0), (52, 2100, 4000, 0), (53, 2101, 4000, 0)], "fixed", winner=99,
          support=2)
    # a break left of the trim is skipped, but the read then begins where the break ends; one right of it ends the splice
    a = plant("left_of_trim", four(7, 7, 7, 7), "fixed", length=-2200)
    trim[a] = (2500, int(rl[a]))
    a = plant("right_of_trim", four(7, 7, 7, 7), "fixed", length_abs=1500)
    trim[a] = (0, 1500)
    # a break far left of the trim: the read then begins at the break's end, 1700 bases before its trim
    a = plant("far_left_of_trim", [r for k in range(4) for r in brk(40 + k, 7, 1000, 1100)], "fixed", bad=(10,), length=-1200)
    trim[a] = (3000, int(rl[a]))
    a = plant("convert", four(7, 7, 7, 7), "fixed", length=+7)
    cv[a] = [(100, 300), (1800, 2300), (2000, 2100), (1899, 1903), (3000, 3200)]
    # the longest read of the database: the one pile over a segment limit set to the second longest planted read
    assert rl[104] == rl.max() and len(piles) <= 104
    plant("longest", [span(99), span(50)], "fixed", at=104, winner=99)
    nrec = sum(p["nrec"] for p in plants.values())
    return b"".join(piles), nrec, plants, q, trim, rep, cv


def bases_of(db, r):
    """read r of a fixture database as the letters a FASTA holds"""
    idx = open(os.path.join(q_common.GOLDEN, db, ".G.idx"), "rb").read()
    n = struct.unpack_from("<i", idx, 0)[0]
    recs = np.frombuffer(idx, dtype="<i8", offset=len(idx) - 32 * n).reshape(n, 4)
    rlen, boff = int(recs[r, 0] & 0xffffffff), int(recs[r, 1])
    raw = np.frombuffer(open(os.path.join(q_common.GOLDEN, db, ".G.bps"), "rb").read(), dtype=np.uint8, count=(rlen + 3) // 4, offset=boff)
    two = np.stack([(raw >> 6) & 3, (raw >> 4) & 3, (raw >> 2) & 3, raw & 3], axis=1).reshape(-1)[:rlen]
    return np.array(list(b"acgt"), dtype=np.uint8)[two].tobytes()


def track(iv, nreads, flat=False):
    anno, data = [0], []
    for r in range(nreads):
        for x in iv.get(r, []):
            data += list(x) if not flat else [x]
        anno.append(4 * len(data))
    return np.array(anno, dtype=np.uint64), np.array(data, dtype=np.int32)


def run(exe, opts, work):
    return subprocess.run([exe] + opts + ["G", fc.LAS, fc.OUT], cwd=work, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def main():
    tmp = tempfile.mkdtemp(prefix="fix_golden_")
    try:
        lafix = build_tool(tmp)
        shutil.rmtree(OUT, ignore_errors=True)
        os.makedirs(OUT)
        rl = q_common.db_read_len("tiny2")
        body, nrec, plants, q, trim, rep, cv = synth(rl)
        open(os.path.join(OUT, "synth.las"), "wb").write(struct.pack("<qi", nrec, TW) + body)
        assert os.path.getsize(os.path.join(OUT, "synth.las")) < MAX_FILE
        tr = {}
        tr["q_anno"], tr["q_data"] = track({r: list(v) for r, v in q.items()}, len(rl), flat=True)
        tr["trim_anno"], tr["trim_data"] = track({r: [v] for r, v in trim.items()}, len(rl))
        tr["rep_anno"], tr["rep_data"] = track(rep, len(rl))
        tr["cv1_anno"], tr["cv1_data"] = track(cv, len(rl))
        tr["cv2_anno"], tr["cv2_data"] = track({r: v[:1] for r, v in cv.items()}, len(rl))
        np.savez_compressed(os.path.join(OUT, "synth_tracks.npz"), **tr)

        # the -Q value: the first of the list, all below the default, for which a real file yields patched reads that the
        # default run does not give
        fixed_at, qv, base = {}, None, {}
        for cand in (28,) + fc.Q_LIST:
            n = 0
            for inp in fc.REAL:
                work = fc.workdir(tempfile.mkdtemp(dir=tmp), inp)
                r = run(lafix, ["-t", "trim", "-Q", str(cand)], work)
                assert r.returncode == 0, (inp, r.stderr)
                text = open(os.path.join(work, fc.OUT)).read()
                if cand == 28:
                    base[inp] = text
                elif text != base[inp] and ">fixed_" in text:
                    n += 1
            if cand == 28:
                continue
            fixed_at[str(cand)] = n
            if n > 0:
                qv = cand
                break
        note = "-Q %d patches %d of the real files otherwise than the default does" % (qv, fixed_at[str(qv)]) if qv is not None else \
            "no listed -Q value gives a patched read on any real file: the planted file alone carries the repairs"
        print(note)
        qv = qv if qv is not None else fc.Q_LIST[0]

        cases, by_name = [], {}
        for inp in fc.REAL + ("fsynth",):
            for v, opts in fc.variants(qv):
                name = "%s_%s" % (v, inp.replace("fsynth", "synth"))
                work = fc.workdir(tempfile.mkdtemp(dir=tmp), inp)
                r = run(lafix, opts, work)
                assert r.returncode == 0, (name, r.stderr)
                buf = open(os.path.join(work, fc.OUT), "rb").read()
                heads, lens, crcs = fc.digest(buf)
                case = dict(name=name, input=inp, opts=opts, rc=r.returncode, stdout=r.stdout, stderr=r.stderr,
                            md5=fc.md5(os.path.join(work, fc.OUT)), md5_T=fc.md5(os.path.join(work, fc.TOUT)))
                cases.append(case)
                by_name[name] = (case, heads, lens, buf)
                keep = dict(heads=np.array(heads), lens=lens, crcs=crcs)
                dst = os.path.join(OUT, "expected_%s.npz" % name)
                np.savez_compressed(dst, fasta=np.frombuffer(buf, dtype=np.uint8), **keep)     # the whole FASTA where it fits
                if os.path.getsize(dst) >= MAX_FILE:
                    assert inp != "fsynth"
                    np.savez_compressed(dst, **keep)
                assert os.path.getsize(dst) < MAX_FILE, (name, os.path.getsize(dst))
                print("%-12s %4d reads, %3d fixed, %s" % (name, len(heads), sum(h.startswith("fixed_") for h in heads),
                                                         r.stdout.splitlines()[-1]))

        # the plants against what the reference made of them
        def read_of(name, a):
            _, heads, lens, _ = by_name[name]
            hit = [i for i, h in enumerate(heads) if h.split()[0].split("_")[1] == str(a)]
            return (heads[hit[0]], int(lens[hit[0]])) if hit else (None, 0)
        for tag, pl in plants.items():
            a = pl["aread"]
            head, n = read_of("def_synth", a)
            assert head is not None and head.startswith(pl["head"] + "_"), (tag, head)
            span = (2500, int(rl[a])) if tag == "left_of_trim" else (0, 1500) if tag == "right_of_trim" else (0, int(rl[a]))
            if "length" in pl or "length_abs" in pl:
                assert n == pl.get("length_abs", rl[a] + pl.get("length", 0)), (tag, n, rl[a])
            elif pl["head"] == "trimmed" and "flips" not in pl:
                assert n == span[1] - span[0], (tag, n)
            if "length_r" in pl:
                assert read_of("r_synth", a)[1] == rl[a] + pl["length_r"], tag
            if "flips" in pl:
                assert "%8d %s @" % (a, pl["flips"]) in by_name["def_synth"][0]["stdout"], tag
                assert n < rl[a], tag
        assert read_of("g_synth", plants["gap_300"]["aread"])[1] == rl[plants["gap_300"]["aread"]]        # cut: the weak segment alone
        assert read_of("g_synth", plants["gap_200"]["aread"])[1] == rl[plants["gap_200"]["aread"]] + 7
        assert "due to missed adapter" in by_name["x_synth"][0]["stdout"]
        at = lambda case, tag: read_of(case, plants[tag]["aread"])
        rlen = lambda tag: int(rl[plants[tag]["aread"]])
        assert at("g_synth", "gap_b299")[1] == rlen("gap_b299") + 99 and at("g_synth", "gap_b300")[0].startswith("trimmed_")
        assert at("g0_synth", "ten_times")[0].startswith("trimmed_")                         # the 10x rule alone
        assert at("g0_synth", "nine_times") == ("fixed_%d source=%d" % ((plants["nine_times"]["aread"],) * 2), rlen("nine_times") + 2600)
        # patched and then too short: no header under -x 6000, but its repair is counted (one more than the reads show)
        assert at("x_synth", "short_after")[0] is None and "skip read %d " % plants["short_after"]["aread"] not in by_name["x_synth"][0]["stdout"]
        # -c: (100,300) before the patch, (1800,2300) across it, (2000,2100) inside it and gone, (1899,1903) cut to one
        # base and dropped as shorter than 6, (3000,3200) after it and moved by 7
        assert at("c_synth", "convert")[0] == "fixed_%d source=%d cv1=100,300,1800,2307,3007,3207 cv2=100,300" % \
            ((plants["convert"]["aread"],) * 2), at("c_synth", "convert")[0]
        assert " cv1=" in read_of("c_synth", plants["convert"]["aread"])[0] and " cv2=" in read_of("c_synth", plants["convert"]["aread"])[0]
        assert by_name["T_synth"][0]["md5_T"] is not None
        # the sort tie comes out in input order: break_sup4's four candidates are equal in interval and quality, and the
        # first of them in the file (B read 40) takes the others in, so it is read 40's bases that fill the hole
        a = plants["break_sup4"]["aread"]
        block = by_name["def_synth"][3].split(b">fixed_%d " % a)[1].split(b">")[0]
        got = block.partition(b"\n")[2].replace(b"\n", b"")
        assert got[1900:2207] == bases_of("tiny2", 40)[2000:2307], "the planted sort tie did not come out in input order"

        # the two rules for what the reference reads out of range: the model counts every q value asked for beyond the
        # track's data and every scan that ran to the read's border, over all inputs and the parameters of the cases
        seen = {}
        for inp in fc.REAL + ("fsynth",):
            batch, irl = fc.batch_of(inp)
            t = fc.tracks(inp)
            whole = np.stack([np.zeros(len(batch["pile_aread"]), dtype=np.int32), irl[batch["pile_aread"]]], axis=1)
            for trims in (fc.trims_of(batch, irl, t["trim"]), whole):
                for kw in (dict(), dict(low_q=qv), dict(low_coverage=True), dict(max_gap=-1), dict(repeats=t["rep"])):
                    for k, v in fix_model.patches(batch, irl, trims, t["q"], **kw)[1].items():
                        seen[k] = seen.get(k, 0) + v
        assert seen == dict(q_beyond_data=0, scan_hit_border=0), seen

        work = fc.workdir(tempfile.mkdtemp(dir=tmp), "tiny2")
        errors = []
        for name, args in fc.ERRORS:
            r = subprocess.run([lafix] + args, cwd=work, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            errors.append(dict(name=name, args=args, rc=r.returncode, stdout=r.stdout, stderr=r.stderr,
                               md5=fc.md5(os.path.join(work, fc.OUT)) if name in ("q_count", "trim_outside") else None))
            assert r.returncode == 1, (name, r.returncode, r.stderr)
        for name, text in (("q_count", "Q track entries"), ("trim_outside", "outside read length")):
            assert text in next(e for e in errors if e["name"] == name)["stderr"], name
        json.dump(dict(cases=cases, errors=errors, plants=plants, q_picked=qv, q_note=note, fixed_at=fixed_at,
                       rules_note="no fixture's result depends on the two out-of-range rules: over every input, with and without "
                                  "the trim track and under the parameters of the cases, no q value is read beyond the track's data and "
                                  "no scan for the first or last scored segment reaches the read's border (counted by tests/fix_model.py)",
                       rules_seen=seen),
                  open(os.path.join(OUT, "cases.json"), "w"), indent=1)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
