#!/usr/bin/env python3
"""Fixtures of LAfilter (tests/golden/filter/) from the REFERENCE.

Runs only where the reference sources lie (REF_SRC, default /root/reference): LAfilter is compiled with a plain gcc line into
a temporary directory outside the repository, run on .las files this repository already holds (with the trim tracks of the
LAtrim fixtures and a repeat track made here) and on one synthetic file written here, and only data is kept: synth.las,
tracks.npz, cases.json (options, exit status, stdout, stderr, md5 of the output and of the -a file; the error runs; the read
lists; what synth.las plants) and expected_<input>.npz (per case the expected records: where only tlen, diffs, aepos, bepos
and flags can differ from the input, the entries that do; under -p or -T the ten words of every record).  Nothing compiled is kept.
The asserts hold the plants of the synthetic file to the branches they were made for.

    python tests/golden/make_filter_golden.py
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
import filter_common as fc                             # noqa: E402
import trim_common as tc                               # noqa: E402

OUT = fc.FDIR
TW = fc.TW
G = fc.MAXGROUP
MAX_FILE = 1 << 20
MAXLEN = 400000                                        # DAMAR_FILTER_MAXLEN
COMP, DISCARD, REPEAT, LOCAL, DIFF, OLEN, RLEN, STITCH, CONT, SYM = 0x1, 0x2, 0x8, 0x10, 0x20, 0x200, 0x400, 0x80, 0x8000, 0x100


def build_tool(tmp):
    s = lambda *p: os.path.join(SRC, *p)
    subprocess.run(["gcc", "-O3", "-w", "-fno-strict-aliasing", "-I" + SRC, "-o", os.path.join(tmp, "LAfilter"), s("scrub", "LAfilter.c"),
                    s("lib", "read_loader.c"), s("lib", "utils.c"), s("lib", "tracks.c"), s("lib", "pass.c"), s("lib", "oflags.c"),
                    s("lib", "compression.c"), s("lib", "trim.c"), s("db", "QV.c"), s("db", "DB.c"), s("dalign", "align.c"),
                    "-lm", "-lz", "-lpthread"], cwd=tmp, check=True)
    return os.path.join(tmp, "LAfilter")


def rec(a, b, ab, ae, bb, be=None, flags=0, diffs=0):
    """one record with a trace of its own: B's bases shared out over A's intervals, the differences on the first"""
    be = bb + (ae - ab) if be is None else be
    cuts = [ab] + list(range((ab // TW + 1) * TW, ae, TW)) + [ae]
    al = np.diff(cuts)
    extra = (be - bb) - (ae - ab)
    bl = al + extra // len(al) + (np.arange(len(al)) < extra % len(al))
    assert np.all(bl >= 0) and np.all(bl <= 255) and bl.sum() == be - bb
    tr = np.zeros(2 * len(al), dtype=np.uint8)
    tr[1::2] = bl
    left = diffs
    for k in range(len(al)):                           # shared out, at most 40 a segment
        tr[2 * k] = min(left, 40)
        left -= int(tr[2 * k])
    assert left == 0
    return struct.pack("<10i", len(tr), diffs, ab, bb, ae, be, flags, a, b, 0) + tr.tobytes()


def synth(rl):
    """-> (file body, record count, plants, trim pairs, repeat intervals, read lists)"""
    plants, piles, rep = {}, [], {}
    trim = {r: (0, int(rl[r])) for r in range(len(rl))}
    big = [int(r) for r in np.argsort(-rl, kind="stable")]           # the reads, the longest first

    def partners(a, k):
        """k B reads at least as long as read a"""
        out = [r for r in big if r != a and rl[r] >= rl[a]][:k]
        assert len(out) == k, (a, k)
        return sorted(out)

    def plant(tag, recs, min_len=0, max_len=1 << 30, **expect):
        while not (min_len <= rl[len(piles)] <= max_len):
            piles.append(b"")
        a = len(piles)
        recs = recs(a) if callable(recs) else recs
        for r in recs:
            be = r[4] if len(r) > 4 and r[4] is not None else r[3] + r[2] - r[1]
            assert 0 <= r[1] <= r[2] <= rl[a] and 0 <= r[3] <= be <= rl[r[0]], (tag, r)
        piles.append(b"".join(rec(a, *r) for r in recs))             # in the order given: runs of one B read as they lie
        plants[tag] = dict(aread=a, nrec=len(recs), expect=expect)
        return a

    L = 104                                                          # the longest read: a B read for everything
    assert rl[L] == rl.max()
    # -A: the list of read 0 comes first and is not ended, so it runs on into read 1's; a pair with aread > bread
    plant("sym0", [(60, 0, 1000, 0), (70, 0, 1000, 0), (71, 0, 1000, 0)], A="SS.")
    plant("sym_swap", [(0, 0, 1000, 0), (70, 0, 1000, 0), (71, 0, 1000, 0)], A="SS.")
    lists = {"sym.txt": "0 1\n0 60\n1 70\n", "x.txt": "50\n104\n", "i.txt": "104\n89\n"}
    # sizes of piles and of runs
    plant("one", [(L, 0, 1000, 0)])
    plant("n64", [(b, 0, 1000, 0) for b in range(40, 104)])
    plant("n65", [(b, 0, 1000, 0) for b in range(39, 104)])
    plant("n129", [r for b in range(10, 75) for r in ((b, 0, 1000, 0), (b, 3000, 4000, 3000))][:129])
    plant("g64", [(L, 50 * k, 50 * k + 800, 50 * k) for k in range(G)], s="?" * G)
    plant("g65", [(L, 50 * k, 50 * k + 800, 50 * k) for k in range(G + 1)], s="?" * (G + 1))
    # stitch
    plant("chain3", [(L, 0, 1000, 0), (L, 1010, 2000, 1010), (L, 2005, 3000, 2005)], s=".TT", S=".TT")
    plant("refuse40", [(L, 0, 1000, 0), (L, 1010, 2000, 1100)], s="..", S=".T")
    plant("two_cand", [(L, 0, 1000, 0), (L, 1010, 1500, 1010), (L, 1020, 2500, 1020)], s="..T")
    plant("undiscard", [(L, 0, 1000, 0, None, DISCARD | LOCAL), (L, 1010, 2000, 1010)], **{"def": "L.", "s": ".T"})
    # filter() at its bounds (the cases d: -d 20, o: -o 1000, u: -u 100, l: -l 9000)
    full = lambda a, ab, bb: (L, ab, int(rl[a]), bb, bb + int(rl[a]) - ab)
    plant("u_at", lambda a: [full(a, 100, 100)], max_len=15000, u=".")
    plant("u_over", lambda a: [full(a, 101, 101)], max_len=15000, u="L")
    plant("u_end_at", lambda a: [(L, 0, int(rl[a]) - 100, 0)], u=".")
    plant("u_end_over", lambda a: [(L, 0, int(rl[a]) - 101, 0)], u="L")
    trim[80] = (200, int(rl[80]) - 300)                              # mirrored for a complement record: [300, blen - 200)
    plant("u_comp_at", lambda a: [(80, 101, int(rl[a]), 400, 400 + int(rl[a]) - 101, COMP)], max_len=int(rl[80]) - 700, u=".")
    plant("u_comp_over", lambda a: [(80, 101, int(rl[a]), 401, 401 + int(rl[a]) - 101, COMP)], max_len=int(rl[80]) - 700, u="L")
    plant("o_thr", [(L, 0, 1000, 0), (89, 0, 999, 0)], o=".O")
    a = plant("l_at", [(L, 0, 1000, 0)], min_len=9000, l=".")
    trim[a] = (0, 9000)
    a = plant("l_under", [(L, 0, 1000, 0)], min_len=9000, l="R")
    trim[a] = (0, 8999)
    plant("d_thr", [(L, 0, 1000, 0, None, 0, 200), (89, 0, 1000, 0, None, 0, 201)], d=".F")
    # -n 500, alone and with -Y 300
    a = plant("n_a_at", [(L, 0, 1000, 0)], n=".", nY=".")
    rep[a] = [(0, 500)]
    a = plant("n_a_over", [(L, 0, 1000, 0)], n="P")
    rep[a] = [(0, 501)]
    plant("n_b_only", [(88, 0, 1000, 0)], n="P")
    rep[88] = [(0, 501)]
    a = plant("tip_begin", [(L, 0, 790, 0)], n=".", nY="P")
    rep[a] = [(0, 150)]
    a = plant("tip_end", lambda a: [(L, int(rl[a]) - 790, int(rl[a]), 0)], n=".", nY="P")
    rep[a] = [(int(rl[a]) - 150, int(rl[a]))]
    a = plant("tips_cross", [(L, 0, 500, 0)], min_len=600, nY="P")
    trim[a] = (0, 500)
    rep[a] = [(0, 500)]
    # -R 6
    plant("dup_id", lambda a: [(a, 0, 1000, 2000), (a, 0, 1000, 2000)], R63=".C", R6=".C")
    plant("chain_mid", [(L, 0, 3000, 0), (L, 100, 2900, 100, None, DISCARD), (L, 200, 2800, 200)], R6=".DC")
    plant("self1", lambda a: [(a, 0, 1000, 0)], R63="C", R6="C")
    # -w
    plant("mm_pair", [(L, 0, 2000, 0), (L, 500, 1500, 5000)], vw="DD")
    plant("mm_none", [(L, 0, 1000, 0), (L, 2000, 3000, 2000)], vw="..")
    # -R 4
    plant("spec", lambda a: [(L, 0, int(rl[a]), 0), (L, 500, 1500, 3000)], max_len=15000, R4=".D")
    # -z 2: bases / length at the bound, one short on entering alone, and comfortably inside
    whole = lambda a, k, ab=0: [(b, ab, int(rl[a]), ab) for b in partners(a, k)]
    plant("z_ok", lambda a: whole(a, 3), max_len=14000, wz="...")
    plant("z_bound", lambda a: whole(a, 2), max_len=14000, wz="DD")
    plant("z_enter", lambda a: whole(a, 1) + whole(a, 4, 1)[1:], max_len=14000, wz="DDDD")

    # -z 2 -u 200: the uncovered bases of the trim interval exactly at -u and one over
    def holed(hole):
        def make(a):
            out = []
            for b in partners(a, 4):
                out += [(b, 0, 3000, int(rl[b]) - 3000), (b, 3000 + hole, int(rl[a]), 0)]
            return out
        return make
    plant("zu_at", holed(200), max_len=14000, zu="." * 8)
    plant("zu_over", holed(201), max_len=14000, zu="D" * 8)
    while len(piles) < L:                                            # the longest read: over a lowered DAMAR_TEST_FILTER_LEN
        piles.append(b"")
    plant("longest", lambda a: [(b, 0, 7000, 0) for b in (50, 51, 52)], zu="LLL")
    nrec = sum(p["nrec"] for p in plants.values())
    return b"".join(piles), nrec, plants, trim, rep, lists


def code(f):
    return ("S" if f & SYM else "C" if f & CONT else "T" if f & STITCH else "P" if f & REPEAT else "L" if f & LOCAL else "O" if f & OLEN else
            "R" if f & RLEN else "F" if f & DIFF else "D" if f & DISCARD else ".")


def track_arrays(iv, nreads):
    anno, data = [0], []
    for r in range(nreads):
        for b, e in iv.get(r, []):
            data += [b, e]
        anno.append(4 * len(data))
    return np.array(anno, dtype=np.uint64), np.array(data, dtype=np.int32)


def made_repeats(rl, seed):
    """a repeat track for a real input: up to three intervals on two reads of three, seeded"""
    rng = np.random.default_rng(seed)
    iv = {}
    for r in range(len(rl)):
        if rng.integers(3) == 0:
            continue
        cuts = np.sort(rng.integers(0, int(rl[r]) + 1, size=2 * int(rng.integers(1, 4))))
        iv[r] = [(int(cuts[2 * k]), int(cuts[2 * k + 1])) for k in range(len(cuts) // 2) if cuts[2 * k] < cuts[2 * k + 1]]
    return iv


def run(tool, opts, work):
    return subprocess.run([tool] + opts + ["G", fc.LAS, fc.OUT], cwd=work, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def main():
    tmp = tempfile.mkdtemp(prefix="filter_golden_")
    try:
        tool = build_tool(tmp)
        shutil.rmtree(OUT, ignore_errors=True)
        os.makedirs(OUT)
        rl = q_common.db_read_len("tiny2")
        body, nrec, plants, trim, rep, lists = synth(rl)
        open(os.path.join(OUT, "synth.las"), "wb").write(struct.pack("<qi", nrec, TW) + body)
        assert os.path.getsize(os.path.join(OUT, "synth.las")) < MAX_FILE
        tracks = {}
        tracks["fsynth_trim_anno"], tracks["fsynth_trim_data"] = track_arrays({r: [v] for r, v in trim.items()}, len(rl))
        tracks["fsynth_rep_anno"], tracks["fsynth_rep_data"] = track_arrays(rep, len(rl))
        for k, inp in enumerate(fc.REAL):
            lens = q_common.db_read_len(fc.INPUTS[inp][0])
            tracks[inp + "_rep_anno"], tracks[inp + "_rep_data"] = track_arrays(made_repeats(lens, 100 + k), len(lens))
        np.savez_compressed(os.path.join(OUT, "tracks.npz"), **tracks)

        # the cap: no run of one B read above the kernel's group, no read above its coverage bits, but for the planted ones
        for inp in fc.REAL + ("fsynth",):
            cols = tc.read_records(os.path.join(q_common.GOLDEN, fc.INPUTS[inp][1]))[0]
            key = cols[:, 7].astype(np.int64) << 32 | cols[:, 8]
            edges = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1], [True]]))
            runs = np.diff(edges)
            over = cols[edges[:-1][runs > G], 7]
            assert list(over) == ([plants["g65"]["aread"]] if inp == "fsynth" else []), (inp, over)
            assert q_common.db_read_len(fc.INPUTS[inp][0]).max() <= MAXLEN, inp

        # the plan's thresholds: the first of each list that changes what the reference writes for tiny2
        work = tempfile.mkdtemp(dir=tmp)
        fc.workdir(work, "tiny2", lists)
        run(tool, [], work)
        base = tc.md5(os.path.join(work, fc.OUT))

        def first(opt, values):
            for v in values:
                r = run(tool, [opt, str(v)], work)
                assert r.returncode == 0, r.stderr
                if tc.md5(os.path.join(work, fc.OUT)) != base:
                    return v
            raise AssertionError(opt)
        d, n, o = first("-d", (40, 35, 30, 25, 20)), first("-n", (100, 300, 500, 1000, 2000)), first("-o", (500, 1000, 2000, 3000))
        variants = fc.variants(d, n, o)
        case_list = ([("%s_%s" % (v, inp), inp, op) for inp in fc.REAL for v, op in variants] +
                     [("%s_synth" % v, "fsynth", op) for v, op in variants + fc.SYNTH_ONLY])
        cases, md5s, own_L, full_out, store, inputs = [], {}, {}, {}, {}, {}
        for name, inp, opts in case_list:
            work = tempfile.mkdtemp(dir=tmp)
            fc.workdir(work, inp, lists)
            if "-L" in opts:                                             # the reference's own -L run is only compared, not kept
                r = run(tool, opts, work)
                own_L[inp] = tc.md5(os.path.join(work, fc.OUT)) if r.returncode == 0 else None
            r = run(tool, [x for x in opts if x != "-L"], work)
            assert r.returncode == 0, (name, r.stderr)
            out = os.path.join(work, fc.OUT)
            cols, trace, novl, tspace = tc.read_records(out)
            case = dict(name=name, input=inp, opts=opts, rc=r.returncode, stdout=r.stdout, stderr=r.stderr, md5=tc.md5(out),
                        md5_a=fc.md5_or_none(os.path.join(work, fc.A_FILE)))
            full_out[name] = r.stdout
            if len(r.stdout) > fc.STDOUT_KEPT:                          # many lines: their md5 stands for them
                case["stdout"], case["stdout_md5"] = None, fc.text_md5(r.stdout)
            cases.append(case)
            md5s[name] = case["md5"]
            if inp not in inputs:
                inputs[inp] = tc.read_records(os.path.join(work, fc.LAS))[0]
            keep = store.setdefault(inp, dict(tspace=tspace))
            same = [c["name"] for c in cases[:-1] if c["input"] == inp and c["md5"] == case["md5"]]
            if same:                                                     # the records of an earlier case of this input
                case["same_as"] = same[0]
            elif "-p" in opts or "-T" in opts:
                keep[name + ":cols"] = cols
            else:                                                        # the five words that can change, where they do
                assert len(cols) == len(inputs[inp]) and np.array_equal(cols[:, fc.FIXED], inputs[inp][:, fc.FIXED]), name
                for k in fc.LOOSE:
                    at = np.flatnonzero(cols[:, k] != inputs[inp][:, k]).astype(np.int32)
                    keep["%s:i%d" % (name, k)], keep["%s:v%d" % (name, k)] = at, cols[at, k]
            print("%-14s %6d records out, %6d discarded, %5d lines" % (name, novl, int(np.sum((cols[:, 6] & DISCARD) != 0)), r.stdout.count("\n")))
            if inp == "fsynth" and "-p" not in opts:
                key = name.rsplit("_", 1)[0]
                for tag, pl in plants.items():
                    rows = np.flatnonzero(cols[:, 7] == pl["aread"])
                    assert len(rows) == pl["nrec"], (name, tag)
                    got = "".join(code(int(f)) for f in cols[rows, 6])
                    pl.setdefault("seen", {})[key] = got
                    exp = pl["expect"].get(key)
                    assert exp is None or all(e in ("?", g) for e, g in zip(exp, got)), "%s: plant %s came out as %s, planted %s" % (name, tag, got, exp)
        for inp, keep in store.items():
            dst = os.path.join(OUT, "expected_%s.npz" % inp)
            np.savez_compressed(dst, **keep)
            assert os.path.getsize(dst) < MAX_FILE, (inp, os.path.getsize(dst))
        json.dump(dict(cases=cases), open(os.path.join(OUT, "cases.json"), "w"))   # for fc.expected below; written whole at the end
        same_L = {inp: own_L[inp] == md5s["def_" + inp.replace("fsynth", "synth")] for inp in own_L}
        print("-L equals the run without it:", same_L)
        # plants whose branch shows in the lines or in the coordinates
        out = {k: dict(stdout=v) for k, v in full_out.items()}
        a = plants["chain3"]["aread"]
        row = fc.expected("s_synth")["cols"]
        row = row[row[:, 7] == a][0]
        assert (row[0], row[4], row[5]) == (0, 3000, 3000), row                      # the head runs to the end of the third, its trace gone
        row = fc.expected("s_synth")["cols"]
        row = row[row[:, 7] == plants["two_cand"]["aread"]][0]
        assert row[4] == 2500, row                                                  # the longer candidate
        assert "overlap (0 x 70): in list of discarded overlaps" in out["A_synth"]["stdout"]           # the run-on list
        assert "overlap (1 x 0): in list of discarded overlaps" in out["A_synth"]["stdout"]
        for tag in ("n_a_over", "tip_begin", "tip_end", "tips_cross"):
            assert "overlap %d -> 104: drop due to repeat in a" % plants[tag]["aread"] in out["nY_synth" if tag != "n_a_over" else "n_synth"]["stdout"], tag
        assert "overlap %d -> 88: drop due to repeat in b" % plants["n_b_only"]["aread"] in out["n_synth"]["stdout"]
        assert "found contained OVL: %d vs %d a[0,1000] equals" % ((plants["self1"]["aread"],) * 2) in out["R6_synth"]["stdout"]
        assert "in a[0,3000] b[0,3000]" in out["R6_synth"]["stdout"]
        assert "falls into multi mapper interval: %d vs" % plants["mm_pair"]["aread"] in out["vw_synth"]["stdout"]
        assert "falls into multi mapper interval: %d vs" % plants["mm_none"]["aread"] not in out["vw_synth"]["stdout"]

        work = tempfile.mkdtemp(dir=tmp)
        fc.workdir(work, "tiny2", lists)
        errors = []
        for name, args in fc.ERRORS:
            r = subprocess.run([tool] + args, cwd=work, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            errors.append(dict(name=name, args=args, rc=r.returncode, stdout=r.stdout, stderr=r.stderr))
            assert r.returncode == 1, (name, r.returncode, r.stderr)
        for pl in plants.values():
            pl.pop("seen", None)
        with open(os.path.join(OUT, "cases.json"), "w") as f:          # one case, error run or plant a line
            line = lambda kind, items: '"%s": [\n%s\n]' % (kind, ",\n".join(json.dumps(x) for x in items))
            f.write("{\n" + line("cases", cases) + ",\n" + line("errors", errors) + ",\n")
            f.write('"plants": {\n%s\n},\n' % ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in plants.items()))
            f.write('"same_L": %s,\n"files": %s,\n"plan": %s\n}\n' % (json.dumps(same_L), json.dumps(lists), json.dumps(dict(d=d, n=n, o=o))))
        assert os.path.getsize(os.path.join(OUT, "cases.json")) < MAX_FILE
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
