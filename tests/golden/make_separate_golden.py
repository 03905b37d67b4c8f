#!/usr/bin/env python3
"""Fixtures of LAseparate (tests/golden/separate/) from the REFERENCE.

Runs only where the reference sources lie (REF_SRC, default /root/reference): LAseparate is compiled with a plain gcc line
into a temporary directory outside the repository, run on the .las files this repository already holds (with the repeat
tracks the LAfilter fixtures hold for them, which LArepeat made, under the name rep, and their trim tracks as rep2) and on
one planted file written here, and only data is kept: synth.las, its two tracks (synth_tracks.npz), cases.json (options,
exit status, stdout, stderr, md5 of both outputs; the error runs; what synth.las plants) and expected.npz (per case and
input record the flags word of the reference's first pass).  Nothing compiled is kept.

tests/separate_model.py is held to the reference here: on every case its flags must give the reference's two files, and
every plant must come out of the model as the branch it was made for.  On the real files the model must find no group
beyond the limits the library is built with.

    python tests/golden/make_separate_golden.py
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
import separate_common as sc                           # noqa: E402
import separate_model as sm                            # noqa: E402
import trim_common as tc                               # noqa: E402

OUT = sc.SDIR
TW = sc.TW
MAX_FILE = 1 << 20
COMP, DISCARD, CONT = 0x1, 0x2, 0x8000
MAXGROUP, MAXCHAINS = 64, 16            # include/damar_hip.h DAMAR_SEPARATE_MAXGROUP, DAMAR_SEPARATE_MAXCHAINS


def build_tool(tmp):
    s = lambda *p: os.path.join(SRC, *p)
    subprocess.run(["gcc", "-O3", "-w", "-fno-strict-aliasing", "-I" + SRC, "-o", os.path.join(tmp, "LAseparate"), s("scrub", "LAseparate.c"),
                    s("lib", "read_loader.c"), s("lib", "utils.c"), s("lib", "tracks.c"), s("lib", "pass.c"), s("lib", "oflags.c"),
                    s("lib", "compression.c"), s("lib", "trim.c"), s("db", "QV.c"), s("db", "DB.c"), s("dalign", "align.c"),
                    "-lm", "-lz", "-lpthread"], cwd=tmp, check=True)
    return os.path.join(tmp, "LAseparate")


def rec(a, b, ab, ae, bb, be=None, flags=0):
    """one record with a trace of its own: no differences, B's bases shared out over A's intervals.  LAseparate reads no
    base of a read, so a plant's coordinates may lie beyond its reads' ends where a look-ahead of 30 000 needs the room."""
    be = bb + (ae - ab) if be is None else be
    cuts = [ab] + list(range((ab // TW + 1) * TW, ae, TW)) + [ae]
    al = np.diff(cuts)
    extra = (be - bb) - (ae - ab)
    bl = al + extra // len(al) + (np.arange(len(al)) < extra % len(al))
    assert np.all(bl >= 0) and np.all(bl <= 255) and bl.sum() == be - bb
    tr = np.zeros(2 * len(al), dtype=np.uint8)
    tr[1::2] = bl
    return struct.pack("<10i", len(tr), 0, ab, bb, ae, be, flags, a, b, 0) + tr.tobytes()


def synth(rl):
    """-> (file body, record count, plants, the two tracks as {read: intervals}).  A plant is one group on an A read of its
    own (a pile of several groups where the pile is the plant); `model` is what the model must make of it for -T0:
    (chains, members of the best chain, proper), `t1` the characters of its records after -T1 ('.' kept, 'D' discarded)."""
    plants, piles, piles_of = {}, [], {}
    rep, rep2 = {}, {}
    long_reads = [r for r in range(len(rl)) if rl[r] >= 7000]
    assert len(long_reads) >= 95, len(long_reads)
    nexta = iter(long_reads)

    def plant(tag, recs, b=None, model=None, t1=None, a=None):
        a = next(nexta) if a is None else a
        b = long_reads[-1 - len(plants) % 40] if b is None else b
        while len(piles) <= a:
            piles.append([])
        piles[a].append(b"".join(rec(a, b, *r) for r in recs))
        plants[tag] = dict(aread=a, bread=b, nrec=len(recs), model=model, t1=t1)
        return a, b

    AL = lambda a: int(rl[a])
    # groups of one record: proper and real at both ends, improper at its begin, proper and not real
    a = next(nexta); plant("one_real", [(0, AL(a), 0, AL(a))], a=a, model=(0, [], True), t1="D")
    plant("one_improper", [(2000, 5000, 2000, 5000)], model=(0, [], False), t1="D")
    a = next(nexta); plant("one_proper", [(500, AL(a), 500, AL(a))], a=a, model=(0, [], True), t1=".")
    # one chain of two records that reaches the read's end; one record contained in the other: a chain of one
    a = next(nexta); plant("two", [(0, 3000, 0, 3000), (3100, AL(a), 3100, AL(a))], a=a, model=(1, [0, 1], True), t1="..")
    a = next(nexta); plant("chain_of_one", [(0, AL(a), 0, AL(a)), (1000, 2000, 1000, 2000)], a=a, model=(1, [0], True), t1="DD")
    # the look-ahead: at a gap of exactly 5 000 (30 000) the shorter record is met in the first (last) step and taken, the
    # longer one a base further away is never looked at again; on the left the same
    plant("right_5000", [(0, 4000, 0, 4000), (9000, 11000, 9000, 11000), (9001, 12500, 9001, 12500)], model=(1, [0, 1], None))
    plant("right_both_5000", [(0, 4000, 0, 4000), (9000, 11000, 9000, 11000), (9000, 12500, 9000, 12500)], model=(1, [0, 2], None))
    plant("right_30000", [(0, 4000, 0, 4000), (34000, 36000, 34000, 36000), (34001, 37500, 34001, 37500)], model=(1, [0, 1], None))
    plant("right_30001", [(0, 4000, 0, 4000), (34001, 36000, 34001, 36000)], model=(2, [0], None))
    plant("left_5000", [(31500, 34999, 31500, 34999), (33000, 35000, 33000, 35000), (40000, 44000, 40000, 44000)], model=(1, [1, 2], None))
    plant("left_30000", [(6500, 9999, 6500, 9999), (8000, 10000, 8000, 10000), (40000, 44000, 40000, 44000)], model=(1, [1, 2], None))
    plant("left_30001", [(8000, 9999, 8000, 9999), (40000, 44000, 40000, 44000)], model=(2, [1], None))
    # two candidates in one step: the right side keeps the minimum of the two unique counts and moves on to the longer
    # record, the left side keeps their sum, which the longer record's minimum does not beat
    plant("right_min", [(0, 4000, 0, 4000), (6000, 8000, 6000, 8000), (6001, 9500, 6001, 9500)], model=(1, [0, 2], None))
    plant("left_sum", [(34500, 37999, 34500, 37999), (36000, 38000, 36000, 38000), (40000, 44000, 40000, 44000)], model=(1, [1, 2], None))
    # the overhang of a half: at equality admitted, a base more refused (and discarded as a bystander)
    plant("overhang_eq", [(0, 4000, 0, 4000), (3000, 5000, 3000, 5000)], model=(1, [0, 1], None))
    plant("overhang_over", [(0, 4000, 0, 4000), (2999, 5000, 2999, 5000)], model=(1, [0], None), t1="DD")
    # a gap filler at the slack of 100 bases, and one over it (a bystander, discarded)
    plant("fill", [(0, 4000, 0, 4000), (3901, 6099, 3901, 6099), (6000, 10000, 6000, 10000)], model=(1, [0, 1, 2], None))
    plant("fill_over", [(0, 4000, 0, 4000), (3900, 6099, 3900, 6099), (6000, 10000, 6000, 10000)], model=(1, [0, 2], None))
    # a second chain inside the span of the first: a complemented one is refused, another is not looked at (the `&&`)
    plant("sanity_comp", [(0, 3000, 0, 3000), (4000, 5000, 20000, 21000, COMP), (6000, 9000, 6000, 9000)], model=(1, [0, 2], None))
    plant("sanity_norm", [(0, 3000, 0, 3000), (4000, 5000, 20000, 21000), (6000, 9000, 6000, 9000)], model=(2, [0, 2], None))
    # the order of the chains: the pair's length is its two spans less one (5 499), not less the intersection of 500
    plant("len_tie", [(0, 3000, 0, 3000), (2500, 5000, 2500, 5000), (50000, 55499, 60000, 65499, COMP)], model=(2, [2], None))
    plant("len_arith", [(0, 3000, 0, 3000), (2500, 5000, 2500, 5000), (50000, 55498, 60000, 65498, COMP)], model=(2, [0, 1], None))
    # overlapBases * 0.3 against the gap: 5 000 bases and a gap of 1 500 is not proper, of 1 499 is
    for tag, gap, ok in (("gap_eq", 1500, False), ("gap_under", 1499, True)):
        b = long_reads[-45]
        d = int(rl[b]) - (5000 + gap)                                    # the chain ends with its B read
        plant(tag, [(0, 3000, d, d + 3000), (3000 + gap, 5000 + gap, d + 3000 + gap, d + 5000 + gap)], b=b, model=(1, [0, 1], ok))
    # an intersection of 1 000 between two members, and of 1 001
    for tag, its, ok in (("its_1000", 1000, True), ("its_1001", 1001, False)):
        a = next(nexta)
        e = AL(a)
        plant(tag, [(0, 4000, 0, 4000), (4000 - its, e, 4000 - its, e)], a=a, model=(1, [0, 1], ok))
    # the repeats: a read without an interval, with one, with several; a self overlap; a complemented record whose B
    # interval the reference maps through the overlap's span
    a, b = plant("rep_one", [(0, 3000, 0, 3000), (3100, 6000, 3100, 6000)], model=(1, [0, 1], None))
    rep[a] = [(0, 2900)]
    a, b = plant("rep_many", [(0, 3000, 0, 3000), (3100, 6000, 3100, 6000), (6100, 8000, 6100, 8000)], model=(1, [0, 1, 2], None))
    rep[a] = [(100, 200), (1000, 2900), (3100, 5000), (7000, 9000)]
    a = next(nexta)
    plant("self", [(0, 3000, 4000, 7000), (3100, 6000, 7100, 10000)], a=a, b=a, model=(1, [0, 1], None))
    rep[a] = [(0, 1000), (7000, 8000)]
    a, b = plant("comp_span", [(0, 3000, 2000, 5000, COMP), (3100, 5600, 5100, 7600, COMP)], b=long_reads[-42], model=(1, [0, 1], None))
    rep[a] = [(0, 20000)]
    rep[b] = [(0, 1000)]
    # "for repetitive genomes": every interval twice, so that the unique counts are negative and only the last step's
    # branch can take the record that contains the seed
    a, b = plant("repetitive", [(1000, 5000, 1000, 5000), (500, 10000, 500, 10000)], b=long_reads[-43], model=(1, [0, 1], None))
    rep[a] = [(0, 50000), (0, 50000)]
    rep[b] = [(5000, 10000), (5000, 10000)]
    a, b = plant("not_repetitive", [(1000, 5000, 1000, 5000), (500, 10000, 500, 10000)], b=long_reads[-44])
    # the seed: two records that cannot chain and intersect, so that the seed's chain of one discards the other.  The first
    # is proper, the second longer and not.  With the second's bases mostly in repeats the first is the seed (by unique
    # bases, against the longest record) and -T0 discards the group; without the track the second would be, and keep it.
    b = long_reads[-46]
    a, b = plant("seed_unique", [(0, 3000, int(rl[b]) - 3000, int(rl[b])), (2000, 6000, 2000, 6000)], b=b, model=(1, [0], True))
    rep[a] = [(3000, 6000)]
    rep[b] = [(3000, 6000)]
    # the same two records with next to nothing unique in either (10 bases and none): below the trace spacing the longest
    # record is the seed after all, and -T0 keeps the group
    b = long_reads[-47]
    a, b = plant("seed_fallback", [(0, 3000, int(rl[b]) - 3000, int(rl[b])), (2000, 6000, 2000, 6000)], b=b, model=(1, [1], False))
    rep[a] = [(10, 6000)]
    rep[b] = [(0, int(rl[b]))]
    # a gap filler of 80 bases that fits the gap on either side of a chain member of 100 bases: it enters the chain twice,
    # the chain is longer than its group, and the count of records left goes below zero
    twice = [(0, 4000, 0, 4000), (8910, 8990, 8910, 8990), (8900, 9000, 8900, 9000), (9100, 13000, 9100, 13000)]
    plant("fill_twice", twice, model=(1, [0, 2, 1, 1], None))
    # ... and in a group of 64 records whose chain so has 65 members: more than a lane's list holds
    plant("fill_twice_64", twice + [(13100 + 3000 * k, 16000 + 3000 * k, 13100 + 3000 * k, 16000 + 3000 * k) for k in range(60)],
          model=(1, [0, 2, 1, 1] + list(range(3, 63)), None))
    # the limits: groups of 64 and 65 records in one chain, groups of 16 and 17 chains, piles of 64 and 65 groups of two
    plant("group_64", [(3000 * k, 3000 * k + 2900, 3000 * k, 3000 * k + 2900) for k in range(64)], model=(1, list(range(64)), None))
    plant("group_65", [(3000 * k, 3000 * k + 2900, 3000 * k, 3000 * k + 2900) for k in range(65)], model=(1, list(range(65)), None))
    plant("chains_16", [(40000 * k, 40000 * k + 2000 + k, 40000 * k, 40000 * k + 2000 + k) for k in range(16)], model=(16, [15], None))
    plant("chains_17", [(40000 * k, 40000 * k + 2000 + k, 40000 * k, 40000 * k + 2000 + k) for k in range(17)], model=(17, [16], None))
    for tag, ng in (("pile_64", 64), ("pile_65", 65)):
        a = next(nexta)
        plain = [r for r in range(len(rl)) if r != a and r not in rep]       # B reads without an interval
        for k in range(ng):
            plant("%s_%d" % (tag, k), [(0, 3000, 0, 3000), (3100, 6000 + k, 3100, 6000 + k)], a=a, b=plain[k], model=(1, [0, 1], None))
        piles_of[tag] = dict(aread=a, groups=ng, nrec=2 * ng)
    # the second track: the first one's intervals moved, so that -r changes counts
    for r, iv in rep.items():
        rep2[r] = [(x + 700, y + 700) for x, y in iv[:1]]
    nrec = sum(p["nrec"] for p in plants.values())
    return b"".join(b"".join(p) for p in piles), nrec, plants, rep, rep2, piles_of


def split_of(inp_cols, out_cols, out2_cols):
    """the reference's two files back onto the input's records: -> the flags word per input record (OVL_DISCARD set where
    the record went to the second file)"""
    flags = np.zeros(len(inp_cols), dtype=np.int32)
    i1 = i2 = 0
    key = [0, 1, 2, 3, 4, 5, 7, 8, 9]
    for i, row in enumerate(inp_cols):
        if i1 < len(out_cols) and np.array_equal(out_cols[i1, key], row[key]):
            flags[i] = out_cols[i1, 6]
            i1 += 1
        else:
            assert i2 < len(out2_cols) and np.array_equal(out2_cols[i2, key], row[key]), i
            flags[i] = out2_cols[i2, 6] | DISCARD
            i2 += 1
    assert (i1, i2) == (len(out_cols), len(out2_cols))
    return flags


def main():
    tmp = tempfile.mkdtemp(prefix="separate_golden_")
    try:
        tool = build_tool(tmp)
        shutil.rmtree(OUT, ignore_errors=True)
        os.makedirs(OUT)
        rl = q_common.db_read_len("tiny2")
        body, nrec, plants, rep, rep2, piles_of = synth(rl)
        open(os.path.join(OUT, "synth.las"), "wb").write(struct.pack("<qi", nrec, TW) + body)
        assert os.path.getsize(os.path.join(OUT, "synth.las")) < MAX_FILE
        tracks = {}
        for nm, iv in (("rep", rep), ("rep2", rep2)):
            anno, data = [0], []
            for r in range(len(rl)):
                for b, e in iv.get(r, []):
                    data += [b, e]
                anno.append(4 * len(data))
            tracks[nm + "_anno"], tracks[nm + "_data"] = np.array(anno, dtype=np.uint64), np.array(data, dtype=np.int32)
        np.savez_compressed(os.path.join(OUT, "synth_tracks.npz"), **tracks)

        cases, expected, longest, share = [], {}, 0, {}
        for name, inp, opts in sc.CASES:
            work = tempfile.mkdtemp(dir=tmp)
            sc.workdir(work, inp)
            r = sc.run_tool(opts, work, exe=tool)
            assert r.returncode == 0, (name, r.stderr)
            p = lambda f: os.path.join(work, f)
            case = dict(name=name, input=inp, opts=opts, rc=r.returncode, stdout=r.stdout, stderr=r.stderr, md5=tc.md5(p(sc.OUT)),
                        md5_discard=tc.md5(p(sc.OUT2)))
            cols = tc.read_records(p(sc.LAS))[0]
            flags = split_of(cols, tc.read_records(p(sc.OUT))[0], tc.read_records(p(sc.OUT2))[0])
            if name.startswith("T0L_"):                                  # the options that reach nothing
                twin = next(c for c in cases if c["name"] == "T0_" + inp)
                assert (case["md5"], case["md5_discard"], case["stdout"]) == (twin["md5"], twin["md5_discard"], twin["stdout"]), name
                case["same_as"] = twin["name"]
            else:
                expected[name] = flags
            cases.append(case)
            # the model against the reference's files, and what it finds beyond the limits
            batch = sc.batch_of(p(sc.LAS))
            rlen = q_common.db_read_len(sc.INPUTS[inp][0])
            mf, mg, full = sc.model_batch(batch, rlen, sc.tracks(inp)[sc.track_of(opts)], TW if inp == "ssynth" else tc.read_records(p(sc.LAS))[3],
                                          sc.kind_of(opts))
            assert np.array_equal(mf & ~sc.TEMP, flags), (name, np.flatnonzero((mf & ~sc.TEMP) != flags)[:8])
            kept = sum(m["counts"][0] for m in full)
            gone = sum(m["counts"][1] for m in full)
            assert r.stdout == sc.PASS + "Kept    ovls: %10d\nDiscard ovls: %10d\n" % (kept, gone) + sc.PASS + \
                "Kept    ovls: %10d\nDiscard ovls: %10d\n" % (gone, kept), name
            sizes = [len(g[1]) for g in sc.groups_of(batch)]
            over = [i for i, (m, s) in enumerate(zip(full, sizes)) if sc.beyond_limits(m, s, MAXGROUP, MAXCHAINS)]
            case["host_groups"] = len(over)
            if inp != "ssynth":
                assert not over, "%s: the model finds groups beyond the built limits: raise them" % name
                longest = max(longest, max(sizes))
                share[inp] = (sum(1 for s in sizes if s > 1), len(sizes))
            print("%-12s %6d kept %6d discarded, %5d groups, %4d of more than one record, longest %d, most chains %d" %
                  (name, kept, gone, len(sizes), sum(1 for s in sizes if s > 1), max(sizes), max(g[0] for g in mg)))
        np.savez_compressed(os.path.join(OUT, "expected.npz"), **expected)
        assert os.path.getsize(os.path.join(OUT, "expected.npz")) < MAX_FILE

        # every plant against the model: the branch it was made for
        batch = sc.batch_of(os.path.join(OUT, "synth.las"))
        rep_t = (tracks["rep_anno"], tracks["rep_data"])
        groups = sc.groups_of(batch)
        for kind in (0, 1):
            mf, mg, full = sc.model_batch(batch, rl, rep_t, TW, kind)
            for tag, pl in plants.items():
                gi = next(i for i, (g0, recs) in enumerate(groups) if recs[0]["aread"] == pl["aread"] and recs[0]["bread"] == pl["bread"])
                g0 = groups[gi][0]
                if kind == 0:
                    if pl["model"] is not None:
                        want = [pl["model"][0], pl["model"][1], mg[gi][2] if pl["model"][2] is None else pl["model"][2]]    # None: not the plant's point
                        assert list(mg[gi]) == want, (tag, mg[gi], pl["model"])
                    pl["seen"] = [mg[gi][0], mg[gi][1], mg[gi][2]]
                elif pl["t1"] is not None:
                    got = "".join("D" if f & DISCARD else "." for f in mf[g0:g0 + pl["nrec"]])
                    assert got == pl["t1"], (tag, got, pl["t1"])
        gi = lambda tag: next(i for i, (g0, recs) in enumerate(groups) if recs[0]["aread"] == plants[tag]["aread"] and recs[0]["bread"] == plants[tag]["bread"])
        # the branch for repetitive genomes made the chain of two; without the doubled intervals the same records are one chain by the plain rule
        assert plants["repetitive"]["seen"][:2] == [1, [0, 1]]
        # the complemented record's count is the reference's mapping, not the read's
        o = groups[gi("comp_span")][1][0]
        assert sm.repeat_bases(rep_t, o, o["bread"]) == 1000
        blen = int(rl[o["bread"]])
        assert sm.intersect(blen - o["be"], blen - o["bb"], 0, 1000) == 0
        # the self overlap counts A's coordinates for both reads
        o = groups[gi("self")][1][0]
        assert sm.repeat_bases(rep_t, o, o["bread"]) == sm.repeat_bases(rep_t, o, o["aread"]) == 1000

        # the seed plants decide what the reference's files show: without the track the first, with a trace spacing of 0 the
        # second comes out the other way round, and so does at least one record of the -T0 files
        mf0, mg0, _ = sc.model_batch(batch, rl, rep_t, TW, 0)
        for tag, other in (("seed_unique", sc.model_batch(batch, rl, None, TW, 0)), ("seed_fallback", sc.model_batch(batch, rl, rep_t, 0, 0))):
            g0, n = groups[gi(tag)][0], plants[tag]["nrec"]
            assert mg0[gi(tag)][1] != other[1][gi(tag)][1] and mg0[gi(tag)][2] != other[1][gi(tag)][2], tag
            assert np.all((mf0[g0:g0 + n] ^ other[0][g0:g0 + n]) & DISCARD), tag
            assert np.array_equal(mf0[g0:g0 + n] & ~sc.TEMP, expected["T0_ssynth"][g0:g0 + n]), tag
        # the filler taken twice: a chain longer than its group, in the second plant longer than a lane's list
        for tag, n in (("fill_twice", 5), ("fill_twice_64", 65)):
            m = sc.model_batch(batch, rl, rep_t, TW, 0)[2][gi(tag)]
            assert len(m["best"]) == n and m["best"].count(1) == 2, (tag, m["best"])
        # the piles of 64 and 65 groups: every group one chain of its two records; one entry a pile is kept
        for tag, pl in piles_of.items():
            mine = [plants.pop("%s_%d" % (tag, k)) for k in range(pl["groups"])]
            assert all(m["seen"][:2] == [1, [0, 1]] for m in mine), tag
        plants.update(piles_of)

        # the group the reference aborts on: recorded, not kept as a case
        work = tempfile.mkdtemp(dir=tmp)
        sc.workdir(work, "fusion")
        sc.flag_first_pair(os.path.join(work, sc.LAS))
        r = sc.run_tool(["-T0"], work, exe=tool)
        assert r.returncode == -6 and "nKeptOvls + sctx.nDiscardOvls == pctx->novl" in r.stderr, (r.returncode, r.stderr)
        aborts = dict(rc=r.returncode, assertion="sctx.nKeptOvls + sctx.nDiscardOvls == pctx->novl")     # its message names the source's place too

        work = tempfile.mkdtemp(dir=tmp)
        sc.workdir(work, "tiny2")
        errors = []
        for name, args in sc.ERRORS:
            r = sc.run_tool([], work, args=args, exe=tool)
            errors.append(dict(name=name, args=args, rc=r.returncode, stdout=r.stdout, stderr=r.stderr))
            assert r.returncode == 1, (name, r.returncode, r.stderr)
        json.dump(dict(cases=cases, errors=errors, plants=plants, reference_aborts=aborts, longest_real_group=longest, multi_share=share),
                  open(os.path.join(OUT, "cases.json"), "w"), indent=1)
        print("longest group of the real files:", longest, " groups of more than one record:", share)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
