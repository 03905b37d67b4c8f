#!/usr/bin/env python3
"""Fixtures of DBdust (tests/golden/dust/) from the REFERENCE's DBdust.

Runs only where oracle/_ref/ is built (FA2db, DBsplit, DBdust) and this project's library as well: the plants that need a
search (an interval of an exact length, two intervals a base apart) are looked for with the host routine and the model of
tests/dust_model.py, and then asserted in what the reference wrote.  Kept: the planted database P (one block) and the
database A of the append run, expected.npz with the reference's track files (and, for -m1, which it refuses, its stderr and
exit status) per option set, the tracks of mask_dust's two blocks, the stderr of the error runs, and cases.json with what
each planted read is there for.

    python tests/golden/make_dust_golden.py
"""
import json
import os
import random
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
REF = os.path.join(ROOT, "oracle", "_ref")
OUT = os.path.join(HERE, "dust")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import dust_common as dc          # noqa: E402
import dust_model                 # noqa: E402
from make_golden import write_fasta          # noqa: E402
from damar_amd import api         # noqa: E402

MAX_FILE = 1 << 20
W, M = 64, 10
P = api.dust_limits()[0]          # the kernel's piece: a border lies at every multiple of it


def rnd(rng, n):
    return [rng.randrange(4) for _ in range(n)]


def host(seq, **kw):
    return [tuple(x) for x in api.dust_host_read(np.array(seq, dtype=np.uint8), **kw)[0].tolist()]


def with_run(rng, total, at, run):
    s = rnd(rng, total)
    s[at:at + len(run)] = run
    return s


def search(what, build, ok, tries=4000):
    for k in range(tries):
        s = build(random.Random(1000 * sum(map(ord, what)) + k), k)
        if ok(s):
            return s
    raise AssertionError("no read found for " + what)


def exact_length(side, length):
    """a short run whose interval (with -m2) has exactly `length` bases and lies wholly on one side of the border P, no
    other interval within 2 W of the border"""
    def build(rng, k):
        at = (P - 40 if side < 0 else P + 8) + k % 5
        return with_run(rng, 2 * P - 100, at, [k % 4] * (6 + (k // 5) % 10))

    def ok(s):
        near = [(b, e) for b, e in host(s, minlen=2) if e > P - 2 * W and b < P + 2 * W]
        return len(near) == 1 and near[0][1] - near[0][0] == length and (near[0][1] <= P if side < 0 else near[0][0] >= P)
    return search("len%d_%d" % (length, side), build, ok)


def gap_across(apart):
    """two masked intervals, the first of candidates that start before the border P, the second of candidates that start
    behind it, with `apart` bases between the last base of the one and the first of the other: 0 is joined by the + 1
    rule, 1 just is not"""
    def build(rng, k):
        s = rnd(rng, 2 * P - 50)
        at = P - 30 - k % 7
        s[at:at + 24] = [k % 4] * 24
        at = P - 6 - k % 7 + (k // 64) % 12
        s[at:at + 24] = [(k // 4) % 4, (k // 16) % 4] * 12
        return s

    def ok(s):
        end = None                                 # the last base of the mask so far
        for b, e in api.dust_host_candidates(np.array(s, dtype=np.uint8))[0].tolist():
            if end is not None and b >= P and end + 1 + apart == b and first < P:
                return True
            if end is None or end + 1 < b:
                first, end = b, e + 2
            else:
                end = max(end, e + 2)
        return False
    return search("gap%d" % apart, build, ok)


def longest_list():
    best, at = None, 0
    for k in range(400):
        rng = random.Random(7000 + k)
        x, y = rng.randrange(4), rng.randrange(4)
        s = rnd(rng, 100) + [x if rng.randrange(3 + k % 4) else y for _ in range(400)] + rnd(rng, 100)
        n = api.dust_host_read(np.array(s, dtype=np.uint8))[1]
        if n > at:
            best, at = s, n
    return best, at


def plants():
    rng = random.Random(20240613)
    out = []                                      # (what, bases)
    for n in (0, 1, 2, 3, W - 3, W - 2, W - 1, W, W + 1):
        out.append(("poly_a_len_%d" % n, [0] * n))
    for n in (P - 1, P, P + 1, 2 * P, 2 * P + 1):                       # triplets: two more bases
        s = rnd(rng, n + 2)
        for at in range(P - 20, n - 10, P):                              # a period-2 run over every border inside
            s[at:at + 40] = [1, 3] * 20
        out.append(("triplets_%d" % n, s))
    out.append(("homopolymer", [2] * 3000))
    out.append(("period_2", [0, 3] * 1250))
    out.append(("period_3", [0, 1, 2] * 834))
    out.append(("run_over_border", with_run(rng, 2 * P + 300, P - 24, [0] * 100)))
    out.append(("run_ends_at_border", with_run(rng, 2 * P + 300, P - 124, [3] * 124)))
    out.append(("run_begins_at_border", with_run(rng, 2 * P + 300, P, [1] * 126)))
    out.append(("joined_across_border", gap_across(0)))
    out.append(("not_joined_across_border", gap_across(1)))
    out.append(("exactly_m_before_border", exact_length(-1, M)))
    out.append(("exactly_m_behind_border", exact_length(+1, M)))
    out.append(("m_less_1_before_border", exact_length(-1, M - 1)))
    out.append(("m_less_1_behind_border", exact_length(+1, M - 1)))
    out.append(("run_at_read_end", rnd(rng, 1500) + [0, 2] * 20))
    s, n = longest_list()
    out.append(("longest_candidate_list_%d" % n, s))
    return out, n


def run(cmd, cwd, **kw):
    return subprocess.run(cmd, cwd=cwd, check=True, **kw)


def make_db(d, root, reads):
    write_fasta(os.path.join(d, root + ".fasta"), ["".join("acgt"[x] for x in s) for s in reads])
    run([os.path.join(REF, "FA2db"), "-x0", root, root + ".fasta"], d, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)


def ref_dust(args, cwd):
    return subprocess.run([os.path.join(REF, "DBdust")] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def check_plants(names, reads, by_set):
    """what each plant was planted for, in the reference's own output"""
    dflt, m2 = by_set["default"], by_set["m2"]
    iv = lambda track, what: [tuple(x) for x in track[names.index(what)].tolist()]
    for i, what in enumerate(names):
        n = len(reads[i])
        if what.startswith("poly_a_len_"):
            assert iv(dflt, what) == ([(0, n)] if n >= M else []), (what, iv(dflt, what))
        if what.startswith("triplets_"):
            for at in range(P, n - 2, P):
                assert any(b < at < e for b, e in iv(dflt, what)), what
        if what in ("homopolymer", "period_2", "period_3"):
            assert iv(dflt, what) == [(0, n)], what
    assert any(P - W <= b < P < e for b, e in iv(dflt, "run_over_border")), iv(dflt, "run_over_border")
    assert any(P <= e <= P + 3 for b, e in iv(dflt, "run_ends_at_border")), iv(dflt, "run_ends_at_border")
    assert any(P - 3 <= b <= P for b, e in iv(dflt, "run_begins_at_border")), iv(dflt, "run_begins_at_border")
    assert any(b < P < e for b, e in iv(m2, "joined_across_border"))
    v = iv(m2, "not_joined_across_border")
    assert any(v[k][1] + 1 == v[k + 1][0] and v[k][0] < P <= v[k + 1][0] for k in range(len(v) - 1)), v
    for side, where in ((-1, "before"), (1, "behind")):
        near = lambda t, w: [(b, e) for b, e in iv(t, w) if e > P - 2 * W and b < P + 2 * W]
        a, b = "exactly_m_%s_border" % where, "m_less_1_%s_border" % where
        assert [e - s for s, e in near(m2, a)] == [M] and near(dflt, a) == near(m2, a), a
        assert [e - s for s, e in near(m2, b)] == [M - 1] and near(dflt, b) == [], b
    last = iv(dflt, "run_at_read_end")[-1]
    assert last[1] == len(reads[names.index("run_at_read_end")]), last


def main():
    for t in ("FA2db", "DBsplit", "DBdust"):
        assert os.path.exists(os.path.join(REF, t)), "build oracle/_ref first"
    planted, longest = plants()
    names, reads = [p[0] for p in planted], [p[1] for p in planted]
    if os.path.isdir(OUT):
        shutil.rmtree(OUT)
    os.makedirs(OUT)
    exp, by_set = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        make_db(tmp, "P", reads)
        run([os.path.join(REF, "DBsplit"), "-s1", "P"], tmp, stdout=subprocess.DEVNULL)
        got, _ = dc.db_reads(tmp, "P")
        assert len(got) == len(reads) and all(list(a) == b for a, b in zip(got, reads)), "the database does not hold the plants"
        for name, opts in dc.OPTION_SETS.items():
            for blk in ("P.1", "P"):
                r = ref_dust(opts + [blk], tmp)
                if name in dc.ERROR_SETS:
                    assert r.returncode != 0
                    exp["%s/%s.stderr" % (name, blk)] = ("%s\nrc %d\n" % (r.stderr, r.returncode)).encode()
                else:
                    assert r.returncode == 0, r.stderr
            files = dc.dust_files(tmp)
            if name not in dc.ERROR_SETS:
                assert files[".P.dust.anno"] == files[".P.1.dust.anno"] and files[".P.dust.data"] == files[".P.1.dust.data"]
                by_set[name] = dc.track_intervals(files[".P.dust.anno"], files[".P.dust.data"])
            for f, b in files.items():
                exp["%s/%s" % (name, f)] = b
                os.remove(os.path.join(tmp, f))
        check_plants(names, reads, by_set)
        for f in dc.DB_FILES:
            shutil.copy(os.path.join(tmp, f), os.path.join(OUT, f))
        # the error runs
        for name, args in dc.ERROR_RUNS.items():
            r = ref_dust(args, tmp)
            assert r.returncode != 0
            exp["errors/%s" % name] = ("%s\nrc %d\n" % (r.stderr, r.returncode)).encode()
        # append: a database of the first reads, its track, two more reads, the command again
        sub = os.path.join(tmp, "app")
        os.makedirs(sub)
        pick = [names.index(w) for w in ("poly_a_len_%d" % W, "run_over_border", "period_3")]
        make_db(sub, "A", [reads[i] for i in pick])
        assert ref_dust(["A"], sub).returncode == 0
        for f, b in dc.dust_files(sub).items():
            exp["append_before/%s" % f] = b
        write_fasta(os.path.join(sub, "B.fasta"), ["".join("acgt"[x] for x in reads[names.index(w)])
                                                   for w in ("run_at_read_end", "homopolymer")])
        run([os.path.join(REF, "FA2db"), "-x0", "A", "B.fasta"], sub, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        assert ref_dust(["A"], sub).returncode == 0
        for f, b in dc.dust_files(sub).items():
            exp["append_after/%s" % f] = b
        assert exp["append_after/.A.dust.data"].startswith(exp["append_before/.A.dust.data"])
        assert len(exp["append_after/.A.dust.anno"]) == len(exp["append_before/.A.dust.anno"]) + 16
        for f in ("A.db", ".A.idx", ".A.bps"):
            shutil.copy(os.path.join(sub, f), os.path.join(OUT, f))
        # the blocks of the mask_dust database
        sub = os.path.join(tmp, "md")
        os.makedirs(sub)
        dc.planted_workdir(sub, ("G.db", ".G.idx", ".G.bps"), dc.MASK_DUST)
        for blk in ("G.1", "G.2"):
            assert ref_dust([blk], sub).returncode == 0
        for f, b in dc.dust_files(sub).items():
            exp["mask_dust/%s" % f] = b
    np.savez_compressed(os.path.join(OUT, "expected.npz"), **{k: np.frombuffer(v, dtype=np.uint8) for k, v in exp.items()})
    json.dump(dict(piece=P, window=W, minlen=M, longest_candidate_list=longest, reads=names,
                   host_sets=list(dc.HOST_SETS), error_sets=list(dc.ERROR_SETS)),
              open(os.path.join(OUT, "cases.json"), "w"), indent=1)
    for f in os.listdir(OUT):
        assert os.path.getsize(os.path.join(OUT, f)) < MAX_FILE, f
    print("planted reads: %d, longest candidate list: %d, files: %s" % (len(reads), longest, sorted(os.listdir(OUT))))


if __name__ == "__main__":
    main()
