#!/usr/bin/env python3
"""Regenerates tests/golden/ from the REAL reference (oracle/_ref, compiled from
/root/reference by oracle/Makefile.ref).  Run in the build container only:

    python tests/golden/make_golden.py

Fixtures are data: small read databases (.db/.idx/.bps written by damar_amd/bin/simdb, or
by the reference's own FA2db/DBsplit for the derived-read cases) and the .las files the
reference daligner produced from them.  No reference source is stored here.

config2_ref_md5.txt is different: md5 of the 16 .las files the reference daligner -j16
wrote for BASELINE config 2 (`simdb . SIM 27 -c20 -r2 -e.15 -S135`, full HPCdaligner plan)
on the MI355X box's host (scripts/gpu_c2_parity.sh).

`make_golden.py memlimit` prints the known answer of the memory-limit case (filter.c:2634-2699
under -M1): `simdb . R 0.1 -c250 -r5 -e.15 -S200 ; daligner -v -k14 -M1 -j8 R R` with the real
reference -> caps 210 / 184, hit counts 16,418,362 / 13,604,118, R.las 164343834 bytes, md5
759225b7cbbae785076eec906a56859f (tests/test_gpu_parity.py::test_gpu_cli_memory_limit_known_answer).
"""
import os
import random
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
REF = os.path.join(ROOT, "oracle", "_ref")
SIMDB = os.path.join(ROOT, "damar_amd", "bin", "simdb")

# name -> (how to make the DB, daligner options, plan lines)
CASES = {
    "tiny2":   dict(sim=["0.1", "-c12", "-r11", "-e.15", "-S1"], opts=["-k14", "-j4"], plan="all"),
    # reads of 60-160 kb: several 50 kb A-panels per read pair (filter.c:2251), long waves
    "long":    dict(sim=["0.4", "-c6", "-r41", "-e.15", "-m110000", "-s25000", "-x60000", "-S200"], opts=["-k14", "-j4"],
                    plan=[("1", ["1"])]),
    "tiny_j1": dict(db="tiny2", opts=["-k14", "-j1"], plan=[("1", ["1"])]),
    "tiny_s":  dict(db="tiny2", opts=["-k14", "-j4", "-s126", "-l800", "-e.75"], plan=[("2", ["2", "1"])]),
    "tiny_t":  dict(db="tiny2", opts=["-k14", "-j2", "-t12"], plan=[("1", ["1"])]),
    "tiny_I":  dict(db="tiny2", opts=["-k14", "-j4", "-I"], plan=[("1", ["1"])]),
    "tiny_A":  dict(db="tiny2", opts=["-k14", "-j4", "-A"], plan=[("2", ["2", "1"])]),
    "tiny_k12": dict(db="tiny2", opts=["-k12", "-w5", "-h30", "-j4"], plan=[("1", ["1"])]),
    # -O (only identity overlaps survive Write_Overlap_Buffer, align.c:6172-6200; needs -I and reads that
    # overlap themselves off the main diagonal -- the tandem-array reads -- to produce any)
    # and -T (no trace points stored, align.c:5989, 6040, 6086)
    "tan_O":   dict(db="tandem", opts=["-k14", "-j4", "-I", "-O"], plan=[("1", ["1"])]),
    "tiny_T":  dict(db="tiny2", opts=["-k14", "-j4", "-T"], plan=[("2", ["2", "1"])]),
    "indel":   dict(derive="indel", opts=["-k14", "-j4"], plan=[("1", ["1"])]),
    "noisy":   dict(derive="noisy", opts=["-k14", "-j4"], plan=[("1", ["1"])]),
    "tandem":  dict(derive="tandem", opts=["-k14", "-j4"], plan=[("1", ["1"])]),
    "tandem2": dict(derive="tandem2", opts=["-k14", "-j4"], plan=[("1", ["1"])], md5_only=True),      # (a 9.9 MB .las)
    "wide":    dict(derive="wide2m", opts=["-k14", "-j1"], plan=[("1", ["1"])], md5_only=True),       # (reads of 2.1 Mb)
    "fusion":  dict(derive="fusion32", opts=["-k14", "-j4"], plan=[("1", ["1"])]),
    "fusion2": dict(derive="fusion31", opts=["-k14", "-j4"], plan=[("1", ["1"])]),
    # mask tracks (-m): a DBdust track made by the reference's own DBdust on reads with
    # low-complexity inserts, and a second, synthetic interval track (so that the merge of
    # daligner.c:263-439 and the per-block slicing of the track files are exercised)
    "mask_dust": dict(derive="lowcomp", tracks=["dust"], opts=["-k14", "-j4", "-mdust"], plan="all"),
    "mask_two":  dict(db="mask_dust", tracks=["dust", "rnd"], opts=["-k14", "-j4", "-mdust", "-mrnd"], plan="all"),
    # the same two tracks, the second one stored in lib/tracks.c's compressed .a2/.d2 form
    "mask_a2":   dict(db="mask_dust", tracks=["dust", "rz"], opts=["-k14", "-j4", "-mdust", "-mrz"], plan="all"),
    # -b (biased k-mers, filter.c:549-688) on reads of skewed base composition, plain and masked
    "bias":      dict(sim=["0.1", "-c12", "-r51", "-e.15", "-b.3", "-S1"], opts=["-k14", "-j4", "-b"], plan="all"),
    "bias_mask": dict(db="mask_dust", tracks=["dust", "rnd"], opts=["-k14", "-j4", "-b", "-mdust", "-mrnd"], plan="all"),
    # the production parameterisation of the reference's scripts
    "prod":      dict(db="mask_dust", tracks=["dust", "rnd"],
                      opts=["-k14", "-e0.7", "-l700", "-I", "-mdust", "-mrnd", "-j4", "-r2"], plan="all"),
    # datander (scrub/datander.c) on the tandem-array reads and on plain reads (0 records)
    "tan_tandem": dict(db="tandem", tool="datander", opts=["-j4"], plan=[("1", [])]),
    "tan_k10":    dict(db="tandem", tool="datander", opts=["-k10", "-w3", "-h28", "-l400", "-j2"], plan=[("1", [])]),
    "tan_plain":  dict(db="tiny2", tool="datander", opts=["-j4"], plan=[("1", []), ("2", [])]),
    # a read of 2.1 Mb with tandem arrays (21 000 trace spacings at -s100: beyond the packed pebbles of the GPU kernels, the
    # wide kernel's work behind datander) beside an ordinary read with one array
    "tan_wide":   dict(derive="tanwide", tool="datander", opts=["-j4"], plan=[("1", [])], md5_only=True),
    # k > 16: 64-bit k-mer codes (scrub/tandem.c:132-149)
    "tan_k18":    dict(db="tandem", tool="datander", opts=["-k18", "-w4", "-h40", "-l400", "-j2"], plan=[("1", [])]),
}


def run(cmd, cwd, **kw):
    subprocess.run(cmd, cwd=cwd, check=True, **kw)


def unpack_reads(dbdir, root):
    import numpy as np
    idx = np.fromfile(os.path.join(dbdir, ".%s.idx" % root), dtype=np.uint8)
    nreads = int(np.frombuffer(idx[:4].tobytes(), dtype="<i4")[0])
    recs = idx[88:88 + 32 * nreads].reshape(nreads, 32)
    bps = np.fromfile(os.path.join(dbdir, ".%s.bps" % root), dtype=np.uint8)
    reads = []
    for r in recs:
        rlen = int(np.frombuffer(r[0:4].tobytes(), dtype="<i4")[0])
        boff = int(np.frombuffer(r[8:16].tobytes(), dtype="<i8")[0])
        b = bps[boff:boff + (rlen + 3) // 4]
        s = np.stack([(b >> 6) & 3, (b >> 4) & 3, (b >> 2) & 3, b & 3], axis=1).reshape(-1)[:rlen]
        reads.append("".join("acgt"[x] for x in s))
    return reads


def write_fasta(path, reads):
    with open(path, "w") as f:
        for i, s in enumerate(reads):
            f.write(">Sim/%d/0_%d RQ=0.850\n" % (i + 1, len(s)))
            for j in range(0, len(s), 80):
                f.write(s[j:j + 80] + "\n")


def rnd_seq(rng, n):
    return "".join(rng.choice("acgt") for _ in range(n))


def derive(kind, work):
    """SURVEY.md App. E recipes; every derived DB goes through the reference's own FA2db."""
    rng = random.Random(12345)
    base = os.path.join(work, "base")
    os.makedirs(base)
    if kind in ("tandem", "tandem2"):
        # tandem2: the genome of SURVEY App. E at its full size (13 spacers of 25 kb, 12 arrays, 20x): the reference
        # bridged 456 + 372 times on its like; "tandem" is the small version (6 arrays, 14x)
        big = kind == "tandem2"
        if big:
            rng = random.Random(424242)
        units = [40, 75, 120, 200, 350]
        genome = ""
        for i in range(12 if big else 6):
            genome += rnd_seq(rng, 25000 if big else 12000)
            u = rnd_seq(rng, units[i % 5])
            for c in range(rng.choice([8, 12, 20, 30] if big else [8, 12, 20])):
                genome += "".join(ch if rng.random() > .03 else rng.choice("acgt") for ch in u)
        genome += rnd_seq(rng, 25000 if big else 12000)
        reads = []
        tot = 0
        comp = {"a": "t", "c": "g", "g": "c", "t": "a"}
        while tot < (20 if big else 14) * len(genome):
            ln = max(4000, int(rng.gauss(10000, 2000))) if big else max(3000, int(rng.gauss(7000, 1500)))
            ln = min(ln, len(genome))
            st = rng.randrange(0, len(genome) - ln + 1)
            out = []
            for ch in genome[st:st + ln]:
                x = rng.random()
                if x < .03:
                    continue
                if x < .08:
                    ch = rng.choice("acgt")
                out.append(ch)
                if rng.random() < .07:
                    out.append(rng.choice("acgt"))
            s = "".join(out)
            if rng.random() < .5:
                s = "".join(comp[ch] for ch in reversed(s))
            reads.append(s)
            tot += len(s)
    elif kind == "wide2m":
        # two reads of 2.1 Mb that overlap by 1.6 Mb (one on the other strand), a 30 kb read inside the overlap and a
        # second one beside it: at -s100 the long reads have 21 000 trace spacings (the packed pebbles of the GPU kernels hold
        # 16 000) and their alignment drops far more than 2^18 pebbles -- the pairs with a long read are the wide kernel's
        # (kernels/report.hip report_wide_kernel), the pair of the two short reads the two-pair kernel's
        rng = random.Random(777)
        genome = rnd_seq(rng, 2600000)
        comp = {"a": "t", "c": "g", "g": "c", "t": "a"}

        def noisy(seq):
            out = []
            for ch in seq:
                x = rng.random()
                if x < .03:
                    continue
                if x < .04:
                    ch = rng.choice("acgt")
                out.append(ch)
                if rng.random() < .11:
                    out.append(rng.choice("acgt"))
            return "".join(out)
        reads = [noisy(genome[0:2100000]),
                 "".join(comp[ch] for ch in reversed(noisy(genome[500000:2600000]))),
                 noisy(genome[1000000:1030000]),
                 noisy(genome[1010000:1040000])]
    elif kind == "tanwide":
        # one read of 2.1 Mb: ten stretches of 200 kb, each followed by a tandem array (unit 40 ... 350 bp, 8 ... 30 copies,
        # 3 % divergence per copy), and a read of 42 kb with one array: datander's self-alignments lie on the long read,
        # whose trace grid the packed chain heads of the GPU kernels cannot index
        rng = random.Random(888)
        units = [40, 75, 120, 200, 350]

        def array(i):
            u = rnd_seq(rng, units[i % 5])
            return "".join("".join(ch if rng.random() > .03 else rng.choice("acgt") for ch in u)
                           for _ in range(rng.choice([8, 12, 20, 30])))

        def noisy(seq):
            out = []
            for ch in seq:
                x = rng.random()
                if x < .03:
                    continue
                if x < .04:
                    ch = rng.choice("acgt")
                out.append(ch)
                if rng.random() < .11:
                    out.append(rng.choice("acgt"))
            return "".join(out)
        genome = ""
        for i in range(10):
            genome += rnd_seq(rng, 200000) + array(i)
        genome += rnd_seq(rng, 60000)
        reads = [noisy(genome), noisy(rnd_seq(rng, 30000) + array(2) + rnd_seq(rng, 10000))]
    elif kind == "lowcomp":
        # homopolymer and short-period stretches dropped into ordinary simulated reads: what
        # DBdust masks, and what floods the seed filter with chance k-mer hits when unmasked
        run([SIMDB, base, "B", "0.1", "-c14", "-r31", "-e.15", "-S200"], ROOT, stdout=subprocess.DEVNULL)
        reads = unpack_reads(base, "B")
        out = []
        for i, s in enumerate(reads):
            for _ in range(rng.choice([1, 2, 3])):
                p = rng.randrange(200, len(s) - 200)
                unit = rng.choice(["a", "t", "c", "g", "at", "ac", "gt", "ag", "aat", "ggc"])
                ln = rng.randrange(25, 140)
                ins = (unit * (ln // len(unit) + 1))[:ln]
                ins = "".join(ch if rng.random() > .02 else rng.choice("acgt") for ch in ins)
                s = s[:p] + ins + s[p:]
            out.append(s)
        reads = out
    elif kind.startswith("fusion"):
        # 300-800 bp windows with 25-45 % substitutions in every other read: the alignment
        # breaks inside the window and the two pieces share a trace point -> Fusion
        seed = int(kind[6:])
        rng = random.Random(seed)
        run([SIMDB, base, "B", "0.15", "-c20", "-r%d" % seed, "-e.15", "-S200"], ROOT, stdout=subprocess.DEVNULL)
        reads = unpack_reads(base, "B")
        out = []
        for i, s in enumerate(reads):
            if i % 2 == 0:
                w = rng.randrange(300, 800)
                p = rng.randrange(500, max(501, len(s) - w - 500))
                rate = rng.uniform(.25, .45)
                seg = "".join(ch if rng.random() > rate else rng.choice("acgt") for ch in s[p:p + w])
                s = s[:p] + seg + s[p + w:]
            out.append(s)
        reads = out
    else:
        run([SIMDB, base, "B", "0.06", "-c14", "-r21", "-e.15", "-S200"], ROOT, stdout=subprocess.DEVNULL)
        reads = unpack_reads(base, "B")
        out = []
        for i, s in enumerate(reads):
            mid = len(s) // 2
            if kind == "indel":
                if i % 3 == 0:
                    s = s[:mid] + rnd_seq(rng, rng.choice([60, 150, 400])) + s[mid:]
                elif i % 3 == 1:
                    s = s[:mid] + s[mid + rng.choice([80, 200]):]
            else:
                if i % 2 == 0:
                    w = rng.randrange(200, 1500)
                    p = rng.randrange(500, max(501, len(s) - w - 500))
                    rate = rng.uniform(.35, .75)
                    seg = "".join(ch if rng.random() > rate else rng.choice("acgt") for ch in s[p:p + w])
                    if i % 4 == 0:
                        q = len(seg) // 2
                        seg = seg[:q] + rnd_seq(rng, rng.randrange(8, 40)) + seg[q:]
                    s = s[:p] + seg + s[p + w:]
            out.append(s)
        reads = out
    dbdir = os.path.join(work, "db")
    os.makedirs(dbdir)
    write_fasta(os.path.join(dbdir, "reads.fasta"), reads)
    run([os.path.join(REF, "FA2db"), "G", "reads.fasta"], dbdir, stdout=subprocess.DEVNULL)
    run([os.path.join(REF, "DBsplit"), "-s1" if kind == "lowcomp" else "-s200", "G"], dbdir, stdout=subprocess.DEVNULL)
    return dbdir, "G"


def read_lengths(dbdir, root):
    import numpy as np
    idx = np.fromfile(os.path.join(dbdir, ".%s.idx" % root), dtype=np.uint8)
    nreads = int(np.frombuffer(idx[:4].tobytes(), dtype="<i4")[0])
    recs = idx[88:88 + 32 * nreads].reshape(nreads, 32)
    return [int(np.frombuffer(r[0:4].tobytes(), dtype="<i4")[0]) for r in recs]


def make_tracks(dbdir, root, tracks):
    """Interval tracks in the DAZZ_DB layout (db/DB.c:1113 Load_Track): .anno = int tracklen,
    int size(8), int64 byte offsets[tracklen+1]; .data = int pairs [beg,end)."""
    import struct
    import zlib
    for t in tracks:
        if t == "dust":
            run([os.path.join(REF, "DBdust"), root], dbdir, stdout=subprocess.DEVNULL)
        elif t == "rz":
            # the intervals of "rnd" in the compressed form: header {u16 version=2, u16 size=8, u32 pad,
            # u64 len, clen, cdlen, 4 x u64 reserved}, payloads = {u64 n, n bytes of zlib stream}*
            if not os.path.exists(os.path.join(dbdir, ".%s.rnd.anno" % root)):
                make_tracks(dbdir, root, ["rnd"])
            a = open(os.path.join(dbdir, ".%s.rnd.anno" % root), "rb").read()
            d = open(os.path.join(dbdir, ".%s.rnd.data" % root), "rb").read()
            n = struct.unpack("<i", a[:4])[0]
            anno = a[8:]

            def chunks(buf, step=8 * 1024 * 1024):
                out = b""
                for i in range(0, len(buf), step):
                    z = zlib.compress(buf[i:i + step])
                    out += struct.pack("<Q", len(z)) + z
                return out
            ca, cd = chunks(anno), chunks(d)
            with open(os.path.join(dbdir, ".%s.rz.a2" % root), "wb") as f:
                f.write(struct.pack("<HHIQQQQQQQ", 2, 8, 0, n, len(ca), len(cd), 0, 0, 0, 0))
                f.write(ca)
            with open(os.path.join(dbdir, ".%s.rz.d2" % root), "wb") as f:
                f.write(cd)
        else:
            rng = random.Random(77)
            lens = read_lengths(dbdir, root)
            offs, data = [0], []
            for ln in lens:
                pts = sorted(rng.sample(range(0, ln), 2 * rng.choice([0, 1, 1, 2, 3])))
                for b, e in zip(pts[0::2], pts[1::2]):
                    e = min(ln, b + min(e - b, 400) + 1)
                    data += [b, e]
                # keep them disjoint and sorted as a real track is
                clean = []
                for b, e in zip(data[offs[-1] // 4::2], data[offs[-1] // 4 + 1::2]):
                    if clean and b <= clean[-1][1]:
                        clean[-1][1] = max(clean[-1][1], e)
                    else:
                        clean.append([b, e])
                data = data[:offs[-1] // 4] + [x for iv in clean for x in iv]
                offs.append(4 * len(data))
            with open(os.path.join(dbdir, ".%s.%s.anno" % (root, t)), "wb") as f:
                f.write(struct.pack("<ii", len(lens), 8))
                f.write(struct.pack("<%dq" % len(offs), *offs))
            with open(os.path.join(dbdir, ".%s.%s.data" % (root, t)), "wb") as f:
                f.write(struct.pack("<%di" % len(data), *data))


def memlimit():
    import hashlib
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        run([SIMDB, d, "R", "0.1", "-c250", "-r5", "-e.15", "-S200"], d, stdout=subprocess.DEVNULL)
        out = subprocess.run([os.path.join(REF, "daligner"), "-v", "-k14", "-M1", "-j8", "R", "R"], cwd=d, check=True,
                             stdout=subprocess.PIPE, text=True).stdout
        for ln in out.splitlines():
            if "Capping" in ln or "Hit count" in ln:
                print(ln.strip())
        las = os.path.join(d, "R.las")
        print(os.path.getsize(las), hashlib.md5(open(las, "rb").read()).hexdigest())


def fa2db_md5():
    """The reference's FA2db + DBsplit on the FASTA files of tests/test_host.py::fasta_inputs ->
    fa2db_ref_md5.txt (md5 per database file; of the .idx only the fields the reference defines)."""
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_host
    with tempfile.TemporaryDirectory() as d:
        files = test_host.fasta_inputs(d)
        run([os.path.join(REF, "FA2db"), "-x1000", "T"] + files, d, stderr=subprocess.DEVNULL)
        run([os.path.join(REF, "DBsplit"), "-s1", "T"], d)
        dig = test_host.db_digest(d)
    with open(os.path.join(HERE, "fa2db_ref_md5.txt"), "w") as f:
        for name, md5 in sorted(dig.items()):
            f.write("%s %s\n" % (md5, name))
    print(dig)
    with tempfile.TemporaryDirectory() as d:          # adding to an existing database, then -a
        test_host.fasta_inputs(d)
        dig = test_host.append_sequence(REF, d)
    with open(os.path.join(HERE, "fa2db_append_ref_md5.txt"), "w") as f:
        for name, md5 in sorted(dig.items()):
            f.write("%s %s\n" % (md5, name))
    print(dig)
    with tempfile.TemporaryDirectory() as d:          # -b
        files = test_host.fasta_inputs(d)
        run([os.path.join(REF, "FA2db"), "-x1000", "-b", "T"] + files, d, stderr=subprocess.DEVNULL)
        dig = test_host.db_digest(d)
    with open(os.path.join(HERE, "fa2db_best_ref_md5.txt"), "w") as f:
        for name, md5 in sorted(dig.items()):
            f.write("%s %s\n" % (md5, name))
    print(dig)
    with tempfile.TemporaryDirectory() as d:          # -c / -Q: header arguments as tracks, FullHqRead filter
        dig = test_host.header_track_digests(REF, d)
    with open(os.path.join(HERE, "fa2db_tracks_ref_md5.txt"), "w") as f:
        for name, md5 in sorted(dig.items()):
            f.write("%s %s\n" % (md5, name))
    print(dig)


def trace_md5():
    """md5 of the dumps the REAL Compute_Trace_PTS leaves for every golden .las (oracle/ref_lastrace.c
    around align.c:5577, all three modes) -> trace_ref_md5.txt, the fixture that pins oracle/trace.c."""
    import hashlib
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import conftest
    with tempfile.TemporaryDirectory() as d:
        # the same for Compute_Trace_MID (align.c:5694, as corrector/LAcorrect.c:545 calls it) -> trace_mid_ref_md5.txt
        for fixture, extra in (("trace_ref_md5.txt", []), ("trace_mid_ref_md5.txt", ["mid"])):
            lines = []
            for name in conftest.golden_cases():
                c = conftest.read_case(name)
                for las in c["las"]:
                    for mode in (0, -1, 1):
                        out = os.path.join(d, "t.bin")
                        run([os.path.join(REF, "ref_lastrace"), os.path.join(c["dbdir"], "G"),
                             os.path.join(c["lasdir"], las), out, str(mode)] + extra, d)
                        lines.append("%s %s %s %d" % (hashlib.md5(open(out, "rb").read()).hexdigest(), name, las, mode))
            with open(os.path.join(HERE, fixture), "w") as f:
                f.write("\n".join(lines) + "\n")
            print("%s: %d dumps" % (fixture, len(lines)))


def simulator_md5():
    """The reference's simulator | FA2db ; DBsplit of tests/test_host.py::test_simdb_equals_simulator_fa2db_dbsplit ->
    simulator_ref_md5.txt (md5 per database file; of the .idx only the fields the reference defines)."""
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_host
    with tempfile.TemporaryDirectory() as d:
        dig = test_host.simulator_ref_digest(REF, d)
    with open(os.path.join(HERE, "simulator_ref_md5.txt"), "w") as f:
        for name, md5 in sorted(dig.items()):
            f.write("%s %s\n" % (md5, name))
    print(dig)


def random_md5():
    """md5 of the .las files the reference daligner writes for the 32 seeded option combinations of
    tests/test_oracle_golden.py::test_oracle_random_option_combinations_equal_reference -> random_ref_md5.txt"""
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import conftest
    import test_oracle_golden
    lines = []
    with tempfile.TemporaryDirectory() as d:
        for n, gold, opts, blocks in test_oracle_golden.random_option_cases():
            w = os.path.join(d, "r%d" % n)
            conftest.link_db(os.path.join(HERE, gold), w)
            run([os.path.join(REF, "daligner")] + opts + blocks, w, stdout=subprocess.DEVNULL)
            lines += ["%s %d %s" % (m, n, rel) for rel, m in sorted(test_oracle_golden.las_md5s(w).items())]
    with open(os.path.join(HERE, "random_ref_md5.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("random_ref_md5.txt: %d files" % len(lines))


# BASELINE config 4 (`simulator 248 -c80 -m15000 -s3000 -e.15 -r4`, DBsplit -s78 -> 256 blocks) is too
# large to run whole anywhere but on an 8-GPU node; parity is checked on seeded random samples of its
# block pairs.  "lead": pairs among the first C4_LEAD blocks, which `simdb -N<C4_LEAD>` reproduces
# without generating the other 18 Gbp (the generator is sequential, so they are the same blocks);
# "full": pairs from the whole 256 x 256 triangle (needs the whole DB: ~2.5 min of simdb).
C4_SIM = ["248", "-c80", "-m15000", "-s3000", "-e.15", "-r4", "-S78"]
C4_LEAD = 24


def c4_samples(nblocks=256):
    rng = random.Random(4)
    lead, full = [], []
    while len(lead) < 8:
        a, b = rng.randint(1, C4_LEAD), rng.randint(1, C4_LEAD)
        p = (max(a, b), min(a, b))
        if p not in lead and (len(lead) >= 2 or a == b):          # the first two are self pairs
            lead.append(p)
    while len(full) < 8:
        a, b = rng.randint(1, nblocks), rng.randint(1, nblocks)
        p = (max(a, b), min(a, b))
        if p not in full and (len(full) >= 2 or a == b):
            full.append(p)
    return lead, full


def big_md5(dbdir=None):
    """config4_ref_md5.txt and config5_ref_md5.txt: md5 of what the REAL reference writes for the sampled
    block pairs of config 4 and for datander on config-2-scale blocks (plain and with tandem arrays
    implanted by `simdb -T.3`).  `python make_golden.py big [<dir holding the full config-4 DB>]`."""
    import hashlib
    import tempfile

    def md5(path):
        return hashlib.md5(open(path, "rb").read()).hexdigest()

    with tempfile.TemporaryDirectory(dir="/dev/shm") as d:
        if dbdir is None:
            dbdir = d
            run([SIMDB, d, "SIM"] + C4_SIM, d, stdout=subprocess.DEVNULL)
        nblocks = int(open(os.path.join(dbdir, "SIM.db")).read().split("blocks =")[1].split()[0])
        lead, full = c4_samples(nblocks)
        rdir = os.path.join(d, "run")
        os.makedirs(rdir)
        for f in ("SIM.db", ".SIM.idx", ".SIM.bps"):
            os.symlink(os.path.join(dbdir, f), os.path.join(rdir, f))
        lines = ["# config 4: simdb . SIM %s -> %d blocks; reference daligner -k14 -j8 SIM.<a> SIM.<b>" % (" ".join(C4_SIM), nblocks),
                 "# <md5> <sample> <a> <b> <file>"]
        for tag, pairs in (("lead", lead), ("full", full)):
            for a, b in pairs:
                shutil.rmtree(os.path.join(rdir, "d001_%05d" % a), ignore_errors=True)
                shutil.rmtree(os.path.join(rdir, "d001_%05d" % b), ignore_errors=True)
                run([os.path.join(REF, "daligner"), "-k14", "-j8", "SIM.%d" % a, "SIM.%d" % b], rdir, stdout=subprocess.DEVNULL)
                for x, y in ((a, b), (b, a)) if a != b else ((a, b),):
                    rel = "d001_%05d/SIM.%d.SIM.%d.las" % (x, x, y)
                    lines.append("%s %s %d %d %s" % (md5(os.path.join(rdir, rel)), tag, a, b, rel))
                print(tag, a, b, flush=True)
        with open(os.path.join(HERE, "config4_ref_md5.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    config5_md5()


def config5_md5():
    """config5_ref_md5.txt alone: `python make_golden.py c5` (every block of the config-2 DB, plain and with tandem arrays)."""
    import hashlib
    import tempfile

    def md5(path):
        return hashlib.md5(open(path, "rb").read()).hexdigest()

    with tempfile.TemporaryDirectory(dir="/dev/shm") as d:
        lines = ["# config 5: reference datander -j8 SIM.<block> on the config-2 DB (simdb . SIM 27 -c20 -r2 -e.15 -S135),",
                 "# plain and with tandem arrays implanted into 30 % of the reads (simdb ... -T.3)",
                 "# <md5> <variant> <block> <records>"]
        for tag, extra in (("plain", []), ("tandem", ["-T.3"])):
            w = os.path.join(d, tag)
            os.makedirs(w)
            run([SIMDB, w, "SIM", "27", "-c20", "-r2", "-e.15", "-S135"] + extra, w, stdout=subprocess.DEVNULL)
            for blk in (1, 2, 3, 4):
                run([os.path.join(REF, "datander"), "-j8", "SIM.%d" % blk], w, stdout=subprocess.DEVNULL)
                las = os.path.join(w, "tan", "SIM.%d.SIM.%d.las" % (blk, blk))
                import struct
                novl = struct.unpack("<q", open(las, "rb").read(8))[0]
                lines.append("%s %s %d %d" % (md5(las), tag, blk, novl))
                print(tag, blk, novl, flush=True)
        with open(os.path.join(HERE, "config5_ref_md5.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    if not os.path.exists(os.path.join(REF, "daligner")):
        sys.exit("oracle/_ref/daligner missing: make -C oracle -f Makefile.ref")
    if sys.argv[1:2] == ["big"]:
        return big_md5(sys.argv[2] if len(sys.argv) > 2 else None)
    if sys.argv[1:] == ["c5"]:
        return config5_md5()
    if sys.argv[1:] == ["memlimit"]:
        return memlimit()
    if sys.argv[1:] == ["trace"]:
        return trace_md5()
    if sys.argv[1:] == ["fa2db"]:
        return fa2db_md5()
    if sys.argv[1:] == ["simulator"]:
        return simulator_md5()
    if sys.argv[1:] == ["random"]:
        return random_md5()
    import tempfile
    dbs = {}
    only = set(sys.argv[1:])
    for name, c in CASES.items():
        if only and name not in only:
            if "sim" in c:
                dbs[name] = os.path.join(HERE, name)
            continue
        out = os.path.join(HERE, name)
        shutil.rmtree(out, ignore_errors=True)
        os.makedirs(out)
        with tempfile.TemporaryDirectory() as work:
            if "sim" in c:
                run([SIMDB, out, "G"] + c["sim"], ROOT, stdout=subprocess.DEVNULL)
                dbs[name] = out
                dbdir, root = out, "G"
            elif "derive" in c:
                dbdir, root = derive(c["derive"], work)
                for f in ("G.db", ".G.idx", ".G.bps"):
                    shutil.copy(os.path.join(dbdir, f), os.path.join(out, f))
                dbdir = out
            else:
                dbdir, root = os.path.join(HERE, c["db"]), "G"
            tfiles = []
            for t in c.get("tracks", []):
                ext = (".a2", ".d2") if t == "rz" else (".anno", ".data")
                if not os.path.exists(os.path.join(dbdir, ".G.%s%s" % (t, ext[0]))):
                    make_tracks(dbdir, "G", [t])
                tfiles += [".G.%s%s" % (t, e) for e in ext]
            nblocks = int(open(os.path.join(dbdir, "G.db")).read().split("blocks =")[1].split()[0])
            plan = c["plan"]
            if plan == "all":
                plan = [(str(a), [str(b) for b in range(a, 0, -1)]) for a in range(1, nblocks + 1)]
            rdir = os.path.join(work, "run")
            os.makedirs(rdir)
            for f in ["G.db", ".G.idx", ".G.bps"] + tfiles:
                os.symlink(os.path.join(dbdir, f), os.path.join(rdir, f))
            for a, bs in plan:
                if c.get("tool") == "datander":
                    run([os.path.join(REF, "datander")] + c["opts"] + ["G." + a], rdir, stdout=subprocess.DEVNULL)
                else:
                    run([os.path.join(REF, "daligner")] + c["opts"] + ["G." + a] + ["G." + b for b in bs], rdir,
                        stdout=subprocess.DEVNULL)
            n = 0
            for dp, _, fs in os.walk(rdir):
                for f in fs:
                    if f.endswith(".las"):
                        rel = os.path.relpath(os.path.join(dp, f), rdir)
                        if c.get("md5_only"):
                            import hashlib
                            with open(os.path.join(out, "las.md5"), "a") as g:
                                g.write("%s %s\n" % (hashlib.md5(open(os.path.join(dp, f), "rb").read()).hexdigest(), rel))
                        else:
                            os.makedirs(os.path.join(out, "las", os.path.dirname(rel)), exist_ok=True)
                            shutil.copy(os.path.join(dp, f), os.path.join(out, "las", rel))
                        n += 1
            with open(os.path.join(out, "case.txt"), "w") as f:
                f.write("db %s\nopts %s\ntool %s\n" % (c.get("db", name), " ".join(c["opts"]), c.get("tool", "daligner")))
                for a, bs in plan:
                    f.write("line %s %s\n" % (a, " ".join(bs)))
            print(name, "->", n, ".las files")


if __name__ == "__main__":
    main()
