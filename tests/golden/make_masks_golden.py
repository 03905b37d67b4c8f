#!/usr/bin/env python3
"""Fixtures of the mask tools (tests/golden/masks_*/) from the REFERENCE's LArepeat and TANmask.

Runs only where the reference sources lie (REF_SRC, default /root/reference) and oracle/_ref/ is built: the two tools are
compiled with plain gcc lines (source sets of scrub/Makefile.in) into a temporary directory outside the repository, run,
and only data is kept: the trace-less merged .las, the database's stub and index, and expected_*.npz with the inflated
anno / data arrays and the numbers of the tools' stdout.  Nothing compiled is kept.

    python tests/golden/make_masks_golden.py
"""
import hashlib
import json
import os
import random
import re
import shutil
import struct
import subprocess
import sys
import tempfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
REF = os.path.join(ROOT, "oracle", "_ref")
SRC = os.environ.get("REF_SRC", "/root/reference")

FLAGGED = "G.1f.las"        # the merged file with identity overlaps and discarded records planted (flag_records)
REPEAT_CASES = [            # name, options[, .las file]
    ("c", ["-c", "8"]),
    ("est", []),
    ("C", ["-c", "8", "-C"]),
    ("Cm", ["-c", "8", "-C", "-m", "500"]),
    ("m", ["-c", "8", "-m", "500"]),
    ("I", ["-c", "8", "-I"]),
    ("o", ["-c", "8", "-o", "2000"]),
    ("hl", ["-c", "8", "-h", "3", "-l", "1.2"]),
    ("bt", ["-c", "8", "-b", "1", "-t", "rep"]),
    ("c_f", ["-c", "8"], FLAGGED),
    ("I_f", ["-c", "8", "-I"], FLAGGED),
    ("est_f", [], FLAGGED),
]
TAN_CASES = [("tan_tandem", "tan_tandem/las/tan/G.1.G.1.las"), ("tan_k10", "tan_k10/las/tan/G.1.G.1.las")]


def run(cmd, cwd, **kw):
    return subprocess.run(cmd, cwd=cwd, check=True, **kw)


def build_tools(tmp):
    cc = ["gcc", "-O3", "-w", "-fno-strict-aliasing", "-I" + SRC]
    s = lambda *p: os.path.join(SRC, *p)
    run(cc + ["-o", os.path.join(tmp, "LArepeat"), s("scrub", "LArepeat.c"), s("lib", "borders.c"), s("lib", "utils.c"),
              s("lib", "tracks.c"), s("lib", "pass.c"), s("db", "QV.c"), s("dalign", "align.c"), s("db", "DB.c"),
              s("lib", "compression.c"), "-lm", "-lz", "-lpthread"], tmp)
    run(cc + ["-o", os.path.join(tmp, "TANmask"), s("scrub", "TANmask.c"), s("dalign", "align.c"), s("db", "DB.c"),
              s("db", "QV.c"), "-lm", "-lpthread"], tmp)


def inflate(buf):
    out, at = b"", 0
    while at < len(buf):
        n = struct.unpack_from("<Q", buf, at)[0]
        out += zlib.decompress(buf[at + 8:at + 8 + n])
        at += 8 + n
    return out


def read_a2(prefix):
    a = open(prefix + ".a2", "rb").read()
    version, size, _pad, length, clen, cdlen = struct.unpack_from("<HHIQQQ", a, 0)
    anno = np.frombuffer(inflate(a[64:64 + clen]), dtype="<u8")
    data = np.frombuffer(inflate(open(prefix + ".d2", "rb").read()), dtype="<i4")
    return dict(version=version, size=size, len=length, anno=anno, data=data)


def strip_traces(src, dst):
    """the records of a .las without their trace bytes (tlen = 0): all the mask tools read"""
    buf = open(src, "rb").read()
    novl, tspace = struct.unpack_from("<qi", buf, 0)
    out, at = [buf[:12]], 12
    tb = 1 if tspace <= 125 else 2
    for _ in range(novl):
        rec = bytearray(buf[at:at + 40])
        tlen = struct.unpack_from("<i", rec, 0)[0]
        struct.pack_into("<i", rec, 0, 0)
        out.append(bytes(rec))
        at += 40 + tb * tlen
    open(dst, "wb").write(b"".join(out))


def flag_records(src, dst, rng):
    """a trace-less .las with one record in nine marked OVL_DISCARD and, in every fourth pile, two records made identity
    overlaps (bread = aread): a daligner self-comparison writes neither, and -I and both discard filters see nothing without"""
    buf = bytearray(open(src, "rb").read())
    novl = struct.unpack_from("<q", buf, 0)[0]
    last, pile = -1, 0
    for i in range(novl):
        at = 12 + 40 * i
        flags, aread = struct.unpack_from("<Ii", buf, at + 24)
        if aread != last:
            last, pile, left = aread, pile + 1, 2 if pile % 4 == 0 else 0
        if left > 0 and rng.random() < 0.2:
            struct.pack_into("<i", buf, at + 32, aread)
            left -= 1
        elif rng.random() < 1 / 9:
            struct.pack_into("<I", buf, at + 24, flags | 2)
    open(dst, "wb").write(bytes(buf))


def las_piles(path):
    """the one batch of a trace-less .las in the layout tests/masks_model.py reads"""
    buf = open(path, "rb").read()
    novl = struct.unpack_from("<q", buf, 0)[0]
    rec = np.frombuffer(buf, dtype="<i4", count=10 * novl, offset=12).reshape(novl, 10)
    aread = rec[:, 7]
    cut = np.flatnonzero(np.diff(aread)) + 1
    off = np.concatenate([[0], cut, [novl]]).astype(np.int64)
    return dict(pile_off=off, pile_aread=aread[off[:-1]].copy(), abpos=rec[:, 2].copy(), aepos=rec[:, 4].copy(), bbpos=rec[:, 3].copy(),
                bepos=rec[:, 5].copy(), bread=rec[:, 8].copy(), flags=rec[:, 6].copy())


def exercised(piles, read_len, opts, data, width):
    """(start extensions, end extensions, values the first-k-records quirk decides) in the reference's data: against the plain
    sweep of tests/masks_model.py without the edge step, and with the edge step's support counted over the whole pile"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import masks_model
    kw, i = {}, 0
    names = {"-c": ("cov", int), "-h": ("xcov_enter", float), "-l": ("xcov_leave", float), "-m": ("merge_dist", int), "-o": ("min_aln_len", int)}
    while i < len(opts):
        if opts[i] in names:
            kw[names[opts[i]][0]] = names[opts[i]][1](opts[i + 1])
            i += 1
        elif opts[i] == "-C":
            kw["inccov"] = 1
        elif opts[i] == "-I":
            kw["inc_identity"] = 1
        elif opts[i] in ("-b", "-t"):
            i += 1
        i += 1
    full = masks_model.repeats(piles, read_len, **kw)[1]
    assert np.array_equal(full, data), "the model and the reference part ways"
    bare = masks_model.repeats(piles, read_len, edges=False, **kw)[1]
    whole = masks_model.repeats(piles, read_len, first_k=False, **kw)[1]
    assert len(bare) == len(data) == len(whole)
    moved = np.flatnonzero(bare != data)
    count = masks_model.repeats(piles, read_len, edges=False, **kw)[0]
    pos = np.concatenate([np.arange(c) % width for c in count]) if len(count) else np.zeros(0, dtype=int)     # per pile: 0 begin, 1 end
    return int(np.sum(pos[moved] == 0)), int(np.sum(pos[moved] == 1)), int(np.sum(whole != data))


def planted_reads(rng):
    """a 90 kbp genome with seven copies of a 3.2 kbp element, shredded into error-free reads; some reads are cut so that
    a copy of the element is their first or their last kilobase and a half.  Every copy is two halves of the element
    around 300 bases of its own, so each leaves two regions a merge distance of 500 joins."""
    base = lambda n: "".join(rng.choice("acgt") for _ in range(n))
    elem = base(3200)
    genome, copies = "", []
    for _ in range(7):
        genome += base(rng.randint(9000, 12000))
        copies.append(len(genome))
        genome += elem[:1450] + base(300) + elem[1750:]
    genome += base(10000)
    reads = []
    for _ in range(150):
        n = rng.randint(5000, 9000)
        at = rng.randint(0, len(genome) - n)
        reads.append(genome[at:at + n])
    for c in copies[:4]:
        for _ in range(2):
            reads.append(genome[c - rng.randint(300, 700):c + 3200 + rng.randint(4000, 6000)])       # element near the start
            reads.append(genome[c - rng.randint(4000, 6000):c + 3200 + rng.randint(300, 700)])       # ... near the end
    rng.shuffle(reads)
    return reads


def stdout_numbers(text):
    text = re.sub(r"\x1b\[[0-9;]*m", "", text)
    out = {}
    hist = [int(m.group(2)) for m in re.finditer(r"^COV (\d+) READS (-?\d+)$", text, re.M)]
    if hist:
        out["histo"] = np.array(hist, dtype=np.int64)
    for key in ("MAX", "AVG_RLEN", "REGIONS", "MERGED", "BASES_TOTAL", "BASES_REPEAT"):
        m = re.search(r"^%s (-?\d+)" % key, text, re.M)
        if m:
            out[key] = np.int64(m.group(1))
    m = re.search(r"^INACTIVE (-?\d+) \((-?\d+)%\) OF (-?\d+)", text, re.M)
    if m:
        out["INACTIVE"] = np.array([int(m.group(1)), int(m.group(2)), int(m.group(3))], dtype=np.int64)
    return out


def make_repeat(tmp):
    out = os.path.join(HERE, "masks_rep")
    shutil.rmtree(out, ignore_errors=True)
    os.makedirs(out)
    work = os.path.join(tmp, "rep")
    os.makedirs(work)
    reads = planted_reads(random.Random(20240611))
    with open(os.path.join(work, "reads.fasta"), "w") as f:
        for i, s in enumerate(reads):
            f.write(">Sim/%d/0_%d RQ=0.850\n" % (i + 1, len(s)))
            for j in range(0, len(s), 80):
                f.write(s[j:j + 80] + "\n")
    run([os.path.join(REF, "FA2db"), "G", "reads.fasta"], work, stdout=subprocess.DEVNULL)
    run([os.path.join(REF, "DBsplit"), "-s200", "G"], work, stdout=subprocess.DEVNULL)
    run([os.path.join(REF, "daligner"), "-k14", "-j4", "G.1", "G.1"], work, stdout=subprocess.DEVNULL)
    run([os.path.join(REF, "LAmerge"), "-n", "8", "G", "G.1.las", "d001_00001"], work, stdout=subprocess.DEVNULL)
    strip_traces(os.path.join(work, "G.1.las"), os.path.join(out, "G.1.las"))
    shutil.copy(os.path.join(out, "G.1.las"), os.path.join(work, "G.1.las"))
    for f in ("G.db", ".G.idx"):
        shutil.copy(os.path.join(work, f), os.path.join(out, f))
    flag_records(os.path.join(out, "G.1.las"), os.path.join(out, FLAGGED), random.Random(7))
    shutil.copy(os.path.join(out, FLAGGED), os.path.join(work, FLAGGED))
    read_len = np.array([len(s) for s in reads], dtype=np.int32)
    cases, empty, ext_start, ext_end, quirk = [], False, 0, 0, 0
    for name, opts, *rest in REPEAT_CASES:
        las = rest[0] if rest else "G.1.las"
        r = run([os.path.join(tmp, "LArepeat")] + opts + ["G", las], work, stdout=subprocess.PIPE, text=True)
        num = stdout_numbers(r.stdout)
        track = opts[opts.index("-t") + 1] if "-t" in opts else "repeats"
        block = int(opts[opts.index("-b") + 1]) if "-b" in opts else 0
        t = read_a2(os.path.join(work, ".G.%s%s" % ("%d." % block if block else "", track)))
        assert num["REGIONS"] >= 50, (name, num["REGIONS"])
        if "-m" in opts:
            assert num["MERGED"] >= 5, (name, num["MERGED"])
        width = 3 if "-C" in opts else 2
        if "-m" not in opts or "-C" in opts:
            assert int(t["anno"][-1]) == 4 * len(t["data"])
            empty = empty or bool(np.any(np.diff(t["anno"].astype(np.int64)) == 0))
        cov = opts[opts.index("-c") + 1] if "-c" in opts else str(int(num["MAX"]))
        s, e, q = exercised(las_piles(os.path.join(out, las)), read_len, opts if "-c" in opts else opts + ["-c", cov], t["data"], width)
        print("%-6s regions %4d merged %3d  start extensions %d  end extensions %d  decided by the first-k quirk %d"
              % (name, num["REGIONS"], num.get("MERGED", 0), s, e, q))
        ext_start, ext_end, quirk = ext_start + s, ext_end + e, quirk + q
        np.savez_compressed(os.path.join(out, "expected_%s.npz" % name), version=t["version"], size=t["size"], len=t["len"],
                            anno=t["anno"], data=t["data"], width=width, **num)
        cases.append(dict(name=name, opts=opts, track=track, block=block, las=las))
    assert empty, "no read without a region"
    assert ext_start >= 1 and ext_end >= 1, "no region extended to a read's start (%d) or end (%d)" % (ext_start, ext_end)
    assert quirk >= 1, "no value depends on the edge step reading the first k records of the unfiltered pile"
    assert not np.array_equal(np.load(os.path.join(out, "expected_c_f.npz"))["data"], np.load(os.path.join(out, "expected_I_f.npz"))["data"]), \
        "-I changes nothing on the flagged file"
    assert not np.array_equal(np.load(os.path.join(out, "expected_c_f.npz"))["data"], np.load(os.path.join(out, "expected_c.npz"))["data"]), \
        "the discarded records change nothing"
    json.dump(cases, open(os.path.join(out, "cases.json"), "w"), indent=1)


def make_tan(tmp):
    out = os.path.join(HERE, "masks_tan")
    shutil.rmtree(out, ignore_errors=True)
    os.makedirs(out)
    cases = []
    for name, rel in TAN_CASES:
        for whole in (0, 1):
            work = tempfile.mkdtemp(dir=tmp)
            for f in ("G.db", ".G.idx", ".G.bps"):
                shutil.copy(os.path.join(HERE, "tandem", f), os.path.join(work, f))
            las = "G.1.G.1.las" if not whole else "Gall.las"
            shutil.copy(os.path.join(HERE, rel), os.path.join(work, las))
            run([os.path.join(tmp, "TANmask"), "G", las], work)
            pre = os.path.join(work, ".G.tan" if whole else ".G.1.tan")
            anno = np.fromfile(pre + ".anno", dtype=np.uint8)
            data = np.fromfile(pre + ".data", dtype=np.uint8)
            assert len(data) // 8 >= 20, (name, len(data) // 8)
            # -l does not reach the reference's sweep: the same bytes whatever it is given
            for l in ("-l500", "-l50000"):
                run([os.path.join(tmp, "TANmask"), l, "-mtl", "G", las], work)
                assert open(pre.replace(".tan", ".tl") + ".data", "rb").read() == data.tobytes(), "TANmask -l changes the mask"
            np.savez_compressed(os.path.join(out, "expected_%s_%s.npz" % (name, "whole" if whole else "block")), anno=anno, data=data)
            cases.append(dict(name="%s_%s" % (name, "whole" if whole else "block"), db="tandem", las=rel, whole=whole))
    json.dump(cases, open(os.path.join(out, "cases.json"), "w"), indent=1)


def make_chain(tmp):
    """reference datander -> reference TANmask -> reference daligner -mtan on the `tandem` database: md5s only"""
    work = os.path.join(tmp, "chain")
    os.makedirs(work)
    for f in ("G.db", ".G.idx", ".G.bps"):
        shutil.copy(os.path.join(HERE, "tandem", f), os.path.join(work, f))
    run([os.path.join(REF, "datander"), "-j4", "G.1"], work, stdout=subprocess.DEVNULL)
    run([os.path.join(tmp, "TANmask"), "G", "tan/G.1.G.1.las"], work)
    run([os.path.join(REF, "daligner"), "-k14", "-j4", "-mtan", "G.1", "G.1"], work, stdout=subprocess.DEVNULL)
    md5 = lambda p: hashlib.md5(open(os.path.join(work, p), "rb").read()).hexdigest()
    with open(os.path.join(HERE, "masks_tan", "chain_md5.txt"), "w") as f:
        for p in (".G.1.tan.anno", ".G.1.tan.data", "d001_00001/G.1.G.1.las"):
            f.write("%s %s\n" % (md5(p), p))


def main():
    tmp = tempfile.mkdtemp(prefix="masks_golden_")
    try:
        build_tools(tmp)
        make_repeat(tmp)
        make_tan(tmp)
        make_chain(tmp)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
