"""What tests/test_filter_host.py, tests/test_gpu_filter.py and tests/golden/make_filter_golden.py share: the option sets of
the LAfilter fixtures (tests/golden/filter/), the working directory of a case, and how a command's output is compared with
the fixtures."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np

import q_common
import trim_common as tc

ROOT = q_common.ROOT
GOLDEN = q_common.GOLDEN
FDIR = os.path.join(GOLDEN, "filter")
BIN = q_common.BIN
LAS = tc.LAS
OUT = tc.OUT
TW = 100
MAXGROUP = 64                           # DAMAR_FILTER_MAXGROUP, what the planted runs are sized by

INPUTS = dict(q_common.INPUTS, fsynth=("tiny2", "filter/synth.las"))
TRIM_OF = dict(tiny2="def_tiny2", tandem="def_tandem", fusion="def_fusion", long="def_long", tiny_s="def_tiny_s")
REAL = ("tiny2", "fusion", "tandem", "long", "tiny_s")
BIG = "fusion"                          # the largest real fixture file
A_FILE = "discarded.txt"                # what a case's -a file is called
STDOUT_KEPT = 1 << 12                   # a longer stdout is kept as its md5
FIXED, LOOSE = [2, 3, 7, 8, 9], [0, 1, 4, 5, 6]      # the words of a record LAfilter leaves without -T, and those it may change


def variants(d, n, o):
    """the option sets run on every input; d, n, o: the plan's thresholds as the generator picked them"""
    plan = ["-d", str(d), "-n", str(n), "-o", str(o), "-u", "0", "-r", "repeats", "-t", "trim", "-T", "-p", "-s", "300"]
    return [("def", []), ("p", ["-p"]), ("plan", plan), ("vplan", ["-v"] + plan), ("S", ["-S", "300"]), ("R63", ["-R", "6", "-R", "3"]),
            ("R20", ["-R", "2", "-R", "0"]), ("wz", ["-w", "-z", "2"]), ("zu", ["-z", "2", "-u", "200"]), ("b", ["-b", "30"]),
            ("Y", ["-n", str(n), "-Y", "300"]), ("L", ["-L"]), ("vR6s", ["-v", "-s", "300", "-R", "6", "-R", "2"])]


# on the planted file alone
SYNTH_ONLY = [("A", ["-v", "-A", "sym.txt"]), ("a", ["-a", A_FILE, "-o", "1000"]), ("x", ["-x", "x.txt"]), ("I", ["-I", "i.txt"]),
              ("f", ["-f", "50"]), ("R4", ["-R", "4"]), ("R5", ["-R", "5"]), ("d", ["-v", "-d", "20"]), ("o", ["-v", "-o", "1000"]), ("u", ["-v", "-u", "100"]), ("l", ["-l", "9000"]),
              ("n", ["-v", "-n", "500"]), ("nY", ["-v", "-n", "500", "-Y", "300"]), ("vw", ["-v", "-w", "-R", "6"]), ("R6", ["-v", "-R", "6"]), ("s", ["-s", "300"])]
ERRORS = (("R7", ["-R", "7", "G", LAS, OUT]), ("x_and_I", ["-x", "x.txt", "-I", "i.txt", "G", LAS, OUT]), ("f100", ["-f", "100", "G", LAS, OUT]),
          ("no_r_track", ["-n", "100", "-r", "nosuch", "G", LAS, OUT]), ("no_las", ["G", "nosuch.las", OUT]), ("no_args", ["G", LAS]),
          ("bad_option", ["-Q", "G", LAS, OUT]))
# this project's own: what is not built says so
UNSUPPORTED = (("-m", "3", "-m (repeat modules)"), ("-M", "3", "-M (repeat modules)"), ("-y", "50", "-y (repeat modules)"),
               ("-P", "sp.txt", "-P (repeat spanners)"), ("-Z", "5", "-Z (worst alignments)"), ("-D", "dust", "-D (repeat interval analysis)"),
               ("-V", "2400", "-V (repeat interval analysis)"), ("-W", "600", "-W (repeat interval analysis)"), ("-c", "3,1000", "-c (chimer detection)"),
               ("-j", None, "-j (obsolete indel trimming)"))


def load_cases(what="cases"):
    """the tool cases, ("errors") the runs that end with a message, ("plants") what synth.las plants, ("files") the lists"""
    return json.load(open(os.path.join(FDIR, "cases.json")))[what]


class Expected(dict):
    files = ("novl", "tspace", "cols")


def expected(name):
    """the expected records of a case: novl, tspace and cols (the ten words of every record), put together from the input
    and what tests/golden/make_filter_golden.py kept of the case"""
    case = next(c for c in load_cases() if c["name"] == name)
    name = case.get("same_as", name)
    z = np.load(os.path.join(FDIR, "expected_%s.npz" % case["input"]))
    if name + ":cols" in z.files:
        cols = z[name + ":cols"]
    else:
        cols = tc.read_records(os.path.join(GOLDEN, INPUTS[case["input"]][1]))[0].copy()
        for k in LOOSE:
            cols[z["%s:i%d" % (name, k)], k] = z["%s:v%d" % (name, k)]
    return Expected(novl=len(cols), tspace=int(z["tspace"]), cols=cols)


def tracks(inp):
    """(trim anno, trim data, repeat anno, repeat data) of an input"""
    t = np.load(os.path.join(FDIR, "tracks.npz"))
    if inp == "fsynth":
        return t["fsynth_trim_anno"], t["fsynth_trim_data"], t["fsynth_rep_anno"], t["fsynth_rep_data"]
    tr = tc.expected(TRIM_OF[inp])
    return tr["trim_anno"], tr["trim_data"], t[inp + "_rep_anno"], t[inp + "_rep_data"]


def workdir(tmp, inp, files=None):
    """the database, the input, both tracks and the read lists of a case in tmp"""
    db = INPUTS[inp][0]
    for f in ("G.db", ".G.idx", ".G.bps"):
        shutil.copy(os.path.join(GOLDEN, db, f), os.path.join(tmp, f))
    shutil.copy(os.path.join(GOLDEN, INPUTS[inp][1]), os.path.join(tmp, LAS))
    ta, td, ra, rd = tracks(inp)
    tc.write_track_a2(os.path.join(tmp, ".G.trim"), len(ta) - 1, ta, td)
    tc.write_track_a2(os.path.join(tmp, ".G.repeats"), len(ra) - 1, ra, rd)
    for name, text in (load_cases("files") if files is None else files).items():
        open(os.path.join(tmp, name), "w").write(text)
    return tmp


def run_tool(opts, tmp, env_extra=None, timeout_s=None, args=("G", LAS, OUT), drop=()):
    cmd = [os.path.join(BIN, "LAfilter")] + list(opts) + list(args)
    if timeout_s:
        cmd = ["timeout", "-k", "10", str(timeout_s)] + cmd
    env = {k: v for k, v in os.environ.items() if k not in drop}
    env.update(env_extra or {})
    return subprocess.run(cmd, cwd=tmp, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def md5_or_none(path):
    return hashlib.md5(open(path, "rb").read()).hexdigest() if os.path.exists(path) else None


def text_md5(text):
    return hashlib.md5(text.encode()).hexdigest()


def check_output(case, r, tmp):
    if case["stdout"] is None:
        assert text_md5(r.stdout) == case["stdout_md5"], "stdout differs (%d lines)" % r.stdout.count("\n")
        case = dict(case, stdout=r.stdout)
    tc.check_output(case, expected(case["name"]), r, os.path.join(tmp, OUT))
    assert md5_or_none(os.path.join(tmp, A_FILE)) == case["md5_a"], "the -a file differs"


def run_case(case, tmp, env_extra=None, timeout_s=None, drop=()):
    workdir(tmp, case["input"])
    r = run_tool(case["opts"], tmp, env_extra, timeout_s, drop=drop)
    check_output(case, r, tmp)
    return r


def keeps_traces(case):
    """whether LAcheck -p can pass on a case's output: a stitched head and every record under -R 2 is written without its
    trace, in the reference as here, and LAcheck holds the trace of each record against its B interval"""
    cols = expected(case["name"])["cols"]
    return bool(np.all(cols[:, 0] > 0))


def lacheck(tmp):
    return subprocess.run([os.path.join(BIN, "LAcheck"), "-p", "G", OUT], cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True)


def trace_batch(path):
    """a .las file as api.pile_filter takes it: the dict of piles with diffs, tlen, trace_off and the trace bytes"""
    b = q_common.read_las(path)
    cols = tc.read_records(path)[0]
    aread = cols[:, 7]
    starts = np.flatnonzero(np.concatenate([[True], aread[1:] != aread[:-1]])) if len(aread) else np.zeros(0, dtype=np.int64)
    off = np.concatenate([starts, [len(aread)]]).astype(np.int64)
    tlen = cols[:, 0].astype(np.int32)
    toff = np.concatenate([[0], np.cumsum(tlen.astype(np.int64) * b["tbytes"])[:-1]]).astype(np.int64) if len(tlen) else np.zeros(0, np.int64)
    return dict(pile_off=off, pile_aread=aread[starts].astype(np.int32), abpos=cols[:, 2], aepos=cols[:, 4], bbpos=cols[:, 3], bepos=cols[:, 5],
                bread=cols[:, 8], flags=cols[:, 6], diffs=cols[:, 1], tlen=tlen, trace_off=toff, trace=np.asarray(b["trace"], dtype=np.uint8),
                tbytes=int(b["tbytes"]), tspace=int(b["tspace"]))


def trim_pairs(anno, data):
    """get_trim of every read"""
    n = len(anno) - 1
    out = np.zeros(2 * n, dtype=np.int32)
    for r in range(n):
        ob, oe = int(anno[r]) // 4, int(anno[r + 1]) // 4
        if oe - ob == 2 and data[ob] < data[ob + 1]:
            out[2 * r], out[2 * r + 1] = data[ob], data[ob + 1]
    return out


def sym_lists(text, nreads):
    """the -A file as the reference lays it out: (off, len, data), with the list of read 0 running on when it comes first"""
    pairs = [tuple(int(x) for x in line.split()) for line in text.splitlines() if line.strip()]
    data, off, prev = [], [-1] * (nreads + 1), -2
    for a, b in pairs:
        if a != prev:
            if prev > 0:
                data.append(-1)
            off[a] = len(data)
        data.append(b)
        prev = a
    data.append(-1)
    ln = [0] * (nreads + 1)
    for r in range(nreads + 1):
        if off[r] < 0:
            off[r] = 0
            continue
        while data[off[r] + ln[r]] > -1:
            ln[r] += 1
    return np.array(off, dtype=np.int32), np.array(ln, dtype=np.int32), np.array(data, dtype=np.int32)


def opts_to_params(opts, inp, files, own=None):
    """the options of a case as api.pile_filter takes them (without -T, -p, -a, -L, -v, which the pile call does not see);
    own: (trim anno, trim data, repeat anno, repeat data) in place of the input's tracks"""
    ta, td, ra, rd = own or tracks(inp)
    nreads = len(ta) - 1
    kw = dict(trim=trim_pairs(ta, td), remove=0)
    ints = {"-f": "downsample", "-b": "seg_rate", "-l": "min_rlen", "-o": "min_olen", "-u": "max_unaligned", "-n": "min_nonrep", "-Y": "merge_tips",
            "-z": "lowcov"}
    i = 0
    while i < len(opts):
        o = opts[i]
        if o in ints:
            kw[ints[o]] = int(opts[i + 1])
        elif o == "-d":
            kw["max_diffs"] = float(opts[i + 1]) / 100.0
        elif o in ("-s", "-S"):
            kw["stitch"], kw["stitch_aggr"] = int(opts[i + 1]), o == "-S"
        elif o == "-R":
            kw["remove"] |= 1 << int(opts[i + 1])
        elif o == "-w":
            kw["multi"] = True
        elif o == "-A":
            kw["sym"] = sym_lists(files[opts[i + 1]], nreads)
        elif o in ("-x", "-I"):
            st = np.zeros(nreads, dtype=np.uint8)
            st[[int(x) for x in files[opts[i + 1]].split()]] = 1 if o == "-x" else 2
            kw["read_state"], kw["include"] = st, o == "-I"
        if o in ints or o in ("-d", "-s", "-S", "-R", "-A", "-x", "-I", "-r", "-t", "-a"):
            i += 1
        i += 1
    if "min_nonrep" in kw:
        kw["repeats"] = (ra, rd)
    return kw


def random_piles():
    """seeded piles of 1 to 200 records on the reads of tiny2: runs of one B read of 1 to 5 records, every kind of flag in
    the input, traces that add up (and a few that do not), self overlaps and duplicates among them"""
    rl = q_common.db_read_len("tiny2")
    rng = np.random.default_rng(20261020)
    cols = {k: [] for k in ("abpos", "aepos", "bbpos", "bepos", "bread", "flags", "diffs", "tlen", "trace_off")}
    trace, off, areads = [], [0], []
    for a in rng.choice(len(rl), size=60, replace=False):
        n, alen = int(rng.integers(1, 201)), int(rl[a])
        areads.append(int(a))
        while n > 0:
            b = int(a) if rng.integers(12) == 0 else int(rng.integers(len(rl)))
            run = min(n, int(rng.integers(1, 6)))
            n -= run
            prev = None
            for _ in range(run):
                blen = int(rl[b])
                if prev is not None and rng.integers(4) == 0:                       # a duplicate, a contained or a stitchable record
                    kind = int(rng.integers(3))
                    ab, ae, bb, be = prev
                    if kind == 1:
                        ab, ae, bb, be = ab + (ae - ab) // 4, ae - (ae - ab) // 4, bb + (be - bb) // 4, be - (be - bb) // 4
                    elif kind == 2:
                        d = int(rng.integers(0, 60))
                        ab, bb = min(ae + d, alen), min(be + d + int(rng.integers(0, 60)), blen)
                        ae, be = min(ab + 1500, alen), min(bb + 1500, blen)
                else:
                    ab = int(rng.integers(0, alen - 200))
                    ae = int(rng.integers(ab + 100, alen + 1)) if rng.integers(3) else alen
                    ab = 0 if rng.integers(4) == 0 else ab
                    if b == a and rng.integers(2):
                        bb, be = ab, ae
                    else:
                        span = min(ae - ab + int(rng.integers(-50, 50)), blen)
                        bb = int(rng.integers(0, blen - max(span, 1) + 1))
                        be = bb + max(span, 0)
                if ae <= ab or be < bb:
                    ab, ae, bb, be = 0, min(500, alen), 0, min(500, blen)
                prev = (ab, ae, bb, be)
                nseg = (ae - 1) // TW - ab // TW + 1
                bl = np.full(nseg, (be - bb) // nseg)
                bl[:(be - bb) % nseg] += 1
                if bl.max() > 255:
                    bl = np.minimum(bl, 255)
                tr = np.zeros(2 * nseg, dtype=np.uint8)
                tr[1::2] = bl
                tr[0::2] = rng.integers(0, 45, size=nseg)
                if rng.integers(10) == 0:
                    tr[1] = (int(tr[1]) + 1) % 256                                  # trace points that do not add up
                flags = int(rng.integers(2)) | (int(rng.choice([0, 0x2, 0x12, 0x80 | 0x2, 0x20000 | 0x2, 0x40000, 0x8000 | 0x2, 0x10000])) if rng.integers(5) == 0 else 0)
                for k, v in zip(("abpos", "aepos", "bbpos", "bepos", "bread", "flags", "diffs", "tlen", "trace_off"),
                                (ab, ae, bb, be, b, flags, int(tr[0::2].sum()), len(tr), sum(len(x) for x in trace))):
                    cols[k].append(v)
                trace.append(tr)
        off.append(len(cols["abpos"]))
    batch = {k: np.array(v, dtype=np.int64 if k == "trace_off" else np.int32) for k, v in cols.items()}
    batch.update(pile_off=np.array(off, dtype=np.int64), pile_aread=np.array(areads, dtype=np.int32), trace=np.concatenate(trace), tbytes=1, tspace=TW)
    return batch, rl
