"""What tests/test_gpu_read_align.py, tests/test_read_align_host.py, tests/golden/make_read_align_golden.py and
scripts/read_align_timing.py share: the boxes of read length in tests/golden/correct/read_boxes.npz (four bases to a byte)
and how a result of api.align_reads is held to them."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "correct", "read_boxes.npz")

MAXDIFF = 8000                          # DAMAR_READ_MAXDIFF: the most differences kernels/read_align.hip holds
THREADS = 512                           # RA_THREADS: the lanes of its workgroup
_BOXES = None


def pack(bases):
    b = np.concatenate([np.asarray(bases, dtype=np.uint8), np.zeros(-len(bases) % 4, dtype=np.uint8)]).reshape(-1, 4)
    return (b[:, 0] | (b[:, 1] << 2) | (b[:, 2] << 4) | (b[:, 3] << 6)).astype(np.uint8)


def unpack(packed, n):
    p = np.asarray(packed, dtype=np.uint8)
    return np.stack([p & 3, (p >> 2) & 3, (p >> 4) & 3, (p >> 6) & 3], axis=1).reshape(-1)[:n]


def boxes():
    """the box cases, loaded once and left unchanged: m, n, aoff, boff, bases (one per byte), what the reference's
    Compute_Alignment(DIFF_ALIGN) made of them (diffs, soff, script), family[i] (an index into families) and planted[i]
    (the differences planted into a ladder or cap box, -1 elsewhere)"""
    global _BOXES
    if _BOXES is None:
        z = np.load(PATH)
        bx = {k: z[k] for k in z.files if k != "packed"}
        bx["bases"] = unpack(z["packed"], int(z["nbases"]))
        for v in bx.values():
            v.setflags(write=False)
        _BOXES = bx
    return _BOXES


def family_rows(bx, name):
    return np.flatnonzero(bx["family"] == list(bx["families"]).index(name))


def box_seqs(bx, idx):
    a = [bx["bases"][bx["aoff"][i]:bx["aoff"][i] + bx["m"][i]] for i in idx]
    b = [bx["bases"][bx["boff"][i]:bx["boff"][i] + bx["n"][i]] for i in idx]
    return a, b


def check(bx, diffs, scripts, idx):
    idx = list(idx)
    assert len(diffs) == len(idx) and len(scripts) == len(idx)
    for j, i in enumerate(idx):
        want = bx["script"][bx["soff"][i]:bx["soff"][i + 1]]
        assert int(diffs[j]) == int(bx["diffs"][i]), "box %d (%d x %d): %d differences against %d" % (i, bx["m"][i], bx["n"][i],
                                                                                                     diffs[j], bx["diffs"][i])
        assert np.array_equal(scripts[j], want), "box %d (%d x %d): the scripts part ways" % (i, bx["m"][i], bx["n"][i])


def run_family(bx, idx, limit=MAXDIFF):
    """api.align_reads on the boxes idx, held to the fixture; -> (read_last(), the boxes with more than `limit` differences)"""
    from damar_amd import api
    a, b = box_seqs(bx, idx)
    diffs, scripts = api.align_reads(a, b)
    check(bx, diffs, scripts, idx)
    last = api.read_last()
    assert last[1] == len(idx) and last[3] == int(np.sum(bx["soff"][np.asarray(idx) + 1] - bx["soff"][np.asarray(idx)]))
    return last, int(np.sum(bx["diffs"][np.asarray(idx)] > limit))
