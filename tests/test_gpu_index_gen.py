"""The packed k-mer index whose unsorted keys are never in HBM: the radix sort's histogram and first pass make the key of
every k-mer slot from the block's 2-bit bases (kernels/kernels.h KmerCursor, kernels/radix_sort.hip) instead of reading
what kmer_tuples wrote.  Every index here is compared, element for element (code, read, position), with

  * the oracle's index (oracle_sort_kmers), and
  * the index of the old path -- kmer_tuples, then the sort over its keys -- built by a fresh child process under
    DAMAR_INDEX_GEN=0 (the switch is read once per process).

A tile of the sort is 8192 slots, a wavefront owns 512 consecutive slots of it in eight rounds of 64, and a lane's eight
slots lie 64 apart; the shapes below put read borders at all of these grains.

Reads shorter than k are not among them: damar_index_build refuses a block that has one, as the reference does
(daligner.c:499-504, "Block contains reads < kbp long"), on either path.  The shortest read a block may hold has k bases and
one k-mer; the `short` block is full of them."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

TILE = 8192


def _synthetic(lens, seed):
    """A HITS_DB (db/DB.h layout: a 4 in front of the first read and behind every read) of random reads."""
    import la_shapes
    rng = np.random.RandomState(seed)
    return la_shapes.make_db([rng.randint(0, 4, int(n)).astype(np.uint8) for n in lens])


def _lens_with_kmers(k, want, first):
    """read lengths whose k-mers (len + 1 - k each) add up to `want`"""
    lens, have = [], 0
    for n in first:
        lens.append(n)
        have += n + 1 - k
    assert want - have >= 1
    lens.append(want - have + k - 1)
    return lens


# name -> (k, how the block is made); `sim*` blocks come from the simulator and are read by name
def _short_lens(k, seed):
    rng = np.random.RandomState(seed)
    a = np.where(rng.rand(6000) < .5, k, k + rng.randint(0, 12, 6000))      # half of the reads hold ONE k-mer
    a[2000:2100] = 700                                                     # and a stretch of ordinary ones in between
    return a


CASES = {
    "sim_k14":   (14, "sim"),
    "sim_k12":   (12, "sim"),
    "sim_k16":   (16, "sim"),
    "sim_k14_c": (14, "simc"),                                     # the complement block (Block.upload_complement)
    "short":     (14, lambda: _synthetic(_short_lens(14, 5), 6)),  # dozens of reads per round of 64 slots, some hundred per tile
    "short_k16": (16, lambda: _synthetic(_short_lens(16, 7), 8)),
    "tile":      (14, lambda: _synthetic(_lens_with_kmers(14, TILE, [1000, 2100, 333]), 11)),
    "tile+1":    (14, lambda: _synthetic(_lens_with_kmers(14, TILE + 1, [1000, 2100, 333]), 12)),
    "tile-1":    (14, lambda: _synthetic(_lens_with_kmers(14, TILE - 1, [1000, 2100, 333]), 13)),
    "one_read":  (14, lambda: _synthetic([30011], 14)),            # a single read over 3.7 tiles
    "biased":    (14, "sim"),                                      # -b: the old path, whatever the switch says
}


def _sim_dir(tmp):
    from damar_amd import api
    if not os.path.exists(os.path.join(tmp, "S.db")):
        assert api.sim_write_db(tmp, "S", 1.0, coverage=2., seed=17) == 1          # 1 Mbp at 2x: one block of 2 Mbp
    return os.path.join(tmp, "S.1")


def _block(name, tmp):
    """-> (HITS_DB for the device, HITS_DB for the oracle, whatever has to stay alive)"""
    from damar_amd import api
    k, how = CASES[name]
    if how in ("sim", "simc"):
        db = api.read_block(_sim_dir(tmp))
        if how == "simc":
            import oracle_api as O
            cdb = api.HITS_DB()
            api.lib().damar_complement_copy(C.byref(db), C.byref(cdb))
            odb = O.read_block(_sim_dir(tmp))                       # the oracle complements a block of its own
            O.lib().damar_complement_block(C.byref(odb), 1)
            return cdb, odb, db
        return db, db, None
    db = how()
    return db, db, None


def _gpu_index(name, tmp):
    """the case's index as KmerPos records, and whether the build made its keys inside the sort"""
    import oracle_api as O
    from damar_amd import api
    L = api.lib()
    assert L.damar_hip_init(0) >= 1
    k, _ = CASES[name]
    db, _, keep = _block(name, tmp)
    assert L.Set_Filter_Params(k, 6, 0, 35, 4) == 0
    api.set_globals(biased=1 if name == "biased" else 0)
    L.damar_bias_reset()
    n = C.c_int(0)
    blk = L.damar_block_upload(C.byref(db))
    idx = L.damar_index_build(blk, 0, C.byref(n))
    made = L.damar_index_last_made()
    got = np.zeros(n.value, dtype=O.KMER_DT)
    L.damar_index_download(idx, got.ctypes.data)
    L.damar_index_free(idx)
    L.damar_block_free(blk)
    api.set_globals()
    L.Set_Filter_Params(14, 6, 0, 35, 4)
    return got, made


@pytest.fixture(scope="module")
def workdir(built, tmp_path_factory):
    return str(tmp_path_factory.mktemp("index_gen"))


@pytest.fixture(scope="module")
def old_path(workdir):
    """every case's index from ONE child process that runs under DAMAR_INDEX_GEN=0"""
    out = os.path.join(workdir, "old.npz")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), workdir, out], cwd=ROOT,
                       env=dict(os.environ, DAMAR_INDEX_GEN="0"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    return np.load(out)


def _oracle_index(name, tmp):
    import oracle_api as O
    k, _ = CASES[name]
    _, odb, keep = _block(name, tmp)
    prm = O.params(k=k)
    prm.biased = 1 if name == "biased" else 0
    p, n, want = O.sort_kmers(odb, prm)
    if p:
        O.lib().free(p)
    return want


@pytest.mark.parametrize("name", [c for c in CASES if c != "biased"])
def test_gpu_index_with_made_keys_equals_old_path_and_oracle(workdir, old_path, name):
    got, made = _gpu_index(name, workdir)
    assert made == 1                                       # the new path is what ran here ...
    assert int(old_path[name + "__made"]) == 0              # ... and kmer_tuples in the child
    old = old_path[name]
    print("%s: %d k-mers, %d tiles" % (name, len(got), (len(got) + TILE - 1) // TILE))
    assert len(got) == len(old) and len(got) > 0
    assert np.array_equal(got, old.view(got.dtype))
    want = _oracle_index(name, workdir)
    assert len(want) == len(got)
    assert np.array_equal(got, want)
    if name.startswith("tile"):
        assert len(got) == TILE + {"tile": 0, "tile+1": 1, "tile-1": -1}[name]
    if name == "one_read":
        assert len(got) == 30011 + 1 - 14 and len(got) > 3 * TILE
    if name.startswith("short"):                           # read borders inside a lane's eight slots, a round, a tile
        assert (np.bincount(got["read"]) == 1).sum() > 2000


def test_gpu_biased_build_keeps_the_old_path_with_the_switch_on(workdir, old_path):
    """-b walks every read (biased_tuples) and squeezes what it keeps: nothing for the sort to make.  The switch is on
    (default), the build must say it took the old path, and its index is the child's and the oracle's."""
    assert os.environ.get("DAMAR_INDEX_GEN", "1") != "0"
    got, made = _gpu_index("biased", workdir)
    assert made == 0
    old = old_path["biased"]
    assert len(got) == len(old) and len(got) > 0
    assert np.array_equal(got, old.view(got.dtype))
    assert np.array_equal(got, _oracle_index("biased", workdir))


if __name__ == "__main__":                                 # the child: every case on the path the environment selects
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    res = {}
    for case in CASES:
        res[case], res[case + "__made"] = _gpu_index(case, sys.argv[1])
    np.savez(sys.argv[2], **res)
