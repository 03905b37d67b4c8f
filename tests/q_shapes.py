"""Random trace batches at the shapes where kernels/pile_quality.hip can go wrong, for tests/test_gpu_q.py (and a few of
them on the host path in tests/test_q_host.py): make(i) -> (batch, read lengths, options of q_model.tile_q)."""
import numpy as np

SCAN_TILE = 4096            # DAMAR_SCAN_TILE (kernels/kernels.h): items per workgroup of the scan of the depths

# spacing, options, piles: ("full", tiles, extra bases, depth): `depth` records over the whole read, no spill, so every tile
# has exactly that depth; ("rand", tiles, extra bases, records): random spans with every rule on and off, spills, identity
# and discarded records; extra bases: 0 -> alen = tiles * tw, 1 -> (tiles - 1) * tw + 1
SHAPES = [
    (100, dict(segmax=20), [("full", 4, 1, 0), ("full", 3, 0, 1), ("full", 5, 1, 19), ("full", 5, 0, 20), ("full", 4, 1, 21), ("rand", 40, 1, 60)]),
    (100, dict(segmax=64), [("full", 3, 0, 63), ("full", 3, 1, 64), ("full", 3, 0, 65), ("rand", 30, 0, 200)]),
    (100, dict(segmax=1000), [("full", 3, 1, 255), ("full", 2, 0, 256), ("full", 3, 0, 257), ("full", 1, 1, 5000), ("full", 2, 0, 1200)]),
    (126, dict(segmax=20), [("rand", 1, 1, 9), ("rand", 1, 0, 30), ("rand", 25, 0, 80), ("rand", 25, 1, 80), ("full", 2, 1, 64)]),
    (500, dict(segmax=1), [("rand", 12, 1, 90), ("rand", 7, 0, 300), ("full", 3, 0, 65)]),
    (100, dict(segmax=20, segmin=3, ccs=True), [("rand", 60, 1, 150)]),                     # 1 pile
    (500, dict(segmax=64), [("rand", 9, 0, 700), ("full", 1, 0, 300)]),
] + [(100, dict(segmax=5), total) for total in (SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 2 * SCAN_TILE + 1)]


def make(i):
    tw, kw, piles = SHAPES[i]
    rng = np.random.default_rng(7000 + i)
    if isinstance(piles, int):                              # that many tiles in all, in piles of 10 tiles and a rest
        total = piles
        piles = [("rand", 10, k % 2, 4) for k in range(total // 10)] + ([("rand", total % 10, 1, 6)] if total % 10 else [])
    tb = 1 if tw <= 125 else 2
    vmax = 255 if tb == 1 else 3 * tw - 1
    rl, recs, off = [], [], [0]
    for a, (kind, tiles, extra, n) in enumerate(piles):
        alen = tiles * tw if not extra else (tiles - 1) * tw + 1
        rl.append(alen)
        for k in range(n):
            if kind == "full":
                ab, ae = 0, alen
            else:
                ab = int(rng.integers(0, max(1, alen - 1)))
                ab -= ab % tw if rng.random() < 0.5 else 0
                ae = int(rng.integers(ab + 1, alen + 1))
                r = rng.random()
                ae = alen if r < 0.3 else (max(ab + 1, ae - ae % tw) if r < 0.6 else ae)
            nseg = (ae + tw - 1) // tw - ab // tw
            small = tw if (tw > 64 and k % 3 == 0) else 30  # some records over all value bins, most near the low end
            v = rng.integers(0, small, nseg)
            if kind == "rand":
                spill = rng.random(nseg) < 0.08
                v = np.where(spill, rng.integers(tw, vmax + 1, nseg), v)
            bread = a if (kind == "rand" and rng.random() < 0.1) else (a + 1 + int(rng.integers(0, 5)))
            flags = int(rng.integers(0, 2)) | (2 if rng.random() < 0.15 else 0)
            recs.append((ab, ae, bread, flags, np.stack([v, np.full(nseg, tw)], axis=1).reshape(-1)))
        off.append(len(recs))
    rl += [tw] * 6                                          # the reads the B sides name
    dt = np.uint8 if tb == 1 else np.dtype("<u2")
    traces = [np.minimum(r[4], 255 if tb == 1 else 65535).astype(dt).view(np.uint8) for r in recs]
    tlen = np.array([len(r[4]) for r in recs], dtype=np.int32)
    toff = np.concatenate([[0], np.cumsum(tlen.astype(np.int64) * tb)])[:-1].astype(np.int64) if recs else np.zeros(0, dtype=np.int64)
    col = lambda j: np.array([r[j] for r in recs], dtype=np.int32)
    b = dict(pile_off=np.array(off, dtype=np.int64), pile_aread=np.arange(len(piles), dtype=np.int32), abpos=col(0), aepos=col(1),
             bbpos=col(0), bepos=col(1), bread=col(2), flags=col(3), tlen=tlen, trace_off=toff,
             trace=np.concatenate(traces) if traces else np.zeros(0, dtype=np.uint8), tbytes=tb, tspace=tw)
    return b, np.array(rl, dtype=np.int32), kw
