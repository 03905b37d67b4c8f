/* tile_consensus.hip -- the consensus of a batch of tiles on gfx950 (corrector/consensus.c: consensus_add, v3_align_onp,
 * consensus_sequence, as corrector/LAcorrect.c's single_tile_consensus drives them).
 *
 * Mapping.  The tiles are the parallel axis: a pile gives ceil(alen / twidth) of them, a batch of piles thousands.  Inside
 * a tile the adds are sequential -- each sequence is aligned against the profile the one before it left -- and inside one
 * wave of an alignment every cell needs its neighbour just computed (the free move of the O(NP) scheme, see the header of
 * trace_pts.hip).  So: one lane per tile, as trace_waves has one lane per segment.  The host deals the tiles in
 * descending order of their weight, so the 64 lanes of a wavefront hold tiles of about the same work and lane i of the
 * grid takes tiles i, i + lanes, ...
 *
 * Storage.  Everything a lane needs beyond registers is its own stripe of an HBM work area: the profile (five count bytes
 * per column), the per-column match codes, the script of the add in flight and the waves (int16 furthest point, int8
 * code per cell, rows packed back to back).  A stripe is 28 KB: 64 lanes of it do not fit the 160 KB of LDS of a CU even at
 * one wavefront per CU, and the waves are walked again in an order no lane shares with its neighbours, so LDS would buy
 * no coalescing either.  (Whether the stripes stay in L2 -- 4 MB per XCD against 1.8 MB per resident wavefront -- is not
 * measured.)
 *
 * The text of the method is kernels/tile_core.h, which host/correct.c compiles as well.  Integer work only; every loop is
 * bounded by the tile's sizes or by a step count.  A tile that meets a limit (columns, script, cells) is left alone with
 * status TC_ROOM: the host routine does it.  Nothing is dropped silently. */
#include "kernels.h"

#define TC_FN __device__ __forceinline__
#define TC_VT short
#define TC_ST short
#include "tile_core.h"

#define TCN_THREADS 64

__global__ __launch_bounds__(TCN_THREADS)
void tile_consensus(TileArgs a)
{ const u32 tid = blockIdx.x * TCN_THREADS + threadIdx.x;
  const u32 nlanes = gridDim.x * TCN_THREADS;
  tc_work w;
  u8 *stripe = a.work + (size_t) tid * a.stripe;
  w.cnt = stripe;
  w.pc = stripe + 5 * (size_t) a.maxcols;
  w.script = (short *) (stripe + 6 * (size_t) a.maxcols);
  w.vf = w.script + a.maxscript;
  w.hf = (signed char *) (w.vf + a.cells);
  w.cap = a.cells;
  w.maxcols = a.maxcols;
  w.maxscript = a.maxscript;
  for (u32 it = tid; it < a.ntasks; it += nlanes)
    { const u32 t = a.order[it];
      const long long e0 = a.ent_off[t];
      const int nent = (int) (a.ent_off[t + 1] - e0);
      int n = 0;
      const int st = tc_tile(&w, a.bases, a.seq_off + e0, a.seq_len + e0, nent, a.out + (size_t) it * a.maxcols, &n);
      a.status[it] = st;
      a.len[it] = st ? 0 : n;
    }
}

void damar_launch_tile_consensus(const TileArgs *a, hipStream_t st)
{ if (a->ntasks == 0)
    return;
  hipLaunchKernelGGL(tile_consensus, dim3(a->blocks), dim3(TCN_THREADS), 0, st, *a);
}
