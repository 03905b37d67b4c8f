/* pile_quality.hip -- LAq's quality value per trace-spacing segment ("tile") of every A read of a batch of piles, for gfx950
 * (scrub/LAq.c:312-409; the plain version is host/quality.c damar_host_pile_quality).
 *
 * The work is per trace segment, not per record: every segment a record's trace holds for the A read names one tile and one
 * difference count, and a tile's value is the mean of its segmax lowest counts.  Three kernels around one scan:
 *   q_count    a wavefront per record walks its trace (lanes over segments, so neighbouring lanes read neighbouring
 *              bytes), applies the three inclusion rules and the spill rule, and adds 1 to the tile's depth counter;
 *   (scan)     exclusive scan of the depths (sort_scan.hip) -> where each tile's run of values begins;
 *   q_scatter  the same walk again, each value as a u16 into its tile's run; a slot is taken by counting the depth
 *              counter down again, so order inside a run is whatever the hardware made it -- the result does not depend on it;
 *   q_select   a wavefront per tile, four tiles per workgroup: the segmax smallest of the run by a count over 64 value bins
 *              in the wave's own LDS, walked chunk by chunk with the count and the sum carried.  The next chunk begins at the
 *              smallest value the pass saw beyond the current one, so a run costs one pass per occupied chunk it needs, not
 *              tspace / 64 of them: any depth, any segmax, any spacing up to 65535.
 * No float, no 64-bit sort; the only atomics are the depth counters and the LDS bins.  Every tile index is checked against
 * its pile's tile count before it is used, whatever the records' coordinates claim.
 */
#include "dev_common.h"
#include "kernels.h"

#define PQ_THREADS 256
#define PQ_WAVES   (PQ_THREADS / WAVE)
#define PQ_MAX_BLOCKS 65536u

/* LDS traffic of one wave reaches the LDS in program order; this keeps the compiler from moving it */
__device__ __forceinline__ void wave_lds_sync()
{ __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

/* The inclusion rules (LAq.c:340-361): the first segment counts only if the overlap begins on a tile boundary, the last one
   only if it ends on one or at the read's end, the ones between always; identity overlaps never; OVL_DISCARD is not looked
   at.  A record of one segment (tlen 2 or 3) has a first and no last.  The spill rule: the reference's histogram is flat over
   the read, so q >= tspace differences count in tile + q / tspace at q % tspace; beyond the read's tiles they are dropped. */
template <int SCATTER>
__global__ __launch_bounds__(PQ_THREADS)
void q_walk(QArgs a)
{ const int l = lane_id();
  const u32 nwaves = gridDim.x * PQ_WAVES;
  const u32 tw = (u32) a.tspace;
  for (u32 r = blockIdx.x * PQ_WAVES + (threadIdx.x >> 6); r < a.nrec; r += nwaves)
    { u32 lo = 0, hi = a.npiles;                 /* pile_off[lo] <= r < pile_off[hi]: the record's pile, empty piles skipped */
      while (hi - lo > 1)
        { const u32 mid = lo + (hi - lo) / 2;
          if (a.pile_off[mid] <= (long long) r) lo = mid; else hi = mid;
        }
      if (a.bread[r] == a.pile_aread[lo])
        continue;
      const int  alen = a.pile_alen[lo];
      const u32  g0 = a.pile_tile0[lo], ntiles = a.pile_tile0[lo + 1] - g0;
      const int  ab = a.abpos[r], ae = a.aepos[r], nseg = a.tlen[r] >> 1;
      const u32  t0 = (u32) ab / tw;
      const bool first_ok = ((u32) ab % tw) == 0;
      const bool last_ok = (ae % (int) tw) == 0 || ae == alen;
      const u8  *tr = a.trace + a.trace_off[r];
      for (int s = l; s < nseg; s += WAVE)
        { if (s == 0 ? !first_ok : (s == nseg - 1 && !last_ok))
            continue;
          u32 v;
          if (a.tbytes == 1)
            v = tr[2 * (size_t) s];
          else
            v = (u32) tr[4 * (size_t) s] | ((u32) tr[4 * (size_t) s + 1] << 8);
          const u64 tile = (u64) t0 + (u32) s + v / tw;
          if (tile >= ntiles)
            continue;
          const u32 g = g0 + (u32) tile;
          if (!SCATTER)
            atomicAdd(&a.depth[g], 1u);
          else
            { const u32 k = atomicSub(&a.depth[g], 1u) - 1u;      /* 0 <= k < the tile's depth: q_count took the same walk */
              a.vals[(size_t) a.off[g] + k] = (u16) (v % tw);
            }
        }
    }
}

__global__ __launch_bounds__(PQ_THREADS)
void q_select(QArgs a)
{ __shared__ u32 s_bins[PQ_WAVES][WAVE];
  const int l = lane_id(), w = (int) (threadIdx.x >> 6);
  u32 *bins = s_bins[w];
  const u32 nwaves = gridDim.x * PQ_WAVES;
  for (u32 t = blockIdx.x * PQ_WAVES + (u32) w; t < a.ntiles; t += nwaves)
    { const u32 lo = a.off[t], hi = a.off[t + 1];
      u32 count = 0, base = 0;
      u64 sum = 0;
      while (hi > lo && count < a.segmax)        /* count, base and the exits are the same in all lanes: a wave-uniform loop */
        { bins[l] = 0;
          wave_lds_sync();
          int next = 0x7fffffff;                 /* the smallest value beyond this chunk (values are u16) */
          for (u32 i = lo + (u32) l; i < hi; i += WAVE)
            { const u32 v = a.vals[i];
              if (v >= base)
                { if (v - base < WAVE) atomicAdd(&bins[v - base], 1u);
                  else if ((int) v < next) next = (int) v;
                }
            }
          wave_lds_sync();
          const u32 h = bins[l];
          wave_lds_sync();
          const u32 excl = (u32) wave_incl_scan_i((int) h) - h;          /* a run holds fewer than 2^31 values */
          const u32 room = a.segmax - count;
          const u32 take = (excl >= room) ? 0u : (h < room - excl ? h : room - excl);
          const u64 part = (u64) take * (u64) (base + (u32) l);          /* < 2^31 * 2^16: summed in two halves of 24 bits */
          sum += ((u64) (u32) wave_sum_i((int) (u32) (part >> 24)) << 24) + (u64) (u32) wave_sum_i((int) (u32) (part & 0xffffffu));
          count += (u32) wave_sum_i((int) take);
          next = wave_min_i(next);
          if (next == 0x7fffffff)
            break;
          base = (u32) next;
        }
      if (l == 0)
        { int q;
          if (count < a.segmin)
            q = a.ccs ? 25 : 0;
          else
            { if (sum == 0) sum = count;                                 /* LAq.c:396-399 */
              q = (int) ((2 * sum + count) / (2 * (u64) count));         /* (int) ((float) sum / count + 0.5), in integers */
            }
          a.q[t] = q;
        }
    }
}

static u32 blocks_for(u32 n)
{ const u32 b = (n + PQ_WAVES - 1) / PQ_WAVES;
  return b < 1 ? 1 : (b > PQ_MAX_BLOCKS ? PQ_MAX_BLOCKS : b);
}

void damar_launch_q_count(const QArgs *a, hipStream_t st)
{ if (a->nrec > 0)
    hipLaunchKernelGGL(q_walk<0>, dim3(blocks_for(a->nrec)), dim3(PQ_THREADS), 0, st, *a);
}

void damar_launch_q_scatter(const QArgs *a, hipStream_t st)
{ if (a->nrec > 0)
    hipLaunchKernelGGL(q_walk<1>, dim3(blocks_for(a->nrec)), dim3(PQ_THREADS), 0, st, *a);
}

void damar_launch_q_select(const QArgs *a, hipStream_t st)
{ if (a->ntiles > 0)
    hipLaunchKernelGGL(q_select, dim3(blocks_for(a->ntiles)), dim3(PQ_THREADS), 0, st, *a);
}
