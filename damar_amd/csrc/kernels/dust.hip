/* dust.hip -- the low-complexity mask of reads: db/DBdust.c, Myers' incremental SDUST, which the reference runs one read
 * after the other on one thread.  A read is cut into pieces of DAMAR_DUST_PIECE triplet starts; a piece starts from an empty
 * state DAMAR_DUST_HALO triplets before its first start and runs `window` steps beyond its last, which makes its retired
 * candidates the whole read's.  One wavefront does one piece:
 *
 *   - lane p & 63 holds the triplet at position p of the window (at most 62 of them) and r, the number of later positions
 *     of the window with the same triplet.  When triplet j arrives, the lanes that hold its like raise r: a compare.  The
 *     score of the suffix that starts at p is then the sum of r over the positions from p on, so the window's score wsqr
 *     and the admissible suffix's lsqr follow the reference's updates from r and one ballot, as wave-uniform integers;
 *   - only when wsqr > lsqr * t (the reference's own test, :427) are the scores of all starts made, by one scan over the
 *     lanes, and tested against t * (j - c) in all lanes at once;
 *   - the starts that pass are walked as the reference walks them: descending, one after the other over the bits of the
 *     ballot, with its candidate rule in its forms on doubles (no contraction: see the Makefile);
 *   - a candidate's start lies in the window, so its slot is start & 63: the list is a 64-bit mask and, per wavefront, 64
 *     ends and 64 scores in LDS.  The one candidate whose start leaves the window is retired into the piece's stripe.
 *
 * dust_join then takes a read's stripes in order, one lane per read: the +1 joining rule and the -m cut (:409-425, :482-494),
 * compacted in place; dust_gather moves every read's pairs to where the host's offsets put them. */
#include "dev_common.h"
#include "kernels.h"
#include "damar_hip.h"

#define DUST_WAVES   4
#define DUST_STRETCH (DAMAR_DUST_HALO + DAMAR_DUST_PIECE + DAMAR_DUST_MAXWINDOW)

__device__ __forceinline__ u64 rotr64(u64 x, int k) { k &= 63;  return k ? ((x >> k) | (x << (64 - k))) : x; }
__device__ __forceinline__ u64 rotl64(u64 x, int k) { return rotr64(x, 64 - (k & 63)); }

__global__ void __launch_bounds__(DUST_WAVES * WAVE) dust_pieces_kernel(DustArgs a)
{ __shared__ u8     s_tri[DUST_WAVES][DUST_STRETCH];
  __shared__ int    s_end[DUST_WAVES][WAVE];
  __shared__ double s_score[DUST_WAVES][WAVE];

  const int wv = (int) (threadIdx.x >> 6), lane = lane_id();
  const u32 piece = blockIdx.x * DUST_WAVES + (u32) wv;
  if (piece >= a.npieces)
    return;
  u8     *tri = s_tri[wv];
  int    *c_end = s_end[wv];
  double *c_score = s_score[wv];

  const u32       rd = a.piece_read[piece];
  const long long ro = a.read_off[rd];
  const int       ntri = (int) (a.read_off[rd + 1] - ro) - 2;
  const int       own_beg = a.piece_first[piece];
  const int       own_end = min(own_beg + DAMAR_DUST_PIECE, ntri);
  const int       s = max(own_beg - DAMAR_DUST_HALO, 0), e = min(own_end + a.window, ntri);
  const int       w = a.window, thresh2i = a.thresh2i;
  const double    t = a.thresh;
  const u8       *seq = a.bases + ro;
  int            *stripe = a.cand + (size_t) piece * 2 * (size_t) a.stripe;

  for (int k = s + lane; k < e; k += WAVE)                /* e <= ntri: the last base read is seq[ntri + 1] */
    tri[k - s] = (u8) ((seq[k] << 4) | (seq[k + 1] << 2) | seq[k + 2]);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

  int code = -1, r = 0;                                   /* this lane's position of the window: none */
  int wb = s - 1, lb = s - 1, wsqr = 0, lsqr = 0, nout = 0;
  u32 walks = 0;
  u64 cm = 0;                                             /* bit q: a candidate that starts at the position of lane q */

#define DUST_RETIRE(beg, end)                                                         \
  { if ((beg) >= own_beg && (beg) < own_end)                                          \
      { if (nout < a.stripe && lane == 0)                                             \
          { stripe[2 * nout] = (beg);                                                 \
            stripe[2 * nout + 1] = (end);                                             \
          }                                                                           \
        nout += 1;                                                                    \
      }                                                                               \
  }

  for (int j = s; j < e; j++)
    { const int c = first_i((int) tri[j - s]), jl = j & 63;
      if (j - s > w - 3)                                  /* the window's oldest position leaves: its lane is free again */
        { wb += 1;
          const int el = wb & 63, rel = bcast_i(r, el);
          wsqr -= rel;
          if (lb < wb)
            { lb = wb;
              lsqr -= rel;
            }
          if (lane == el)
            { code = -1;
              r = 0;
            }
        }
      const u64 m = wballot(code == c);                   /* the window's positions before j that hold c */
      wsqr += __popcll(m);
      if (code == c)
        r += 1;
      /* those of them in the suffix (lb, j): bit k of `suf` is position lb + 1 + k */
      const u64 suf = rotr64(m, lb + 1) & lanes_below(j - 1 - lb);
      const int trun = __popcll(suf);
      lsqr += trun;
      if (lane == jl)
        { code = c;
          r = 0;
        }
      if (trun >= thresh2i)                               /* c too often: the suffix starts behind the first of them */
        { const int k = __ffsll((long long) suf) - 1;
          lsqr -= wave_sum_i((((lane - (lb + 1)) & 63) <= k) ? r : 0);
          lb += 1 + k;
        }
      if (wb >= s && ((cm >> (wb & 63)) & 1))             /* the one candidate whose start has left the window */
        { DUST_RETIRE(wb, c_end[wb & 63])
          cm &= ~(1ull << (wb & 63));
        }
      if (!((double) wsqr > (double) lsqr * t))
        continue;

      walks += 1;
      /* score[lane]: of the suffix that starts at this lane's position, age = j - position steps back */
      const int P = wave_incl_scan_i(r), Pj = bcast_i(P, jl), P63 = bcast_i(P, 63);
      const int score = (lane <= jl) ? (Pj - P + r) : (Pj + P63 - P + r);
      const int age = (j - lane) & 63;
      const bool pass = age >= j - lb && age < j - wb && (double) score >= t * (double) age;
      /* both masks turned so that bit 63 - age is the position j - age: descending positions are descending bits */
      u64 pm = rotl64(wballot(pass), 63 - jl), rest = rotl64(cm, 63 - jl);
      double mscore = 0.;
      while (pm != 0)
        { const int bit = 63 - __clzll((long long) pm), back = 63 - bit, slot = (j - back) & 63;
          pm &= ~(1ull << bit);
          u64 look = rest & (~0ull << bit);               /* the candidates from this start on not looked at yet */
          rest &= ~(~0ull << bit);
          while (look != 0)
            { const int b2 = 63 - __clzll((long long) look);
              const double sc = c_score[(j - (63 - b2)) & 63];
              look &= ~(1ull << b2);
              if (sc > mscore)
                mscore = sc;
            }
          const int sq = bcast_i(score, slot);
          if ((double) sq >= mscore * (double) back)
            { mscore = (1. * (double) sq) / (double) back;
              c_end[slot] = j;                            /* every lane writes the same, and reads what it wrote */
              c_score[slot] = mscore;
              cm |= 1ull << slot;
            }
        }
    }
  if (e == ntri)                                          /* the read's end: every candidate left, earliest start first */
    { u64 left = rotr64(cm, wb + 1);
      while (left != 0)
        { const int k = __ffsll((long long) left) - 1, beg = wb + 1 + k;
          left &= left - 1;
          DUST_RETIRE(beg, c_end[beg & 63])
        }
    }
  if (lane == 0)
    { a.ncand[piece] = nout;
      atomicAdd(a.steps, (u64) (e - s));
      atomicAdd(a.steps + 1, (u64) walks);
    }
}

/* one lane per read: the candidates of its pieces' stripes, in order of their starts, joined and cut to minlen, written
   back from the start of its first stripe; nint[read] pairs, or -1 where a stripe was too small */
__global__ void __launch_bounds__(256) dust_join_kernel(DustArgs a)
{ const u32 rd = blockIdx.x * 256 + threadIdx.x;
  if (rd >= a.nreads)
    return;
  const u32 p0 = a.read_piece[rd], p1 = a.read_piece[rd + 1];
  int *dst = a.cand + (size_t) p0 * 2 * (size_t) a.stripe;
  int  m = 0, have = 0, beg = 0, end = -2;
  for (u32 p = p0; p < p1; p++)
    if (a.ncand[p] > a.stripe)
      { a.nint[rd] = -1;
        return;
      }
  for (u32 p = p0; p < p1; p++)
    { const int *src = a.cand + (size_t) p * 2 * (size_t) a.stripe;
      const int  n = a.ncand[p];
      for (int k = 0; k < n; k++)
        { const int cb = src[2 * k], ce = src[2 * k + 1] + 2;
          if (have && end + 1 >= cb)
            { if (end < ce)
                end = ce;
              continue;
            }
          if (have && end - beg >= a.minlen - 1)          /* behind what has been read: m pairs from at most m candidates */
            { dst[2 * m] = beg;
              dst[2 * m + 1] = end + 1;
              m += 1;
            }
          beg = cb;  end = ce;  have = 1;
        }
    }
  if (have && end - beg >= a.minlen - 1)
    { dst[2 * m] = beg;
      dst[2 * m + 1] = end + 1;
      m += 1;
    }
  a.nint[rd] = m;
}

/* one wavefront per read: its pairs to out + out_off[read] (ints) */
__global__ void __launch_bounds__(DUST_WAVES * WAVE) dust_gather_kernel(DustArgs a)
{ const u32 rd = blockIdx.x * DUST_WAVES + (threadIdx.x >> 6);
  if (rd >= a.nreads)
    return;
  const int n = a.nint[rd];
  if (n <= 0)
    return;
  const int *src = a.cand + (size_t) a.read_piece[rd] * 2 * (size_t) a.stripe;
  int       *dst = a.out + a.out_off[rd];
  for (int k = lane_id(); k < 2 * n; k += WAVE)
    dst[k] = src[k];
}

void damar_launch_dust_pieces(const DustArgs *a, hipStream_t st)
{ if (a->npieces > 0)
    hipLaunchKernelGGL(dust_pieces_kernel, dim3((a->npieces + DUST_WAVES - 1) / DUST_WAVES), dim3(DUST_WAVES * WAVE), 0, st, *a);
  if (a->nreads > 0)
    hipLaunchKernelGGL(dust_join_kernel, dim3((a->nreads + 255) / 256), dim3(256), 0, st, *a);
}

void damar_launch_dust_gather(const DustArgs *a, hipStream_t st)
{ if (a->nreads > 0)
    hipLaunchKernelGGL(dust_gather_kernel, dim3((a->nreads + DUST_WAVES - 1) / DUST_WAVES), dim3(DUST_WAVES * WAVE), 0, st, *a);
}
