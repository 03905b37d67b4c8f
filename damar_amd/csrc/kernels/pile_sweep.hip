/* pile_sweep.hip -- mask tracks from piles of overlaps on gfx950: the sweeps of scrub/LArepeat.c (coverage estimate
 * :168-233, repeat regions :282-494) and scrub/TANmask.c (:115-207), which the reference runs one read at a time behind a
 * qsort per pile.
 *
 * Here every kept record of a batch becomes two u64 event keys  pile << (pbits + 1) | coordinate << 1 | tie  (pile_events,
 * the filters run there; a dropped record writes two keys of pile number npiles, which sort behind everything), ONE radix
 * sort over exactly the used bits orders all piles at once, and pile_sweep walks each pile's run of sorted events with one
 * workgroup: 256 events at a time, every step of the reference's sequential loop restated as a scan with a carry from
 * chunk to chunk, so a pile of any size takes the same path.
 *   depth      inclusive sum of +1 / -1
 *   state      "inside a region" after an event = the value of the LAST event that set it (depth > enter sets 1, depth <
 *              leave sets 0, anything else leaves it): a max-scan over index << 1 | value
 *   -C value   max of the depth over starts since the last opening event, the opening event itself excluded: a scan of
 *              (reset, max) pairs
 *   regions    openings and closings are the 0->1 and 1->0 steps of the state; the count of openings so far is a region's
 *              number in its pile
 * Merging (-m), the reference's edge extension and the compaction to one data array follow per pile in the same kernel.
 * Wave size 64, plain C++ stores only. */
#include "dev_common.h"
#include "kernels.h"

#define PS_THREADS 256
#define PS_EDGE_DIST 1000            /* LArepeat.c:38-39 */
#define PS_EDGE_FUZZ 200
#define PS_SEP_FUZZ  20              /* TANmask.c:82 */
#define PS_DISCARD   0x2             /* lib/oflags.h:5 OVL_DISCARD */
#define PS_DB_BEST   0x0800          /* db/DB.h DB_BEST */

/***** events ***********************************************************************************/

__global__ __launch_bounds__(PS_THREADS)
void pile_events(PileArgs a)
{ __shared__ u32 s_kept;
  __shared__ u64 s_bases;
  const u32 p = blockIdx.x;
  if (threadIdx.x == 0)
    { s_kept = 0;
      s_bases = 0;
    }
  __syncthreads();
  const long long lo = a.pile_off[p], hi = a.pile_off[p + 1];
  const int  ar   = a.pile_aread[p];
  const u64  top  = (u64) p << (a.pbits + 1);
  const u64  sent = (u64) a.npiles << (a.pbits + 1);
  const int  pmax = (int) ((1u << a.pbits) - 1u);
  u32 k = 0;
  u64 bs = 0;
  for (long long i = lo + threadIdx.x; i < hi; i += PS_THREADS)
    { const int ab = a.abpos[i], ae = a.aepos[i];
      bool keep;
      int  p0, p1, t0, t1;
      if (a.mode == DAMAR_PILE_REPEAT)
        { keep = !(a.flags[i] & PS_DISCARD) && (a.inc_identity || a.bread[i] != ar) && ae - ab >= a.min_len;
          p0 = ab;      t0 = 1;                    /* on one coordinate an end sorts before a start (:107-120) */
          p1 = ae - 1;  t1 = (p1 > 0) ? 0 : 1;     /* the reference keeps an end as -(aepos - 1): at 0 it reads as a start */
        }
      else if (a.mode == DAMAR_PILE_COVER)
        { keep = (a.read_flags[a.bread[i]] & PS_DB_BEST) && !(a.flags[i] & PS_DISCARD) && a.bread[i] != ar &&
                 ae - ab >= a.min_len;
          p0 = ab;  t0 = 1;
          p1 = ae;  t1 = 0;
          if (keep) bs += (u64) (ae - ab);
        }
      else
        { keep = ab - a.bepos[i] <= PS_SEP_FUZZ && ae - a.bbpos[i] > a.min_len;
          p0 = a.bbpos[i];  t0 = 0;                /* a start sorts before an end: add[i] <= del[j], TANmask.c:174 */
          p1 = ae;          t1 = 1;
        }
      if (keep && (p0 < 0 || p1 < 0 || p0 > pmax || p1 > pmax))
        { atomicOr(a.err, DAMAR_PILE_ERR_RANGE);
          keep = false;
        }
      a.keys[2 * i]     = keep ? (top | ((u64) (u32) p0 << 1) | (u64) t0) : sent;
      a.keys[2 * i + 1] = keep ? (top | ((u64) (u32) p1 << 1) | (u64) t1) : sent;
      k += keep ? 1u : 0u;
    }
  if (k) atomicAdd(&s_kept, k);
  if (bs) atomicAdd((unsigned long long *) &s_bases, (unsigned long long) bs);
  __syncthreads();
  if (threadIdx.x == 0)
    { a.kept[p] = s_kept;
      if (a.mode == DAMAR_PILE_COVER) a.bases[p] = s_bases;
    }
}

/***** scans of one 256-event chunk *************************************************************/

struct OpAdd { __device__ int operator()(int x, int y) const { return x + y; } };
struct OpMax { __device__ int operator()(int x, int y) const { return x > y ? x : y; } };
/* (reset, max): y after x */
struct OpPeak
{ __device__ int2 operator()(int2 x, int2 y) const
  { return y.x ? y : make_int2(x.x, x.y > y.y ? x.y : y.y); }
};

/* inclusive scan over the workgroup's 256 values (Hillis-Steele through LDS, buf holds 2 x 256) */
template <typename T, typename Op>
__device__ __forceinline__ T chunk_scan(T v, T *buf, Op op)
{ const int t = threadIdx.x;
  int cur = 0;
  __syncthreads();
  buf[t] = v;
  __syncthreads();
  for (int o = 1; o < PS_THREADS; o <<= 1)
    { T x = buf[cur * PS_THREADS + t];
      if (t >= o) x = op(buf[cur * PS_THREADS + t - o], x);
      cur ^= 1;
      buf[cur * PS_THREADS + t] = x;
      __syncthreads();
    }
  return buf[cur * PS_THREADS + t];
}

struct Carry { int span, state, peak, n; };

/***** the sweep: one workgroup per pile ********************************************************/

__global__ __launch_bounds__(PS_THREADS)
void pile_sweep(PileArgs a)
{ __shared__ int2  s_buf[2 * PS_THREADS];
  __shared__ int   s_state[PS_THREADS];
  __shared__ Carry s_carry;
  __shared__ u64   s_acc[2];
  __shared__ int   s_sup[2];
  int *ibuf = (int *) s_buf;
  const int t = threadIdx.x;
  const u32 p = blockIdx.x;
  const u32 kept = a.kept[p], nev = 2 * kept;
  const u64 e0 = 2 * (u64) a.koff[p];
  const u64 *keys = a.keys + e0;
  const int pmask = (int) ((1u << a.pbits) - 1u);
  const size_t obase = 3 * (size_t) a.koff[p];

  if (t == 0)
    { s_carry.span = 0;  s_carry.state = 0;  s_carry.peak = 0;  s_carry.n = 0;
      s_acc[0] = s_acc[1] = 0;
    }
  __syncthreads();

  if (a.mode == DAMAR_PILE_COVER)
    { u64 act = 0;
      for (u32 c0 = 0; c0 < nev; c0 += PS_THREADS)
        { const u32  i  = c0 + t;
          const bool ok = i < nev;
          const u64  key = ok ? keys[i] : 0;
          const int  pos = (int) (key >> 1) & pmask;
          const int  span = s_carry.span + chunk_scan<int>(ok ? ((key & 1) ? 1 : -1) : 0, ibuf, OpAdd());
          if (ok && span > 0 && i + 1 < nev)
            act += (u64) (((int) (keys[i + 1] >> 1) & pmask) - pos);
          __syncthreads();
          if (t == PS_THREADS - 1) s_carry.span = span;
          __syncthreads();
        }
      if (act) atomicAdd((unsigned long long *) &s_acc[0], (unsigned long long) act);
      __syncthreads();
      if (t == 0) a.active[p] = (int) s_acc[0];
      return;
    }

  if (a.mode == DAMAR_PILE_TANDEM)
    { for (u32 c0 = 0; c0 < nev; c0 += PS_THREADS)
        { const u32  i  = c0 + t;
          const bool ok = i < nev;
          const u64  key = ok ? keys[i] : 0;
          const bool plus = ok && !(key & 1);
          const int  span = s_carry.span + chunk_scan<int>(ok ? (plus ? 1 : -1) : 0, ibuf, OpAdd());
          const bool emit = ok && (plus ? span == 1 : span == 0);
          const int  idx  = s_carry.n + chunk_scan<int>(emit ? 1 : 0, ibuf, OpAdd());
          if (emit) a.out[obase + (size_t) (idx - 1)] = (int) (key >> 1) & pmask;
          __syncthreads();
          if (t == PS_THREADS - 1)
            { s_carry.span = span;
              s_carry.n = idx;
            }
          __syncthreads();
        }
      if (t == 0) a.count[p] = (u32) s_carry.n;
      return;
    }

  /* DAMAR_PILE_REPEAT, LArepeat.c:327-413 */
  int *rb = a.rb + a.koff[p], *re = a.re + a.koff[p], *rc = a.rc + a.koff[p];
  for (u32 c0 = 0; c0 < nev; c0 += PS_THREADS)
    { const u32  i  = c0 + t;
      const bool ok = i < nev;
      const u64  key = ok ? keys[i] : 0;
      const int  pos = (int) (key >> 1) & pmask;
      const bool plus = ok && (key & 1);
      const Carry cy = s_carry;
      const int  span = cy.span + chunk_scan<int>(ok ? (plus ? 1 : -1) : 0, ibuf, OpAdd());
      const int  set  = !ok ? -1 : span > a.enter ? 1 : span < a.leave ? 0 : -1;
      const int  last = chunk_scan<int>(set >= 0 ? ((t << 1) | set) : -1, ibuf, OpMax());
      const int  state = last >= 0 ? (last & 1) : cy.state;
      s_state[t] = state;
      __syncthreads();
      const int  prev = t ? s_state[t - 1] : cy.state;
      const bool opens = ok && state && !prev, closes = ok && !state && prev;
      const int2 pk = chunk_scan<int2>(make_int2(opens ? 1 : 0, (plus && !opens) ? span : 0), s_buf, OpPeak());
      const int  peak = pk.x ? pk.y : (cy.peak > pk.y ? cy.peak : pk.y);
      const int  nopen = cy.n + chunk_scan<int>(opens ? 1 : 0, ibuf, OpAdd());
      if (opens) rb[nopen - 1] = pos;
      if (closes)
        { re[nopen - 1] = pos;
          rc[nopen - 1] = peak;
        }
      __syncthreads();
      if (t == PS_THREADS - 1)
        { s_carry.span = span;  s_carry.state = state;  s_carry.peak = peak;  s_carry.n = nopen; }
      __syncthreads();
    }
  const int  nreg = s_carry.n;
  const bool dangling = s_carry.state != 0;         /* open at the pile's last event: the reference has written its begin only */
  if (t == 0 && dangling) re[nreg - 1] = -1;
  __syncthreads();

  /* -m (:390-402): region i joins its predecessor when it begins less than merge_dist behind the predecessor's own end.
     The thread of a chain's first region walks the chain; a scan of the head flags numbers the chains. */
  const int width = 2 + (a.inccov ? 1 : 0);
  int nfinal = 0;
  u64 merged = 0, rbases = 0;
  for (int c0 = 0; c0 < nreg; c0 += PS_THREADS)
    { const int  i  = c0 + t;
      const bool ok = i < nreg;
      const bool head = ok && !(i > 0 && rb[i] - re[i - 1] < a.merge_dist);
      const int  f = nfinal + chunk_scan<int>(head ? 1 : 0, ibuf, OpAdd());
      if (head)
        { const int b0 = rb[i];
          int e = re[i], c = rc[i], j = i + 1;
          if (e >= 0) rbases += (u64) (e - b0);
          while (j < nreg && rb[j] - re[j - 1] < a.merge_dist)
            { merged += 1;
              e = re[j];
              if (e >= 0)
                { c = rc[j] > c ? rc[j] : c;
                  rbases += (u64) (e - b0);          /* :366: every closing counts from the chain's begin */
                }
              j += 1;
            }
          int *o = a.out + obase + (size_t) (f - 1) * width;
          o[0] = b0;
          if (e >= 0)
            { o[1] = e;
              if (a.inccov) o[2] = c;
            }
        }
      __syncthreads();
      if (t == PS_THREADS - 1) s_carry.n = f;
      __syncthreads();
      nfinal = s_carry.n;
    }
  if (merged) atomicAdd((unsigned long long *) &s_acc[0], (unsigned long long) merged);
  if (rbases) atomicAdd((unsigned long long *) &s_acc[1], (unsigned long long) rbases);
  __syncthreads();
  const int ncomplete = nfinal - (dangling ? 1 : 0);
  if (t == 0)
    { a.count[p] = (u32) (ncomplete * width + (dangling ? 1 : 0));
      if (s_acc[0]) atomicAdd((unsigned long long *) &a.stats[0], (unsigned long long) s_acc[0]);
      if (s_acc[1]) atomicAdd((unsigned long long *) &a.stats[1], (unsigned long long) s_acc[1]);
    }

  /* edge extension (:439-487).  The reference counts support over the FIRST kept RECORDS OF THE UNFILTERED PILE (novl is
     overwritten at :323, ovl + j indexed at :451, 472): kept here likewise. */
  const long long lo = a.pile_off[p];
  const int alen = a.read_len[a.pile_aread[p]];
  for (int f = 0; f < ncomplete; f++)
    { int *o = a.out + obase + (size_t) f * width;
      const int  rbv = o[0], rev = o[1];
      const bool c1 = rbv > 0 && rbv < PS_EDGE_DIST && rev < alen - PS_EDGE_DIST;
      const bool c2 = rev < alen - 1 && rev > alen - PS_EDGE_DIST && rbv > PS_EDGE_DIST;
      if (!c1 && !c2)
        continue;                                    /* uniform: every thread read the same two values */
      if (t == 0) s_sup[0] = s_sup[1] = 0;
      __syncthreads();
      int n1 = 0, n2 = 0;
      for (u32 j = t; j < kept; j += PS_THREADS)
        { const int ab = a.abpos[lo + j], ae = a.aepos[lo + j];
          n1 += (ae > rev - PS_EDGE_FUZZ && ae < rev + PS_EDGE_FUZZ && ab == 0) ? 1 : 0;
          n2 += (ab > rbv - PS_EDGE_FUZZ && ab < rbv + PS_EDGE_FUZZ && ae == alen) ? 1 : 0;
        }
      if (n1) atomicAdd(&s_sup[0], n1);
      if (n2) atomicAdd(&s_sup[1], n2);
      __syncthreads();
      if (t == 0)
        { if (c1 && s_sup[0] > 2) o[0] = 0;
          if (c2 && s_sup[1] > 2) o[1] = alen;
        }
      __syncthreads();
    }
}

/* the piles' ints, which lie at 3 * koff[p], back to back at doff[p] */
__global__ __launch_bounds__(PS_THREADS)
void pile_gather(const int *__restrict__ out, const u32 *__restrict__ koff, const u32 *__restrict__ count,
                 const u32 *__restrict__ doff, int *__restrict__ dst)
{ const u32 p = blockIdx.x, n = count[p];
  const int *src = out + 3 * (size_t) koff[p];
  int *d = dst + doff[p];
  for (u32 i = threadIdx.x; i < n; i += PS_THREADS)
    d[i] = src[i];
}

void damar_launch_pile_events(const PileArgs *a, hipStream_t st)
{ if (a->npiles == 0) return;
  hipLaunchKernelGGL(pile_events, dim3(a->npiles), dim3(PS_THREADS), 0, st, *a);
  HIP_CHECK(hipGetLastError());
}

void damar_launch_pile_sweep(const PileArgs *a, hipStream_t st)
{ if (a->npiles == 0) return;
  hipLaunchKernelGGL(pile_sweep, dim3(a->npiles), dim3(PS_THREADS), 0, st, *a);
  HIP_CHECK(hipGetLastError());
}

void damar_launch_pile_gather(const int *out, const u32 *koff, const u32 *count, const u32 *doff, u32 npiles, int *dst, hipStream_t st)
{ if (npiles == 0) return;
  hipLaunchKernelGGL(pile_gather, dim3(npiles), dim3(PS_THREADS), 0, st, out, koff, count, doff, dst);
  HIP_CHECK(hipGetLastError());
}
