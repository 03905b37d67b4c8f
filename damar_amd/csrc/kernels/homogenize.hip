/* homogenize.hip -- TKhomogenize's repeat intervals carried across overlaps, for gfx950 (scrub/TKhomogenize.c:346-546,
 * 193-226 and 230-321; the plain version is host/homogenize.c).
 *
 * The output is indexed by the B read, so the accumulator is a bit mask of the whole database that stays in HBM from one
 * batch of piles to the next; marking is atomicOr on its 32-bit words and does not depend on order.  Four kernels:
 *   hom_mark   a wavefront per record.  Lanes take the A read's intervals, 64 at a time and in the track's order: the
 *              reference's walk skips an interval shorter than 500 and STOPS at the first other one that begins behind the
 *              overlap, whatever follows it, so the first stopping lane (one ballot) cuts the chunk and ends the loop -- a
 *              binary search would only be right for a sorted track, which nothing promises.  The trace is not walked per
 *              interval: the A offset of segment j is closed-form (abpos for j = 0, (abpos / tw + j) * tw after that), so the
 *              segments of an interval's two ends are arithmetic, and the B offsets come from inclusive prefix sums of the
 *              trace's B lengths taken through the wave in chunks of 64 segments with a carry; each lane picks its two
 *              segments' sums out of the chunk they fall into with a shuffle.  Then the lanes of the wave share one
 *              projected range at a time: partial first word, full words, partial last word.
 *   hom_seed   -m: a wavefront per read sets the read's own long intervals with the same range function.
 *   hom_count  a wavefront per read counts the run starts of its mask words;
 *   hom_emit   after a scan of the counts, the same pass again writes every run's begin and end at its place.
 *
 * The one float step is done as the reference does it: a DOUBLE division tw / b rounded to float, then a FLOAT division
 * adiff / ratio, then truncation.  Both divisions must stay correctly rounded (IEEE): this file is compiled without
 * fast-math and without a relaxed-division switch, and the intrinsics below say so once more; an approximate reciprocal
 * would move a range by one base where the quotient lies next to an integer.
 * Wave size 64, plain C++ and vector atomics only.  Every bit index is held to its read's bits before a word is touched.
 */
#include "dev_common.h"
#include "kernels.h"

#define HM_THREADS 256
#define HM_WAVES   (HM_THREADS / WAVE)
#define HM_MAX_BLOCKS 65536u
#define HM_MIN_INT_LEN 500                /* TKhomogenize.c:49 */

/* the bits of a read that are read back (the spare one follows them) */
__device__ __forceinline__ int hom_alen(int rlen, int res)
{ return res > 1 ? (rlen + res - 1) / res : rlen; }

/* ba_assign_range(mask, beg, end, 1) (lib.ext/bitarr.c:263-284) by the whole wave: bits beg .. end inclusive, the single
   bit beg when end < beg.  A word that already holds all its bits is left alone: the plain read may be stale, which costs an
   atomic that changes nothing. */
__device__ __forceinline__ void wave_mark_range(u32 *words, int nbits, int beg, int end, int l)
{ if (end < beg) end = beg;
  if (beg < 0 || beg >= nbits) return;
  if (end >= nbits) end = nbits - 1;
  const int w0 = beg >> 5, w1 = end >> 5;
  for (int w = w0 + l; w <= w1; w += WAVE)
    { u32 m = 0xffffffffu;
      if (w == w0) m &= 0xffffffffu << (beg & 31);
      if (w == w1) m &= 0xffffffffu >> (31 - (end & 31));
      if ((words[w] & m) != m)
        atomicOr(&words[w], m);
    }
}

/* TKhomogenize.c:444-450 / 464-467 at segment j: the full spacing over the segment's B length even where the first segment
   is a partial one; a B length of 0 makes the ratio infinite and the offset 0 */
__device__ __forceinline__ int hom_project(int ab, int bb, int t0, int tw, int j, int bsum_excl, int blen_seg, int x, int bepos)
{ const int   aoff = (j == 0) ? ab : (t0 + j) * tw;
  const float ratio = (float) __ddiv_rn((double) tw, (double) blen_seg);
  const int   off = (int) __fdiv_rn((float) (x - aoff), ratio);
  const int   v = bb + bsum_excl + off;
  return v < bepos ? v : bepos;
}

__global__ __launch_bounds__(HM_THREADS)
void hom_mark(HomArgs a)
{ const int l = lane_id();
  const u32 nwaves = gridDim.x * HM_WAVES;
  const int tw = a.tspace, res = a.res;
  u32 marked = 0;                                 /* the same in all lanes */
  for (u32 r = blockIdx.x * HM_WAVES + (threadIdx.x >> 6); r < a.nrec; r += nwaves)
    { u32 lo = 0, hi = a.npiles;                  /* pile_off[lo] <= r < pile_off[hi]: the record's pile, empty piles skipped */
      while (hi - lo > 1)
        { const u32 mid = lo + (hi - lo) / 2;
          if (a.pile_off[mid] <= (long long) r) lo = mid; else hi = mid;
        }
      const int ar = a.pile_aread[lo], br = a.bread[r];
      const int nseg = a.tlen[r] >> 1;
      if (ar == br || nseg == 0)                  /* OVL_DISCARD is not looked at */
        continue;
      const int  ab = a.abpos[r], ae = a.aepos[r], bb = a.bbpos[r], be = a.bepos[r];
      const bool comp = (a.flags[r] & 1) != 0;
      const int  blen = a.read_len[br];
      const int  nbits = hom_alen(blen, res) + 1;
      const int  t0 = ab / tw;
      const u64  ob = a.iv_anno[ar] >> 2, oe = a.iv_anno[ar + 1] >> 2;
      const int  nint = (int) ((oe - ob) >> 1);
      const int *iv = a.iv_data + ob;
      const u8  *tr = a.trace + a.trace_off[r];
      u32       *words = a.words + a.woff[br];
      int trim_b = 0, trim_e = blen;
      if (a.trim != NULL)
        { trim_b = a.trim[2 * (size_t) br];
          trim_e = a.trim[2 * (size_t) br + 1];
        }
      for (int base = 0; base < nint; base += WAVE)
        { const int  k = base + l;
          const bool have = k < nint;
          const int  beg = have ? iv[2 * k] : 0, end = have ? iv[2 * k + 1] : 0;
          const bool lng = have && (long long) end - beg >= HM_MIN_INT_LEN;
          const u64  stop = wballot(lng && beg > ae);
          const bool before = stop == 0 || l < __ffsll((long long) stop) - 1;
          const int  iab = beg > ab ? beg : ab, iae = end < ae ? end : ae;
          const int  jb = (iab - ab <= tw) ? 0 : (iab + tw - 1) / tw - 1 - t0;     /* the first j with aoff_j + tw >= iab */
          const int  je = (iae - ab <= tw) ? 0 : (iae + tw - 1) / tw - 1 - t0;
          const bool act = lng && before && iab < iae && je < nseg;                /* jb <= je: a trace too short for iae yields nothing */
          u64 am = wballot(act);
          if (am != 0)
            { const int jmax = wave_max_i(act ? je : -1);
              int carry = 0, ibb = 0, ibe = 0;
              for (int c = 0; c <= jmax; c += WAVE)
                { const int s = c + l;
                  int bl = 0;
                  if (s < nseg)
                    bl = (a.tbytes == 1) ? (int) tr[2 * (size_t) s + 1]
                                         : (int) tr[4 * (size_t) s + 2] | ((int) tr[4 * (size_t) s + 3] << 8);
                  const int incl = wave_incl_scan_i(bl) + carry;
                  carry = __shfl(incl, WAVE - 1);
                  const int sb = (jb - c) & (WAVE - 1), se = (je - c) & (WAVE - 1);
                  const int pb = __shfl(incl, sb), lb = __shfl(bl, sb);
                  const int pe = __shfl(incl, se), le = __shfl(bl, se);
                  if (act && jb >= c && jb < c + WAVE)
                    ibb = hom_project(ab, bb, t0, tw, jb, pb - lb, lb, iab, be);
                  if (act && je >= c && je < c + WAVE)
                    ibe = hom_project(ab, bb, t0, tw, je, pe - le, le, iae, be);
                }
              if (comp)
                { const int t = ibb;
                  ibb = blen - ibe;
                  ibe = blen - t;
                }
              while (am != 0)                      /* one range at a time, all lanes on its words */
                { const int src = __ffsll((long long) am) - 1;
                  am &= am - 1;
                  const int rb = __shfl(ibb, src), re = __shfl(ibe, src);
                  if (a.ends == -1)
                    { wave_mark_range(words, nbits, (rb + res - 1) / res, re / res, l);
                      marked += 1;
                    }
                  else
                    { if (rb < a.ends + trim_b)
                        { const int cut = a.ends + trim_b < re ? a.ends + trim_b : re;
                          wave_mark_range(words, nbits, (rb + res - 1) / res, cut / res, l);
                          marked += 1;
                        }
                      if (re > trim_e - a.ends)
                        { const int from = trim_e - a.ends > rb ? trim_e - a.ends : rb;
                          wave_mark_range(words, nbits, (from + res - 1) / res, re / res, l);
                          marked += 1;
                        }
                    }
                }
            }
          if (stop != 0)
            break;
        }
    }
  if (l == 0 && marked != 0)
    atomicAdd(a.nranges, (u64) marked);
}

/* TKhomogenize.c:193-226 */
__global__ __launch_bounds__(HM_THREADS)
void hom_seed(HomArgs a)
{ const int l = lane_id();
  const u32 nwaves = gridDim.x * HM_WAVES;
  u32 marked = 0;
  for (u32 r = blockIdx.x * HM_WAVES + (threadIdx.x >> 6); r < a.nreads; r += nwaves)
    { const u64 ob = a.iv_anno[r] >> 2, oe = a.iv_anno[r + 1] >> 2;
      const int nbits = hom_alen(a.read_len[r], a.res) + 1;
      u32 *words = a.words + a.woff[r];
      for (u64 k = ob; k + 1 < oe; k += 2)
        { const int beg = a.iv_data[k], end = a.iv_data[k + 1];
          if ((long long) end - beg < HM_MIN_INT_LEN)
            continue;
          wave_mark_range(words, nbits, (beg + a.res - 1) / a.res, end / a.res, l);
          marked += 1;
        }
    }
  if (l == 0 && marked != 0)
    atomicAdd(a.nranges, (u64) marked);
}

/* TKhomogenize.c:243-310: the runs of set bits among a read's bits 0 .. alen - 1.  A run [j0, j1] is written as
   (j0 * res, min(j1 * res, rlen)); one that reaches the last bit as (j0 * res, rlen - 1). */
template <int EMIT>
__global__ __launch_bounds__(HM_THREADS)
void hom_readout(HomArgs a)
{ const int l = lane_id();
  const u32 nwaves = gridDim.x * HM_WAVES;
  for (u32 r = blockIdx.x * HM_WAVES + (threadIdx.x >> 6); r < a.nreads; r += nwaves)
    { const int rlen = a.read_len[r], alen = hom_alen(rlen, a.res);
      const int nw = (alen + 31) >> 5;
      const u32 last = (alen & 31) ? (1u << (alen & 31)) - 1u : 0xffffffffu;       /* the spare bit and what follows it are not read */
      const u32 *words = a.words + a.woff[r];
      int *out = EMIT ? a.out + 2 * (size_t) a.off[r] : NULL;
      int nstart = 0, nend = 0;
      for (int c = 0; c < nw; c += WAVE)
        { const int w = c + l;
          u32 v = 0, prev = 0, next = 0;
          if (w < nw)
            { v = words[w] & (w == nw - 1 ? last : 0xffffffffu);
              if (w > 0) prev = words[w - 1];
              if (w + 1 < nw) next = words[w + 1] & (w + 1 == nw - 1 ? last : 0xffffffffu);
            }
          u32 s = v & ~((v << 1) | (prev >> 31));
          if (!EMIT)
            nstart += __popc(s);
          else
            { u32 e = v & ~((v >> 1) | (next << 31));
              const int ps = __popc(s), pe = __popc(e);
              const int is = wave_incl_scan_i(ps), ie = wave_incl_scan_i(pe);
              int ks = nstart + is - ps, ke = nend + ie - pe;
              while (s != 0)
                { const int j0 = 32 * w + __ffs((int) s) - 1;
                  s &= s - 1;
                  out[2 * (size_t) ks++] = j0 * a.res;
                }
              while (e != 0)
                { const int j1 = 32 * w + __ffs((int) e) - 1;
                  e &= e - 1;
                  const long long at = (long long) j1 * a.res;
                  out[2 * (size_t) ke++ + 1] = (j1 == alen - 1) ? rlen - 1 : (int) (at < rlen ? at : rlen);
                }
              nstart += __shfl(is, WAVE - 1);
              nend += __shfl(ie, WAVE - 1);
            }
        }
      if (!EMIT)
        { const int total = wave_sum_i(nstart);
          if (l == 0) a.count[r] = (u32) total;
        }
    }
}

static u32 blocks_for(u32 n)
{ const u32 b = (n + HM_WAVES - 1) / HM_WAVES;
  return b < 1 ? 1 : (b > HM_MAX_BLOCKS ? HM_MAX_BLOCKS : b);
}

void damar_launch_hom_mark(const HomArgs *a, hipStream_t st)
{ if (a->nrec > 0)
    hipLaunchKernelGGL(hom_mark, dim3(blocks_for(a->nrec)), dim3(HM_THREADS), 0, st, *a);
}

void damar_launch_hom_seed(const HomArgs *a, hipStream_t st)
{ if (a->nreads > 0)
    hipLaunchKernelGGL(hom_seed, dim3(blocks_for(a->nreads)), dim3(HM_THREADS), 0, st, *a);
}

void damar_launch_hom_count(const HomArgs *a, hipStream_t st)
{ if (a->nreads > 0)
    hipLaunchKernelGGL(hom_readout<0>, dim3(blocks_for(a->nreads)), dim3(HM_THREADS), 0, st, *a);
}

void damar_launch_hom_emit(const HomArgs *a, hipStream_t st)
{ if (a->nreads > 0)
    hipLaunchKernelGGL(hom_readout<1>, dim3(blocks_for(a->nreads)), dim3(HM_THREADS), 0, st, *a);
}
