/* pile_patch.hip -- LAfix's search per pile for gfx950: the breaks between two records of one B read, and for every weak
 * segment of the A read the B stretch that replaces it (scrub/LAfix.c:1896-2402 of fix_process, :1413 spanners_point; the
 * plain version is host/fix.c damar_host_fix_pile).
 *
 * One wavefront per pile, one wavefront per workgroup.  LDS of a workgroup, 48 KiB, so three piles are resident on a CU:
 *   s_q     int[DAMAR_FIX_MAXSEGS]       the A read's q values, one per segment
 *   s_g     int[DAMAR_FIX_MAXREP][8]     the candidate list (DAMAR_FIX_MAXCAND of it), later the repairs: a damar_fix_gap each
 *   breaks  a lane per pair of neighbouring records, 64 pairs a step.  A lane takes its pair through the tests that need only
 *           the pair and B's q; then, one surviving pair after the other, all lanes count the records across the two borders
 *           (wave sums -- the reference stops counting beyond maxspanners, which changes nothing of the answer); the lane goes
 *           on with the tests on A's q and its pair is appended in pair order, the place from a ballot.
 *   merges  lane 0 alone over s_g: a stable insertion sort by (ab, ae, diff), the -g cut, the two merges, the support and
 *           bad-segment filters.  These depend on the order candidates are met in and are few.
 *   weak    the bad segments of the trimmed read one after the other, the same in all lanes.  Lanes stride over the records; a
 *           record across the segment walks its trace to it, sums B's q, and the wave takes the minimum over (q_new as float
 *           bits, record index) by two reductions, so among equals the lowest index wins as in the reference's loop; support
 *           is a wave sum.  The winning lane appends the repair.
 *   order   lane 0 sorts the list again (stable), then the lanes copy it out.
 * diff and q_new are computed with the reference's operations: double arithmetic, the quotient narrowed to float for q_new
 * and cut to int for diff; q_new > 0 always, so its bits order as it does.
 * B's q is indexed flat into the track's data, an index outside counts as 0 (q_at).  The trace walk never passes tlen.
 * A pile on a read of more than maxsegs segments, one marked by the host, one with more than DAMAR_FIX_MAXCAND candidates
 * and one with more than DAMAR_FIX_MAXREP repairs is left to the host: status 1, its other outputs are not to be looked at. */
#include "dev_common.h"
#include "damar_hip.h"
#include "kernels.h"

#define PP_THREADS 64
#define PP_MAX_BLOCKS 65536u
#define PP_MIN_SPAN 400                   /* LAfix.c:42-43 */
#define PP_MIN_SPAN_REPEAT 800
#define F_COMP 0x1                        /* lib/oflags.h */
#define G_INTS 8                          /* damar_fix_gap: ab ae bb be diff b support comp */
enum { G_AB = 0, G_AE, G_BB, G_BE, G_DIFF, G_B, G_SUP, G_COMP };
#define NONE 0x7fffffff

__device__ __forceinline__ void wave_lds_sync()
{ __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ int q_at(const FixArgs &a, long long base, long long k)
{ const long long at = base + k;
  return (at < 0 || at >= a.q_ndata) ? 0 : a.q_data[at];
}

__device__ __forceinline__ int trace_at(const FixArgs &a, const u8 *tr, int k)
{ return a.tbytes == 1 ? (int) tr[k] : ((int) tr[2 * (size_t) k] | ((int) tr[2 * (size_t) k + 1] << 8));
}

/* getRepeatCount(aread, pt, pt + 1) != 0: the same in all lanes, every lane walks the read's few intervals */
__device__ __forceinline__ int min_span_at(const FixArgs &a, int aread, int pt)
{ if (a.rep_anno == NULL)
    return PP_MIN_SPAN;
  int n = 0;
  for (u64 rb = a.rep_anno[aread] / 4, re = a.rep_anno[aread + 1] / 4; rb < re; rb += 2)
    { const int lo = pt > a.rep_data[rb] ? pt : a.rep_data[rb], hi = pt + 1 < a.rep_data[rb + 1] ? pt + 1 : a.rep_data[rb + 1];
      if (lo < hi)
        n += hi - lo;
    }
  return n ? PP_MIN_SPAN_REPEAT : PP_MIN_SPAN;
}

__device__ __forceinline__ bool gap_before(const int *x, const int *y)
{ if (x[G_AB] != y[G_AB]) return x[G_AB] < y[G_AB];
  if (x[G_AE] != y[G_AE]) return x[G_AE] < y[G_AE];
  return x[G_DIFF] < y[G_DIFF];
}

/* one lane: the stable insertion sort of host/fix.c sort_gaps */
__device__ void sort_gaps(int (*g)[G_INTS], int n)
{ for (int i = 1; i < n; i++)
    { int x[G_INTS];
      for (int c = 0; c < G_INTS; c++) x[c] = g[i][c];
      int j = i;
      for (; j > 0 && gap_before(x, g[j - 1]); j--)
        for (int c = 0; c < G_INTS; c++) g[j][c] = g[j - 1][c];
      for (int c = 0; c < G_INTS; c++) g[j][c] = x[c];
    }
}

__global__ __launch_bounds__(PP_THREADS)
void pile_patch(FixArgs a)
{ __shared__ int s_q[DAMAR_FIX_MAXSEGS];
  __shared__ int s_g[DAMAR_FIX_MAXREP][G_INTS];
  __shared__ int s_n;
  const int l = lane_id();
  const int tw = a.tspace;
  for (u32 p = blockIdx.x; p < a.npiles; p += gridDim.x)
    { const long long lo = a.pile_off[p];
      const int n = (int) (a.pile_off[p + 1] - lo);
      const int aread = a.pile_aread[p];
      const int trim_ab = a.trim[2 * (size_t) p], trim_ae = a.trim[2 * (size_t) p + 1];
      const int nsegs = (a.read_len[aread] + tw - 1) / tw;
      if (trim_ab >= trim_ae)
        { if (l == 0)
            { a.status[p] = 0;
              a.ngaps[p] = 0;
            }
          continue;
        }
      if (a.skip[p] || nsegs > a.maxsegs || nsegs > DAMAR_FIX_MAXSEGS)
        { if (l == 0) a.status[p] = 1;
          continue;
        }
      const int *ab = a.abpos + lo, *ae = a.aepos + lo, *bb = a.bbpos + lo, *be = a.bepos + lo, *br = a.bread + lo, *fl = a.flags + lo;
      const int *tl = a.tlen + lo;
      const long long *toff = a.trace_off + lo;
      const long long qa = (long long) (a.q_anno[aread] / 4);
      const int room = (int) (a.slot_off[p + 1] - a.slot_off[p]);
      wave_lds_sync();
      for (int i = l; i < nsegs; i += WAVE)
        s_q[i] = q_at(a, qa, i);
      wave_lds_sync();
      #define QA(k) (((k) >= 0 && (k) < nsegs) ? s_q[(k)] : q_at(a, qa, (k)))

      /* the breaks */
      int ncand = 0, over = 0;
      for (int base = 1; base < n && !over; base += WAVE)
        { const int s = base + l;
          bool live = s < n && br[s - 1] == br[s] && ae[s - 1] < ab[s] && !((fl[s - 1] ^ fl[s]) & F_COMP);
          int sa = 0, se = 0, gb = 0, ge = 0, q = 0;
          if (live)
            { sa = (ae[s - 1] - 1) / tw;
              se = ab[s] / tw + 1;
              gb = be[s - 1] - trace_at(a, a.trace + toff[s - 1], tl[s - 1] - 1);
              ge = bb[s] + trace_at(a, a.trace + toff[s], 1);
              live = gb < ge;
            }
          if (live)
            { if (fl[s] & F_COMP)
                { const int blen = a.read_len[br[s]], was = gb;
                  gb = blen - ge;
                  ge = blen - was;
                }
              const long long qb = (long long) (a.q_anno[br[s]] / 4);
              for (int k = gb / tw, end = ge / tw + 1; k < end; k++)
                { const int v = q_at(a, qb, k);
                  if (v == 0)
                    live = false;
                  q += v;
                }
            }
          /* the records across the two borders of every pair that is still there, counted by the whole wave */
          u64 todo = wballot(live);
          bool both = false;
          while (todo != 0)
            { const int w = __ffsll((unsigned long long) todo) - 1;
              todo &= todo - 1;
              const int p1 = __shfl(sa, w) * tw, p2 = __shfl(se, w) * tw;
              const int m1 = min_span_at(a, aread, p1), m2 = min_span_at(a, aread, p2);
              int c1 = 0, c2 = 0;
              for (int i = l; i < n; i += WAVE)
                { c1 += (ab[i] < p1 - m1 && ae[i] > p1 + m1) ? 1 : 0;
                  c2 += (ab[i] < p2 - m2 && ae[i] > p2 + m2) ? 1 : 0;
                }
              c1 = wave_sum_i(c1);
              c2 = wave_sum_i(c2);
              if (l == w)
                both = c1 > a.maxspanners && c2 > a.maxspanners;
            }
          if (live && both)
            live = false;
          if (live)
            { int scored = 0;
              for (int k = sa + 1; k < se - 1; k++)
                scored += QA(k) != 0 ? 1 : 0;
              if (scored > 1 || (se - sa) * tw * 10 < ge - gb)
                live = false;
            }
          const u64 keep = wballot(live);
          const int at = ncand + __popcll((unsigned long long) (keep & lanes_below(l)));
          const int more = __popcll((unsigned long long) keep);
          if (ncand + more > DAMAR_FIX_MAXCAND)
            { over = 1;
              break;
            }
          if (live)
            { s_g[at][G_AB] = sa * tw;  s_g[at][G_AE] = se * tw;  s_g[at][G_BB] = gb;  s_g[at][G_BE] = ge;
              s_g[at][G_DIFF] = (int) ((double) tw * 1.0 * (double) q / (double) (ge - gb));
              s_g[at][G_B] = br[s];  s_g[at][G_SUP] = 1;  s_g[at][G_COMP] = fl[s] & F_COMP;
            }
          ncand += more;
        }
      if (over)
        { if (l == 0) a.status[p] = 1;
          continue;
        }
      wave_lds_sync();

      /* sort, cut, merge, filter: one lane, in the reference's order */
      if (l == 0)
        { sort_gaps(s_g, ncand);
          for (int i = 0; i < ncand; i++)
            { if (s_g[i][G_SUP] == -1)
                continue;
              const int la = s_g[i][G_AE] - s_g[i][G_AB], lb = s_g[i][G_BE] - s_g[i][G_BB];
              if (a.maxgap != -1 && (la >= a.maxgap || (lb < 0 ? -lb : lb) >= a.maxgap))
                { s_g[i][G_SUP] = -1;
                  continue;
                }
              for (int j = i + 1; j < ncand && s_g[i][G_AB] == s_g[j][G_AB] && s_g[i][G_AE] == s_g[j][G_AE]; j++)
                { if (s_g[j][G_SUP] == -1)
                    continue;
                  const int d = (s_g[j][G_BE] - s_g[j][G_BB]) - lb;
                  if ((d < 0 ? -d : d) < 50)
                    { s_g[i][G_SUP] += 1;
                      s_g[j][G_SUP] = -1;
                    }
                }
            }
          for (int i = 0; i < ncand; i++)
            { if (s_g[i][G_SUP] == -1)
                continue;
              for (int j = i + 1; j < ncand && s_g[i][G_AE] > s_g[j][G_AB] && s_g[i][G_AB] < s_g[j][G_AE]; j++)
                { if (s_g[j][G_SUP] == -1)
                    continue;
                  if (s_g[i][G_SUP] > s_g[j][G_SUP])
                    { s_g[i][G_SUP] += s_g[j][G_SUP];
                      s_g[j][G_SUP] = -1;
                    }
                  else
                    { s_g[j][G_SUP] += s_g[i][G_SUP];
                      s_g[i][G_SUP] = -1;
                      break;
                    }
                }
            }
          int kept = 0;
          for (int i = 0; i < ncand; i++)
            { if (s_g[i][G_SUP] < a.minsupport)
                continue;
              bool bad = false;
              for (int k = s_g[i][G_AB] / tw; k < s_g[i][G_AE] / tw && !bad; k++)
                { const int v = QA(k);
                  bad = v == 0 || v >= a.lowq;
                }
              if (!bad)
                continue;
              for (int c = 0; c < G_INTS; c++) s_g[kept][c] = s_g[i][c];
              kept += 1;
            }
          s_n = kept;
        }
      wave_lds_sync();
      int cur = s_n;

      /* the weak segments */
      int seg_first = trim_ab / tw, seg_last = trim_ae / tw;
      while (seg_first < nsegs && QA(seg_first) == 0)
        seg_first += 1;
      while (seg_last > 0 && QA(seg_last - 1) == 0)
        seg_last -= 1;
      for (int s = seg_first; s < seg_last && !over; s++)
        { const int v = QA(s), wa = s * tw, we = (s + 1) * tw;
          if (v != 0 && v < a.lowq)
            continue;
          bool inside = false;
          for (int j = 0; j < cur && !inside; j++)
            inside = s_g[j][G_SUP] != -1 && s_g[j][G_AB] <= wa && s_g[j][G_AE] >= we;
          if (inside)
            continue;
          int border = 0, best = NONE, best_bits = NONE, best_bb = 0, best_be = 0;
          for (int r = l; r < n; r += WAVE)
            { const int rab = ab[r], rae = ae[r];
              if ((rab >= wa && rab <= we) || (rae >= wa && rae <= we))
                border += 1;
              if (!(rab + tw <= wa && rae - tw >= we))
                continue;
              const u8 *tr = a.trace + toff[r];
              int gb = -1, ge = bb[r], apos = rab, k = 0;
              while (apos <= wa && k + 1 < tl[r])
                { apos = (apos / tw + 1) * tw;
                  gb = ge;
                  ge += trace_at(a, tr, k + 1);
                  k += 2;
                }
              if (fl[r] & F_COMP)
                { const int blen = a.read_len[br[r]], was = gb;
                  gb = blen - ge;
                  ge = blen - was;
                }
              const long long qb = (long long) (a.q_anno[br[r]] / 4);
              const int beg = gb / tw, end = ge / tw;
              int q = 0;
              for (k = beg; k < end; k++)
                { const int w = q_at(a, qb, k);
                  if (w == 0)
                    { q = 0;
                      break;
                    }
                  q += w;
                }
              if (q == 0)
                continue;
              const float q_new = (float) (1.0 * (double) q / (double) (end - beg));
              const int bits = __float_as_int(q_new);
              if (best == NONE || bits < best_bits)
                { best = r;  best_bits = bits;  best_bb = gb;  best_be = ge; }
            }
          const int win_bits = wave_min_i(best_bits);
          const int win = wave_min_i(best_bits == win_bits ? best : NONE);
          border = wave_sum_i(border);
          if (win == NONE)
            continue;
          if (cur >= DAMAR_FIX_MAXREP)
            { over = 1;
              break;
            }
          if (best == win)             /* one lane: a record belongs to one lane */
            { s_g[cur][G_AB] = wa;  s_g[cur][G_AE] = we;  s_g[cur][G_BB] = best_bb;  s_g[cur][G_BE] = best_be;
              s_g[cur][G_DIFF] = (int) __int_as_float(best_bits);
              s_g[cur][G_B] = br[win];  s_g[cur][G_SUP] = border;  s_g[cur][G_COMP] = fl[win] & F_COMP;
            }
          cur += 1;
          wave_lds_sync();
        }
      #undef QA
      if (over || cur > room)
        { if (l == 0) a.status[p] = 1;
          continue;
        }
      wave_lds_sync();
      if (l == 0)
        sort_gaps(s_g, cur);
      wave_lds_sync();
      int *dst = a.gaps + (size_t) a.slot_off[p] * G_INTS;
      for (int i = l; i < cur * G_INTS; i += WAVE)
        dst[i] = s_g[i / G_INTS][i % G_INTS];
      if (l == 0)
        { a.status[p] = 0;
          a.ngaps[p] = cur;
        }
    }
}

void damar_launch_pile_patch(const FixArgs *a, hipStream_t st)
{ if (a->npiles == 0)
    return;
  const u32 blocks = a->npiles < PP_MAX_BLOCKS ? a->npiles : PP_MAX_BLOCKS;
  hipLaunchKernelGGL(pile_patch, dim3(blocks), dim3(PP_THREADS), 0, st, *a);
}
