/* pile_gaps.hip -- LAgap's per-pile work for gfx950: containments dropped, the coverage of the remaining records counted
 * over bins of 100 bases, and every run of thin bins turned into an event (scrub/LAgap.c:1782-1871 drop_containments,
 * :1616-1780 handle_gaps_and_breaks, :159-238 drop_break, :300-354 stitchable; the plain version is host/gap.c
 * damar_host_gap_pile).
 *
 * One wavefront per pile, one wavefront per workgroup, the bins in the workgroup's LDS:
 *   groups    the records of one B read are a run (the shim hands piles whose B reads do not ascend to the host).  The
 *             lane whose record begins a run walks the run alone, in the reference's order: the containment pairs, then
 *             the OVL_TEMP marks, then each record that is left adds +1 / -1 to a difference array over the bins (LDS
 *             atomics).  Runs are met 64 records at a time, so a pile of any number of B reads takes the same path.
 *   bins      the difference array summed in place, 64 bins a step with the carry handed on; the first and last covered
 *             base from two wave reductions.
 *   breaks    the bins scanned 64 at a time through ballots; the state (a run is open since bin `beg`) is the same in all
 *             lanes.  Per break: the exclude intervals and the stitchable pairs looked at with the lanes over intervals and
 *             records, the pile's longest live record found by two reductions (length, then the lowest index of that
 *             length), the drop done with the lanes over the records.  Breaks are taken one after the other, since a drop
 *             changes which record is the longest for the next.
 * The flags word of a record is read and written by its own pile's wavefront alone, but by different lanes of it in the
 * different phases: those accesses go past the vector L1 (agent scope), with the wave's memory operations drained between
 * the phases.  Every bin index is held inside the pile's bins whatever the coordinates claim.
 * A pile on a read of more bins than `maxbins`, one marked by the host, and one with more events than `maxev` is left to
 * the host: status 1, its other outputs are not to be looked at. */
#include "dev_common.h"
#include "damar_hip.h"
#include "kernels.h"

#define PG_THREADS 64
#define PG_MAX_BLOCKS 65536u
#define PG_BIN   100                      /* LAgap.c:33-34 */
#define PG_MINLR 450

#define F_COMP    0x1                     /* lib/oflags.h */
#define F_DISCARD 0x2
#define F_STITCH  0x80
#define F_TEMP    0x800
#define F_CONT    0x8000
#define F_GAP     0x10000
#define F_TRIM    0x20000

__device__ __forceinline__ void wave_lds_sync()
{ __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ int  ldf(const int *p)      { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void stf(int *p, int v)     { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int contained(int ab, int ae, int bb, int be)
{ if (ab >= bb && ae <= be) return 1;
  if (bb >= ab && be <= ae) return 2;
  return 0;
}

/* drop_break (LAgap.c:159-238) with the lanes over the pile's n records: the longest live record decides the side, the
   first of that length (two reductions: the length, then the lowest index of it).  Returns the kind, *d the records that
   were live and are dropped now.  The same in all lanes; the drop is visible to every lane afterwards. */
__device__ __forceinline__ int drop_break(int l, int n, const int *ab, const int *ae, int *fl, int p1, int p2, int *d)
{ int bl = 0, bi = 0x7fffffff, gone = 0;
  for (int i = l; i < n; i += WAVE)
    { if (ldf(&fl[i]) & F_DISCARD)
        continue;
      const int len = ae[i] - ab[i];
      if (len > bl) { bl = len; bi = i; }
    }
  const int m = wave_max_i(bl);
  const int idx = wave_min_i(bl == m ? bi : 0x7fffffff);
  *d = 0;
  if (m == 0)
    return DAMAR_GAP_DROP_NONE;
  const bool left = ab[idx] < p1;
  for (int i = l; i < n; i += WAVE)
    { const int fi = ldf(&fl[i]);
      if (!left ? ab[i] < p1 : (!(fi & F_DISCARD) && ae[i] > p2))
        { gone += (fi & F_DISCARD) ? 0 : 1;
          stf(&fl[i], fi | F_DISCARD | F_GAP);
        }
    }
  *d = wave_sum_i(gone);
  wave_mem_sync();
  return left ? DAMAR_GAP_DROP_R : DAMAR_GAP_DROP_L;
}

/* event number nev of pile p into its slot; 1 when the slot is full (the pile is the host's then) */
__device__ __forceinline__ int put_event(const GapArgs &a, u32 p, int l, int nev, int beg, int b, int kind, int v0, int v1, int d)
{ if (nev >= a.maxev || nev >= DAMAR_GAP_MAXEVENTS)
    return 1;
  if (l == 0)
    { int *e = a.ev + ((size_t) p * DAMAR_GAP_MAXEVENTS + (size_t) nev) * DAMAR_GAP_EVENT_INTS;
      e[0] = beg;  e[1] = b;  e[2] = kind;  e[3] = v0;  e[4] = v1;  e[5] = d;
    }
  return 0;
}

__global__ __launch_bounds__(PG_THREADS)
void pile_gaps(GapArgs a)
{ __shared__ int s_bins[DAMAR_GAP_MAXBINS + WAVE];
  const int l = lane_id();
  for (u32 p = blockIdx.x; p < a.npiles; p += gridDim.x)
    { const long long lo = a.pile_off[p];
      const int n = (int) (a.pile_off[p + 1] - lo);
      const int aread = a.pile_aread[p];
      const int nb = (a.read_len[aread] + PG_BIN) / PG_BIN;
      if (a.skip[p] || nb > a.maxbins || nb > DAMAR_GAP_MAXBINS || nb < 1)
        { if (l == 0) a.status[p] = 1;
          continue;
        }
      const int *ab = a.abpos + lo, *ae = a.aepos + lo, *bb = a.bbpos + lo, *be = a.bepos + lo, *br = a.bread + lo;
      int *fl = a.flags_out + lo;
      const int nbr = (nb + WAVE) & ~(WAVE - 1);           /* nb + 1 entries, rounded up to whole steps of the scan */
      for (int i = l; i < n; i += WAVE)
        stf(&fl[i], a.flags[lo + i]);
      for (int i = l; i < nbr; i += WAVE)
        s_bins[i] = 0;
      wave_mem_sync();
      wave_lds_sync();

      /* the runs of one B read: containments, OVL_TEMP, coverage */
      int tb = 0x7fffffff, te = 0, gone = 0;
      for (int base = 0; base < n; base += WAVE)
        { const int i0 = base + l;
          if (i0 >= n || (i0 > 0 && br[i0] == br[i0 - 1]))
            continue;
          const int bread = br[i0], blen = a.read_len[bread];
          int g1 = i0 + 1;
          while (g1 < n && br[g1] == bread) g1++;
          if (bread != aread)
            for (int i = i0; i < g1; i++)
              { int fi = ldf(&fl[i]);
                if (fi & F_DISCARD)
                  continue;
                const int ab1 = ab[i], ae1 = ae[i];
                const int bb1 = (fi & F_COMP) ? blen - be[i] : bb[i], be1 = (fi & F_COMP) ? blen - bb[i] : be[i];
                for (int k = i + 1; k < g1; k++)
                  { const int fk = ldf(&fl[k]);
                    if (fk & F_DISCARD)
                      continue;
                    const int bb2 = (fk & F_COMP) ? blen - be[k] : bb[k], be2 = (fk & F_COMP) ? blen - bb[k] : be[k];
                    const int cont = contained(ab1, ae1, ab[k], ae[k]);
                    if (cont && contained(bb1, be1, bb2, be2))
                      { gone += 1;
                        if (cont == 1)
                          { stf(&fl[i], fi | F_DISCARD | F_CONT);
                            break;
                          }
                        stf(&fl[k], fk | F_DISCARD | F_CONT);
                      }
                  }
              }
          if (bread != aread)
            for (int i = i0; i < g1; i++)
              { int fi = ldf(&fl[i]);
                if (fi & F_DISCARD)
                  continue;
                const int ab1 = ab[i], ae1 = ae[i];
                for (int j = i + 1; j < g1; j++)
                  { const int ib = ab1 > ab[j] ? ab1 : ab[j], ie = ae1 < ae[j] ? ae1 : ae[j];
                    if (ib < ie)
                      { if (ae1 - ab1 < ae[j] - ab[j])
                          { fi |= F_TEMP;
                            stf(&fl[i], fi);
                          }
                        else
                          stf(&fl[j], ldf(&fl[j]) | F_TEMP);
                      }
                  }
                if (fi & F_TEMP)
                  continue;
                tb = ab1 < tb ? ab1 : tb;
                te = ae1 > te ? ae1 : te;
                int b = (ab1 + PG_MINLR) / PG_BIN, e = (ae1 - PG_MINLR) / PG_BIN;
                b = b < 0 ? 0 : b;
                e = e > nb ? nb : e;
                if (b < e)
                  { atomicAdd(&s_bins[b], 1);
                    atomicAdd(&s_bins[e], -1);
                  }
              }
        }
      wave_mem_sync();
      wave_lds_sync();
      gone = wave_sum_i(gone);
      tb = wave_min_i(tb);
      te = wave_max_i(te);

      int nev = 0, breaks = 0, dropped = 0, over = 0;
      if (tb < te)
        { int carry = 0;
          for (int base = 0; base < nbr; base += WAVE)
            { const int inc = wave_incl_scan_i(s_bins[base + l]) + carry;
              s_bins[base + l] = inc;
              carry = bcast_i(inc, WAVE - 1);
            }
          wave_lds_sync();

          const int b0 = (tb + PG_MINLR) / PG_BIN;
          int e0 = (te - PG_MINLR) / PG_BIN;
          e0 = e0 > nb ? nb : e0;
          int beg = -1;
          for (int base = b0; base < e0 && !over; base += WAVE)
            { const int  bin = base + l;
              const bool in = bin < e0;
              const u64  vm = wballot(in), lm = wballot(in && s_bins[bin] <= 1);
              int pos = 0;
              while (pos < WAVE && !over)
                { const u64 rest = (beg == -1 ? lm : (vm & ~lm)) & (~0ull << pos);
                  if (rest == 0)
                    break;
                  const int q = __ffsll((unsigned long long) rest) - 1;
                  pos = q + 1;
                  if (beg == -1)
                    { beg = base + q;
                      continue;
                    }
                  /* a break: bins beg .. b - 1 are thin, bin b is not */
                  const int b = base + q, p1 = (beg - 1) * PG_BIN, p2 = (b + 1) * PG_BIN;
                  int kind = -1, v0 = 0, v1 = 0, d = 0;
                  if (a.ex_anno != NULL)
                    { const u64 t0 = a.ex_anno[aread] / 4, t1 = a.ex_anno[aread + 1] / 4;
                      const int npair = (int) ((t1 - t0) / 2);
                      int best = 0x7fffffff;
                      for (int j = l; j < npair; j += WAVE)
                        if (p1 > a.ex_data[t0 + 2 * (u64) j] && p2 < a.ex_data[t0 + 2 * (u64) j + 1])
                          { best = j;
                            break;
                          }
                      best = wave_min_i(best);
                      if (best != 0x7fffffff)
                        { kind = DAMAR_GAP_MASKED;
                          v0 = a.ex_data[t0 + 2 * (u64) best];
                          v1 = a.ex_data[t0 + 2 * (u64) best + 1];
                        }
                    }
                  if (kind < 0 && a.stitch > 0 && n >= 2)
                    { const int ignore = F_TEMP | F_CONT | F_TRIM | F_STITCH;
                      int t = 0;
                      for (int i = l; i < n; i += WAVE)
                        { const int fi = ldf(&fl[i]);
                          if (fi & ignore)
                            continue;
                          for (int k = i + 1; k < n && br[k] == br[i]; k++)
                            { const int fk = ldf(&fl[k]);
                              if ((fk & ignore) || ((fi ^ fk) & F_COMP))
                                continue;
                              const int da = ae[i] - ab[k], db = be[i] - bb[k];
                              if ((da < 0 ? -da : da) < a.stitch && (db < 0 ? -db : db) < a.stitch && ab[i] < p1 - PG_MINLR &&
                                  ae[k] > p2 + PG_MINLR)
                                t += 1;
                            }
                        }
                      t = wave_sum_i(t);
                      if (t != 0)
                        { kind = DAMAR_GAP_STITCHABLE;
                          v0 = t;
                        }
                    }
                  if (kind < 0)
                    { kind = drop_break(l, n, ab, ae, fl, p1, p2, &d);
                      breaks += 1;
                      dropped += d;
                    }
                  over = put_event(a, p, l, nev, beg, b, kind, v0, v1, d);
                  nev += 1;
                  beg = -1;
                }
            }
          if (beg != -1 && !over)
            { /* the run still open at the end: always dropped (LAgap.c:1770-1777) */
              int d;
              const int kind = drop_break(l, n, ab, ae, fl, (beg - 1) * PG_BIN, (e0 + 1) * PG_BIN, &d);
              breaks += 1;
              dropped += d;
              over = put_event(a, p, l, nev, beg, e0, kind | DAMAR_GAP_TRAILING, 0, 0, d);
              nev += 1;
            }
          wave_lds_sync();
        }
      if (l == 0)
        { a.status[p] = over;
          a.nev[p] = nev;
          a.cnt[3 * (size_t) p] = gone;
          a.cnt[3 * (size_t) p + 1] = breaks;
          a.cnt[3 * (size_t) p + 2] = dropped;
        }
    }
}

void damar_launch_pile_gaps(const GapArgs *a, u32 grid, hipStream_t st)
{ if (a->npiles == 0)
    return;
  if (grid < 1 || grid > PG_MAX_BLOCKS)
    grid = PG_MAX_BLOCKS;
  const u32 blocks = a->npiles < grid ? a->npiles : grid;
  hipLaunchKernelGGL(pile_gaps, dim3(blocks), dim3(PG_THREADS), 0, st, *a);
}

u32 damar_pile_gaps_grid(void) { return PG_MAX_BLOCKS; }
