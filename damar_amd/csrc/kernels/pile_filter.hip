/* pile_filter.hip -- LAfilter's per-pile work for gfx950 (scrub/LAfilter.c:2550-2813 filter_handler, :1257-1683 filter,
 * :492-610 stitch, :272-422 removeOvls; the plain version is host/filter.c damar_host_filter_pile).
 *
 * One wavefront per pile, one wavefront per workgroup.  The steps follow the reference's order, and between two steps in
 * which different lanes touch a record the wave's memory operations are drained:
 *   records   the steps that look at one record alone have the lanes strided over the pile: -f, -b over the trace bytes,
 *             filter() with the trace-point sum of -R 2, the first loop of removeOvls, the read states of -x / -I.  The A
 *             read's repeat intervals are staged once per pile in LDS (FL_REPCAP values; a read with more keeps them in HBM),
 *             its trim pair in registers; the B read's intervals and the -A list come from their CSR arrays in HBM.
 *   runs      the records of one B read in a row are a run, as they lie.  The lane whose record begins a run walks it alone
 *             and in the reference's order: stitch, the multi-mapper screen, -R 4, -R 6.  Runs are met 64 records at a time.
 *             A pile with a run of more than `maxgroup` records is left to the host.
 *   pile      -z: the three sums by wave reductions; under -u the covered bases of the trim interval from one bit per base
 *             in LDS (dynamic, sized by the host for the longest A read of the batch, `maxlen` at the most; a longer read
 *             sends its pile to the host).
 * The outputs of a record are read and written by its own pile's wavefront alone, but by different lanes of it in the
 * different steps: those accesses go past the vector L1 (agent scope).
 * A pile with status 1 afterwards is the host's; its other outputs are not to be looked at. */
#include "dev_common.h"
#include "damar_hip.h"
#include "kernels.h"

#define FL_THREADS 64
#define FL_MAX_BLOCKS 65536u
#define FL_REPCAP 1024                    /* ints of the A read's repeat intervals kept in LDS */

#define F_COMP    0x1                     /* lib/oflags.h */
#define F_DISCARD 0x2
#define F_REPEAT  0x8
#define F_LOCAL   0x10
#define F_DIFF    0x20
#define F_OLEN    0x200
#define F_RLEN    0x400
#define F_STITCH  0x80
#define F_CONT    0x8000
#define F_GAP     0x10000
#define F_TRIM    0x20000
#define F_MODULE  0x40000
#define F_SYM     0x100

#define R_STITCH 0x1                      /* LAfilter.c:49-55 */
#define R_MOD    0x2
#define R_TP     0x4
#define R_NONID  0x8
#define R_SPEC   0x10
#define R_ID     0x20
#define R_CONT   0x40

__device__ __forceinline__ void wave_lds_sync()
{ __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ int  ldf(const int *p)      { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void stf(int *p, int v)     { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int iabs(int v)             { return v < 0 ? -v : v; }
__device__ __forceinline__ int contained(int ab, int ae, int bb, int be) { return ab >= bb && ae <= be; }
__device__ __forceinline__ int intersect(int ab, int ae, int bb, int be)
{ const int b = ab > bb ? ab : bb, e = ae < be ? ae : be;
  return b < e ? e - b : 0;
}

__device__ __forceinline__ int trace_val(const FilterArgs &a, long long rec, int k)
{ const u8 *q = a.trace + a.trace_off[rec] + (long long) a.tbytes * k;
  return a.tbytes == 1 ? q[0] : (q[0] | (q[1] << 8));
}

/* the view of one pile */
struct PileV
{ long long lo;
  int n, aread, alen;
  const int *ab, *bb, *br;
  int *fl, *ae, *be, *df, *tl, *why, *by;
};

/* filter() for record i: what is or'ed into its flags; c[] the pile's counters of this lane.  ra: the A read's repeat
   values (na of them), in LDS or in HBM */
__device__ int filter_record(const FilterArgs &a, const PileV &v, int i, const int *ra, int na, int *c)
{ const int ab = v.ab[i], ae = ldf(&v.ae[i]), bb = v.bb[i], be = ldf(&v.be[i]), bread = v.br[i];
  const int fi = ldf(&v.fl[i]), comp = fi & F_COMP;
  const int alen = v.alen, blen = a.read_len[bread];
  const int nlen = ae - ab < be - bb ? ae - ab : be - bb;
  int tab = 0, tae = alen, tbb = 0, tbe = blen, talen = alen, tblen = blen, ret = 0, why = ldf(&v.why[i]);

  if (a.trim != NULL)
    { tab = a.trim[2 * v.aread];  tae = a.trim[2 * v.aread + 1];
      talen = tae - tab;
      tbb = a.trim[2 * bread];  tbe = a.trim[2 * bread + 1];
      tblen = tbe - tbb;
      if (comp)
        { const int x = tbb;
          tbb = blen - tbe;
          tbe = blen - x;
        }
    }
  if (a.sym_off != NULL)
    { const int r0 = v.aread < bread ? v.aread : bread, r1 = v.aread < bread ? bread : v.aread;
      const int *list = a.sym_data + a.sym_off[r0];
      const int  nl = a.sym_len[r0];
      for (int j = 0; j < nl; j++)
        if (list[j] == r1)
          { ret |= F_DISCARD | F_SYM;
            c[DAMAR_FC_SYM] += 1;
            why |= DAMAR_FR_SYM;
            break;
          }
    }
  if (a.min_rlen != -1 && (talen < a.min_rlen || tblen < a.min_rlen))
    { c[DAMAR_FC_READLEN] += 1;
      ret |= F_DISCARD | F_RLEN;
    }
  if (a.min_olen != -1 && nlen < a.min_olen)
    { c[DAMAR_FC_LENGTH] += 1;
      why |= DAMAR_FR_OLEN;
      ret |= F_DISCARD | F_OLEN;
    }
  if (a.max_unaligned != -1)
    { const int u = a.max_unaligned;
      if ((ab - tab > u && bb - tbb > u) || (tae - ae > u && tbe - be > u))
        { c[DAMAR_FC_UNALIGNED] += 1;
          why |= DAMAR_FR_LOCAL;
          ret |= F_DISCARD | F_LOCAL;
        }
    }
  if (a.max_diffs > 0 && 1.0 * ldf(&v.df[i]) / nlen > (double) a.max_diffs)      /* in double against the float */
    { c[DAMAR_FC_DIFFS] += 1;
      why |= DAMAR_FR_DIFF;
      ret |= F_DISCARD | F_DIFF;
    }
  if (a.min_nonrep != -1)
    { const int *rb = a.rep_data + a.rep_anno[bread] / 4;
      const int  nb = (int) ((a.rep_anno[bread + 1] - a.rep_anno[bread]) / 4);
      const int  tips = a.merge_tips, need = a.min_nonrep;
      int tip_ab = tab, tip_ae = tae, site = 0, ovllen, repeat;
      if (tips)
        { int cum = 0;
          for (int k = 0; k < na; k += 2)
            { const int b0 = ra[k], e0 = ra[k + 1];
              if (b0 > tab + tips)
                break;
              if (e0 < tab)
                continue;
              cum += b0 < tab ? e0 - tab : e0 - b0;
              if (e0 > tab + tips)
                break;
            }
          if (cum > 1 + tips / 3)
            tip_ab = tab + tips;
          cum = 0;
          for (int k = 0; k < na; k += 2)
            { const int b0 = ra[k], e0 = ra[k + 1];
              if (e0 < tae - tips)
                continue;
              if (b0 > tae)
                break;
              cum += e0 > tae ? tae - b0 : e0 - b0;
            }
          if (cum > 1 + tips / 3)
            tip_ae = tae - tips;
        }
      if (tip_ae < tip_ab)
        site = DAMAR_FR_REPA_TIPS;
      ovllen = (ae < tip_ae ? ae : tip_ae) - (ab > tip_ab ? ab : tip_ab);
      if (!site && ovllen < need)
        site = DAMAR_FR_REPA_LEN;
      if (!site)
        { repeat = 0;
          for (int k = 0; k < na; k += 2)
            { int b0 = ra[k], e0 = ra[k + 1];
              if (e0 < tip_ab || b0 > tip_ae)
                continue;
              if (b0 < tip_ab) b0 = tip_ab;
              if (e0 > tip_ae) e0 = tip_ae;
              repeat += intersect(ab, ae, b0, e0);
            }
          if (repeat > 0 && ovllen - repeat < need)
            site = DAMAR_FR_REPA;
        }
      if (!site)
        { ovllen = be - bb;
          if (ae > tip_ae) ovllen -= ae - tip_ae;
          if (ab < tip_ab) ovllen -= tip_ab - ab;
          if (ovllen < need)
            site = DAMAR_FR_REPB_LEN;
        }
      if (!site)
        { int b0, e0;
          if (comp)
            { b0 = ae > tip_ae ? blen - (be - (ae - tip_ae)) : blen - be;
              e0 = ab < tip_ab ? blen - (bb - (tip_ab - ab)) : blen - bb;
            }
          else
            { b0 = ab < tip_ab ? bb + (tip_ab - ab) : bb;
              e0 = ae > tip_ae ? be - (ae - tip_ae) : be;
            }
          repeat = 0;
          for (int k = 0; k < nb; k += 2)
            repeat += intersect(b0, e0, rb[k], rb[k + 1]);
          if (repeat > 0 && ovllen - repeat < need)
            site = DAMAR_FR_REPB;
        }
      if (site)
        { c[DAMAR_FC_REPEAT] += 1;
          why |= site;
          ret |= F_DISCARD | F_REPEAT;
        }
    }
  if (!(fi & F_DISCARD) && (a.remove & R_TP))
    { const int tl = ldf(&v.tl[i]);
      int bpos = bb;
      for (int k = 0; k < tl; k += 2)
        bpos += trace_val(a, v.lo + i, k + 1);
      if (bpos != be)
        { ret |= F_DISCARD;
          why |= DAMAR_FR_TP;
        }
    }
  stf(&v.why[i], why);
  return ret;
}

/* stitch() on the run [j, g1) */
__device__ int stitch_run(const FilterArgs &a, const PileV &v, int j, int g1)
{ const int ignore = F_CONT | F_STITCH | F_GAP | F_TRIM;
  int stitched = 0;
  if (g1 - j < 2)
    return 0;
  for (int i = j; i < g1; i++)
    { int fi = ldf(&v.fl[i]);
      if (fi & ignore)
        continue;
      int ae1 = ldf(&v.ae[i]), be1 = ldf(&v.be[i]), found = 1;
      while (found)
        { int maxk = 0, maxlen = 0;
          found = 0;
          for (int k = i + 1; k < g1; k++)
            { const int fk = ldf(&v.fl[k]);
              if ((fk & ignore) || ((fi ^ fk) & F_COMP))
                continue;
              const int da = iabs(ae1 - v.ab[k]), db = iabs(be1 - v.bb[k]), len = ldf(&v.ae[k]) - v.ab[k];
              if (da < a.stitch && db < a.stitch && (a.stitch_aggr || iabs(da - db) < 40) && len > maxlen)
                { found = 1;
                  maxk = k;
                  maxlen = len;
                }
            }
          if (found)
            { ae1 = ldf(&v.ae[maxk]);
              be1 = ldf(&v.be[maxk]);
              stf(&v.ae[i], ae1);
              stf(&v.be[i], be1);
              stf(&v.df[i], ldf(&v.df[i]) + ldf(&v.df[maxk]));
              stf(&v.tl[i], 0);
              stf(&v.why[i], ldf(&v.why[i]) | DAMAR_FR_HEAD);
              fi &= ~(F_DISCARD | F_LOCAL);
              stf(&v.fl[i], fi);
              stf(&v.fl[maxk], ldf(&v.fl[maxk]) | F_DISCARD | F_STITCH);
              stitched += 1;
            }
        }
    }
  return stitched;
}

__device__ __forceinline__ int proper(const PileV &v, int i, int blen)
{ return (v.ab[i] == 0 || v.bb[i] == 0) && (ldf(&v.ae[i]) == v.alen || ldf(&v.be[i]) == blen);
}

__device__ __forceinline__ int self_equal(const PileV &v, int i)
{ return v.aread == v.br[i] && v.ab[i] == v.bb[i] && ldf(&v.ae[i]) == ldf(&v.be[i]);
}

/* the end of the run that begins at record i0, or -1 when it has more than `cap` records */
__device__ __forceinline__ int run_end(const PileV &v, int i0, int cap)
{ int g1 = i0 + 1;
  while (g1 < v.n && v.br[g1] == v.br[i0])
    { if (g1 - i0 >= cap)
        return -1;
      g1++;
    }
  return g1;
}

__global__ __launch_bounds__(FL_THREADS)
void pile_filter(FilterArgs a)
{ extern __shared__ u32 s_mask[];
  __shared__ int s_rep[FL_REPCAP];
  const int l = lane_id();
  const int cap = a.maxgroup < DAMAR_FILTER_MAXGROUP ? a.maxgroup : DAMAR_FILTER_MAXGROUP;
  for (u32 p = blockIdx.x; p < a.npiles; p += gridDim.x)
    { PileV v;
      v.lo = a.pile_off[p];
      v.n = (int) (a.pile_off[p + 1] - v.lo);
      v.aread = a.pile_aread[p];
      v.alen = a.read_len[v.aread];
      v.ab = a.abpos + v.lo;  v.bb = a.bbpos + v.lo;  v.br = a.bread + v.lo;
      v.fl = a.o_flags + v.lo;  v.ae = a.o_ae + v.lo;  v.be = a.o_be + v.lo;  v.df = a.o_df + v.lo;  v.tl = a.o_tl + v.lo;
      v.why = a.o_why + v.lo;  v.by = a.o_by + v.lo;
      const int n = v.n;
      const bool do_main = (a.steps & DAMAR_FILTER_MAIN) != 0;
      const bool cover = a.lowcov && a.max_unaligned != -1;
      int c[DAMAR_FC_COUNT];
      for (int k = 0; k < DAMAR_FC_COUNT; k++) c[k] = 0;

      /* what the kernel does not take */
      int over = 0;
      if (do_main)
        { for (int i = l; i < n; i += WAVE)
            if ((i == 0 || v.br[i] != v.br[i - 1]) && run_end(v, i, cap) < 0)
              over = 1;
          const int words = (v.alen + 31) / 32 + 1;
          if (cover && (v.alen > a.maxlen || v.alen > DAMAR_FILTER_MAXLEN || words > a.mask_words))
            over = 1;
        }
      if (wany(over != 0))
        { if (l == 0) a.status[p] = 1;
          continue;
        }

      for (int i = l; i < n; i += WAVE)
        { int f = a.flags[v.lo + i];
          const int tl = a.tlen[v.lo + i];
          if (a.steps & DAMAR_FILTER_PRE)
            { if (a.downsample && (v.aread > a.max_rid || v.br[i] > a.max_rid))
                f |= F_DISCARD;
              if (a.seg_rate >= 0 && a.seg_rate <= 100)
                for (int k = 0; k < tl - 2; k += 2)
                  if (trace_val(a, v.lo + i, k) * 100.0 / trace_val(a, v.lo + i, k + 1) > a.seg_rate)
                    { f |= F_DISCARD | F_DIFF;
                      c[DAMAR_FC_DIFFS] += 1;
                      break;
                    }
            }
          stf(&v.fl[i], f);
          stf(&v.ae[i], a.aepos[v.lo + i]);
          stf(&v.be[i], a.bepos[v.lo + i]);
          stf(&v.df[i], a.diffs[v.lo + i]);
          stf(&v.tl[i], tl);
          stf(&v.why[i], 0);
          stf(&v.by[i], -1);
        }
      wave_mem_sync();

      if (do_main && n > 0)
        { /* -s / -S */
          if (a.stitch >= 0)
            { for (int base = 0; base < n; base += WAVE)
                { const int i0 = base + l;
                  if (i0 >= n || (i0 > 0 && v.br[i0] == v.br[i0 - 1]))
                    continue;
                  c[DAMAR_FC_STITCHED] += stitch_run(a, v, i0, run_end(v, i0, cap));
                }
              wave_mem_sync();
            }

          /* filter() */
          int na = 0;
          const int *ra = NULL;
          if (a.min_nonrep != -1)
            { const u64 r0 = a.rep_anno[v.aread] / 4;
              na = (int) (a.rep_anno[v.aread + 1] / 4 - r0);
              ra = a.rep_data + r0;
              if (na <= FL_REPCAP)
                { for (int k = l; k < na; k += WAVE)
                    s_rep[k] = ra[k];
                  ra = s_rep;
                }
              wave_lds_sync();
            }
          for (int i = l; i < n; i += WAVE)
            { const int ret = filter_record(a, v, i, ra, na, c);
              stf(&v.fl[i], ldf(&v.fl[i]) | ret);
            }
          wave_mem_sync();
          wave_lds_sync();

          /* -w */
          if (a.multi)
            { for (int base = 0; base < n; base += WAVE)
                { const int i0 = base + l;
                  if (i0 >= n || (i0 > 0 && v.br[i0] == v.br[i0 - 1]))
                    continue;
                  const int g1 = run_end(v, i0, cap);
                  bool found = false;
                  for (int x = i0; x < g1 && !found; x++)
                    { if (ldf(&v.fl[x]) & (F_STITCH | F_DISCARD))
                        continue;
                      const int ab1 = v.ab[x], ae1 = ldf(&v.ae[x]), bb1 = v.bb[x], be1 = ldf(&v.be[x]);
                      for (int y = x + 1; y < g1 && !found; y++)
                        { if (ldf(&v.fl[y]) & (F_STITCH | F_DISCARD))
                            continue;
                          const int ab2 = v.ab[y], ae2 = ldf(&v.ae[y]), bb2 = v.bb[y], be2 = ldf(&v.be[y]);
                          found = contained(ab1, ae1, ab2, ae2) || contained(ab2, ae2, ab1, ae1) || contained(bb1, be1, bb2, be2) ||
                                  contained(bb2, be2, bb1, be1);
                        }
                    }
                  if (found)
                    for (int x = i0; x < g1; x++)
                      { stf(&v.fl[x], ldf(&v.fl[x]) | F_DISCARD);
                        stf(&v.why[x], ldf(&v.why[x]) | DAMAR_FR_MULTI);
                        c[DAMAR_FC_MULTI] += 1;
                        c[DAMAR_FC_MULTI_BASES] += ldf(&v.ae[x]) - v.ab[x];
                      }
                }
              wave_mem_sync();
            }

          /* -z */
          if (a.lowcov)
            { const int tb = a.trim != NULL ? a.trim[2 * v.aread] : 0, te = a.trim != NULL ? a.trim[2 * v.aread + 1] : v.alen;
              if (te - tb > 0)
                { int enter = 0, leave = 0, bases = 0, active = 0;
                  for (int i = l; i < n; i += WAVE)
                    { if (ldf(&v.fl[i]) & F_DISCARD)
                        continue;
                      const int ae = ldf(&v.ae[i]);
                      enter += v.ab[i] <= tb;
                      leave += ae >= te;
                      bases += ae - v.ab[i];
                    }
                  enter = wave_sum_i(enter);
                  leave = wave_sum_i(leave);
                  bases = wave_sum_i(bases);
                  if (cover)
                    { const int words = (v.alen + 31) / 32 + 1;
                      for (int w = l; w < words; w += WAVE)
                        s_mask[w] = 0;
                      wave_lds_sync();
                      for (int i = 0; i < n; i++)                     /* all lanes on one record: its words dealt to them */
                        { if (ldf(&v.fl[i]) & F_DISCARD)
                            continue;
                          const int c0 = v.ab[i] < 0 ? 0 : v.ab[i], ae = ldf(&v.ae[i]), c1 = ae > v.alen ? v.alen : ae;
                          if (c0 >= c1)
                            continue;
                          const int w0 = c0 >> 5, w1 = (c1 - 1) >> 5;
                          for (int w = w0 + l; w <= w1; w += WAVE)
                            { u32 m = ~0u;
                              if (w == w0) m &= ~0u << (c0 & 31);
                              if (w == w1) m &= ~0u >> (31 - ((c1 - 1) & 31));
                              s_mask[w] |= m;
                            }
                          wave_lds_sync();
                        }
                      const int w0 = tb >> 5, w1 = (te - 1) >> 5;
                      for (int w = w0 + l; w <= w1 && w < words; w += WAVE)
                        { u32 m = ~0u;
                          if (w == w0) m &= ~0u << (tb & 31);
                          if (w == w1) m &= ~0u >> (31 - ((te - 1) & 31));
                          active += __popc(s_mask[w] & m);
                        }
                      active = wave_sum_i(active);
                      wave_lds_sync();
                    }
                  if (bases / (te - tb) <= a.lowcov || leave < a.lowcov || enter < a.lowcov || (cover && (te - tb) - active > a.max_unaligned))
                    for (int i = l; i < n; i += WAVE)
                      { const int fi = ldf(&v.fl[i]);
                        if (!(fi & F_DISCARD))
                          { stf(&v.fl[i], fi | F_DISCARD);
                            c[DAMAR_FC_LOWCOV] += 1;
                          }
                      }
                }
              wave_mem_sync();
            }

          /* -R */
          if (a.remove)
            { const int rm = a.remove;
              for (int i = l; i < n; i += WAVE)
                { int fi = ldf(&v.fl[i]);
                  if (rm & R_TP)
                    stf(&v.tl[i], 0);
                  if ((rm & R_MOD) && (fi & F_MODULE))
                    fi |= F_DISCARD;
                  else if ((rm & R_STITCH) && ((rm & R_TP) || ldf(&v.tl[i]) == 0))
                    fi |= F_DISCARD;
                  else if ((rm & R_NONID) && v.aread != v.br[i])
                    fi |= F_DISCARD;
                  else if ((rm & R_ID) && v.aread == v.br[i])
                    fi |= F_DISCARD;
                  stf(&v.fl[i], fi);
                }
              wave_mem_sync();
              if (rm & (R_SPEC | R_CONT))
                { for (int base = 0; base < n; base += WAVE)
                    { const int i0 = base + l;
                      if (i0 >= n || (i0 > 0 && v.br[i0] == v.br[i0 - 1]))
                        continue;
                      const int g1 = run_end(v, i0, cap);
                      if (rm & R_SPEC)
                        { const int blen = a.read_len[v.br[i0]];
                          int np = 0;
                          for (int x = i0; x < g1; x++)
                            np += proper(v, x, blen);
                          if (i0 > 0)                                 /* the reference counts the head of a later run twice */
                            np += proper(v, i0, blen);
                          if (np == 1 && g1 - i0 > 1)
                            for (int x = i0; x < g1; x++)
                              if (!proper(v, x, blen))
                                stf(&v.fl[x], ldf(&v.fl[x]) | F_DISCARD);
                        }
                      if (!(rm & R_CONT))
                        continue;
                      if (g1 - i0 == 1)
                        { if (self_equal(v, i0))
                            { stf(&v.fl[i0], ldf(&v.fl[i0]) | F_DISCARD | F_CONT);
                              stf(&v.why[i0], ldf(&v.why[i0]) | DAMAR_FR_SELF);
                              c[DAMAR_FC_CONTAINED] += 1;
                            }
                          continue;
                        }
                      const bool other = v.aread != v.br[i0];
                      for (int x = i0; x < g1; x++)
                        { if (ldf(&v.fl[x]) & F_DISCARD)
                            continue;
                          if (self_equal(v, x))
                            { stf(&v.fl[x], ldf(&v.fl[x]) | F_DISCARD | F_CONT);
                              stf(&v.why[x], ldf(&v.why[x]) | DAMAR_FR_SELF);
                              c[DAMAR_FC_CONTAINED] += 1;
                              continue;
                            }
                          const int ab1 = v.ab[x], ae1 = ldf(&v.ae[x]), bb1 = v.bb[x], be1 = ldf(&v.be[x]);
                          for (int y = x + 1; y < g1; y++)
                            { const int fy = ldf(&v.fl[y]);
                              if (fy & F_DISCARD)
                                continue;
                              const int ab2 = v.ab[y], ae2 = ldf(&v.ae[y]), bb2 = v.bb[y], be2 = ldf(&v.be[y]);
                              const bool gone = other ? (contained(ab2, ae2, ab1, ae1) && contained(bb2, be2, bb1, be1))
                                                      : (ab2 == ab1 && ae2 == ae1 && bb2 == bb1 && be2 == be1);
                              if (gone)
                                { stf(&v.fl[y], fy | F_DISCARD | F_CONT);
                                  stf(&v.why[y], ldf(&v.why[y]) | DAMAR_FR_CONT);
                                  stf(&v.by[y], x);
                                  c[DAMAR_FC_CONTAINED] += 1;
                                }
                            }
                        }
                    }
                  wave_mem_sync();
                }
            }

          /* -x / -I */
          if (a.read_state != NULL)
            { const int sa = a.read_state[v.aread];
              for (int i = l; i < n; i += WAVE)
                { const int sb = a.read_state[v.br[i]];
                  if ((sa & 1) || (sb & 1) || (a.include && !(sa & 2) && !(sb & 2)))
                    stf(&v.fl[i], ldf(&v.fl[i]) | F_DISCARD);
                }
            }
        }

      for (int k = 0; k < DAMAR_FC_COUNT; k++)
        { const int s = wave_sum_i(c[k]);
          if (l == 0) a.cnt[(size_t) p * DAMAR_FC_COUNT + k] = s;
        }
      if (l == 0) a.status[p] = 0;
      wave_mem_sync();
    }
}

void damar_launch_pile_filter(const FilterArgs *a, u32 grid, hipStream_t st)
{ if (a->npiles == 0)
    return;
  if (grid < 1 || grid > FL_MAX_BLOCKS)
    grid = FL_MAX_BLOCKS;
  const u32 blocks = a->npiles < grid ? a->npiles : grid;
  hipLaunchKernelGGL(pile_filter, dim3(blocks), dim3(FL_THREADS), sizeof(u32) * (size_t) a->mask_words, st, *a);
}

u32 damar_pile_filter_grid(void) { return FL_MAX_BLOCKS; }
