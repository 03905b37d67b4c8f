/* filter.c -- LAfilter (scrub/LAfilter.c without its experimental branches) as calls: the overlaps of a pile screened by
 * divergence, length, overhang and repeat content, stitched cheaply, and dropped where they are contained, map more than
 * once, leave a read thinly covered or stand in a list.
 *   - damar_host_filter_pile: the plain routine, the reference's loops as written (DAMAR_PILES=host, the piles
 *     kernels/pile_filter.hip leaves, and the second opinion for that kernel),
 *   - damar_filter_inputs_valid: what both paths index with,
 *   - damar_filter_las: the pass over a file -- per batch of whole piles -f and -b, the trim (-T, host/trim.c), the rest,
 *     the reference's lines, the records written.
 * Nothing here touches the GPU runtime. */
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "damar_hip.h"
#include "damar_host.h"

#define R_STITCH 0x1                      /* LAfilter.c:49-55 */
#define R_MOD    0x2
#define R_TP     0x4
#define R_NONID  0x8
#define R_SPEC   0x10
#define R_ID     0x20
#define R_CONT   0x40

static int pairs_valid(const uint64 *anno, int64 ndata, int nreads)
{ int r;
  if (anno == NULL || ndata < 0 || anno[0] % 8 || anno[nreads] > 4 * (uint64) ndata)
    return 0;
  for (r = 0; r < nreads; r++)
    if (anno[r] > anno[r + 1] || anno[r + 1] % 8)
      return 0;
  return 1;
}

int damar_filter_inputs_valid(const damar_trace_batch *t, const int *diffs, const damar_filter_params *p, const damar_filter_out *out)
{ const damar_pile_batch *b = t != NULL ? &t->p : NULL;
  const char *why = "malformed batch";
  int64 i, pi;
  int   r;
  if (b == NULL || p == NULL || out == NULL || b->npiles < 0 || b->nrec < 0 || b->npiles > 0x7fffffff || b->nrec > 0x7fffffff || b->nreads <= 0)
    goto bad;
  if (b->npiles == 0 ? b->nrec != 0 : (b->pile_off[0] != 0 || b->pile_off[b->npiles] != b->nrec))
    goto bad;
  if ((t->tbytes != 1 && t->tbytes != 2) || (p->steps & ~(DAMAR_FILTER_PRE | DAMAR_FILTER_MAIN)) || p->steps == 0)
    goto bad;
  if (b->nrec > 0 && (diffs == NULL || out->flags == NULL || out->aepos == NULL || out->bepos == NULL || out->diffs == NULL || out->tlen == NULL ||
                      out->reason == NULL || out->cont_by == NULL))
    goto bad;
  if (b->npiles > 0 && out->cnt == NULL)
    goto bad;
  for (pi = 0; pi < b->npiles; pi++)
    { if (b->pile_off[pi] > b->pile_off[pi + 1] || b->pile_aread[pi] < 0 || b->pile_aread[pi] >= b->nreads)
        goto bad;
      for (i = b->pile_off[pi]; i < b->pile_off[pi + 1]; i++)
        { if (b->bread[i] < 0 || b->bread[i] >= b->nreads)
            { why = "a record's B read is not in the database";
              goto bad;
            }
          if (t->tlen[i] < 0 || (t->tlen[i] & 1) || t->trace_off[i] < 0 || t->trace_off[i] + (int64) t->tbytes * t->tlen[i] > t->trace_bytes)
            { why = "a record's trace lies outside the batch";
              goto bad;
            }
        }
    }
  if (p->trim != NULL)
    for (r = 0; r < b->nreads; r++)
      if (p->trim[2 * r] < 0 || p->trim[2 * r] > p->trim[2 * r + 1] || p->trim[2 * r + 1] > b->read_len[r])
        { why = "the trim track keeps bases a read does not have";
          goto bad;
        }
  if (p->min_nonrep != -1 && !pairs_valid(p->rep_anno, p->rep_ndata, b->nreads))
    { why = "the repeat track is not pairs of ints for the database's reads";
      goto bad;
    }
  if (p->sym_off != NULL)
    for (r = 0; r <= b->nreads; r++)
      if (p->sym_len == NULL || p->sym_len[r] < 0 || (p->sym_len[r] > 0 && (p->sym_off[r] < 0 || (int64) p->sym_off[r] + p->sym_len[r] > p->sym_ndata)))
        { why = "the list of discarded overlaps runs outside its data";
          goto bad;
        }
  return 1;
bad:
  fprintf(stderr, "damar: filter: %s\n", why);
  return 0;
}

/***** the plain routine ************************************************************************/

typedef struct
{ const damar_trace_batch *t;
  const damar_pile_batch  *b;
  const damar_filter_params *p;
  int64 lo;
  int   n, aread;
  int  *fl, *ae, *be, *df, *tl, *why, *by, *cnt;
} Pile;

#define AB(i) (pl->b->abpos[pl->lo + (i)])
#define BB(i) (pl->b->bbpos[pl->lo + (i)])
#define BR(i) (pl->b->bread[pl->lo + (i)])

/* LAfilter.c:492-610 on the run [j, j + n) */
static int stitch_run(Pile *pl, int j, int n, int fuzz, int aggressive)
{ const int ignore = OVL_CONT | OVL_STITCH | OVL_GAP | OVL_TRIM;
  int stitched = 0, i, k;
  if (n < 2)
    return 0;
  for (i = j; i < j + n; i++)
    { int ae1, be1, found = 1;
      if (pl->fl[i] & ignore)
        continue;
      ae1 = pl->ae[i];
      be1 = pl->be[i];
      while (found)
        { int maxk = 0, maxlen = 0;
          found = 0;
          for (k = i + 1; k < j + n; k++)
            { int da, db;
              if ((pl->fl[k] & ignore) || ((pl->fl[i] ^ pl->fl[k]) & OVL_COMP))
                continue;
              da = abs(ae1 - AB(k));
              db = abs(be1 - BB(k));
              if (da < fuzz && db < fuzz && (aggressive || abs(da - db) < 40) && pl->ae[k] - AB(k) > maxlen)
                { found = 1;
                  maxk = k;
                  maxlen = pl->ae[k] - AB(k);
                }
            }
          if (found)
            { pl->ae[i] = ae1 = pl->ae[maxk];
              pl->be[i] = be1 = pl->be[maxk];
              pl->df[i] += pl->df[maxk];
              pl->tl[i] = 0;
              pl->why[i] |= DAMAR_FR_HEAD;
              pl->fl[i] &= ~(OVL_DISCARD | OVL_LOCAL);
              pl->fl[maxk] |= OVL_DISCARD | OVL_STITCH;
              stitched += 1;
            }
        }
    }
  return stitched;
}

/* filter(), LAfilter.c:1257-1683: what is or'ed into record i's flags */
static int filter_record(Pile *pl, int i)
{ const damar_filter_params *p = pl->p;
  const int ab = AB(i), ae = pl->ae[i], bb = BB(i), be = pl->be[i], bread = BR(i), comp = pl->fl[i] & OVL_COMP;
  const int alen = pl->b->read_len[pl->aread], blen = pl->b->read_len[bread];
  int nlen = ae - ab < be - bb ? ae - ab : be - bb;
  int tab = 0, tae = alen, tbb = 0, tbe = blen, talen = alen, tblen = blen, ret = 0;

  if (p->trim != NULL)
    { tab = p->trim[2 * pl->aread];  tae = p->trim[2 * pl->aread + 1];
      talen = tae - tab;
      tbb = p->trim[2 * bread];  tbe = p->trim[2 * bread + 1];
      tblen = tbe - tbb;
      if (comp)
        { const int x = tbb;
          tbb = blen - tbe;
          tbe = blen - x;
        }
    }
  if (p->sym_off != NULL)
    { const int a = pl->aread < bread ? pl->aread : bread, b = pl->aread < bread ? bread : pl->aread;
      int j;
      for (j = 0; j < p->sym_len[a]; j++)
        if (p->sym_data[p->sym_off[a] + j] == b)
          { ret |= OVL_DISCARD | OVL_SYMDISCARD;
            pl->cnt[DAMAR_FC_SYM] += 1;
            pl->why[i] |= DAMAR_FR_SYM;
            break;
          }
    }
  if (p->min_rlen != -1 && (talen < p->min_rlen || tblen < p->min_rlen))
    { pl->cnt[DAMAR_FC_READLEN] += 1;
      ret |= OVL_DISCARD | OVL_RLEN;
    }
  if (p->min_olen != -1 && nlen < p->min_olen)
    { pl->cnt[DAMAR_FC_LENGTH] += 1;
      pl->why[i] |= DAMAR_FR_OLEN;
      ret |= OVL_DISCARD | OVL_OLEN;
    }
  if (p->max_unaligned != -1)
    { const int u = p->max_unaligned;
      if ((ab - tab > u && bb - tbb > u) || (tae - ae > u && tbe - be > u))
        { pl->cnt[DAMAR_FC_UNALIGNED] += 1;
          pl->why[i] |= DAMAR_FR_LOCAL;
          ret |= OVL_DISCARD | OVL_LOCAL;
        }
    }
  if (p->max_diffs > 0 && 1.0 * pl->df[i] / nlen > p->max_diffs)          /* in double against the float, as the reference has it */
    { pl->cnt[DAMAR_FC_DIFFS] += 1;
      pl->why[i] |= DAMAR_FR_DIFF;
      ret |= OVL_DISCARD | OVL_DIFF;
    }
  if (p->min_nonrep != -1)
    { const int *ra = p->rep_data + p->rep_anno[pl->aread] / sizeof(int), *rb = p->rep_data + p->rep_anno[bread] / sizeof(int);
      const int na = (int) ((p->rep_anno[pl->aread + 1] - p->rep_anno[pl->aread]) / sizeof(int));
      const int nb = (int) ((p->rep_anno[bread + 1] - p->rep_anno[bread]) / sizeof(int));
      const int tips = p->merge_tips, need = p->min_nonrep;
      int tip_ab = tab, tip_ae = tae, site = 0, k, ovllen, repeat;
      if (tips)
        { int cum = 0;
          for (k = 0; k < na; k += 2)
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
          for (k = 0; k < na; k += 2)
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
          for (k = 0; k < na; k += 2)
            { int b0 = ra[k], e0 = ra[k + 1];
              if (e0 < tip_ab || b0 > tip_ae)
                continue;
              if (b0 < tip_ab) b0 = tip_ab;
              if (e0 > tip_ae) e0 = tip_ae;
              repeat += damar_intersect(ab, ae, b0, e0);
            }
          if (repeat > 0 && ovllen - repeat < need)
            site = DAMAR_FR_REPA;
        }
      if (!site)
        { ovllen = be - bb;                        /* the tips mapped roughly onto B */
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
          for (k = 0; k < nb; k += 2)
            repeat += damar_intersect(b0, e0, rb[k], rb[k + 1]);
          if (repeat > 0 && ovllen - repeat < need)
            site = DAMAR_FR_REPB;
        }
      if (site)
        { pl->cnt[DAMAR_FC_REPEAT] += 1;
          pl->why[i] |= site;
          ret |= OVL_DISCARD | OVL_REPEAT;
        }
    }
  if (!(pl->fl[i] & OVL_DISCARD) && (p->remove & R_TP))
    { int bpos = bb, k;
      for (k = 0; k < pl->tl[i]; k += 2)
        bpos += damar_trace_value(pl->t, pl->lo + i, k + 1);
      if (bpos != be)
        { ret |= OVL_DISCARD;
          pl->why[i] |= DAMAR_FR_TP;
        }
    }
  return ret;
}

static int proper(const Pile *pl, int i, int alen, int blen)
{ return (AB(i) == 0 || BB(i) == 0) && (pl->ae[i] == alen || pl->be[i] == blen);
}

static int self_equal(const Pile *pl, int i)
{ return pl->aread == BR(i) && AB(i) == BB(i) && pl->ae[i] == pl->be[i];
}

/* filter_handler (LAfilter.c:2550-2813) without the trim, which lies between the two steps */
void damar_host_filter_pile(const damar_trace_batch *t, const int *diffs, int64 pile, const damar_filter_params *p, damar_filter_out *out)
{ Pile  P, *pl = &P;
  const damar_pile_batch *b = &t->p;
  int   i, j, k, l, m;

  P.t = t;  P.b = b;  P.p = p;
  P.lo = b->pile_off[pile];
  P.n = (int) (b->pile_off[pile + 1] - P.lo);
  P.aread = b->pile_aread[pile];
  P.fl = out->flags + P.lo;  P.ae = out->aepos + P.lo;  P.be = out->bepos + P.lo;  P.df = out->diffs + P.lo;  P.tl = out->tlen + P.lo;
  P.why = out->reason + P.lo;  P.by = out->cont_by + P.lo;
  P.cnt = out->cnt + DAMAR_FC_COUNT * pile;
  for (i = 0; i < DAMAR_FC_COUNT; i++)
    P.cnt[i] = 0;
  for (i = 0; i < P.n; i++)
    { P.fl[i] = b->flags[P.lo + i];  P.ae[i] = b->aepos[P.lo + i];  P.be[i] = b->bepos[P.lo + i];
      P.df[i] = diffs[P.lo + i];  P.tl[i] = t->tlen[P.lo + i];  P.why[i] = 0;  P.by[i] = -1;
    }

  if (p->steps & DAMAR_FILTER_PRE)
    { if (p->downsample)
        { const int max_rid = (int) (p->downsample * b->nreads / 100.0);
          for (i = 0; i < P.n; i++)
            if (P.aread > max_rid || BR(i) > max_rid)
              P.fl[i] |= OVL_DISCARD;
        }
      if (p->seg_rate >= 0 && p->seg_rate <= 100)
        for (i = 0; i < P.n; i++)
          for (k = 0; k < P.tl[i] - 2; k += 2)
            if (damar_trace_value(t, P.lo + i, k) * 100.0 / damar_trace_value(t, P.lo + i, k + 1) > p->seg_rate)
              { P.fl[i] |= OVL_DISCARD | OVL_DIFF;
                P.cnt[DAMAR_FC_DIFFS] += 1;
                break;
              }
    }
  if (!(p->steps & DAMAR_FILTER_MAIN) || P.n == 0)
    return;

  if (p->stitch >= 0)
    for (j = 0; j < P.n; j = k + 1)
      { for (k = j; k < P.n - 1 && BR(j) == BR(k + 1); k++)
          ;
        P.cnt[DAMAR_FC_STITCHED] += stitch_run(pl, j, k - j + 1, p->stitch, p->stitch_aggr);
      }
  for (i = 0; i < P.n; i++)
    P.fl[i] |= filter_record(pl, i);

  if (p->multi)
    for (j = 0; j < P.n; j = k + 1)
      { int found = 0;
        for (k = j; k < P.n - 1 && BR(j) == BR(k + 1); k++)
          ;
        for (l = j; l <= k && !found; l++)
          { if (P.fl[l] & (OVL_STITCH | OVL_DISCARD))
              continue;
            for (m = l + 1; m <= k && !found; m++)
              { if (P.fl[m] & (OVL_STITCH | OVL_DISCARD))
                  continue;
                if (damar_contained(AB(l), P.ae[l], AB(m), P.ae[m]) || damar_contained(BB(l), P.be[l], BB(m), P.be[m]))
                  found = 1;
              }
          }
        if (found)
          for (l = j; l <= k; l++)
            { P.fl[l] |= OVL_DISCARD;
              P.why[l] |= DAMAR_FR_MULTI;
              P.cnt[DAMAR_FC_MULTI] += 1;
              P.cnt[DAMAR_FC_MULTI_BASES] += P.ae[l] - AB(l);
            }
      }

  if (p->lowcov)
    { const int alen = b->read_len[P.aread];
      const int tb = p->trim != NULL ? p->trim[2 * P.aread] : 0, te = p->trim != NULL ? p->trim[2 * P.aread + 1] : alen;
      if (te - tb)
        { int enter = 0, leave = 0, bases = 0, active = 0;
          unsigned char *cov = NULL;
          if (p->max_unaligned != -1)
            cov = (unsigned char *) memset(damar_grow(NULL, (size_t) alen + 1, "filter"), 0, (size_t) alen + 1);
          for (i = 0; i < P.n; i++)
            { if (P.fl[i] & OVL_DISCARD)
                continue;
              enter += AB(i) <= tb;
              leave += P.ae[i] >= te;
              bases += P.ae[i] - AB(i);
              if (cov != NULL)                     /* held to the read: the reference's buffer is the longest read's */
                { const int c0 = AB(i) < 0 ? 0 : AB(i), c1 = P.ae[i] > alen ? alen : P.ae[i];
                  if (c0 < c1)
                    memset(cov + c0, 1, (size_t) (c1 - c0));
                }
            }
          if (cov != NULL)
            for (i = tb; i < te; i++)
              active += cov[i];
          free(cov);
          if (bases / (te - tb) <= p->lowcov || leave < p->lowcov || enter < p->lowcov ||
              (p->max_unaligned != -1 && (te - tb) - active > p->max_unaligned))
            for (i = 0; i < P.n; i++)
              if (!(P.fl[i] & OVL_DISCARD))
                { P.fl[i] |= OVL_DISCARD;
                  P.cnt[DAMAR_FC_LOWCOV] += 1;
                }
        }
    }

  if (p->remove)                                   /* removeOvls, LAfilter.c:272-422 */
    { const int rm = p->remove, alen = b->read_len[P.aread];
      for (i = 0; i < P.n; i++)
        { if (rm & R_TP)
            P.tl[i] = 0;
          if ((rm & R_MOD) && (P.fl[i] & OVL_MODULE))
            P.fl[i] |= OVL_DISCARD;
          else if ((rm & R_STITCH) && P.tl[i] == 0)
            P.fl[i] |= OVL_DISCARD;
          else if ((rm & R_NONID) && P.aread != BR(i))
            P.fl[i] |= OVL_DISCARD;
          else if ((rm & R_ID) && P.aread == BR(i))
            P.fl[i] |= OVL_DISCARD;
        }
      if (rm & R_SPEC)
        for (j = 0; j < P.n; j = k + 1)
          { const int blen = b->read_len[BR(j)];
            int np = 0;
            for (k = j; k < P.n - 1 && BR(j) == BR(k + 1); k++)
              ;
            for (l = j; l <= k; l++)
              np += proper(pl, l, alen, blen);
            if (j > 0)                             /* the reference's inner loop starts one record back: the head counts twice */
              np += proper(pl, j, alen, blen);
            if (np == 1 && k > j)
              for (l = j; l <= k; l++)
                if (!proper(pl, l, alen, blen))
                  P.fl[l] |= OVL_DISCARD;
          }
      if (rm & R_CONT)
        for (j = 0; j < P.n; j = k + 1)
          { for (k = j; k < P.n - 1 && BR(j) == BR(k + 1); k++)
              ;
            if (k == j)
              { if (self_equal(pl, j))
                  { P.fl[j] |= OVL_DISCARD | OVL_CONT;
                    P.why[j] |= DAMAR_FR_SELF;
                    P.cnt[DAMAR_FC_CONTAINED] += 1;
                  }
                continue;
              }
            for (l = j; l <= k; l++)
              { if (P.fl[l] & OVL_DISCARD)
                  continue;
                if (self_equal(pl, l))
                  { P.fl[l] |= OVL_DISCARD | OVL_CONT;
                    P.why[l] |= DAMAR_FR_SELF;
                    P.cnt[DAMAR_FC_CONTAINED] += 1;
                    continue;
                  }
                for (m = l + 1; m <= k; m++)
                  { int gone;
                    if (P.fl[m] & OVL_DISCARD)
                      continue;
                    if (P.aread != BR(j))
                      gone = damar_contained(AB(m), P.ae[m], AB(l), P.ae[l]) == 1 && damar_contained(BB(m), P.be[m], BB(l), P.be[l]) == 1;
                    else                           /* identity overlaps: duplicates only */
                      gone = AB(m) == AB(l) && P.ae[m] == P.ae[l] && BB(m) == BB(l) && P.be[m] == P.be[l];
                    if (gone)
                      { P.fl[m] |= OVL_DISCARD | OVL_CONT;
                        P.why[m] |= DAMAR_FR_CONT;
                        P.by[m] = l;
                        P.cnt[DAMAR_FC_CONTAINED] += 1;
                      }
                  }
              }
          }
    }

  if (p->read_state != NULL)
    for (i = 0; i < P.n; i++)
      { if ((p->read_state[P.aread] & 1) || (p->read_state[BR(i)] & 1))
          P.fl[i] |= OVL_DISCARD;
        if (p->include && !(p->read_state[P.aread] & 2) && !(p->read_state[BR(i)] & 2))
          P.fl[i] |= OVL_DISCARD;
      }
}

/***** the pass over a file *********************************************************************/

/* the lines of one pile, in the order the reference meets them: filter()'s under -v, the multi-mapper runs, -R 4's, and
   -R 6's under -v */
static void print_pile(const damar_trace_batch *t, int64 pile, const damar_filter_opts *o, const damar_filter_params *p, const damar_filter_out *out)
{ const damar_pile_batch *b = &t->p;
  const int64 lo = b->pile_off[pile];
  const int   n = (int) (b->pile_off[pile + 1] - lo), a = b->pile_aread[pile], alen = b->read_len[a];
  const int  *fl = out->flags + lo, *ae = out->aepos + lo, *be = out->bepos + lo, *why = out->reason + lo, *by = out->cont_by + lo;
  const int  *ab = b->abpos + lo, *bb = b->bbpos + lo, *br = b->bread + lo;
  int i, j, k, l, m;
  if (o->verbose)
    for (i = 0; i < n; i++)
      { const int w = why[i], nlen = ae[i] - ab[i] < be[i] - bb[i] ? ae[i] - ab[i] : be[i] - bb[i];
        if (w & DAMAR_FR_SYM)
          printf("overlap (%d x %d): in list of discarded overlaps\n", a, br[i]);
        if (w & DAMAR_FR_OLEN)
          printf("overlap %d -> %d: drop due to length %d\n", a, br[i], nlen);
        if (w & DAMAR_FR_LOCAL)
          { const int blen = b->read_len[br[i]];
            int tab = 0, tae = alen, tbb = 0, tbe = blen;
            if (p->trim != NULL)
              { tab = p->trim[2 * a];  tae = p->trim[2 * a + 1];
                tbb = p->trim[2 * br[i]];  tbe = p->trim[2 * br[i] + 1];
                if (fl[i] & OVL_COMP)
                  { const int x = tbb;
                    tbb = blen - tbe;
                    tbe = blen - x;
                  }
              }
            printf("overlap %d -> %d: drop due to unaligned overhang [%d, %d -> trim %d, %d], [%d, %d -> trim %d, %d]\n", a, br[i], ab[i], ae[i],
                   tab, tae, bb[i], be[i], tbb, tbe);
          }
        if (w & DAMAR_FR_DIFF)
          printf("overlap %d -> %d: drop due to diffs %d length %d\n", a, br[i], out->diffs[lo + i], nlen);
        if (w & (DAMAR_FR_REPA_TIPS | DAMAR_FR_REPA_LEN | DAMAR_FR_REPA | DAMAR_FR_REPB_LEN))
          printf("overlap %d -> %d: drop due to repeat in a\n", a, br[i]);
        if (w & DAMAR_FR_REPB)
          printf("overlap %d -> %d: drop due to repeat in b\n", a, br[i]);
        if (w & DAMAR_FR_TP)
          { int bpos = bb[i];                      /* the trace as filter() saw it: none left on a stitched head */
            if (!(w & DAMAR_FR_HEAD))
              for (k = 0; k < t->tlen[lo + i]; k += 2)
                bpos += damar_trace_value(t, lo + i, k + 1);
            printf("overlap (%d x %d): pass-through points inconsistent be = %d (expected %d)\n", a, br[i], bpos, be[i]);
          }
      }
  if (p->multi)
    for (i = 0; i < n; i++)
      if (why[i] & DAMAR_FR_MULTI)
        printf("remove ovl, falls into multi mapper interval: %d vs %d [%d, %d] %c [%d, %d]\n", a, br[i], ab[i], ae[i], (fl[i] & OVL_COMP) ? 'c' : 'n',
               bb[i], be[i]);
  if (p->remove & R_SPEC)
    { printf("REMOVE_SPECREP_OVL\n");
      for (j = 0; j < n; j = k + 1)
        { const int blen = b->read_len[br[j]];
          int np = 0;
          for (k = j; k < n - 1 && br[j] == br[k + 1]; k++)
            ;
          for (l = j; l <= k; l++)
            np += (ab[l] == 0 || bb[l] == 0) && (ae[l] == alen || be[l] == blen);
          if (j > 0)
            np += (ab[j] == 0 || bb[j] == 0) && (ae[j] == alen || be[j] == blen);
          printf("aread: %d bread: %d novl: %d proper: %d\n", a, br[j], k - j + 1, np);
        }
    }
  if ((p->remove & R_CONT) && o->verbose)
    for (j = 0; j < n; j = k + 1)
      { for (k = j; k < n - 1 && br[j] == br[k + 1]; k++)
          ;
        for (l = j; l <= k; l++)
          { if (why[l] & DAMAR_FR_SELF)
              printf("found contained OVL: %d vs %d a[%d,%d] equals b[%d,%d]\n", a, br[l], ab[l], ae[l], bb[l], be[l]);
            for (m = l + 1; m <= k; m++)
              if (by[m] == l)
                printf("found contained OVL: %d vs %d a[%d,%d] b[%d,%d] in a[%d,%d] b[%d,%d]\n", a, br[m], ab[m], ae[m], bb[m], be[m], ab[l], ae[l],
                       bb[l], be[l]);
          }
      }
}

/* track_load's failure: the loader's line first (the reference never sets its program name), then main's */
void damar_filter_no_track(const char *track)
{ fprintf(stderr, "(null): Track '%s' does not exist\n", track);
  fprintf(stderr, "could not load track %s\n", track);
}

/* lib/utils.c fread_integers: the numbers of a file up to the first thing that is none */
static int *read_integers(FILE *f, int *n)
{ int *v = NULL, cap = 0, x;
  *n = 0;
  while (fscanf(f, "%d\n", &x) == 1)
    { if (*n == cap)
        { cap = cap + cap / 4 + 100;
          v = (int *) damar_grow(v, sizeof(int) * (size_t) cap, "filter");
        }
      v[(*n)++] = x;
    }
  return v;
}

/* -A (LAfilter.c:3291-3392): the pairs of the file as the reference lays them out, a list per first read, each ended by a
   -1 -- but for the list of read 0 when it comes first, which the reference does not end: it runs on into the next read's.
   The file must be sorted with first <= second; where the reference fails an assert, a message.  0, or 1 after it. */
static int read_sym_list(const char *path, int nreads, int **off, int **len, int **data, int64 *ndata)
{ FILE *f = fopen(path, "r");
  int   a, b, pa = -2, pb = -1, nb = 0, na = 0, cur = 0, r;
  if (f == NULL)
    { fprintf(stderr, "could not open %s\n", path);
      return 1;
    }
  while (fscanf(f, "%d %d\n", &a, &b) == 2)
    { na += a != pa;
      if (a > b)
        { fprintf(stderr, "[ERROR] - read list must be sorted aread <= bread! Failed at %d, %d!\n", a, b);
          fprintf(stderr, "	    Please sort your file first! awk '{if($1>$2) print $2\" \"$1; else print $1\" \"$2}' INFILE | sort -k 1,1n -k2,2n | uniq > OUTFILE\n");
          fclose(f);
          return 1;
        }
      nb += 1;
      if (a < 0 || pa > a || (pa == a && pb >= b) || a > nreads)
        { fprintf(stderr, "LAfilter: %s is not sorted, or names a read the database does not have, at %d, %d\n", path, a, b);
          fclose(f);
          return 1;
        }
      pa = a;
      pb = b;
    }
  rewind(f);
  *off = (int *) damar_grow(NULL, sizeof(int) * ((size_t) nreads + 1), "filter");
  *len = (int *) memset(damar_grow(NULL, sizeof(int) * ((size_t) nreads + 1), "filter"), 0, sizeof(int) * ((size_t) nreads + 1));
  *data = (int *) damar_grow(NULL, sizeof(int) * ((size_t) nb + na + 10), "filter");
  for (r = 0; r <= nreads; r++)
    (*off)[r] = -1;
  pa = -2;
  while (fscanf(f, "%d %d\n", &a, &b) == 2)
    { if (pa != a)
        { if (pa > 0)
            (*data)[cur++] = -1;
          (*off)[a] = cur;
        }
      (*data)[cur++] = b;
      pa = a;
    }
  (*data)[cur++] = -1;
  fclose(f);
  for (r = 0; r <= nreads; r++)
    if ((*off)[r] < 0)
      (*off)[r] = 0;
    else
      while ((*data)[(*off)[r] + (*len)[r]] > -1)
        (*len)[r] += 1;
  *ndata = cur;
  return 0;
}

/* main of LAfilter.c from its first fopen on (:3137-3458) */
int damar_filter_las(const char *dbname, const char *las, const char *out, const damar_filter_opts *o, damar_filter_stats *st)
{ damar_dbinfo db;
  damar_trimmer *tm = NULL;
  damar_pile_reader *r = NULL;
  damar_trace_batch  t;
  damar_trimmed      res;
  damar_filter_out   fo_, pre;
  damar_filter_params P = o->p, *p0 = &P;
  damar_las_out *wr = NULL;
  FILE   *fa = NULL, *f;
  unsigned char *state = NULL;
  uint64 *ranno = NULL, *tanno = NULL;
  int    *rdata = NULL, *tdata = NULL, *pairs = NULL, *soff = NULL, *slen = NULL, *sdata = NULL;
  int    *buf = NULL, *pbuf = NULL, *cnt = NULL, *pcnt = NULL;
  int64  *toff2 = NULL;
  int64   fcap = 0, ccap = 0, i, pi, tot[DAMAR_FC_COUNT], tndata = 0;
  int     got, rc = 1, have_db = 0, no_track, k, pass;

  memset(st, 0, sizeof(*st));
  memset(tot, 0, sizeof(tot));
  memset(&res, 0, sizeof(res));
  P.trim = NULL;  P.rep_anno = NULL;  P.rep_data = NULL;  P.sym_off = P.sym_len = P.sym_data = NULL;  P.read_state = NULL;  P.include = 0;
  if ((f = fopen(las, "r")) == NULL)
    { fprintf(stderr, "could not open %s\n", las);
      return 1;
    }
  fclose(f);
  if ((wr = damar_las_out_open(out, o->purge)) == NULL)
    { fprintf(stderr, "could not open %s\n", out);
      return 1;
    }
  if (damar_dbinfo_open(dbname, &db))
    { fprintf(stderr, "could not open %s\n", dbname);
      goto done;
    }
  have_db = 1;
  if (P.downsample && (P.downsample > 99 || P.downsample < 0))
    { fprintf(stderr, "invalid downsampling factor %d. must be in [1, 99]\n", P.downsample);
      goto done;
    }
  if (P.min_nonrep != -1)
    { if (damar_track_read_any(&db, o->rep_track, &ranno, &rdata, &P.rep_ndata))
        { damar_filter_no_track(o->rep_track);
          goto done;
        }
      P.rep_anno = ranno;
      P.rep_data = rdata;
    }
  if (damar_track_read_any(&db, o->trim_track, &tanno, &tdata, &tndata))
    { if (o->do_trim)
        { fprintf(stderr, "LAfilter: -T needs the trim track '%s', which does not exist\n", o->trim_track);
          goto done;
        }
      damar_filter_no_track(o->trim_track);            /* as in the reference: said, and done without */
    }
  else
    { pairs = (int *) damar_grow(NULL, sizeof(int) * 2 * ((size_t) db.nreads + 1), "filter");
      if (damar_trim_pairs(tanno, tdata, db.nreads, pairs))
        { fprintf(stderr, "LAfilter: the trim track '%s' does not hold one interval per read at most\n", o->trim_track);
          goto done;
        }
      P.trim = pairs;
    }
  if (o->exclude != NULL && o->include != NULL)
    { fprintf(stderr, "-x and -I cannot be used at the same time!!!");
      goto done;
    }
  for (pass = 0; pass < 2; pass++)
    { const char *path = pass == 0 ? o->exclude : o->include;
      int *v, nv;
      if (path == NULL)
        continue;
      if ((f = fopen(path, "r")) == NULL)
        { fprintf(stderr, "could not open %s\n", path);
          goto done;
        }
      v = read_integers(f, &nv);
      fclose(f);
      printf("%s %d reads\n", pass == 0 ? "excluding" : "including", nv);
      state = (unsigned char *) memset(damar_grow(NULL, (size_t) db.nreads + 1, "filter"), 0, (size_t) db.nreads + 1);
      for (k = 0; k < nv; k++)
        if (v[k] < 0 || v[k] >= db.nreads)
          fprintf(stderr, "[WARNING] LAfilter: %s read %d not possible! Must be in range: [0, %d]", pass == 0 ? "excluding" : "including", v[k],
                  db.nreads - 1);
        else
          state[v[k]] = pass == 0 ? 1 : 2;
      free(v);
      P.read_state = state;
      P.include = pass;
    }
  if (o->discarded_out != NULL && (fa = fopen(o->discarded_out, "w")) == NULL)
    { fprintf(stderr, "could not open %s\n", o->discarded_out);
      goto done;
    }
  if (o->discarded_in != NULL)
    { if (read_sym_list(o->discarded_in, db.nreads, &soff, &slen, &sdata, &P.sym_ndata))
        goto done;
      P.sym_off = soff;  P.sym_len = slen;  P.sym_data = sdata;
    }
  if (o->do_trim && (tm = damar_trimmer_open(dbname, &db, o->trim_track, &no_track)) == NULL)
    goto done;
  if ((r = damar_piles_open_traces(las, 0, 0)) == NULL)
    goto done;
  if (damar_las_out_begin(wr, damar_piles_tspace(r)))
    goto done;
  printf(GREEN "PASS filtering\n" RESET);

  while ((got = damar_piles_next_traces(r, &t)) > 0)
    { damar_trace_batch  m = t;
      damar_filter_params p = *p0;
      const int *rdiffs, *rlast, *dfs;
      double ms[4];
      int64  c3[3];
      const int with_pre = p0->downsample || (p0->seg_rate >= 0 && p0->seg_rate <= 100);

      damar_piles_rest(r, &rdiffs, &rlast);
      if (damar_batch_bind(&m.p, &db, las, DAMAR_BIND_A))
        goto done;
      if (damar_room(&fcap, t.p.nrec, 1024))                   /* one capacity: the three grow together */
        { buf = (int *) damar_grow(buf, sizeof(int) * 7 * (size_t) fcap, "filter");
          pbuf = (int *) damar_grow(pbuf, sizeof(int) * 7 * (size_t) fcap, "filter");
          toff2 = (int64 *) damar_grow(toff2, sizeof(int64) * (size_t) fcap, "filter");
        }
      if (damar_room(&ccap, t.p.npiles, 1024))
        { cnt = (int *) damar_grow(cnt, sizeof(int) * DAMAR_FC_COUNT * (size_t) ccap, "filter");
          pcnt = (int *) damar_grow(pcnt, sizeof(int) * DAMAR_FC_COUNT * (size_t) ccap, "filter");
        }
      fo_.flags = buf;  fo_.aepos = buf + fcap;  fo_.bepos = buf + 2 * fcap;  fo_.diffs = buf + 3 * fcap;  fo_.tlen = buf + 4 * fcap;
      fo_.reason = buf + 5 * fcap;  fo_.cont_by = buf + 6 * fcap;  fo_.cnt = cnt;
      pre.flags = pbuf;  pre.aepos = pbuf + fcap;  pre.bepos = pbuf + 2 * fcap;  pre.diffs = pbuf + 3 * fcap;  pre.tlen = pbuf + 4 * fcap;
      pre.reason = pbuf + 5 * fcap;  pre.cont_by = pbuf + 6 * fcap;  pre.cnt = pcnt;
      dfs = rdiffs;
      p.steps = DAMAR_FILTER_PRE | DAMAR_FILTER_MAIN;
      if (tm != NULL)
        { damar_trace_batch tt = t;
          /* -f and -b see the records as they lie in the file, the rest sees them cut */
          if (with_pre)
            { p.steps = DAMAR_FILTER_PRE;
              if (damar_pile_filter(&m, rdiffs, &p, &pre))
                goto done;
              damar_filter_last(ms, c3);
              st->host_piles += c3[1];
              for (pi = 0; pi < t.p.npiles; pi++)
                tot[DAMAR_FC_DIFFS] += pcnt[DAMAR_FC_COUNT * pi + DAMAR_FC_DIFFS];
              tt.p.flags = pre.flags;
            }
          if (damar_trimmer_batch(tm, &tt, rdiffs, las, st->novl, &st->trim, &res))
            goto done;
          m.p.abpos = res.abpos;  m.p.aepos = res.aepos;  m.p.bbpos = res.bbpos;  m.p.bepos = res.bepos;  m.p.flags = res.flags;
          for (i = 0; i < t.p.nrec; i++)
            toff2[i] = 2 * res.toff[i];
          m.trace = (const unsigned char *) res.trace;  m.trace_off = toff2;  m.tlen = res.tlen;  m.tbytes = 2;
          m.trace_bytes = t.p.nrec > 0 ? toff2[t.p.nrec - 1] + 2 * (int64) res.tlen[t.p.nrec - 1] : 0;
          for (i = 0; i + 1 < t.p.nrec; i++)
            if (toff2[i] + 2 * (int64) res.tlen[i] > m.trace_bytes)
              m.trace_bytes = toff2[i] + 2 * (int64) res.tlen[i];
          dfs = res.diffs;
          p.steps = DAMAR_FILTER_MAIN;
        }
      if (damar_pile_filter(&m, dfs, &p, &fo_))
        goto done;
      damar_filter_last(ms, c3);
      st->piles += c3[0];  st->host_piles += c3[1];
      for (pi = 0; pi < t.p.npiles; pi++)
        for (k = 0; k < DAMAR_FC_COUNT; k++)
          tot[k] += cnt[DAMAR_FC_COUNT * pi + k];
      for (pi = 0; pi < t.p.npiles; pi++)
        print_pile(&m, pi, o, &p, &fo_);

      for (pi = 0; pi < t.p.npiles; pi++)
        for (i = t.p.pile_off[pi]; i < t.p.pile_off[pi + 1]; i++)
          { int rec[10];
            if ((fo_.flags[i] & OVL_DISCARD) && fa != NULL)
              fprintf(fa, "%d %d\n", t.p.pile_aread[pi], t.p.bread[i]);
            rec[0] = fo_.tlen[i];
            rec[1] = fo_.diffs[i];
            rec[2] = m.p.abpos[i];  rec[3] = m.p.bbpos[i];  rec[4] = fo_.aepos[i];  rec[5] = fo_.bepos[i];
            rec[6] = fo_.flags[i];
            rec[7] = t.p.pile_aread[pi];  rec[8] = t.p.bread[i];  rec[9] = rlast[i];
            if (damar_las_out_put(wr, rec, t.trace + t.trace_off[i], tm != NULL ? res.trace + res.toff[i] : NULL, t.tbytes, "(null)"))
              goto done;
          }
      st->novl += t.p.nrec;
    }
  if (got < 0)
    goto done;
  for (k = 0; k < DAMAR_FC_COUNT; k++)
    st->cnt[k] = tot[k];
  /* filter_post, LAfilter.c:1762-1841 */
  if (tm != NULL)
    { printf("trimmed %lld of %lld overlaps\n", (long long) st->trim.ntrimmed, (long long) st->trim.novl);
      printf("trimmed %lld of %lld bases\n", (long long) st->trim.ntrim_bases, (long long) st->trim.novl_bases);
    }
  if (tot[DAMAR_FC_CONTAINED] > 0)
    printf("contained overlaps discarded         %10d\n", (int) tot[DAMAR_FC_CONTAINED]);
  if (tot[DAMAR_FC_READLEN] > 0)
    printf("min read length of %5d discarded         %10d\n", p0->min_rlen, (int) tot[DAMAR_FC_READLEN]);
  if (tot[DAMAR_FC_REPEAT] > 0)
    printf("min non-repeat bases of %4d discarded     %10d\n", p0->min_nonrep, (int) tot[DAMAR_FC_REPEAT]);
  if (tot[DAMAR_FC_DIFFS] > 0)
    printf("diff threshold of %.1f discarded             %d\n", p0->max_diffs * 100., (int) tot[DAMAR_FC_DIFFS]);
  if (tot[DAMAR_FC_LENGTH] > 0)
    printf("min overlap length of %d discarded                %10d\n", p0->min_olen, (int) tot[DAMAR_FC_LENGTH]);
  if (tot[DAMAR_FC_UNALIGNED] > 0)
    printf("unaligned bases threshold of %4d discarded    %10d\n", p0->max_unaligned, (int) tot[DAMAR_FC_UNALIGNED]);
  if (tot[DAMAR_FC_MULTI] > 0)
    printf("multiMapper of %4d discarded    %10d\n", (int) tot[DAMAR_FC_MULTI], (int) tot[DAMAR_FC_MULTI_BASES]);
  if (tot[DAMAR_FC_STITCHED] > 0)
    printf("stitched %4d at fuzzing of                   %10d\n", (int) tot[DAMAR_FC_STITCHED], p0->stitch);
  if (tot[DAMAR_FC_LOWCOV])
    printf("low tip coverage of <%2d discarded                %10d\n", p0->lowcov, (int) tot[DAMAR_FC_LOWCOV]);
  if (tot[DAMAR_FC_SYM])
    printf("symmetrically remove discarded overlaps          %10d\n", (int) tot[DAMAR_FC_SYM]);
  rc = 0;
done:
  if (damar_las_out_close(wr, rc == 0, &st->written, &st->discarded))
    rc = 1;
  fflush(stdout);
  damar_piles_close(r);
  damar_trimmer_close(tm);
  if (have_db) damar_dbinfo_close(&db);
  if (fa != NULL && fclose(fa) != 0 && rc == 0)
    rc = damar_cannot_write(o->discarded_out);
  free(buf);  free(pbuf);  free(cnt);  free(pcnt);  free(toff2);
  free(state);  free(ranno);  free(rdata);  free(tanno);  free(tdata);  free(pairs);  free(soff);  free(slen);  free(sdata);
  return rc;
}
