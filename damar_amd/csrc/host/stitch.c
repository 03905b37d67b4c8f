/* stitch.c -- LAstitch: the records of one (A read, B read) that the overlapper split at a bad stretch are rejoined
 * (scrub/LAstitch.c stitch_handler2, the handler its main hands to the record loop of lib/pass.c with split_b = 1).
 *
 * For a pair of records (i, k > i) of a group that passes the candidate tests, the joint is boxed with margins snapped to
 * the two paths' own trace points (Compute_Bridge_Path), the box is realigned exactly into trace pairs, the result is
 * checked (Check_Bridge) and spliced between the head of i and the tail of k (Bridge); k is flagged.  A success changes
 * record i for every later k, so a group's candidates are a chain.  The reference aligns as it meets them.  Here a batch
 * of whole piles goes through rounds: every group that still has a candidate puts its next box into the round's list, all
 * boxes of the round go through one damar_trace_boxes call (kernels/box_trace.hip, or the host routine), the results are
 * applied and the groups move on.  Nearly all boxes are the first round's.
 * Nothing here touches the GPU runtime but that one call. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "damar_hip.h"
#include "damar_host.h"

#define MAX_STITCH_ALIGN_ERROR 0.57

int damar_stitch_on_host(void)
{ const char *e = getenv("DAMAR_STITCH");
  return e != NULL && strcmp(e, "host") == 0;
}

/***** tracks (-t, -r) ****************************************************************************/

typedef struct
{ uint64 *anno;                /* [nreads + 1] byte offsets */
  int    *data;
  int64   ndata;
} Track;

static int load_track(const damar_dbinfo *db, const char *name, Track *t)
{ int64 j;
  if (damar_track_read_any(db, name, &t->anno, &t->data, &t->ndata))
    { fprintf(stderr, "(null): Track '%s' does not exist\n", name);     /* the loader's line: it never sets its program name */
      fprintf(stderr, "could not load track %s\n", name);
      return 1;
    }
  for (j = 0; j <= db->nreads; j++)                            /* what the walks below index with */
    if (t->anno[j] / sizeof(int) > (uint64) t->ndata || (t->anno[j] / sizeof(int)) % 2 != 0 || (j > 0 && t->anno[j] < t->anno[j - 1]))
      { fprintf(stderr, "damar: track %s is not a track of intervals of this database\n", name);
        return 1;
      }
  return 0;
}

/***** a record while it is worked on ***************************************************************/

typedef struct
{ int   tlen, diffs;
  int   abpos, bbpos, aepos, bepos;
  int   flags;
  int64 toff;                  /* its trace in the pool, two bytes a value */
} SRec;

typedef struct
{ uint16 *val;
  int64   top, max;
} Pool;

typedef struct
{ int64 first;                 /* the group's records: [first, first + n) of the batch */
  int   n, aread, bread;
  int   i, k;                  /* the pair to look at next; k == 0: record i is not begun */
  int   ab1, ae1, bb1, be1;    /* record i as the candidate tests see it (LAstitch.c:969-973, :1114) */
  int   lc;                    /* the pending candidate came through the low-complexity test */
  int   box_ab, box_ae, box_bb, box_be;
} Group;

typedef struct
{ const damar_stitch_params *p;
  const damar_dbinfo *db;
  const Track *lc, *rep;       /* NULL: none */
  int   tw;
  SRec *rec;
  Pool  pool;
  damar_stitch_stats *st;
} Ctx;

/* LAstitch.c:310-361: the bases of [from, to) of a read outside the repeat track (-r, else -t, else all of them) */
static int anchor_bases(const Ctx *c, int read, int from, int to)
{ const Track *t = c->rep ? c->rep : c->lc;
  uint64 rb, re;
  int    rep = 0;
  if (from >= to)
    return 0;
  if (t == NULL)
    return to - from;
  rb = t->anno[read] / sizeof(int);
  re = t->anno[read + 1] / sizeof(int);
  for (; rb < re; rb += 2)
    rep += damar_intersect(from, to, t->data[rb], t->data[rb + 1]);
  return (to - from - rep > 0) ? to - from - rep : 0;
}

/* LAstitch.c:426-497 and :515-581, the verdict on one merged interval [b, e) of the low-complexity track: -1 the interval
   does not decide, else the answer.  last: the call after the loop, whose sixth case divides by the wrong length. */
static int lc_verdict(const Ctx *c, int aread, const SRec *o1, const SRec *o2, int b, int e, int last)
{ int gLenA, gLenB;
  double diff = 1.0;
  if (e - b < c->p->min_len)
    return -1;
  if (!(anchor_bases(c, aread, o1->abpos, b) >= c->p->anchor && o1->aepos + 200 > b && o1->aepos - 25 < e))
    return -1;
  if (!(anchor_bases(c, aread, e, o2->aepos) >= c->p->anchor && o2->abpos + 25 > b && o2->abpos - 200 < e))
    return -1;
  gLenA = o2->abpos - o1->aepos;
  gLenB = o2->bbpos - o1->bepos;
  if (gLenA > 0 && gLenB > 0)
    diff = (gLenA < gLenB) ? 1.0 - gLenA * 1.0 / gLenB : 1.0 - gLenB * 1.0 / gLenA;
  else if (gLenA < 0 && gLenB < 0)
    diff = (gLenA < gLenB) ? 1.0 - gLenB * 1.0 / gLenA : 1.0 - gLenA * 1.0 / gLenB;
  else if (gLenA < 0)
    { gLenB = gLenB + abs(gLenA);
      diff = 1.0 - abs(gLenA) * 1.0 / gLenB;
    }
  else
    { gLenA = gLenA + abs(gLenB);
      diff = last ? 1.0 - abs(gLenB) * 1.0 / gLenB : 1.0 - abs(gLenB) * 1.0 / gLenA;
    }
  return diff < (double) (float) c->p->gap_diff;
}

/* LAstitch.c:363-587 */
static int low_complexity_break(const Ctx *c, int aread, const SRec *o1, const SRec *o2)
{ const Track *t = c->lc;
  uint64 ob, oe;
  int    b, e, v;
  if (t == NULL)
    return 0;
  ob = t->anno[aread];
  oe = t->anno[aread + 1];
  if (ob >= oe)
    return 0;
  ob /= sizeof(int);
  oe /= sizeof(int);
  b = t->data[ob];
  e = t->data[ob + 1];
  for (ob += 2; ob < oe; ob += 2)
    { if (e + c->p->merge >= t->data[ob])                      /* close by: merged when it is long enough, else passed over */
        { if (t->data[ob + 1] - t->data[ob] >= c->p->min_merge)
            e = t->data[ob + 1];
          continue;
        }
      if ((v = lc_verdict(c, aread, o1, o2, b, e, 0)) >= 0)
        return v;
      b = t->data[ob];
      e = t->data[ob + 1];
    }
  v = lc_verdict(c, aread, o1, o2, b, e, 1);
  return v > 0;
}

/* LAstitch.c:665-747 MapToTPAbove / MapToTPBelow with isA = 1, the only way they are called: the trace point of the path
   at or above (below) *x in A; *x is snapped to it, the B coordinate is returned */
static int tp_above(const Ctx *c, const SRec *p, int *x)
{ const uint16 *t = c->pool.val + p->toff;
  const int tw = c->tw;
  int a = (p->abpos / tw) * tw, b = p->bbpos, i;
  for (i = 1; i < p->tlen; i += 2)
    { a += tw;
      b += t[i];
      if (a > p->aepos)
        a = p->aepos;
      if (a >= *x)
        break;
    }
  *x = a;
  return b;
}

static int tp_below(const Ctx *c, const SRec *p, int *x)
{ const uint16 *t = c->pool.val + p->toff;
  const int tw = c->tw;
  int a = ((p->aepos + (tw - 1)) / tw) * tw, b = p->bepos, i;
  for (i = p->tlen - 1; i >= 0; i -= 2)
    { a -= tw;
      b -= t[i];
      if (a < p->abpos)
        a = p->abpos;
      if (a <= *x)
        break;
    }
  *x = a;
  return b;
}

/* LAstitch.c:785-862, Compute_Bridge_Path up to the alignment: the box of the joint of o1 and o2 into g; 1: no box */
static int bridge_box(const Ctx *c, const SRec *o1, const SRec *o2, Group *g)
{ const int tw = c->tw;
  int ain = o2->abpos, aout = o1->aepos, bin, bout, i;
  bin = tp_below(c, o1, &ain);
  bout = tp_above(c, o2, &aout);
  for (i = 0; bin > o2->bbpos && i < 10; i++)                  /* the joint widened by an interval on either side */
    { ain = (ain - tw) / tw * tw;
      aout = (aout + tw) / tw * tw;
      if (ain < o1->abpos || aout > o2->aepos)
        return 1;
      bin = tp_below(c, o1, &ain);
      bout = tp_above(c, o2, &aout);
    }
  if (bout < bin)
    return 1;
  if (i > 0)
    c->st->widened += 1;
  g->box_ab = ain - 2 * tw;
  g->box_ae = aout + 2 * tw;
  g->box_bb = tp_below(c, o1, &g->box_ab);
  g->box_be = tp_above(c, o2, &g->box_ae);
  return 0;
}

/* LAstitch.c:749-783 */
static int check_bridge(const uint16 *t, int tlen, int diffs, int tw)
{ int i, cum = 0, bad = 0;
  for (i = 0; i < tlen; i += 2)
    { if (tw <= TRACE_XOVR && (t[i] > 250 || t[i + 1] > 250))
        return 1;
      cum += t[i];
      if (1.0 * t[i] / t[i + 1] > MAX_STITCH_ALIGN_ERROR && i + 2 < tlen)       /* the last segment is let off */
        bad += 1;
    }
  return cum != diffs || bad > 0;
}

/* LAstitch.c:593-663 Bridge: head := head[.. box] ++ box ++ tail[box ..] in a fresh stretch of the pool.  0, or 1 when the
   pieces do not fit each other (a malformed record) */
static int splice(Ctx *c, SRec *head, const Group *g, const uint16 *box, int box_tlen, const SRec *tail)
{ const int tw = c->tw;
  const int k1 = 2 * ((g->box_ab / tw) - (head->abpos / tw));
  const int k2 = (g->box_ae == tail->aepos) ? tail->tlen : 2 * ((g->box_ae / tw) - (tail->abpos / tw));
  const int total = k1 + box_tlen + (tail->tlen - k2);
  Pool  *P = &c->pool;
  int    j, n = 0, diffs = 0;
  int64  at;
  if (k1 < 0 || k1 > head->tlen || k2 < 0 || k2 > tail->tlen)
    return 1;
  if (P->top + total >= P->max)
    { P->max = (int64) (1.2 * (double) (P->top + total)) + 1000;
      P->val = (uint16 *) damar_grow(P->val, sizeof(uint16) * (size_t) P->max, "stitch");
    }
  at = P->top;
  P->top += total;
  for (j = 0; j < k1; j++)
    P->val[at + n++] = P->val[head->toff + j];
  for (j = 0; j < box_tlen; j++)
    P->val[at + n++] = box[j];
  for (j = k2; j < tail->tlen; j++)
    P->val[at + n++] = P->val[tail->toff + j];
  for (j = 0; j < n; j += 2)
    diffs += P->val[at + j];
  head->aepos = tail->aepos;
  head->bepos = tail->bepos;
  head->diffs = diffs;
  head->toff = at;
  head->tlen = n;
  return 0;
}

/* The loops of stitch_handler2 (LAstitch.c:962-1122) up to the next pair that wants a box: 1 and the box in g, or 0 when the
   group is through. */
static int next_candidate(const Ctx *c, Group *g)
{ SRec *ovl = c->rec + g->first;
  const int fuzz = c->p->fuzz;
  while (g->i < g->n)
    { const SRec *oi = ovl + g->i;
      if (g->k == 0)
        { if (oi->flags & OVL_DISCARD)
            { g->i += 1;
              continue;
            }
          g->ab1 = oi->abpos;  g->ae1 = oi->aepos;  g->bb1 = oi->bbpos;  g->be1 = oi->bepos;
          g->k = g->i + 1;
        }
      for (; g->k < g->n; g->k++)
        { const SRec *ok = ovl + g->k;
          if ((ok->flags & OVL_DISCARD) || (oi->flags & OVL_COMP) != (ok->flags & OVL_COMP))
            continue;
          if (g->ab1 > ok->abpos || g->ae1 > ok->aepos || g->bb1 > ok->bbpos || g->be1 > ok->bepos)
            continue;
          if (anchor_bases(c, g->aread, oi->abpos, oi->aepos) < c->p->anchor || anchor_bases(c, g->aread, ok->abpos, ok->aepos) < c->p->anchor)
            continue;
          g->lc = low_complexity_break(c, g->aread, oi, ok);
          if (!((abs(g->ae1 - ok->abpos) < fuzz && abs(g->be1 - ok->bbpos) < fuzz && abs((g->ae1 - ok->abpos) - (g->be1 - ok->bbpos)) < fuzz) ||
                g->lc))
            continue;
          c->st->candidates += 1;
          if (bridge_box(c, oi, ok, g))
            { c->st->no_box += 1;
              continue;
            }
          return 1;
        }
      g->i += 1;
      g->k = 0;
    }
  return 0;
}

int damar_stitch_las(const char *dbname, const char *las, const char *out, const damar_stitch_params *p, damar_stitch_stats *st)
{ damar_dbinfo db;
  HITS_DB blk;
  Track   lc, rep;
  Ctx     c;
  damar_pile_reader *r = NULL;
  damar_trace_batch  t;
  damar_las_out *wr = NULL;
  Group  *grp = NULL;
  int64  *act = NULL;          /* the groups of the round, one box each */
  int    *arec = NULL, *bm = NULL, *bn = NULL, *bab = NULL, *bdiffs = NULL;
  int64  *baoff = NULL, *bboff = NULL, *toff = NULL;
  char   *bases = NULL;
  int64   rcap = 0, gcap = 0, bcap = 0, basecap = 0, i;
  int     got, rc = 1, have_db = 0, have_blk = 0, tw, tbytes;

  memset(st, 0, sizeof(*st));
  memset(&lc, 0, sizeof(lc));
  memset(&rep, 0, sizeof(rep));
  memset(&c, 0, sizeof(c));
  if (damar_dbinfo_open(dbname, &db))
    return 1;
  have_db = 1;
  c.p = p;
  c.db = &db;
  c.st = st;
  if (p->lc_track != NULL)
    { if (load_track(&db, p->lc_track, &lc))
        goto done;
      c.lc = &lc;
    }
  if (p->rep_track != NULL)
    { if (load_track(&db, p->rep_track, &rep))
        goto done;
      c.rep = &rep;
    }
  if (damar_read_block(dbname, &blk))
    goto done;
  have_blk = 1;
  if ((r = damar_piles_open_traces(las, 0, 0)) == NULL)
    goto done;
  if ((wr = damar_las_out_open(out, p->purge)) == NULL)
    { fprintf(stderr, "could not open '%s'\n", out);
      goto done;
    }
  tw = damar_piles_tspace(r);
  if (tw < 1)
    { fprintf(stderr, "damar: %s: trace spacing %d\n", las, tw);
      goto done;
    }
  c.tw = tw;
  tbytes = (tw <= TRACE_XOVR) ? 1 : 2;
  st->novl = damar_piles_novl(r);
  if (damar_las_out_begin(wr, tw))
    goto done;

  while ((got = damar_piles_next_traces(r, &t)) > 0)
    { const damar_pile_batch *b = &t.p;
      const int *rdiffs, *rlast;
      int64 nval = 0, pi, ngrp = 0, nact, k;
      int   round = 0;

      damar_piles_rest(r, &rdiffs, &rlast);
      for (i = 0; i < b->nrec; i++) nval += t.tlen[i];
      if (damar_room(&rcap, b->nrec, 1024))
        { c.rec = (SRec *) damar_grow(c.rec, sizeof(SRec) * (size_t) rcap, "stitch");
          arec = (int *) damar_grow(arec, sizeof(int) * (size_t) rcap, "stitch");
        }
      if (nval + 1 > c.pool.max)
        { c.pool.max = nval + nval / 2 + 4096;
          c.pool.val = (uint16 *) damar_grow(c.pool.val, sizeof(uint16) * (size_t) c.pool.max, "stitch");
        }
      for (i = 0, nval = 0; i < b->nrec; i++)
        { const unsigned char *src = t.trace + t.trace_off[i];
          SRec *o = c.rec + i;
          o->tlen = t.tlen[i];  o->diffs = rdiffs[i];  o->flags = b->flags[i];  o->toff = nval;
          o->abpos = b->abpos[i];  o->aepos = b->aepos[i];  o->bbpos = b->bbpos[i];  o->bepos = b->bepos[i];
          if (tbytes == 1)
            for (k = 0; k < t.tlen[i]; k++) c.pool.val[nval + k] = src[k];
          else
            memcpy(c.pool.val + nval, src, sizeof(uint16) * (size_t) t.tlen[i]);
          nval += t.tlen[i];
        }
      c.pool.top = nval;

      /* the groups: runs of one (A read, B read) of at least two records that are no identity overlaps */
      for (pi = 0; pi < b->npiles; pi++)
        { const int a = b->pile_aread[pi];
          int64 lo = b->pile_off[pi], hi = b->pile_off[pi + 1], e;
          if (a < 0 || a >= db.nreads)
            { damar_reads_missing(las);
              goto done;
            }
          for (i = lo; i < hi; i++)
            { const SRec *o = c.rec + i;
              const int   br = b->bread[i], nseg = (o->aepos + tw - 1) / tw - o->abpos / tw;
              arec[i] = a;
              if (br < 0 || br >= db.nreads || o->tlen != 2 * nseg || o->abpos < 0 || o->aepos > db.read_len[a] || o->abpos >= o->aepos ||
                  o->bbpos < 0 || o->bepos > db.read_len[br])
                { fprintf(stderr, "damar: %s: record %lld is malformed\n", las, (long long) (damar_las_out_written(wr) + i));
                  goto done;
                }
            }
          for (; lo < hi; lo = e)
            { for (e = lo + 1; e < hi && b->bread[e] == b->bread[lo]; e++)
                ;
              if (e - lo < 2 || b->bread[lo] == a)
                continue;
              if (ngrp >= gcap)
                { gcap = gcap + gcap / 4 + 1024;
                  grp = (Group *) damar_grow(grp, sizeof(Group) * (size_t) gcap, "stitch");
                  act = (int64 *) damar_grow(act, sizeof(int64) * (size_t) gcap, "stitch");
                }
              memset(grp + ngrp, 0, sizeof(Group));
              grp[ngrp].first = lo;  grp[ngrp].n = (int) (e - lo);  grp[ngrp].aread = a;  grp[ngrp].bread = b->bread[lo];
              ngrp += 1;
            }
        }

      /* rounds: at most one box of every group that still has a candidate */
      for (nact = 0, k = 0; k < ngrp; k++)
        if (next_candidate(&c, grp + k))
          act[nact++] = k;
      while (nact > 0)
        { damar_tbox_batch tb;
          uint16 *trace = NULL;
          int64   nbase = 0, keep = 0;
          if (damar_room(&bcap, nact, 1024))
            { bm = (int *) damar_grow(bm, sizeof(int) * (size_t) bcap, "stitch");
              bn = (int *) damar_grow(bn, sizeof(int) * (size_t) bcap, "stitch");
              bab = (int *) damar_grow(bab, sizeof(int) * (size_t) bcap, "stitch");
              bdiffs = (int *) damar_grow(bdiffs, sizeof(int) * (size_t) bcap, "stitch");
              baoff = (int64 *) damar_grow(baoff, sizeof(int64) * (size_t) bcap, "stitch");
              bboff = (int64 *) damar_grow(bboff, sizeof(int64) * (size_t) bcap, "stitch");
              toff = (int64 *) damar_grow(toff, sizeof(int64) * ((size_t) bcap + 1), "stitch");
            }
          for (k = 0; k < nact; k++)
            { const Group *g = grp + act[k];
              bm[k] = g->box_ae - g->box_ab;
              bn[k] = g->box_be - g->box_bb;
              bab[k] = g->box_ab;
              if (bm[k] < 1 || bn[k] < 1)
                { fprintf(stderr, "damar: %s: the joint of two records of reads %d and %d has no box (%d x %d)\n", las, g->aread, g->bread,
                          bm[k], bn[k]);
                  goto done;
                }
              baoff[k] = nbase;
              bboff[k] = nbase + bm[k];
              nbase += bm[k] + bn[k];
              st->box_a += bm[k];
              st->box_b += bn[k];
            }
          bases = (char *) damar_reserve(bases, &basecap, nbase, 1, 4096, "stitch");
          for (k = 0; k < nact; k++)
            { const Group *g = grp + act[k];
              const int comp = c.rec[g->first + g->i].flags & OVL_COMP, blen = db.read_len[g->bread];
              memcpy(bases + baoff[k], (const char *) blk.bases + blk.reads[g->aread].boff + g->box_ab, (size_t) bm[k]);
              /* a complement pair is realigned as the reference realigns it: its B coordinates, which are the complement's
                 already, mapped through the read's length once more (LAstitch.c:856-862) */
              if (comp)
                damar_gather_b(&blk, g->bread, 1, blen - g->box_be, blen - g->box_bb, bases + bboff[k]);
              else
                damar_gather_b(&blk, g->bread, 0, g->box_bb, g->box_be, bases + bboff[k]);
            }
          tb.nbox = nact;  tb.m = bm;  tb.n = bn;  tb.abpos = bab;  tb.aoff = baoff;  tb.boff = bboff;  tb.bases = bases;
          tb.nbases = nbase;  tb.tspace = tw;
          if (damar_trace_boxes(&tb, bdiffs, toff, &trace))
            goto done;
          st->boxes += nact;
          st->round_boxes[round < DAMAR_STITCH_ROUNDS ? round : DAMAR_STITCH_ROUNDS - 1] += nact;
          round += 1;

          for (k = 0; k < nact; k++)
            { Group  *g = grp + act[k];
              SRec   *oi = c.rec + g->first + g->i, *ok = c.rec + g->first + g->k;
              uint16 *bt = trace + toff[k];
              const int btlen = (int) (toff[k + 1] - toff[k]);
              if (oi->flags & OVL_COMP)                   /* ... and its pairs turned round (LAstitch.c:883-897) */
                { int x, y;
                  for (x = 0, y = btlen - 2; x < y; x += 2, y -= 2)
                    { const uint16 d = bt[x], l = bt[x + 1];
                      bt[x] = bt[y];  bt[x + 1] = bt[y + 1];
                      bt[y] = d;      bt[y + 1] = l;
                    }
                }
              if (check_bridge(bt, btlen, bdiffs[k], tw))
                st->refused += 1;
              else
                { int64 bpos;
                  int   j;
                  if (splice(&c, oi, g, bt, btlen, ok))
                    { fprintf(stderr, "damar: %s: the traces of two records of reads %d and %d do not fit their coordinates\n", las, g->aread,
                              g->bread);
                      free(trace);
                      goto done;
                    }
                  for (bpos = oi->bbpos, j = 1; j < oi->tlen; j += 2)
                    bpos += c.pool.val[oi->toff + j];
                  if (bpos != ok->bepos)                       /* the reference's assert (LAstitch.c:1111), which its build keeps */
                    { fprintf(stderr, "LAstitch: the stitched trace of reads %d and %d ends at %lld in B, the record at %d\n", g->aread,
                              g->bread, (long long) bpos, ok->bepos);
                      free(trace);
                      goto done;
                    }
                  ok->flags |= OVL_DISCARD | OVL_STITCH;
                  g->ae1 = ok->aepos;
                  g->be1 = ok->bepos;
                  if (g->lc)
                    st->stitched_lc += 1;
                  else
                    st->stitched += 1;
                }
              g->k += 1;
              if (next_candidate(&c, g))
                act[keep++] = act[k];
            }
          free(trace);
          nact = keep;
        }
      if (round > st->rounds)
        st->rounds = round;

      /* the records as they go to the file */
      for (i = 0; i < b->nrec; i++)
        { const SRec   *o = c.rec + i;
          const uint16 *v = c.pool.val + o->toff;
          int   rec[10];
          rec[0] = o->tlen;  rec[1] = o->diffs;  rec[2] = o->abpos;  rec[3] = o->bbpos;  rec[4] = o->aepos;  rec[5] = o->bepos;
          rec[6] = o->flags;
          rec[7] = arec[i];  rec[8] = b->bread[i];  rec[9] = rlast[i];
          if (damar_las_out_put(wr, rec, NULL, v, tbytes, "(null)"))
            goto done;
        }
    }
  if (got < 0)
    goto done;
  rc = 0;
done:
  if (wr != NULL && damar_las_out_close(wr, rc == 0, &st->written, &st->discarded))
    rc = 1;
  damar_piles_close(r);
  if (have_blk) damar_close_block(&blk);
  if (have_db) damar_dbinfo_close(&db);
  free(lc.anno);  free(lc.data);  free(rep.anno);  free(rep.data);
  free(c.rec);  free(c.pool.val);  free(grp);  free(act);  free(arec);
  free(bm);  free(bn);  free(bab);  free(bdiffs);  free(baoff);  free(bboff);  free(toff);  free(bases);
  return rc;
}
