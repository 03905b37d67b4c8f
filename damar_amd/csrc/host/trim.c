/* trim.c -- LAtrim: every overlap record cut back to the part of both reads that the trim track keeps (lib/trim.c:188-470
 * trim_overlap, around it scrub/LAtrim.c and the record loop of lib/pass.c).
 *
 * A cut on A drops whole trace segments and moves the A coordinates.  A cut on B that falls inside a trace segment needs
 * that one segment aligned exactly: the cut's A coordinate and the differences on either side of it are read off the
 * optimal path.  The reference aligns as it meets the records.  Here a batch of whole piles goes through three phases:
 *   plan    -- from the trim track and the trace alone: each record's fate, everything of its new coordinates and trace
 *              that no alignment decides, and the boxes (at most a left and a right one) it wants aligned;
 *   align   -- all boxes of the batch in one damar_align_boxes call (kernels/box_align.hip, or the host routine);
 *   settle  -- each box's script walked for the cut, the left box's values patched in before the right one's, the final
 *              discard test and the differences summed again from the trace.
 * The three phases are damar_trimmer_batch, on one batch in memory; damar_trim_las is the file loop around it, and gap.c
 * (LAgap -t) runs the same routine on its batches.
 * Nothing here touches the GPU runtime but that one call. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "damar_hip.h"
#include "damar_host.h"

int damar_trim_on_host(void)
{ const char *e = getenv("DAMAR_TRIM");
  return e != NULL && strcmp(e, "host") == 0;
}

/***** the trim track ***************************************************************************/

typedef struct
{ uint64 *anno;                /* [nreads + 1] byte offsets */
  int    *data;
  int64   ndata;
} TrimTrack;

/* lib/utils.c:258-284: a read without an entry, or with an empty one, keeps nothing.  (fix.c's trim_of is another rule:
   it refuses an entry that is no interval and takes a missing track for the whole read.) */
static void trim_of(const TrimTrack *t, int rid, int *b, int *e)
{ const uint64 ob = t->anno[rid] / sizeof(int), oe = t->anno[rid + 1] / sizeof(int);
  *b = *e = 0;
  if (oe - ob >= 2 && oe <= (uint64) t->ndata && t->data[ob] < t->data[ob + 1])
    { *b = t->data[ob];
      *e = t->data[ob + 1];
    }
}

/***** plan *************************************************************************************/

enum { FATE_ASIS = 0, FATE_GONE, FATE_CUT };

typedef struct                 /* a trace segment to align: A[ab, ae) against B[bb, be), the cut at B position stop */
{ int ab, ae, bb, be, stop;
} Seg;

typedef struct
{ int   fate;
  int   t0, tlen;              /* the trace values kept: [t0, t0 + tlen) of the record's */
  int   abpos, aepos, bbpos, bepos;
  int   a_lo, a_hi;            /* A coordinates the cuts are measured from (what the cut on A left) */
  int   keep_lo, keep_hi;      /* what the trim track keeps of B, in the record's orientation */
  int64 lbox, rbox;            /* the record's boxes in the batch's list, -1: none */
  int64 known;                 /* trimmed bases that no alignment decides */
} Plan;

typedef struct
{ Seg   *seg;
  int64 *rec;                  /* the record a box belongs to */
  int64  n, cap;
} SegList;

static int64 add_seg(SegList *L, int64 rec, int ab, int ae, int bb, int be, int stop)
{ if (L->n >= L->cap)
    { L->cap = L->cap + L->cap / 4 + 1024;
      L->seg = (Seg *) damar_grow(L->seg, sizeof(Seg) * (size_t) L->cap, "trim");
      L->rec = (int64 *) damar_grow(L->rec, sizeof(int64) * (size_t) L->cap, "trim");
    }
  L->seg[L->n].ab = ab;  L->seg[L->n].ae = ae;  L->seg[L->n].bb = bb;  L->seg[L->n].be = be;  L->seg[L->n].stop = stop;
  L->rec[L->n] = rec;
  return L->n++;
}

/* One record: tr is its trace, two values (differences, B length) per segment, and is patched where the new value is
   known already.  tw: the trace spacing.  trim.c:188-424 without the two alignments. */
static void plan_record(Plan *p, uint16 *tr, int tlen, int tw, int a_lo, int a_hi, int b_lo, int b_hi, int64 rec, SegList *L,
                        damar_trim_stats *st)
{ int abt, aet, bbt, bet, j;

  p->lbox = p->rbox = -1;
  p->known = 0;
  p->t0 = 0;
  p->tlen = tlen;
  p->keep_lo = b_lo;  p->keep_hi = b_hi;
  abt = (a_lo > p->abpos) ? a_lo : p->abpos;
  aet = (a_hi < p->aepos) ? a_hi : p->aepos;
  bbt = (b_lo > p->bbpos) ? b_lo : p->bbpos;
  bet = (b_hi < p->bepos) ? b_hi : p->bepos;
  if (abt >= aet || bbt >= bet)
    { p->fate = FATE_GONE;
      return;
    }
  if (abt == p->abpos && aet == p->aepos && bbt == p->bbpos && bet == p->bepos)
    { p->fate = FATE_ASIS;
      return;
    }
  p->fate = FATE_CUT;
  st->ntrimmed += 1;

  if (abt != p->abpos || aet != p->aepos)                      /* whole segments go, B follows by their lengths */
    { int drop = abt / tw - p->abpos / tw;
      for (j = 0; j < drop; j++)
        p->bbpos += tr[2 * j + 1];
      p->t0 = 2 * drop;
      p->tlen -= 2 * drop;
      drop = (p->aepos - 1) / tw - (aet - 1) / tw;
      for (j = 0; j < drop; j++)
        p->bepos -= tr[p->t0 + p->tlen - 1 - 2 * j];
      p->tlen -= 2 * drop;
      p->abpos = abt;
      p->aepos = aet;
    }
  p->a_lo = p->abpos;
  p->a_hi = p->aepos;

  bbt = (b_lo > p->bbpos) ? b_lo : p->bbpos;
  bet = (b_hi < p->bepos) ? b_hi : p->bepos;
  if (bbt >= bet || (bbt == p->bbpos && bet == p->bepos))
    return;

  if (p->bbpos < bbt)                                          /* the segment the left cut falls in becomes the first */
    { uint16 *t = tr + p->t0;
      int sab = p->abpos, sae = (p->abpos / tw + 1) * tw, sbb = p->bbpos, sbe = p->bbpos + t[1];
      for (j = 2; j < p->tlen; j += 2)
        { if (sbb <= bbt && sbe > bbt)
            break;
          sab = sae;  sae += tw;
          sbb = sbe;  sbe += t[j + 1];
        }
      if (sbb != bbt)
        { p->lbox = add_seg(L, rec, sab, sae, sbb, sbe, bbt);
          t[j - 1] = (uint16) (sbe - bbt);
          p->known += bbt - p->bbpos;
        }
      else                                                     /* exactly on a segment's B boundary: nothing to align */
        { p->known += (sab - p->abpos) + (sbb - p->bbpos);
          p->abpos = sab;
        }
      p->bbpos = bbt;
      p->t0 += j - 2;
      p->tlen -= j - 2;
    }

  if (p->bepos > bet)                                          /* ... and the one of the right cut the last */
    { uint16 *t = tr + p->t0;
      int sae = p->aepos, sab = (sae % tw) ? sae - sae % tw : sae - tw;
      int sbe = p->bepos, sbb = sbe - t[p->tlen - 1];          /* the first segment's B start is what the left cut set */
      for (j = p->tlen - 4; j >= 0; j -= 2)
        { if (sbb < bet && sbe >= bet)
            break;
          sae = sab;  sab -= tw;
          sbe = sbb;  sbb -= t[j + 1];
        }
      if (sbe != bet)
        { p->rbox = add_seg(L, rec, sab, sae, sbb, sbe, bet);
          t[j + 3] = (uint16) (bet - sbb);
          p->known += p->bepos - bet;
        }
      else
        { p->known += (p->aepos - sae) + (p->bepos - sbe);
          p->aepos = sae;
        }
      p->bepos = bet;
      p->tlen = j + 4;
    }
}

/***** settle ***********************************************************************************/

/* Where the path of a box crosses B position `stop` (all positions counted from the box's corner), and the differences
   on either side of that point: trim.c:71-158. */
typedef struct { const char *A, *B; int a, b, diffs, stop, stop_a, left; } Walk;

static void note_cut(Walk *w)
{ if (w->b == w->stop)
    { w->stop_a = w->a;
      w->left = w->diffs;
      w->diffs = 0;
    }
}

static void walk_column(Walk *w)                               /* a base of A over a base of B */
{ if (w->A[w->a] != w->B[w->b])
    w->diffs += 1;
  w->a += 1;
  w->b += 1;
  note_cut(w);
}

static void walk_script(const char *A, int M, const char *B, const int *script, int slen, int stop, int *stop_a, int *dl, int *dr)
{ Walk w;
  int  t;
  w.A = A;  w.B = B;  w.a = w.b = w.diffs = w.stop_a = w.left = 0;  w.stop = stop;
  for (t = 0; t < slen; t++)
    { const int p = script[t];
      if (p < 0)                                               /* a base of B alone, in front of A position -p - 1 */
        { while (w.a < -p - 1)
            walk_column(&w);
          w.diffs += 1;
          w.b += 1;
          note_cut(&w);
        }
      else                                                     /* a base of A alone, in front of B position p - 1 */
        { while (w.b < p - 1)
            walk_column(&w);
          w.diffs += 1;
          w.a += 1;
        }
    }
  while (w.a < M)
    walk_column(&w);
  *stop_a = w.stop_a;
  *dl = w.left;
  *dr = w.diffs;
}

/***** the pass *********************************************************************************/

/* The A side of a box ends on a segment boundary, which for a cut in a read's last segment lies beyond the read's end.  The
   reference aligns what its read buffer holds there: the end mark, then the bases of the last longer read that was loaded
   for an alignment before.  That buffer is kept here as the reference keeps it, so that such a box sees the same bases. */
typedef struct
{ char *base;                  /* maxlen + one spacing of room, zero at the start */
  int   room, holds;           /* holds: the read loaded last, -1 none */
} ABuffer;

static void load_a(ABuffer *ab, const HITS_DB *blk, int r)
{ if (ab->holds != r)
    { const int len = blk->reads[r].rlen;
      memcpy(ab->base, (const char *) blk->bases + blk->reads[r].boff, (size_t) len);
      ab->base[len] = 4;
      ab->holds = r;
    }
}

/* What a batch needs beyond its records: the track, the bases, and every buffer the three phases work in.  One trimmer
   serves all batches of a file, in file order (the A buffer above depends on that order). */
struct damar_trimmer
{ const damar_dbinfo *db;
  HITS_DB   blk;
  TrimTrack tt;
  int       have_blk;
  uint16 *tr;                  /* the batch's traces, two bytes a value */
  int64  *troff;               /* per record: where its values begin in tr */
  Plan   *plan;
  SegList L;
  ABuffer abuf;
  char   *bases;
  int    *arec;                /* per record: its A read */
  int    *bm, *bn, *bdiffs;
  int64  *baoff, *bboff, *soff;
  int    *o[7];                /* the result's columns */
  int64  *otoff;
  int64   trcap, rcap, bcap, basecap;
};

void damar_trimmer_close(damar_trimmer *tm)
{ int k;
  if (tm == NULL)
    return;
  if (tm->have_blk) damar_close_block(&tm->blk);
  free(tm->tt.anno);  free(tm->tt.data);
  free(tm->tr);  free(tm->troff);  free(tm->plan);  free(tm->arec);  free(tm->L.seg);  free(tm->L.rec);
  free(tm->abuf.base);  free(tm->bases);  free(tm->bm);  free(tm->bn);  free(tm->bdiffs);  free(tm->baoff);  free(tm->bboff);
  free(tm->soff);  free(tm->otoff);
  for (k = 0; k < 7; k++) free(tm->o[k]);
  free(tm);
}

damar_trimmer *damar_trimmer_open(const char *dbname, const damar_dbinfo *db, const char *track, int *no_track)
{ damar_trimmer *tm = (damar_trimmer *) calloc(1, sizeof(*tm));
  *no_track = 0;
  if (tm == NULL)
    return NULL;
  tm->db = db;
  tm->abuf.holds = -1;
  if (damar_track_read_any(db, track, &tm->tt.anno, &tm->tt.data, &tm->tt.ndata))
    { *no_track = 1;
      damar_trimmer_close(tm);
      return NULL;
    }
  if (damar_read_block(dbname, &tm->blk))
    { damar_trimmer_close(tm);
      return NULL;
    }
  tm->have_blk = 1;
  return tm;
}

/* plan, align, settle for one batch of whole piles: rdiffs are the records' differences as the file has them, `first` the
   number of the batch's first record in the file (for messages), st is added to.  0, or 1 after a message. */
int damar_trimmer_batch(damar_trimmer *tm, const damar_trace_batch *tb, const int *rdiffs, const char *las, int64 first,
                        damar_trim_stats *st, damar_trimmed *res)
{ const damar_pile_batch *b = &tb->p;
  const damar_dbinfo *db = tm->db;
  const damar_trace_batch t = *tb;
  const int tw = t.tspace, tbytes = t.tbytes;
  uint16 *tr;
  int64  *troff;
  Plan   *plan;
  int    *arec, *bm, *bn, *bdiffs, *script = NULL;
  int64  *baoff, *bboff, *soff;
  char   *bases;
  SegList *Lp = &tm->L;
  ABuffer *abuf = &tm->abuf;
  int64 nval = 0, pi, nbase = 0, k, i;
  damar_box_batch bb;

  if (abuf->base == NULL || abuf->room < db->maxlen + (tw > 0 ? tw : 0) + 8)
    { abuf->room = db->maxlen + (tw > 0 ? tw : 0) + 8;
      abuf->base = (char *) damar_grow(abuf->base, (size_t) abuf->room, "trim");
      memset(abuf->base, 0, (size_t) abuf->room);
      abuf->holds = -1;
    }
  for (i = 0; i < b->nrec; i++) nval += t.tlen[i];
  tm->tr = (uint16 *) damar_reserve(tm->tr, &tm->trcap, nval, sizeof(uint16), 1024, "trim");
  if (b->nrec > tm->rcap || tm->plan == NULL)
    { tm->rcap = b->nrec + b->nrec / 4 + 1024;
      tm->troff = (int64 *) damar_grow(tm->troff, sizeof(int64) * (size_t) tm->rcap, "trim");
      tm->otoff = (int64 *) damar_grow(tm->otoff, sizeof(int64) * (size_t) tm->rcap, "trim");
      tm->plan = (Plan *) damar_grow(tm->plan, sizeof(Plan) * (size_t) tm->rcap, "trim");
      tm->arec = (int *) damar_grow(tm->arec, sizeof(int) * (size_t) tm->rcap, "trim");
      for (k = 0; k < 7; k++)
        tm->o[k] = (int *) damar_grow(tm->o[k], sizeof(int) * (size_t) tm->rcap, "trim");
    }
  tr = tm->tr;  troff = tm->troff;  plan = tm->plan;  arec = tm->arec;
  for (i = 0, nval = 0; i < b->nrec; i++)
    { const unsigned char *src = t.trace + t.trace_off[i];
      troff[i] = nval;
      if (tbytes == 1)
        for (k = 0; k < t.tlen[i]; k++) tr[nval + k] = src[k];
      else
        memcpy(tr + nval, src, sizeof(uint16) * (size_t) t.tlen[i]);
      nval += t.tlen[i];
    }

  /* plan */
  Lp->n = 0;
  for (pi = 0; pi < b->npiles; pi++)
    { const int a = b->pile_aread[pi];
      int a_lo, a_hi;
      if (a < 0 || a >= db->nreads)
        return damar_reads_missing(las);
      trim_of(&tm->tt, a, &a_lo, &a_hi);
      for (i = b->pile_off[pi]; i < b->pile_off[pi + 1]; i++)
        { Plan *p = plan + i;
          const int br = b->bread[i];
          int b_lo, b_hi;
          arec[i] = a;
          if (br < 0 || br >= db->nreads || t.tlen[i] < 2 || (t.tlen[i] & 1))
            { fprintf(stderr, "damar: %s: record %lld is malformed\n", las, (long long) (first + i));
              return 1;
            }
          p->abpos = b->abpos[i];  p->aepos = b->aepos[i];  p->bbpos = b->bbpos[i];  p->bepos = b->bepos[i];
          st->novl_bases += (p->aepos - p->abpos) + (p->bepos - p->bbpos);
          trim_of(&tm->tt, br, &b_lo, &b_hi);
          if (a_lo >= a_hi || b_lo >= b_hi)
            { p->fate = FATE_GONE;
              p->t0 = 0;  p->tlen = t.tlen[i];
              p->lbox = p->rbox = -1;
              continue;
            }
          if (b->flags[i] & OVL_COMP)
            { const int blen = db->read_len[br], q = b_lo;
              b_lo = blen - b_hi;
              b_hi = blen - q;
            }
          plan_record(p, tr + troff[i], t.tlen[i], tw, a_lo, a_hi, b_lo, b_hi, i, Lp, st);
        }
    }
  st->novl += b->nrec;

  /* align */
  if (Lp->n > tm->bcap || tm->bm == NULL)
    { tm->bcap = Lp->n + Lp->n / 4 + 1024;
      tm->bm = (int *) damar_grow(tm->bm, sizeof(int) * (size_t) tm->bcap, "trim");
      tm->bn = (int *) damar_grow(tm->bn, sizeof(int) * (size_t) tm->bcap, "trim");
      tm->bdiffs = (int *) damar_grow(tm->bdiffs, sizeof(int) * (size_t) tm->bcap, "trim");
      tm->baoff = (int64 *) damar_grow(tm->baoff, sizeof(int64) * (size_t) tm->bcap, "trim");
      tm->bboff = (int64 *) damar_grow(tm->bboff, sizeof(int64) * (size_t) tm->bcap, "trim");
      tm->soff = (int64 *) damar_grow(tm->soff, sizeof(int64) * ((size_t) tm->bcap + 1), "trim");
    }
  bm = tm->bm;  bn = tm->bn;  bdiffs = tm->bdiffs;  baoff = tm->baoff;  bboff = tm->bboff;  soff = tm->soff;
  for (k = 0; k < Lp->n; k++)
    { bm[k] = Lp->seg[k].ae - Lp->seg[k].ab;
      bn[k] = Lp->seg[k].be - Lp->seg[k].bb;
      st->box_a += bm[k];
      st->box_b += bn[k];
      baoff[k] = nbase;
      bboff[k] = nbase + bm[k];
      nbase += bm[k] + bn[k];
    }
  if (nbase > tm->basecap || tm->bases == NULL)
    { tm->basecap = nbase + nbase / 4 + 4096;
      tm->bases = (char *) damar_grow(tm->bases, (size_t) tm->basecap, "trim");
    }
  bases = tm->bases;
  for (k = 0; k < Lp->n; k++)
    { const int64 rec = Lp->rec[k];
      load_a(abuf, &tm->blk, arec[rec]);
      for (i = 0; i < bm[k]; i++)
        bases[baoff[k] + i] = (Lp->seg[k].ab + i < abuf->room) ? abuf->base[Lp->seg[k].ab + i] : 4;
      damar_gather_b(&tm->blk, b->bread[rec], b->flags[rec] & OVL_COMP, Lp->seg[k].bb, Lp->seg[k].be, bases + bboff[k]);
    }
  if (Lp->n > 0)
    { bb.nbox = Lp->n;  bb.m = bm;  bb.n = bn;  bb.aoff = baoff;  bb.boff = bboff;  bb.bases = bases;  bb.nbases = nbase;
      if (damar_align_boxes(&bb, bdiffs, soff, &script))
        return 1;
      st->boxes += Lp->n;
    }

  /* settle */
  for (i = 0; i < b->nrec; i++)
    { Plan   *p = plan + i;
      uint16 *v = tr + troff[i] + p->t0;
      int     flags = b->flags[i], diffs = rdiffs[i];
      if (p->fate == FATE_GONE)
        flags |= OVL_DISCARD | OVL_TRIM;
      else if (p->fate == FATE_CUT)
        { int stop_a, dl, dr;
          st->ntrim_bases += p->known;
          if (p->lbox >= 0)
            { const Seg *s = Lp->seg + p->lbox;
              walk_script(bases + baoff[p->lbox], bm[p->lbox], bases + bboff[p->lbox], script + soff[p->lbox],
                          (int) (soff[p->lbox + 1] - soff[p->lbox]), s->stop - s->bb, &stop_a, &dl, &dr);
              stop_a += s->ab;
              v[0] = (uint16) dr;
              if (s->ae == stop_a)                         /* the cut would leave an empty first segment */
                stop_a -= 1;
              st->ntrim_bases += stop_a - p->a_lo;
              p->abpos = stop_a;
            }
          if (p->rbox >= 0)
            { const Seg *s = Lp->seg + p->rbox;
              walk_script(bases + baoff[p->rbox], bm[p->rbox], bases + bboff[p->rbox], script + soff[p->rbox],
                          (int) (soff[p->rbox + 1] - soff[p->rbox]), s->stop - s->bb, &stop_a, &dl, &dr);
              stop_a += s->ab;
              v[p->tlen - 2] = (uint16) dl;
              st->ntrim_bases += p->a_hi - stop_a;
              p->aepos = stop_a;
            }
          /* what is left may cover next to nothing of either read (trim.c:442) */
          if (p->abpos >= p->aepos || p->bepos < p->keep_lo || p->bbpos > p->keep_hi)
            flags |= OVL_DISCARD | OVL_TRIM;
          else
            { int j;
              diffs = 0;
              for (j = 0; j < p->tlen; j += 2)
                diffs += v[j];
            }
        }
      tm->o[0][i] = (p->fate == FATE_CUT) ? p->abpos : b->abpos[i];  tm->o[1][i] = (p->fate == FATE_CUT) ? p->aepos : b->aepos[i];
      tm->o[2][i] = (p->fate == FATE_CUT) ? p->bbpos : b->bbpos[i];  tm->o[3][i] = (p->fate == FATE_CUT) ? p->bepos : b->bepos[i];
      tm->o[4][i] = flags;  tm->o[5][i] = diffs;  tm->o[6][i] = p->tlen;
      tm->otoff[i] = troff[i] + p->t0;
    }
  free(script);
  res->abpos = tm->o[0];  res->aepos = tm->o[1];  res->bbpos = tm->o[2];  res->bepos = tm->o[3];
  res->flags = tm->o[4];  res->diffs = tm->o[5];  res->tlen = tm->o[6];
  res->toff = tm->otoff;  res->trace = tr;
  return 0;
}

int damar_trim_las(const char *dbname, const char *las, const char *out, const char *track, int purge, damar_trim_stats *st)
{ damar_dbinfo db;
  damar_trimmer *tm = NULL;
  damar_pile_reader *r = NULL;
  damar_trace_batch  t;
  damar_trimmed      res;
  damar_las_out *wr = NULL;
  int64   i;
  int     got, rc = 1, have_db = 0, no_track;

  memset(st, 0, sizeof(*st));
  if (damar_dbinfo_open(dbname, &db))
    return 1;
  have_db = 1;
  if ((tm = damar_trimmer_open(dbname, &db, track, &no_track)) == NULL)
    { if (no_track)
        { /* the loader's line first, as the reference prints it: it never sets its program name */
          fprintf(stderr, "(null): Track '%s' does not exist\n", track);
          fprintf(stderr, "could not open trim track '%s'\n", track);
        }
      goto done;
    }
  if ((r = damar_piles_open_traces(las, 0, 0)) == NULL)
    goto done;
  if ((wr = damar_las_out_open(out, purge)) == NULL)
    { fprintf(stderr, "could not open '%s'\n", out);
      goto done;
    }
  if (damar_las_out_begin(wr, damar_piles_tspace(r)))
    goto done;

  while ((got = damar_piles_next_traces(r, &t)) > 0)
    { const damar_pile_batch *b = &t.p;
      const int *rdiffs, *rlast;

      damar_piles_rest(r, &rdiffs, &rlast);
      if (damar_trimmer_batch(tm, &t, rdiffs, las, st->novl, st, &res))
        goto done;
      /* the records as they go to the file */
      for (i = 0; i < b->nrec; i++)
        { int rec[10];
          rec[0] = res.tlen[i];  rec[1] = res.diffs[i];
          rec[2] = res.abpos[i];  rec[3] = res.bbpos[i];
          rec[4] = res.aepos[i];  rec[5] = res.bepos[i];
          rec[6] = res.flags[i];
          rec[7] = damar_trimmer_aread(tm, i);  rec[8] = b->bread[i];  rec[9] = rlast[i];
          if (damar_las_out_put(wr, rec, NULL, res.trace + res.toff[i], t.tbytes, "LAtrim"))
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
  damar_trimmer_close(tm);
  if (have_db) damar_dbinfo_close(&db);
  return rc;
}

int damar_trimmer_aread(const damar_trimmer *tm, int64 rec)
{ return tm->arec[rec]; }
