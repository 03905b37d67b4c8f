/* separate.c -- LAseparate (scrub/LAseparate.c) as calls: the overlaps of every (A read, B read) chained, the best chain
 * judged, and the group sent to one of two files by that verdict.
 *   - damar_host_chain_group: the plain routine for one group, kernels/chain_core.h with the host's storage: any number of
 *     records and of chains (DAMAR_PILES=host, the groups kernels/pile_chains.hip leaves, and the second opinion for that
 *     kernel),
 *   - damar_separate_inputs_valid: what both paths index with, and the one input the reference aborts on,
 *   - damar_separate_las: the pass over a file -- per batch of whole piles damar_pile_chains, the records written to both
 *     files from the one verdict.
 * Nothing here touches the GPU runtime. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "damar_hip.h"
#include "damar_host.h"

typedef struct { unsigned char *st; } host_state;
#define CH_FN    static inline
#define CH_MT    int
#define CH_STATE host_state
#define CH_IS(s, i, bits)  ((s)->st[i] & (bits))
#define CH_SET(s, i, bits) ((s)->st[i] |= (bits))
#define CH_CLR(s, i, bits) ((s)->st[i] &= ~(bits))
#include "kernels/chain_core.h"

int damar_separate_inputs_valid(const damar_pile_batch *b, const damar_separate_params *p, const damar_chain_out *out)
{ const char *why = "malformed batch";
  int64 i, pi;
  int   r;
  if (b == NULL || p == NULL || out == NULL || b->npiles < 0 || b->nrec < 0 || b->npiles > 0x7fffffff || b->nrec > 0x7fffffff || b->nreads <= 0)
    goto bad;
  if (b->npiles == 0 ? b->nrec != 0 : (b->pile_off[0] != 0 || b->pile_off[b->npiles] != b->nrec))
    goto bad;
  if (b->nrec > 0 && (out->flags == NULL || out->nchains == NULL || out->proper == NULL || out->nbest == NULL || out->best == NULL))
    goto bad;
  if (p->kind < 0 || p->kind > 1)
    { why = "the type is neither 0 nor 1";
      goto bad;
    }
  for (pi = 0; pi < b->npiles; pi++)
    { if (b->pile_off[pi] > b->pile_off[pi + 1] || b->pile_aread[pi] < 0 || b->pile_aread[pi] >= b->nreads)
        goto bad;
      for (i = b->pile_off[pi]; i < b->pile_off[pi + 1]; i++)
        if (b->bread[i] < 0 || b->bread[i] >= b->nreads)
          { why = "a record's B read is not in the database";
            goto bad;
          }
    }
  if (p->rep_anno != NULL && !p->rep_checked)
    { why = "the repeat track is not pairs of ints for the database's reads";
      if (p->rep_ndata < 0 || (p->rep_ndata > 0 && p->rep_data == NULL) || p->rep_anno[0] % 8 || p->rep_anno[b->nreads] > 4 * (uint64) p->rep_ndata)
        goto bad;
      for (r = 0; r < b->nreads; r++)
        if (p->rep_anno[r] > p->rep_anno[r + 1] || p->rep_anno[r + 1] % 8)
          goto bad;
    }
  /* a group of two or more records that all come discarded or contained leaves chain() without a chain; the reference
     then counts one record of it and dies on its own assert after the first file.  Here it is an error run. */
  for (pi = 0; pi < b->npiles; pi++)
    { int64 g0 = b->pile_off[pi];
      for (i = g0; i < b->pile_off[pi + 1]; i++)
        { int live = 0;
          int64 k;
          if (i + 1 < b->pile_off[pi + 1] && b->bread[i + 1] == b->bread[g0])
            continue;
          for (k = g0; k <= i; k++)
            live += !(b->flags[k] & (OVL_CONT | OVL_DISCARD));
          if (i > g0 && live == 0)
            { fprintf(stderr, "damar: separate: the %lld overlaps of reads %d and %d all come discarded or contained\n", (long long) (i - g0 + 1),
                      b->pile_aread[pi], b->bread[g0]);
              return 0;
            }
          g0 = i + 1;
        }
    }
  return 1;
bad:
  fprintf(stderr, "damar: separate: %s\n", why);
  return 0;
}

/* the two repeat counts of the batch's record i of pile `pile` */
static void record_repeats(const damar_pile_batch *b, int64 pile, int64 i, const damar_separate_params *p, int *arep, int *brep)
{ *arep = *brep = 0;
  if (p->rep_anno != NULL)
    ch_record_repeats((const unsigned long long *) p->rep_anno, p->rep_data, b->pile_aread[pile], b->bread[i], b->abpos[i], b->aepos[i], b->bbpos[i],
                      b->bepos[i], b->flags[i] & OVL_COMP, arep, brep);
}

void damar_host_chain_group(const damar_pile_batch *b, int64 pile, int64 first, int n, const damar_separate_params *p, damar_chain_out *out)
{ const int alen = b->read_len[b->pile_aread[pile]], blen = b->read_len[b->bread[first]];
  const int keep = ~(OVL_TEMP | OVL_CONT | OVL_DISCARD);
  ch_recs    r;
  ch_work    w;
  host_state s;
  int *rep;
  int  i, rc;

  if (n == 1)                             /* the great majority on a daligner file: judged by the record, nothing to chain */
    { const int proper = ch_single_proper(b->abpos[first], b->aepos[first], b->bbpos[first], b->bepos[first], alen, blen, p->kind);
      out->flags[first] = (b->flags[first] & ~OVL_TEMP) | ((p->kind == 0 ? proper : !proper) ? OVL_DISCARD : 0);
      out->proper[first] = proper;
      out->nchains[first] = out->nbest[first] = 0;
      out->best[first] = -1;
      return;
    }
  rep = (int *) damar_grow(NULL, sizeof(int) * 2 * (size_t) n, "separate");
  for (i = 0; i < n; i++)
    record_repeats(b, pile, first + i, p, &rep[i], &rep[n + i]);
  r.ab = b->abpos + first;  r.ae = b->aepos + first;  r.bb = b->bbpos + first;  r.be = b->bepos + first;  r.fl = b->flags + first;
  r.arep = rep;  r.brep = rep + n;
  s.st = (unsigned char *) damar_grow(NULL, (size_t) n, "separate");
  memset(&w, 0, sizeof(w));
  w.maxchains = n;                        /* every chain has a seed of its own */
  w.tab = (int *) damar_grow(NULL, sizeof(int) * CH_TAB_INTS * (size_t) n, "separate");
  w.mcap = n;                             /* more only where a gap filler of under 100 bases enters a chain more than once */
  do
    { w.cur = (int *) damar_grow(w.cur, sizeof(int) * (size_t) w.mcap, "separate");
      w.best = (int *) damar_grow(w.best, sizeof(int) * (size_t) w.mcap, "separate");
      for (i = 0; i < n; i++)
        s.st[i] = (unsigned char) (((b->flags[first + i] & OVL_CONT) ? CH_CONT : 0) | ((b->flags[first + i] & OVL_DISCARD) ? CH_DISC : 0));
      rc = ch_chain(&r, n, alen, blen, p->twidth, &s, &w);
      w.mcap *= 2;
    }
  while (rc == CH_ROOM);
  out->proper[first] = ch_verdict(&r, n, alen, blen, p->kind, &s, &w);
  out->nchains[first] = w.nchains;
  out->nbest[first] = w.nbest;
  for (i = 0; i < n; i++)
    { out->flags[first + i] = (b->flags[first + i] & keep) | ((s.st[i] & CH_TEMP) ? OVL_TEMP : 0) | ((s.st[i] & CH_CONT) ? OVL_CONT : 0) |
                              ((s.st[i] & CH_DISC) ? OVL_DISCARD : 0);
      out->best[first + i] = i < w.nbest ? w.best[i] : -1;
      if (i > 0)
        out->nchains[first + i] = out->proper[first + i] = out->nbest[first + i] = -1;
    }
  free(rep);  free(s.st);  free(w.tab);  free(w.cur);  free(w.best);
}

void damar_host_chain_pile(const damar_pile_batch *b, int64 pile, const damar_separate_params *p, damar_chain_out *out)
{ int64 g0 = b->pile_off[pile], i;
  for (i = g0; i < b->pile_off[pile + 1]; i++)
    if (i + 1 == b->pile_off[pile + 1] || b->bread[i + 1] != b->bread[g0])
      { damar_host_chain_group(b, pile, g0, (int) (i - g0 + 1), p, out);
        g0 = i + 1;
      }
}

/***** the pass over a file *********************************************************************/

int damar_separate_las(const char *dbname, const char *las, const char *out, const char *out_discard, const char *track, int kind,
                       damar_separate_stats *st)
{ damar_dbinfo db;
  damar_separate_params P;
  damar_pile_reader *r = NULL;
  damar_trace_batch  t;
  damar_chain_out    o;
  damar_las_out *wr[2] = { NULL, NULL };
  uint64 *ranno = NULL;
  int    *rdata = NULL, *cols = NULL;
  int64   cap = 0, i, pi, g0, w0, w1;
  int     got, rc = 1, have_db = 0, f;

  memset(st, 0, sizeof(*st));
  memset(&P, 0, sizeof(P));
  if (damar_dbinfo_open(dbname, &db))
    return 1;
  have_db = 1;
  if (damar_track_read_any(&db, track, &ranno, &rdata, &P.rep_ndata))
    { damar_filter_no_track(track);
      goto done;
    }
  P.rep_anno = ranno;  P.rep_data = rdata;  P.kind = kind;
  if ((r = damar_piles_open_traces(las, 0, 0)) == NULL)
    goto done;
  P.twidth = damar_piles_tspace(r);
  for (f = 0; f < 2; f++)
    { if ((wr[f] = damar_las_out_open(f == 0 ? out : out_discard, 1)) == NULL)
        { fprintf(stderr, "could not open %s\n", f == 0 ? out : out_discard);
          goto done;
        }
      if (damar_las_out_begin(wr[f], P.twidth))
        goto done;
    }
  printf(GREEN "PASS separate\n" RESET);

  while ((got = damar_piles_next_traces(r, &t)) > 0)
    { damar_pile_batch b = t.p;
      const int *rdiffs, *rlast;
      double ms[4];
      int64  c3[3];

      damar_piles_rest(r, &rdiffs, &rlast);
      if (damar_batch_bind(&b, &db, las, DAMAR_BIND_AB))
        goto done;
      cols = (int *) damar_reserve(cols, &cap, b.nrec, 5 * sizeof(int), 1024, "separate");
      o.flags = cols;  o.nchains = cols + cap;  o.proper = cols + 2 * cap;  o.nbest = cols + 3 * cap;  o.best = cols + 4 * cap;
      if (damar_pile_chains(&b, &P, &o))
        goto done;
      damar_separate_last(ms, c3);
      P.rep_checked = 1;
      st->groups += c3[0];  st->host_groups += c3[1];  st->multi += c3[2];
      for (pi = 0; pi < b.npiles; pi++)
        for (g0 = i = b.pile_off[pi]; i < b.pile_off[pi + 1]; i++)
          { int rec[10];
            if (o.nchains[i] >= 0)
              g0 = i;
            /* the counters as separate_handler keeps them: a group without a chain counts its first record alone, by the verdict */
            if (o.nchains[g0] == 0)
              { if (i == g0)
                  { if (kind == 0 ? o.proper[g0] : !o.proper[g0]) st->discarded += 1;
                    else st->kept += 1;
                  }
              }
            else if (o.flags[i] & OVL_DISCARD) st->discarded += 1;
            else st->kept += 1;
            rec[0] = t.tlen[i];  rec[1] = rdiffs[i];
            rec[2] = b.abpos[i];  rec[3] = b.bbpos[i];  rec[4] = b.aepos[i];  rec[5] = b.bepos[i];
            rec[7] = b.pile_aread[pi];  rec[8] = b.bread[i];  rec[9] = rlast[i];
            for (f = 0; f < 2; f++)       /* the second file is the complement: the same verdict with the bit inverted */
              { rec[6] = f == 0 ? o.flags[i] : (o.flags[i] ^ OVL_DISCARD);
                if (damar_las_out_put(wr[f], rec, t.trace + t.trace_off[i], NULL, t.tbytes, "(null)"))
                  goto done;
              }
          }
      st->novl += b.nrec;
    }
  if (got < 0)
    goto done;
  /* separate_post of the first pass; the second pass prints the same counters the other way round */
  printf("Kept    ovls: %10d\n", (int) st->kept);
  printf("Discard ovls: %10d\n", (int) st->discarded);
  printf(GREEN "PASS separate\n" RESET);
  printf("Kept    ovls: %10d\n", (int) st->discarded);
  printf("Discard ovls: %10d\n", (int) st->kept);
  rc = 0;
done:
  for (f = 0; f < 2; f++)
    if (wr[f] != NULL && damar_las_out_close(wr[f], rc == 0, f == 0 ? &st->written : &st->written_discard, f == 0 ? &w0 : &w1))
      rc = 1;
  fflush(stdout);
  damar_piles_close(r);
  if (have_db) damar_dbinfo_close(&db);
  free(ranno);  free(rdata);  free(cols);
  return rc;
}
