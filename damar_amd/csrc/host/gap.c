/* gap.c -- LAgap (scrub/LAgap.c without its -C chimer code) as calls: per pile the contained records of every B read
 * dropped, the remaining ones counted over bins of 100 bases, and at every run of bins covered at most once the records on
 * the far side of the pile's longest record dropped, unless an exclude interval or a stitchable pair speaks for the run.
 *   - damar_host_gap_pile: the plain routine, the reference's loops as written (DAMAR_PILES=host, the piles
 *     kernels/pile_gaps.hip leaves, and the second opinion for that kernel),
 *   - damar_gap_inputs_valid: what both paths index with,
 *   - damar_gap_las: the pass over a file -- per batch of whole piles the trim (-t, host/trim.c), damar_pile_gaps, the
 *     reference's lines, the records written.
 * Nothing here touches the GPU runtime. */
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "damar_hip.h"
#include "damar_host.h"

#define BIN_SIZE 100                      /* LAgap.c:33-34 */
#define MIN_LR   450

int damar_gap_inputs_valid(const damar_pile_batch *b, const damar_gap_params *p)
{ const char *why = "malformed batch";
  int64 i, pi;
  if (b == NULL || p == NULL || b->npiles < 0 || b->nrec < 0 || b->npiles > 0x7fffffff || b->nrec > 0x7fffffff || b->nreads <= 0)
    goto bad;
  if (b->npiles == 0 ? b->nrec != 0 : (b->pile_off[0] != 0 || b->pile_off[b->npiles] != b->nrec))
    goto bad;
  for (pi = 0; pi < b->npiles; pi++)
    { int alen;
      if (b->pile_off[pi] > b->pile_off[pi + 1] || b->pile_aread[pi] < 0 || b->pile_aread[pi] >= b->nreads)
        goto bad;
      alen = b->read_len[b->pile_aread[pi]];
      for (i = b->pile_off[pi]; i < b->pile_off[pi + 1]; i++)
        { if (b->bread[i] < 0 || b->bread[i] >= b->nreads)
            { why = "a record's B read is not in the database";
              goto bad;
            }
          /* the bins are indexed with these; a record that comes discarded never reaches a bin, and a trim that leaves
             nothing of a record leaves it with abpos >= aepos (lib/trim.c:442) */
          if (!(b->flags[i] & OVL_DISCARD) && (b->abpos[i] < 0 || b->aepos[i] < b->abpos[i] || b->aepos[i] > alen))
            { why = "a record's A coordinates lie outside its read";
              goto bad;
            }
        }
    }
  if (p->ex_anno != NULL)
    { int r;
      why = "the exclude track is not pairs of ints for the database's reads";
      if (p->ex_ndata < 0 || (p->ex_ndata > 0 && p->ex_data == NULL) || p->ex_anno[0] % 8 || p->ex_anno[b->nreads] > 4 * (uint64) p->ex_ndata)
        goto bad;
      for (r = 0; r < b->nreads; r++)
        if (p->ex_anno[r] > p->ex_anno[r + 1] || p->ex_anno[r + 1] % 8)
          goto bad;
    }
  return 1;
bad:
  fprintf(stderr, "damar: gaps: %s\n", why);
  return 0;
}

/***** the plain routine ************************************************************************/

typedef struct
{ const damar_pile_batch *b;
  int64 lo;                    /* the pile's first record */
  int   n, aread;
  int  *flags;                 /* the pile's, in and out */
} Pile;

#define AB(i) (pl->b->abpos[pl->lo + (i)])
#define AE(i) (pl->b->aepos[pl->lo + (i)])
#define BB(i) (pl->b->bbpos[pl->lo + (i)])
#define BE(i) (pl->b->bepos[pl->lo + (i)])
#define BR(i) (pl->b->bread[pl->lo + (i)])

/* LAgap.c:1782-1871 */
static int64 drop_containments(Pile *pl)
{ int64 gone = 0;
  int   i, k;
  if (pl->n < 2)
    return 0;
  for (i = 0; i < pl->n; i++)
    { const int bread = BR(i), blen = pl->b->read_len[bread];
      int bb1, be1;
      if ((pl->flags[i] & OVL_DISCARD) || pl->aread == bread)
        continue;
      if (pl->flags[i] & OVL_COMP)
        { bb1 = blen - BE(i);  be1 = blen - BB(i); }
      else
        { bb1 = BB(i);  be1 = BE(i); }
      for (k = i + 1; k < pl->n; k++)
        { int bb2, be2, cont;
          if (pl->flags[k] & OVL_DISCARD)
            continue;
          if (BR(k) != bread)
            break;
          if (pl->flags[k] & OVL_COMP)
            { bb2 = blen - BE(k);  be2 = blen - BB(k); }
          else
            { bb2 = BB(k);  be2 = BE(k); }
          cont = damar_contained(AB(i), AE(i), AB(k), AE(k));
          if (cont && damar_contained(bb1, be1, bb2, be2))
            { gone += 1;
              if (cont == 1)
                { pl->flags[i] |= OVL_DISCARD | OVL_CONT;
                  break;
                }
              pl->flags[k] |= OVL_DISCARD | OVL_CONT;
            }
        }
    }
  return gone;
}

/* LAgap.c:300-354 */
static int stitchable(const Pile *pl, int fuzz, int beg, int end)
{ const int ignore = OVL_TEMP | OVL_CONT | OVL_TRIM | OVL_STITCH;
  int t = 0, i, k;
  if (pl->n < 2)
    return 0;
  for (i = 0; i < pl->n; i++)
    { if (pl->flags[i] & ignore)
        continue;
      for (k = i + 1; k < pl->n && BR(k) == BR(i); k++)
        { if ((pl->flags[k] & ignore) || ((pl->flags[i] & OVL_COMP) != (pl->flags[k] & OVL_COMP)))
            continue;
          if (abs(AE(i) - AB(k)) < fuzz && abs(BE(i) - BB(k)) < fuzz && AB(i) < beg - MIN_LR && AE(k) > end + MIN_LR)
            t += 1;
        }
    }
  return t;
}

/* LAgap.c:159-238: *kind receives which side went */
static int drop_break(Pile *pl, int p1, int p2, int *kind)
{ int max = 0, left = 0, dropped = 0, i;
  for (i = 0; i < pl->n; i++)
    { const int len = AE(i) - AB(i);
      if (pl->flags[i] & OVL_DISCARD)
        continue;
      if (len > max)
        { max = len;
          left = AB(i) < p1;
        }
    }
  if (max == 0)
    { *kind = DAMAR_GAP_DROP_NONE;
      return 0;
    }
  *kind = left ? DAMAR_GAP_DROP_R : DAMAR_GAP_DROP_L;
  for (i = 0; i < pl->n; i++)
    if (!left ? AB(i) < p1 : (!(pl->flags[i] & OVL_DISCARD) && AE(i) > p2))
      { if (!(pl->flags[i] & OVL_DISCARD))
          dropped += 1;
        pl->flags[i] |= OVL_DISCARD | OVL_GAP;
      }
  return dropped;
}

static void add_event(damar_gap_list *L, int beg, int b, int kind, int v0, int v1, int dropped)
{ int *e;
  if (L->n >= L->cap)
    { L->cap = L->cap + L->cap / 4 + 256;
      L->ev = (int *) damar_grow(L->ev, sizeof(int) * DAMAR_GAP_EVENT_INTS * (size_t) L->cap, "gap");
    }
  e = L->ev + DAMAR_GAP_EVENT_INTS * L->n++;
  e[0] = beg;  e[1] = b;  e[2] = kind;  e[3] = v0;  e[4] = v1;  e[5] = dropped;
}

/* gaps_handler without the trim: LAgap.c:1782 and :1616-1780 */
void damar_host_gap_pile(const damar_pile_batch *bt, int64 pile, const damar_gap_params *p, int *flags_out, damar_gap_list *L, int64 *cnt)
{ Pile  P, *pl = &P;
  int  *bins;
  int   nbins, trim_b = INT_MAX, trim_e = 0, i, j, b, e, beg = -1, kind;

  P.b = bt;
  P.lo = bt->pile_off[pile];
  P.n = (int) (bt->pile_off[pile + 1] - P.lo);
  P.aread = bt->pile_aread[pile];
  P.flags = flags_out + P.lo;
  for (i = 0; i < P.n; i++)
    P.flags[i] = bt->flags[P.lo + i];
  cnt[0] += drop_containments(pl);

  nbins = (bt->read_len[P.aread] + BIN_SIZE) / BIN_SIZE;
  bins = (int *) calloc((size_t) nbins + 1, sizeof(int));
  if (bins == NULL)
    { fprintf(stderr, "damar: out of memory (gap bins)\n");
      exit(1);
    }
  for (i = 0; i < P.n; i++)
    { if ((P.flags[i] & OVL_DISCARD) || P.aread == BR(i))
        continue;
      for (j = i + 1; j < P.n && BR(j) == BR(i); j++)
        { const int ib = AB(i) > AB(j) ? AB(i) : AB(j), ie = AE(i) < AE(j) ? AE(i) : AE(j);
          if (ib < ie)
            { if (AE(i) - AB(i) < AE(j) - AB(j))
                P.flags[i] |= OVL_TEMP;
              else
                P.flags[j] |= OVL_TEMP;
            }
        }
      if (P.flags[i] & OVL_TEMP)
        continue;
      if (AB(i) < trim_b) trim_b = AB(i);
      if (AE(i) > trim_e) trim_e = AE(i);
      for (b = (AB(i) + MIN_LR) / BIN_SIZE, e = (AE(i) - MIN_LR) / BIN_SIZE; b < e; b++)
        bins[b] += 1;
    }
  if (trim_b >= trim_e)
    { free(bins);
      return;
    }
  for (b = (trim_b + MIN_LR) / BIN_SIZE, e = (trim_e - MIN_LR) / BIN_SIZE; b < e; b++)
    { if (bins[b] <= 1)
        { if (beg == -1)
            beg = b;
          continue;
        }
      if (beg != -1)
        { const int breakb = (beg - 1) * BIN_SIZE, breake = (b + 1) * BIN_SIZE;
          int skip = 0, nst;
          if (p->ex_anno != NULL)
            { uint64 t = p->ex_anno[P.aread] / sizeof(int);
              const uint64 te = p->ex_anno[P.aread + 1] / sizeof(int);
              for (; t < te; t += 2)
                if (breakb > p->ex_data[t] && breake < p->ex_data[t + 1])
                  { add_event(L, beg, b, DAMAR_GAP_MASKED, p->ex_data[t], p->ex_data[t + 1], 0);
                    skip = 1;
                    break;
                  }
            }
          if (!skip && p->stitch > 0 && (nst = stitchable(pl, p->stitch, breakb, breake)) != 0)
            { add_event(L, beg, b, DAMAR_GAP_STITCHABLE, nst, 0, 0);
              skip = 1;
            }
          if (!skip)
            { const int d = drop_break(pl, breakb, breake, &kind);
              add_event(L, beg, b, kind, 0, 0, d);
              cnt[1] += 1;
              cnt[2] += d;
            }
          beg = -1;
        }
    }
  if (beg != -1)
    { const int d = drop_break(pl, (beg - 1) * BIN_SIZE, (b + 1) * BIN_SIZE, &kind);
      add_event(L, beg, b, kind | DAMAR_GAP_TRAILING, 0, 0, d);
      cnt[1] += 1;
      cnt[2] += d;
    }
  free(bins);
}

/***** the pass over a file *********************************************************************/

/* what DEBUG_GAPS prints of one event (LAgap.c:1693-1751, :198, :217) */
static void print_event(int aread, const int *e)
{ const int kind = e[2] & 0xff, p1 = (e[0] - 1) * BIN_SIZE, p2 = (e[1] + 1) * BIN_SIZE;
  if (!(e[2] & DAMAR_GAP_TRAILING))
    { printf("READ %7d BREAK %3d..%3d ", aread, e[0], e[1]);
      if (kind == DAMAR_GAP_MASKED)
        printf(" MASKED %5d..%5d\n", e[3], e[4]);
      else if (kind == DAMAR_GAP_STITCHABLE)
        printf(" STITCHABLE using %d\n", e[3]);
      else
        printf("\n");
    }
  if (kind == DAMAR_GAP_DROP_L)
    printf("DROP L @ %5d..%5d\n", p1, p2);
  else if (kind == DAMAR_GAP_DROP_R)
    printf("DROP R @ %5d..%5d\n", p1, p2);
}

/* track_load's failure: the loader's line first, as the reference prints it (it never sets its program name), then main's */
void damar_gap_no_track(const char *track)
{ fprintf(stderr, "(null): Track '%s' does not exist\n", track);
  fprintf(stderr, "could not open track '%s'\n", track);
}

int damar_gap_las(const char *dbname, const char *las, const char *out, const damar_gap_params *p, damar_gap_stats *st)
{ damar_dbinfo db;
  damar_trimmer *tm = NULL;
  damar_pile_reader *r = NULL;
  damar_trace_batch  t;
  damar_trimmed      res;
  damar_gap_events   ev;
  damar_las_out *wr = NULL;
  int    *flags = NULL, *count = NULL;
  int64   fcap = 0, ccap = 0, i, pi;
  int     got, rc = 1, have_db = 0, no_track;

  memset(st, 0, sizeof(*st));
  memset(&ev, 0, sizeof(ev));
  if (damar_dbinfo_open(dbname, &db))
    return 1;
  have_db = 1;
  if (p->trim_track != NULL && (tm = damar_trimmer_open(dbname, &db, p->trim_track, &no_track)) == NULL)
    { if (no_track)
        damar_gap_no_track(p->trim_track);
      goto done;
    }
  if ((r = damar_piles_open_traces(las, 0, 0)) == NULL)
    goto done;
  if ((wr = damar_las_out_open(out, p->purge)) == NULL)
    { fprintf(stderr, "could not open output track '%s'\n", out);
      goto done;
    }
  if (damar_las_out_begin(wr, damar_piles_tspace(r)))
    goto done;
  printf(GREEN "PASS gaps" RESET "\n");

  while ((got = damar_piles_next_traces(r, &t)) > 0)
    { damar_pile_batch b = t.p;
      const int *rdiffs, *rlast;
      const int *e;
      double ms[4];
      int64  c3[3];

      damar_piles_rest(r, &rdiffs, &rlast);
      if (damar_batch_bind(&b, &db, las, DAMAR_BIND_A))
        goto done;
      if (tm != NULL)
        { if (damar_trimmer_batch(tm, &t, rdiffs, las, st->novl, &st->trim, &res))
            goto done;
          b.abpos = res.abpos;  b.aepos = res.aepos;  b.bbpos = res.bbpos;  b.bepos = res.bepos;  b.flags = res.flags;
        }
      flags = (int *) damar_reserve(flags, &fcap, b.nrec, sizeof(int), 1024, "gap");
      count = (int *) damar_reserve(count, &ccap, b.npiles, sizeof(int), 1024, "gap");
      ev.count = count;
      ev.ev = NULL;
      if (damar_pile_gaps(&b, p, flags, &ev))
        goto done;
      damar_gap_last(ms, c3);
      st->piles += c3[0];  st->host_piles += c3[1];  st->events += c3[2];
      st->contained += ev.contained;  st->breaks += ev.breaks;  st->dropped += ev.dropped;
      for (pi = 0, e = ev.ev; pi < b.npiles; pi++)
        for (i = 0; i < count[pi]; i++, e += DAMAR_GAP_EVENT_INTS)
          print_event(b.pile_aread[pi], e);
      free(ev.ev);
      ev.ev = NULL;

      /* the records as they go to the file.  OVL_TEMP is never cleared inside the pile, but lib/pass.c:230 takes it off every
         record it writes: it does not reach the file */
      for (pi = 0; pi < b.npiles; pi++)
        for (i = b.pile_off[pi]; i < b.pile_off[pi + 1]; i++)
          { int rec[10];
            rec[0] = tm != NULL ? res.tlen[i] : t.tlen[i];
            rec[1] = tm != NULL ? res.diffs[i] : rdiffs[i];
            rec[2] = b.abpos[i];  rec[3] = b.bbpos[i];  rec[4] = b.aepos[i];  rec[5] = b.bepos[i];
            rec[6] = flags[i];
            rec[7] = b.pile_aread[pi];  rec[8] = b.bread[i];  rec[9] = rlast[i];
            if (damar_las_out_put(wr, rec, t.trace + t.trace_off[i], tm != NULL ? res.trace + res.toff[i] : NULL, t.tbytes, "(null)"))
              goto done;
          }
      st->novl += b.nrec;
    }
  if (got < 0)
    goto done;
  /* gaps_post, LAgap.c:1906-1914 */
  if (tm != NULL)
    { printf("%13lld of %13lld overlaps trimmed\n", (long long) st->trim.ntrimmed, (long long) st->trim.novl);
      printf("%13lld of %13lld bases trimmed\n", (long long) st->trim.ntrim_bases, (long long) st->trim.novl_bases);
    }
  printf("dropped %d containments\n", (int) st->contained);
  printf("dropped %d overlaps in %d break/gaps\n", (int) st->dropped, (int) st->breaks);
  rc = 0;
done:
  if (wr != NULL && damar_las_out_close(wr, rc == 0, &st->written, &st->discarded))
    rc = 1;
  fflush(stdout);
  free(ev.ev);
  damar_piles_close(r);
  damar_trimmer_close(tm);
  if (have_db) damar_dbinfo_close(&db);
  free(flags);  free(count);
  return rc;
}
