/* correct.c -- LAcorrect (corrector/LAcorrect.c as it is compiled: USE_A_TILES and TRACK_POSITIONS defined,
 * ADJUST_OFFSETS and FIX_BOUNDARY_ERRORS not; corrector/consensus.c): every read rewritten as the consensus of the tiles
 * that its pile lays over it.
 *   - the tiles of a pile (correct_overlaps, LAcorrect.c:1125-1335) and the entries of each that the consensus takes
 *     (single_tile_consensus, :287): layout_pile;
 *   - the plain routine for one tile, damar_host_tile, the code of kernels/tile_core.h on storage that grows: what
 *     DAMAR_PILES=host runs, and what does the tiles beyond the kernel's limits;
 *   - the pass over a file, damar_correct_las: per batch of whole piles the layout, one damar_tile_consensus call, the reads
 *     put together; the whole-read alignments behind " postrace=" (break_read, :1055-1096) are one damar_align_reads
 *     call per batch (kernels/read_align.hip), or, with DAMAR_POSTRACE=host or DAMAR_PILES=host, damar_exact_box of
 *     host/bridge.c in worker threads, which run while the next batch is laid out and called.
 * Deviations from the reference, both where it reads what it never wrote: a pile whose first record has no trace is used
 * without that record; a -j for which partition_overlaps writes past its offsets is refused with a message. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <pthread.h>
#include <sys/time.h>

#include "damar_hip.h"
#include "damar_host.h"

#define MIN_TWIDTH   20                   /* LAcorrect.c:33-36 */
#define MAX_COVERAGE DAMAR_CORRECT_MAXCOV
#define MAX_TILES    40
#define REC_BYTES    40                   /* a record's header in the file */
#define LINE_WIDTH   100

#define TC_FN static inline
#define TC_VT int
#define TC_ST int
#include "kernels/tile_core.h"

static double now_ms(void)
{ struct timeval tv;
  gettimeofday(&tv, NULL);
  return tv.tv_sec * 1e3 + tv.tv_usec * 1e-3;
}

/***** the plain routine for one tile ************************************************************/

static tc_work g_w;
static long long g_cols, g_script, g_cells;

void damar_host_tile_release(void)
{ free(g_w.cnt);  free(g_w.pc);  free(g_w.vf);  free(g_w.hf);  free(g_w.script);
  memset(&g_w, 0, sizeof(g_w));
  g_cols = g_script = g_cells = 0;
}

int damar_tile_batch_valid(const damar_tile_batch *b)
{ int64 t, e;
  if (b == NULL || b->ntiles < 0 || (b->ntiles > 0 && (b->ent_off == NULL || b->ent_off[0] != 0)))
    { fprintf(stderr, "damar: correct: not a tile batch\n");
      return 0;
    }
  for (t = 0; t < b->ntiles; t++)
    { const int64 n = b->ent_off[t + 1] - b->ent_off[t];
      if (n < 0 || n > MAX_COVERAGE)
        { fprintf(stderr, "damar: correct: tile %lld holds %lld sequences (0 .. %d are taken)\n", (long long) t, (long long) n, MAX_COVERAGE);
          return 0;
        }
      for (e = b->ent_off[t]; e < b->ent_off[t + 1]; e++)
        if (b->seq_len[e] < 1 || b->seq_len[e] > 65535 || b->seq_off[e] < 0 || b->seq_off[e] + b->seq_len[e] > b->nbases)
          { fprintf(stderr, "damar: correct: sequence %lld of tile %lld lies outside the bases\n", (long long) (e - b->ent_off[t]), (long long) t);
            return 0;
          }
    }
  for (e = 0; e < b->nbases; e++)
    if (b->bases[e] > 3)
      { fprintf(stderr, "damar: correct: the bases hold a value above 3\n");
        return 0;
      }
  return 1;
}

/* tile `tile` of the batch: out (room for *cap values, grown here) receives the called bases; returns their number, -1
   after a message */
int damar_host_tile(const damar_tile_batch *b, int64 tile, unsigned char **out, int64 *cap)
{ const int64 e0 = b->ent_off[tile];
  const int   nent = (int) (b->ent_off[tile + 1] - e0);
  long long cols = 0, longest = 0;
  int i, st, n = 0;
  if (nent == 0)
    return 0;
  for (i = 0; i < nent; i++)
    { cols += b->seq_len[e0 + i];
      if (b->seq_len[e0 + i] > longest) longest = b->seq_len[e0 + i];
    }
  if (cols > g_cols)
    { g_cols = cols + cols / 4 + 1024;
      g_w.cnt = (unsigned char *) damar_grow(g_w.cnt, 5 * (size_t) g_cols, "correct");
      g_w.pc = (unsigned char *) damar_grow(g_w.pc, (size_t) g_cols, "correct");
    }
  if (cols + longest > g_script)
    { g_script = cols + longest + 1024;
      g_w.script = (int *) damar_grow(g_w.script, sizeof(int) * (size_t) g_script, "correct");
    }
  *out = (unsigned char *) damar_reserve(*out, cap, cols, 1, 1024, "correct");
  if (g_cells == 0)
    { g_cells = 1 << 16;
      g_w.vf = (int *) damar_grow(g_w.vf, sizeof(int) * (size_t) g_cells, "correct");
      g_w.hf = (signed char *) damar_grow(g_w.hf, (size_t) g_cells, "correct");
    }
  g_w.maxcols = (int) cols;
  g_w.maxscript = (int) (cols + longest);
  for (;;)
    { g_w.cap = g_cells;
      st = tc_tile(&g_w, b->bases, (const long long *) (b->seq_off + e0), b->seq_len + e0, nent, *out, &n);
      if (st != TC_ROOM)
        break;
      if (g_cells > ((long long) 1 << 34))
        { fprintf(stderr, "damar: correct: the waves of tile %lld need more than %lld cells\n", (long long) tile, g_cells);
          return -1;
        }
      g_cells *= 2;
      g_w.vf = (int *) damar_grow(g_w.vf, sizeof(int) * (size_t) g_cells, "correct");
      g_w.hf = (signed char *) damar_grow(g_w.hf, (size_t) g_cells, "correct");
    }
  if (st != 0)
    { fprintf(stderr, "damar: correct: the path of tile %lld left its waves\n", (long long) tile);
      return -1;
    }
  return n;
}

/***** the tiles of a pile ***********************************************************************/

typedef struct { int b, comp, bb, be, qv, apos; } Tile;      /* tile_overlap, LAcorrect.c:89; b = -1: the A read itself */

typedef struct
{ int  *toff, *cur;            /* [ntiles + 1], [ntiles] */
  Tile *tovl, *tmp;
  int  *order, *otmp;          /* the pile's records by A length */
  int64 ntoff, ntovl, norder;
} Layout;

static int valid_pt_points(const damar_trace_batch *t, int64 rec)        /* has_valid_pt_points, LAcorrect.c:173 */
{ const int bbpos = t->p.bbpos[rec], bepos = t->p.bepos[rec], tlen = t->tlen[rec];
  int bb, be = bbpos + damar_trace_value(t, rec, 1), k;
  for (k = 2; k < tlen; k += 2)
    { bb = be;
      if (k == tlen - 1)
        be = bepos + 1;
      else
        be += damar_trace_value(t, rec, k + 1);
      if (bb > be || bb < bbpos || bb > bepos || be < bbpos || be > bepos + 1)
        return 0;
    }
  return 1;
}

static void stable_sort_int(int *v, int *tmp, int n, const int *key, int descending)
{ int w, i;
  for (w = 1; w < n; w *= 2)
    { for (i = 0; i < n; i += 2 * w)
        { int a = i, am = i + w < n ? i + w : n, b = am, bm = i + 2 * w < n ? i + 2 * w : n, o = i;
          while (a < am && b < bm)
            { const int ka = key[v[a]], kb = key[v[b]];
              tmp[o++] = (descending ? kb > ka : kb < ka) ? v[b++] : v[a++];
            }
          while (a < am) tmp[o++] = v[a++];
          while (b < bm) tmp[o++] = v[b++];
        }
      memcpy(v, tmp, sizeof(int) * (size_t) n);
    }
}

static void stable_sort_tiles(Tile *v, Tile *tmp, int n)           /* by qv, ascending: cmp_tovl_qv under glibc's merge sort */
{ int w, i;
  for (w = 1; w < n; w *= 2)
    { for (i = 0; i < n; i += 2 * w)
        { int a = i, am = i + w < n ? i + w : n, b = am, bm = i + 2 * w < n ? i + 2 * w : n, o = i;
          while (a < am && b < bm)
            tmp[o++] = (v[b].qv < v[a].qv) ? v[b++] : v[a++];
          while (a < am) tmp[o++] = v[a++];
          while (b < bm) tmp[o++] = v[b++];
        }
      memcpy(v, tmp, sizeof(Tile) * (size_t) n);
    }
}

/* the tiles of one pile: rec[n] are its records in the reference's order (by A length).  0; 1 after a message. */
static int layout_pile(Layout *L, const damar_trace_batch *t, const int *rec, int64 lo, int n, int aread, int alen, const int *q,
                       const int *read_len, int nreads)
{ const int tw = t->tspace, ntiles = (alen + tw - 1) / tw;
  int i, k, p = 0, tile;
  if ((int64) ntiles + 2 > L->ntoff)
    { L->ntoff = ntiles + ntiles / 4 + 64;
      L->toff = (int *) damar_grow(L->toff, sizeof(int) * (size_t) L->ntoff, "correct");
      L->cur = (int *) damar_grow(L->cur, sizeof(int) * (size_t) L->ntoff, "correct");
    }
  memset(L->toff, 0, sizeof(int) * (size_t) (ntiles + 1));
  memset(L->cur, 0, sizeof(int) * (size_t) ntiles);
  for (i = 0; i < n; i++)
    { const int64 r = lo + rec[i];
      const int tb = t->p.abpos[r] / tw, te = tb + t->tlen[r] / 2 - 1, b = t->p.bread[r];
      int be = t->p.bbpos[r];
      if (t->p.abpos[r] < 0 || te >= ntiles || b < 0 || b >= nreads || t->p.bbpos[r] < 0)
        { fprintf(stderr, "damar: correct: a record of read %d lies outside its reads\n", aread);
          return 1;
        }
      for (k = 1; k < t->tlen[r]; k += 2)
        be += damar_trace_value(t, r, k);
      if (be > read_len[b])
        { fprintf(stderr, "damar: correct: the trace of a record of read %d runs past read %d\n", aread, b);
          return 1;
        }
      for (k = tb; k <= te; k++)
        if (L->toff[k + 1] < MAX_TILES)
          L->toff[k + 1] += 1;
    }
  for (i = 0; i < ntiles; i++)
    if (L->toff[i + 1] < MAX_TILES)
      L->toff[i + 1] += 1;
  for (i = 1; i <= ntiles; i++)
    L->toff[i] += L->toff[i - 1];
  if ((int64) L->toff[ntiles] + 1 > L->ntovl)
    { L->ntovl = L->toff[ntiles] + L->toff[ntiles] / 4 + 1024;
      L->tovl = (Tile *) damar_grow(L->tovl, sizeof(Tile) * (size_t) L->ntovl, "correct");
      L->tmp = (Tile *) damar_grow(L->tmp, sizeof(Tile) * (size_t) L->ntovl, "correct");
    }
  for (i = 0; i < ntiles; i++)
    { Tile *x;
      p = L->toff[i] + L->cur[i];
      L->cur[i] += 1;
      x = L->tovl + p;
      x->b = -1;  x->comp = 0;  x->apos = 0;  x->bb = tw * i;  x->be = tw * (i + 1);  x->qv = q[i];
    }
  L->tovl[p].be = alen;
  /* p, the slot last written, is carried from one record to the next: LAcorrect.c:1242-1319 */
  for (i = 0; i < n; i++)
    { const int64 r = lo + rec[i];
      const int comp = t->p.flags[r] & OVL_COMP, b = t->p.bread[r], abpos = t->p.abpos[r], aepos = t->p.aepos[r];
      int be = t->p.bbpos[r] + damar_trace_value(t, r, 1), bb;
      tile = abpos / tw;
      if (L->cur[tile] < MAX_TILES)
        { Tile *x;
          p = L->toff[tile] + L->cur[tile];
          L->cur[tile] += 1;
          x = L->tovl + p;
          x->b = b;  x->comp = comp;  x->bb = t->p.bbpos[r];  x->be = be;  x->qv = damar_trace_value(t, r, 0);
          x->apos = (abpos % tw) ? abpos : 0;
        }
      for (k = 2; k < t->tlen[r]; k += 2)
        { tile += 1;
          bb = be;
          be += damar_trace_value(t, r, k + 1);
          if (L->cur[tile] < MAX_TILES)
            { Tile *x;
              p = L->toff[tile] + L->cur[tile];
              L->cur[tile] += 1;
              x = L->tovl + p;
              x->b = b;  x->comp = comp;  x->bb = bb;  x->be = be;  x->qv = damar_trace_value(t, r, k);  x->apos = 0;
            }
          else
            p = -1;
        }
      if (p != -1 && aepos < alen && (aepos % tw))
        L->tovl[p].apos = -aepos;
    }
  for (i = 0; i < ntiles; i++)
    stable_sort_tiles(L->tovl + L->toff[i] + 1, L->tmp, L->toff[i + 1] - L->toff[i] - 1);
  return 0;
}

/***** the pass over a file **********************************************************************/

typedef struct                  /* a batch of tiles as it grows */
{ int64 *ent_off, *seq_off;
  int   *seq_len, *weight;
  unsigned char *bases;
  int64  ntiles, nent, nbases, ctile, cent, cbases;
} Tiles;

typedef struct                  /* a read of a batch on its way to the file */
{ int    aread, serial, part, ntiles;
  int64  tile0;
  char  *cons;                  /* the called bases, 0..3 */
  int    len;
  int   *q;                     /* {called bases, sequences added} per tile */
  int   *script, slen;
  double ms;
} Job;

typedef struct
{ Job   *job;
  int    n, next, nthreads, running;
  const HITS_DB *blk;
  pthread_t th[64];
} Wave;

static void *postrace_worker(void *arg)
{ Wave *w = (Wave *) arg;
  for (;;)
    { const int i = __sync_fetch_and_add(&w->next, 1);
      Job *j;
      double t0;
      if (i >= w->n)
        break;
      j = w->job + i;
      if (j->len == 0)
        continue;
      t0 = now_ms();
      { const HITS_READ *rd = w->blk->reads + j->aread;
        const char *A = (const char *) w->blk->bases + rd->boff;
        j->script = (int *) damar_grow(NULL, sizeof(int) * ((size_t) rd->rlen + (size_t) j->len + 8), "correct");
        damar_exact_box(A, rd->rlen, j->cons, j->len, j->script, &j->slen);
      }
      j->ms = now_ms() - t0;
    }
  damar_bridge_release();
  return NULL;
}

static void write_bases(FILE *f, const char *s, int len)            /* write_seq, LAcorrect.c:716 */
{ int j;
  for (j = 0; j + LINE_WIDTH < len; j += LINE_WIDTH)
    fprintf(f, "%.*s\n", LINE_WIDTH, s + j);
  if (j < len)
    fprintf(f, "%.*s\n", len - j, s + j);
}

static void wave_start(Wave *w)
{ int i;
  w->next = 0;
  w->running = 0;
  for (i = 0; i < w->nthreads && i < w->n; i++)
    if (pthread_create(&w->th[w->running], NULL, postrace_worker, w) == 0)
      w->running += 1;
  if (w->running == 0 && w->n > 0)
    postrace_worker(w);
}

/* the same alignments in one damar_align_reads call (kernels/read_align.hip): no thread is started, and wave_finish finds
   the scripts where the workers would have left them.  0; 1 after a message. */
static int wave_device(Wave *w, damar_correct_stats *st)
{ damar_box_batch bb;
  int64  *off, *soff, nbases = 0, at = 0, c3[3];
  int    *mn, *diffs, *script = NULL, i, nb = 0, k = 0;
  char   *bases;
  double  ms[4];
  w->next = w->n;
  w->running = 0;
  for (i = 0; i < w->n; i++)
    if (w->job[i].len > 0)
      { nb += 1;
        nbases += w->blk->reads[w->job[i].aread].rlen + w->job[i].len;
      }
  if (nb == 0)
    return 0;
  mn = (int *) damar_grow(NULL, sizeof(int) * 3 * (size_t) nb, "correct");
  off = (int64 *) damar_grow(NULL, sizeof(int64) * (3 * (size_t) nb + 1), "correct");
  bases = (char *) damar_grow(NULL, (size_t) nbases + 8, "correct");
  diffs = mn + 2 * nb;
  soff = off + 2 * nb;
  for (i = 0; i < w->n; i++)
    { const Job *j = w->job + i;
      const HITS_READ *rd = w->blk->reads + j->aread;
      if (j->len == 0)
        continue;
      mn[k] = rd->rlen;  mn[nb + k] = j->len;
      off[k] = at;
      memcpy(bases + at, (const char *) w->blk->bases + rd->boff, (size_t) rd->rlen);
      at += rd->rlen;
      off[nb + k] = at;
      memcpy(bases + at, j->cons, (size_t) j->len);
      at += j->len;
      k += 1;
    }
  bb.nbox = nb;  bb.m = mn;  bb.n = mn + nb;  bb.aoff = off;  bb.boff = off + nb;  bb.bases = bases;  bb.nbases = nbases;
  if (damar_align_reads(&bb, diffs, soff, &script))
    { free(mn);  free(off);  free(bases);
      return 1;
    }
  for (i = 0, k = 0; i < w->n; i++)
    { Job *j = w->job + i;
      if (j->len == 0)
        continue;
      j->slen = (int) (soff[k + 1] - soff[k]);
      j->script = (int *) damar_grow(NULL, sizeof(int) * ((size_t) j->slen + 1), "correct");
      memcpy(j->script, script + soff[k], sizeof(int) * (size_t) j->slen);
      k += 1;
    }
  damar_read_last(ms, c3);
  st->postrace_boxes += c3[0];  st->postrace_host += c3[1];
  st->ms_postrace_kernel += ms[1];  st->ms_postrace_call += ms[3];
  free(script);  free(mn);  free(off);  free(bases);
  return 0;
}

/* the reads of a wave written in file order: break_read, LAcorrect.c:1012 */
static void wave_finish(Wave *w, FILE **fo, int tw, const int *read_len, damar_correct_stats *st)
{ int i, k;
  const double t0 = now_ms();
  for (i = 0; i < w->running; i++)
    pthread_join(w->th[i], NULL);
  st->ms_postrace_wait += now_ms() - t0;
  for (i = 0; i < w->n; i++)
    { Job *j = w->job + i;
      if (j->len > 0)
        { FILE *f = fo[j->part];
          const int alen = read_len[j->aread], far = (j->ntiles - 1) * tw;
          fprintf(f, ">%d.%d source=%d,%d,%d correctionq=", j->aread, j->serial, j->aread, 0, alen < far ? alen : far);
          for (k = 0; k < j->ntiles; k++)
            fprintf(f, k ? ",%d,%d" : "%d,%d", j->q[2 * k], j->q[2 * k + 1]);
          if (j->slen > 0)
            { fprintf(f, " postrace=");
              for (k = 0; k < j->slen; k++)
                fprintf(f, k ? ",%d" : "%d", j->script[k]);
            }
          fprintf(f, "\n");
          for (k = 0; k < j->len; k++)
            j->cons[k] = "acgt"[(int) j->cons[k] & 3];
          write_bases(f, j->cons, j->len);
          st->reads += 1;
          st->ms_postrace += j->ms;
        }
      free(j->cons);  free(j->q);  free(j->script);
    }
  free(w->job);
  w->job = NULL;
  w->n = 0;
}

/* partition_overlaps, LAcorrect.c:204: where the parts of -j begin.  NULL after a message. */
static int64 *partition(damar_pile_reader *r, int parts, const char *las)
{ int64 *off = (int64 *) calloc((size_t) parts + 2, sizeof(int64));
  damar_trace_batch t;
  int64 pos = 12, offprev = 12, seen = 0, chunk = 0;
  const int64 per = damar_piles_novl(r) / parts;
  int got, aprev = 0;
  if (off == NULL)
    return NULL;
  off[0] = pos;
  if (parts > 1)
    { if (per == 0)
        { fprintf(stderr, "LAcorrect: -j %d: %s holds fewer overlaps than that\n", parts, las);
          free(off);
          return NULL;
        }
      while ((got = damar_piles_next_traces(r, &t)) > 0)
        { int64 pi, i;
          for (pi = 0; pi < t.p.npiles; pi++)
            for (i = t.p.pile_off[pi]; i < t.p.pile_off[pi + 1]; i++)
              { if (t.p.pile_aread[pi] != aprev)
                  { offprev = pos;
                    aprev = t.p.pile_aread[pi];
                  }
                pos += REC_BYTES + (int64) t.tlen[i] * t.tbytes;
                if (seen % per == 0)
                  { if (chunk > parts)
                      { fprintf(stderr, "LAcorrect: -j %d: the reference's partition of %s writes past its %d offsets\n", parts, las, parts + 1);
                        free(off);
                        return NULL;
                      }
                    off[chunk++] = offprev;
                  }
                seen += 1;
              }
        }
      if (got < 0)
        { free(off);
          return NULL;
        }
      damar_piles_rewind(r);
    }
  off[parts] = -1;             /* the file's size: every pile lies below it */
  return off;
}

static int64 *read_ids(const char *path, int *n)                   /* fread_integers, lib/utils.c:118 */
{ FILE *f = fopen(path, "r");
  int64 *v = NULL;
  int cap = 0, x;
  *n = 0;
  if (f == NULL)
    return NULL;
  v = (int64 *) damar_grow(NULL, sizeof(int64), "correct");
  while (fscanf(f, "%d\n", &x) == 1)
    { if (*n == cap)
        { cap = cap + cap / 4 + 100;
          v = (int64 *) damar_grow(v, sizeof(int64) * (size_t) cap, "correct");
        }
      v[(*n)++] = x;
    }
  fclose(f);
  return v;
}

int damar_correct_las(const char *dbname, const char *las, const char *out, const damar_correct_opts *o, damar_correct_stats *st)
{ damar_dbinfo db;
  damar_pile_reader *r = NULL;
  damar_trace_batch  t;
  HITS_DB blk;
  Layout  L;
  Tiles   T;
  Wave    W[2], *prev = NULL, *cur;
  Job    *loose = NULL;          /* the jobs of the batch in the making: nothing of theirs is allocated before the wave starts */
  int     wi = 0;
  FILE  **fo = NULL;
  uint64 *q_anno = NULL;
  int    *q_data = NULL, *order = NULL, *otmp = NULL, *key = NULL, *added = NULL, *serial = NULL;
  int64  *offs = NULL, *cons_off = NULL, q_ndata = 0, ocap = 0, pos = 12, tcap = 0;
  unsigned char *want = NULL, *done = NULL;
  char   *name = NULL;
  const int parts = o->nthreads;
  int     got, rc = 1, have_db = 0, have_blk = 0, i, part = 0, fresh = 1, tw;
  const char *e = getenv("DAMAR_CORRECT_THREADS");
  const double w0 = now_ms();
  const int on_device = !damar_piles_on_host() && !damar_postrace_on_host();      /* the postrace alignments */

  memset(st, 0, sizeof(*st));
  memset(&L, 0, sizeof(L));  memset(&T, 0, sizeof(T));  memset(W, 0, sizeof(W));
  W[0].nthreads = W[1].nthreads = (e != NULL && atoi(e) >= 1 && atoi(e) <= 64) ? atoi(e) : 8;
  if (parts < 1)
    { fprintf(stderr, "LAcorrect: -j %d: at least one part\n", parts);
      return 1;
    }
  if (damar_dbinfo_open(dbname, &db))
    { fprintf(stderr, "could not open '%s'\n", dbname);
      return 1;
    }
  have_db = 1;
  if (damar_track_read_any(&db, o->q_track, &q_anno, &q_data, &q_ndata))
    { fprintf(stderr, "(null): Track '%s' does not exist\n", o->q_track);
      fprintf(stderr, "could not load quality track %s\n", o->q_track);
      goto done;
    }
  if ((r = damar_piles_open_traces(las, 0, 0)) == NULL)
    goto done;
  tw = damar_piles_tspace(r);
  if ((offs = partition(r, parts, las)) == NULL)
    goto done;
  want = (unsigned char *) calloc((size_t) db.nreads + 1, 1);
  done = (unsigned char *) calloc((size_t) db.nreads + 1, 1);
  serial = (int *) calloc((size_t) parts, sizeof(int));
  fo = (FILE **) calloc((size_t) parts, sizeof(FILE *));
  name = (char *) malloc(strlen(out) + 32);
  if (want == NULL || done == NULL || serial == NULL || fo == NULL || name == NULL)
    goto done;
  if (o->read_ids != NULL)
    { int n;
      int64 *v = read_ids(o->read_ids, &n);
      if (v == NULL)
        { fprintf(stderr, "could not open %s\n", o->read_ids);
          goto done;
        }
      for (i = 0; i < n; i++)
        if (v[i] >= 0 && v[i] < db.nreads)
          want[v[i]] = 1;
      free(v);
    }
  else
    memset(want, 1, (size_t) db.nreads);
  for (i = 0; i < parts; i++)
    { sprintf(name, "%s.%02d.fasta", out, i);
      if ((fo[i] = fopen(name, "w")) == NULL)
        { damar_cannot_write(name);
          goto done;
        }
    }
  if (damar_read_block(dbname, &blk))
    goto done;
  have_blk = 1;
  W[0].blk = W[1].blk = &blk;

  while ((got = damar_piles_next_traces(r, &t)) > 0)
    { damar_pile_batch *b = &t.p;
      damar_tile_batch  tb;
      unsigned char *cons = NULL;
      double ms[4], c0;
      int64  c3[3], pi, k;
      int    njob = 0;

      T.ntiles = T.nent = T.nbases = 0;
      cur = &W[wi];
      cur->job = loose = (Job *) damar_grow(NULL, sizeof(Job) * (size_t) (b->npiles + 1), "correct");
      for (pi = 0; pi < b->npiles; pi++)
        { const int64 lo = b->pile_off[pi];
          const int   aread = b->pile_aread[pi], nall = (int) (b->pile_off[pi + 1] - lo);
          int   n = 0, alen, ntiles, bad = -1, first = 0;
          const int64 at = pos;
          Job  *j;

          for (k = lo; k < b->pile_off[pi + 1]; k++)
            pos += REC_BYTES + (int64) t.tlen[k] * t.tbytes;
          if (aread < 0 || aread >= db.nreads)
            { damar_reads_missing(las);
              goto done;
            }
          while (part + 1 < parts && at >= offs[part + 1])
            { part += 1;
              fresh = 1;
            }
          if (damar_room(&ocap, nall, 1024))
            { order = (int *) damar_grow(order, sizeof(int) * (size_t) ocap, "correct");
              otmp = (int *) damar_grow(otmp, sizeof(int) * (size_t) ocap, "correct");
              key = (int *) damar_grow(key, sizeof(int) * (size_t) ocap, "correct");
            }
          /* the records of the pile that the reference keeps: LAcorrect.c:1444-1517.  A thread skips discarded records
             at the head of its part, over piles if need be; after that the first record of a pile is used whatever its
             flags (here: unless it has no trace), the later ones unless they are discarded or have no trace */
          if (fresh)
            while (first < nall && ((b->flags[lo + first] & OVL_DISCARD) || t.tlen[lo + first] == 0))
              first += 1;
          if (first == nall)
            continue;
          fresh = 0;
          for (i = first; i < nall; i++)
            if (t.tlen[lo + i] != 0 && (i == first || !(b->flags[lo + i] & OVL_DISCARD)))
              { key[i] = b->aepos[lo + i] - b->abpos[lo + i];
                order[n++] = i;
              }
          if (n == 0 || !want[aread])
            continue;
          stable_sort_int(order, otmp, n, key, 1);
          alen = db.read_len[aread];
          ntiles = (alen + tw - 1) / tw;
          if (o->verbose)
            printf("T%d READ %8d (%5d)\n", part, aread, alen);
          for (i = 0; i < n && bad < 0; i++)
            if (t.tlen[lo + order[i]] < 2 || !valid_pt_points(&t, lo + order[i]))
              bad = i;
          if (bad >= 0)
            { printf("ERROR: bad pt points ovl %d aread %d bread %d\n", bad, aread, b->bread[lo + order[bad]]);
              continue;
            }
          if ((int64) (q_anno[aread] / 4) + ntiles > q_ndata)
            { fprintf(stderr, "damar: correct: track %s holds fewer values than read %d has tiles\n", o->q_track, aread);
              goto done;
            }
          if (layout_pile(&L, &t, order, lo, n, aread, alen, q_data + q_anno[aread] / 4, db.read_len, db.nreads))
            goto done;
          done[aread] = 1;
          j = cur->job + njob++;
          memset(j, 0, sizeof(*j));
          j->aread = aread;  j->part = part;  j->ntiles = ntiles;  j->tile0 = T.ntiles;
          /* the sequences each tile's consensus takes: single_tile_consensus, LAcorrect.c:287 */
          if (T.ntiles + ntiles + 1 > T.ctile)
            { T.ctile = T.ntiles + ntiles + T.ctile / 4 + 4096;
              T.ent_off = (int64 *) damar_grow(T.ent_off, sizeof(int64) * (size_t) (T.ctile + 1), "correct");
              T.weight = (int *) damar_grow(T.weight, sizeof(int) * (size_t) T.ctile, "correct");
            }
          for (i = 0; i < ntiles; i++)
            { int taken = 0, x, wsum = 0;
              T.ent_off[T.ntiles] = T.nent;
              for (x = L.toff[i]; x < L.toff[i + 1] && taken < MAX_COVERAGE; x++)
                { const Tile *tl = L.tovl + x;
                  const int len = tl->be - tl->bb, rd = tl->b < 0 ? aread : tl->b;
                  const char *s = (const char *) blk.bases + blk.reads[rd].boff;
                  unsigned char *d;
                  int y;
                  if (tl->apos != 0 || len < MIN_TWIDTH)
                    continue;
                  if (T.nent + 1 > T.cent)
                    { T.cent = T.nent + T.cent / 4 + 4096;
                      T.seq_off = (int64 *) damar_grow(T.seq_off, sizeof(int64) * (size_t) T.cent, "correct");
                      T.seq_len = (int *) damar_grow(T.seq_len, sizeof(int) * (size_t) T.cent, "correct");
                    }
                  if (T.nbases + len > T.cbases)
                    { T.cbases = T.nbases + len + T.cbases / 4 + (1 << 16);
                      T.bases = (unsigned char *) damar_grow(T.bases, (size_t) T.cbases, "correct");
                    }
                  d = T.bases + T.nbases;
                  if (!tl->comp)
                    for (y = 0; y < len; y++) d[y] = (unsigned char) (s[tl->bb + y] & 3);
                  else
                    { const int blen = blk.reads[rd].rlen;
                      for (y = 0; y < len; y++) d[y] = (unsigned char) (3 - (s[blen - 1 - (tl->bb + y)] & 3));
                    }
                  T.seq_off[T.nent] = T.nbases;
                  T.seq_len[T.nent] = len;
                  T.nent += 1;
                  T.nbases += len;
                  wsum += tl->qv + 1;
                  taken += 1;
                }
              T.weight[T.ntiles] = wsum;
              T.ntiles += 1;
            }
        }
      if (T.ent_off == NULL)          /* a batch without a tile */
        T.ent_off = (int64 *) damar_grow(NULL, sizeof(int64) * 2, "correct");
      T.ent_off[T.ntiles] = T.nent;
      tb.ntiles = T.ntiles;  tb.ent_off = T.ent_off;  tb.seq_off = T.seq_off;  tb.seq_len = T.seq_len;
      tb.bases = T.bases;  tb.nbases = T.nbases;  tb.weight = T.weight;
      if (T.ntiles + 1 > tcap)
        { tcap = T.ntiles + T.ntiles / 4 + 4096;
          cons_off = (int64 *) damar_grow(cons_off, sizeof(int64) * (size_t) (tcap + 1), "correct");
          added = (int *) damar_grow(added, sizeof(int) * (size_t) tcap, "correct");
        }
      c0 = now_ms();
      if (damar_tile_consensus(&tb, cons_off, &cons, added))
        { cur->job = NULL;
          goto done;
        }
      st->ms_consensus += now_ms() - c0;
      damar_correct_last(ms, c3);
      st->ms_kernel += ms[1];
      st->tiles += c3[0];  st->host_tiles += c3[1];  st->bases += c3[2];
      /* the reads of this batch: the tiles' calls back to back, the serial of the read within its part's file */
      for (i = 0; i < njob; i++)
        { Job *j = cur->job + i;
          const int64 a0 = cons_off[j->tile0], a1 = cons_off[j->tile0 + j->ntiles];
          j->len = (int) (a1 - a0);
          j->q = (int *) damar_grow(NULL, sizeof(int) * 2 * (size_t) j->ntiles, "correct");
          for (k = 0; k < j->ntiles; k++)
            { j->q[2 * k] = (int) (cons_off[j->tile0 + k + 1] - cons_off[j->tile0 + k]);
              j->q[2 * k + 1] = added[j->tile0 + k];
            }
          if (j->len > 0)
            { j->cons = (char *) damar_grow(NULL, (size_t) j->len + 1, "correct");
              memcpy(j->cons, cons + a0, (size_t) j->len);
              j->serial = serial[j->part]++;
            }
        }
      free(cons);
      cur->n = njob;
      if (prev != NULL)
        wave_finish(prev, fo, tw, db.read_len, st);
      loose = NULL;
      prev = cur;
      if (!on_device)
        wave_start(cur);
      else if (wave_device(cur, st))
        goto done;
      wi ^= 1;
    }
  if (prev != NULL)
    wave_finish(prev, fo, tw, db.read_len, st);
  prev = NULL;
  if (got < 0)
    goto done;
  /* the reads that were asked for and not corrected, as they are: LAcorrect.c:1752-1778 */
  { int rb = 0, re = db.nreads;
    if (o->block > 0)
      { if (o->block <= db.nblocks)
          { rb = db.block_first[o->block - 1];
            re = db.block_first[o->block];
          }
        else
          rb = re = -1;
      }
    for (i = rb; i < re; i++)
      if (want[i] && !done[i])
        { const int len = blk.reads[i].rlen;
          const char *s = (const char *) blk.bases + blk.reads[i].boff;
          char *buf = (char *) damar_grow(NULL, (size_t) len + 1, "correct");
          int k;
          for (k = 0; k < len; k++)
            buf[k] = "acgt"[(int) s[k] & 3];
          fprintf(fo[i % parts], ">copy.%d source=%d,%d,%d\n", i, i, -1, -1);
          write_bases(fo[i % parts], buf, len);
          free(buf);
          st->copies += 1;
        }
  }
  rc = 0;
done:
  free(loose);
  if (prev != NULL)
    wave_finish(prev, fo, damar_piles_tspace(r), db.read_len, st);
  if (fo != NULL)
    for (i = 0; i < parts; i++)
      if (fo[i] != NULL && fclose(fo[i]) != 0 && rc == 0)
        { sprintf(name, "%s.%02d.fasta", out, i);
          rc = damar_cannot_write(name);
        }
  fflush(stdout);
  damar_piles_close(r);
  if (have_blk) damar_close_block(&blk);
  if (have_db) damar_dbinfo_close(&db);
  free(q_anno);  free(q_data);  free(order);  free(otmp);  free(key);  free(added);  free(serial);  free(offs);  free(cons_off);
  free(want);  free(done);  free(name);  free(fo);
  free(L.toff);  free(L.cur);  free(L.tovl);  free(L.tmp);
  free(T.ent_off);  free(T.seq_off);  free(T.seq_len);  free(T.weight);  free(T.bases);
  damar_host_tile_release();
  st->ms_total = now_ms() - w0;
  return rc;
}
