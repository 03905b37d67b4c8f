/* piles.c -- the host side of the two mask tools that turn overlaps back into tracks (scrub/LArepeat.c, scrub/TANmask.c):
 *   - the read table of a database without its bases (stub + .idx),
 *   - a streaming reader that cuts a .las file into batches of whole piles (all records of one A read, lib/pass.c:118-249),
 *     without the records' traces (the mask tools) or with them (LAq, host/quality.c),
 *   - the plain sweep of both tools, one pile at a time (DAMAR_PILES=host; the second opinion for kernels/pile_sweep.hip),
 *   - the writers of both track forms (lib/tracks.c:180-270 .a2/.d2, TANmask.c:462-487 .anno/.data).
 * Nothing here touches the GPU runtime: the file builds into a stand-alone program as it is. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>

#include "damar_hip.h"
#include "damar_host.h"

#define EDGE_DIST 1000                    /* LArepeat.c:38-39 */
#define EDGE_FUZZ 200
#define SEP_FUZZ  20                      /* TANmask.c:82 */

int damar_piles_on_host(void)
{ const char *e = getenv("DAMAR_PILES");
  return e != NULL && strcmp(e, "host") == 0;
}

/***** the read table ***************************************************************************/

int damar_dbinfo_open(const char *name, damar_dbinfo *db)
{ char *root = damar_root(name, ".db");
  char  dir[4096], path[8300], line[8300];
  const char *slash = strrchr(name, '/');
  FILE *stub = NULL, *idx = NULL;
  HITS_DB head;
  HITS_READ *reads = NULL;
  int   nfiles, i;

  memset(db, 0, sizeof(*db));
  if (slash == NULL)
    strcpy(dir, ".");
  else
    snprintf(dir, sizeof(dir), "%.*s", (int) (slash - name), name);
  snprintf(path, sizeof(path), "%s/%s.db", dir, root);
  if ((stub = fopen(path, "r")) == NULL)
    { fprintf(stderr, "damar: cannot open database stub %s\n", path);
      goto fail;
    }
  snprintf(path, sizeof(path), "%s/.%s.idx", dir, root);
  if ((idx = fopen(path, "r")) == NULL || fread(&head, sizeof(head), 1, idx) != 1)
    { fprintf(stderr, "damar: cannot read index %s\n", path);
      goto fail;
    }
  db->nreads = head.ureads;
  db->maxlen = head.maxlen;
  reads = (HITS_READ *) damar_grow(NULL, sizeof(HITS_READ) * (size_t) db->nreads, "piles");
  if (fread(reads, sizeof(HITS_READ), (size_t) db->nreads, idx) != (size_t) db->nreads)
    { fprintf(stderr, "damar: index %s is truncated\n", path);
      goto fail;
    }
  db->read_len   = (int *) damar_grow(NULL, sizeof(int) * (size_t) db->nreads, "piles");
  db->read_flags = (int *) damar_grow(NULL, sizeof(int) * (size_t) db->nreads, "piles");
  for (i = 0; i < db->nreads; i++)
    { db->read_len[i]   = reads[i].rlen;
      db->read_flags[i] = reads[i].flags;
    }
  free(reads);
  reads = NULL;
  if (fscanf(stub, "files = %9d\n", &nfiles) != 1)
    goto junk;
  for (i = 0; i < nfiles; i++)
    if (fgets(line, sizeof(line), stub) == NULL)
      goto junk;
  db->nblocks = 0;
  if (fscanf(stub, "blocks = %9d\n", &db->nblocks) == 1)
    { long long size;
      if (fscanf(stub, "size = %9lld\n", &size) != 1)
        goto junk;
      db->block_first = (int *) damar_grow(NULL, sizeof(int) * (size_t) (db->nblocks + 1), "piles");
      for (i = 0; i <= db->nblocks; i++)
        if (fscanf(stub, " %9d\n", &db->block_first[i]) != 1)
          goto junk;
    }
  snprintf(path, sizeof(path), "%s/.%s", dir, root);           /* db/DB.c Open_DB: path = pwd "/." root */
  db->path = strdup(path);
  fclose(stub);
  fclose(idx);
  free(root);
  return 0;
junk:
  fprintf(stderr, "damar: database stub of %s is junk\n", root);
fail:
  if (stub) fclose(stub);
  if (idx) fclose(idx);
  free(reads);
  free(root);
  damar_dbinfo_close(db);
  return -1;
}

void damar_dbinfo_close(damar_dbinfo *db)
{ free(db->read_len);  free(db->read_flags);  free(db->block_first);  free(db->path);
  memset(db, 0, sizeof(*db));
}

/***** the pile reader **************************************************************************/

struct damar_pile_reader
{ FILE  *f;
  int64  novl, seen, bound;
  int64  size;                 /* of the file in bytes: a trace may not reach beyond it */
  int    tspace, tbytes;
  int    have;                 /* a record read ahead: the first of the next pile */
  int    rec[10];              /* the 40 bytes of a record as they lie in the file */
  int64  cap, pcap;
  int64  pstart, pend;     /* a pile held back for the next batch: where it lies in the columns */
  int    pend_aread;
  int64 *pile_off;
  int   *pile_aread;
  int   *col[9];               /* abpos aepos bbpos bepos bread flags, then diffs and the record's last word (damar_piles_rest),
                                  and the number of trace values (damar_piles_tlen) */
  /* traces on (damar_piles_open_traces): the records' trace bytes as they lie in the file, back to back */
  int    traces;
  int64  tbound;               /* bytes of trace a batch holds at most, a pile alone in its batch excepted */
  unsigned char *rtrace;       /* of the record read ahead */
  int64  rtcap;
  unsigned char *tbuf;
  int64  tcap, ttop;
  int64 *toff;                 /* per record: where its trace begins in tbuf */
  int   *tlen;
};

/* 1: a record, 0: all novl records of the header are through, -1: the file ends before that, on a record boundary or not */
static int next_record(damar_pile_reader *r)
{ if (r->seen >= r->novl)
    return 0;
  if (fread(r->rec, 1, 40, r->f) != 40 || r->rec[0] < 0)
    return -1;
  if (r->traces)
    { const int64 n = (int64) r->tbytes * r->rec[0];
      if ((int64) ftello(r->f) + n > r->size)
        return -1;
      r->rtrace = (unsigned char *) damar_reserve(r->rtrace, &r->rtcap, n, 1, 1024, "piles");
      if (n > 0 && fread(r->rtrace, 1, (size_t) n, r->f) != (size_t) n)
        return -1;
    }
  else if (fseeko(r->f, (off_t) r->tbytes * r->rec[0], SEEK_CUR) != 0 || (int64) ftello(r->f) > r->size)
    return -1;
  r->seen += 1;
  return 1;
}

damar_pile_reader *damar_piles_open(const char *las, int64 bound)
{ damar_pile_reader *r = (damar_pile_reader *) calloc(1, sizeof(*r));
  const char *e = getenv("DAMAR_PILE_BATCH");
  if (r == NULL)
    return NULL;
  if (bound <= 0)
    bound = (int64) 8 << 20;
  if (e != NULL && atoll(e) > 0 && atoll(e) < bound)
    bound = atoll(e);
  r->bound = bound;
  if ((r->f = fopen(las, "r")) == NULL)
    { fprintf(stderr, "could not open '%s'\n", las);
      free(r);
      return NULL;
    }
  if (fread(&r->novl, sizeof(int64), 1, r->f) != 1 || fread(&r->tspace, sizeof(int), 1, r->f) != 1)
    { r->novl = 0;              /* an empty file holds no pile (lib/pass.c:102-107) */
      r->tspace = 0;
    }
  r->tbytes = (r->tspace <= TRACE_XOVR) ? 1 : 2;
  { off_t at = ftello(r->f);
    fseeko(r->f, 0, SEEK_END);
    r->size = (int64) ftello(r->f);
    fseeko(r->f, at, SEEK_SET);
  }
  return r;
}

/* the same reader with the traces on: batches come from damar_piles_next_traces and are bounded by records as above and by
   trace bytes (tbound <= 0: 1 GiB; DAMAR_PILE_TRACE_BYTES lowers it) */
damar_pile_reader *damar_piles_open_traces(const char *las, int64 bound, int64 tbound)
{ damar_pile_reader *r = damar_piles_open(las, bound);
  const char *e = getenv("DAMAR_PILE_TRACE_BYTES");
  if (r == NULL)
    return NULL;
  if (tbound <= 0)
    tbound = (int64) 1 << 30;
  if (e != NULL && atoll(e) > 0 && atoll(e) < tbound)
    tbound = atoll(e);
  r->traces = 1;
  r->tbound = tbound;
  return r;
}

void damar_piles_rewind(damar_pile_reader *r)
{ fseeko(r->f, (off_t) (sizeof(int64) + sizeof(int)), SEEK_SET);
  r->seen = 0;
  r->have = 0;
  r->pend = 0;
}

int damar_piles_tspace(const damar_pile_reader *r) { return r->tspace; }
int64 damar_piles_novl(const damar_pile_reader *r) { return r->novl; }

void damar_piles_close(damar_pile_reader *r)
{ int i;
  if (r == NULL)
    return;
  if (r->f) fclose(r->f);
  free(r->pile_off);  free(r->pile_aread);
  for (i = 0; i < 9; i++) free(r->col[i]);
  free(r->rtrace);  free(r->tbuf);  free(r->toff);  free(r->tlen);
  free(r);
}

/* the next batch of whole piles: piles are added while the batch stays within the bound; a pile that would cross it is
   held back for the next batch, so only a pile that is larger than the bound by itself exceeds it, alone in its batch.
   The arrays belong to the reader and hold until the next call.  1: a batch, 0: no pile is left, -1: the file is damaged. */
static int piles_next(damar_pile_reader *r, damar_pile_batch *b)
{ int64 n = 0, np = 0, start;
  int   i, got, a;

  memset(b, 0, sizeof(*b));
  r->ttop = 0;
  if (r->pend > 0)
    { for (i = 0; i < 9; i++)
        memmove(r->col[i], r->col[i] + r->pstart, sizeof(int) * (size_t) r->pend);
      if (r->traces)
        { const int64 t0 = r->toff[r->pstart];
          int64 k;
          for (k = 0; k < r->pend; k++)
            { r->tlen[k] = r->tlen[r->pstart + k];
              r->toff[k] = r->toff[r->pstart + k] - t0;
            }
          r->ttop = r->toff[r->pend - 1] + (int64) r->tbytes * r->tlen[r->pend - 1];
          memmove(r->tbuf, r->tbuf + t0, (size_t) r->ttop);
        }
      r->pile_off[0] = 0;  r->pile_off[1] = n = r->pend;
      r->pile_aread[0] = r->pend_aread;
      np = 1;
      r->pend = 0;
    }
  else if (!r->have)
    { if ((got = next_record(r)) < 0)
        fprintf(stderr, "damar: .las file ends before the %lld records of its header\n", (long long) r->novl);
      if (got <= 0)
        return got;
      r->have = 1;
    }
  while (r->have && n < r->bound && (!r->traces || r->ttop < r->tbound))
    { start = n;
      a = r->rec[7];
      do
        { if (n >= r->cap)
            { r->cap = r->cap + r->cap / 4 + 1024;
              for (i = 0; i < 9; i++)
                r->col[i] = (int *) damar_grow(r->col[i], sizeof(int) * (size_t) r->cap, "piles");
              if (r->traces)
                { r->toff = (int64 *) damar_grow(r->toff, sizeof(int64) * (size_t) r->cap, "piles");
                  r->tlen = (int *) damar_grow(r->tlen, sizeof(int) * (size_t) r->cap, "piles");
                }
            }
          if (r->traces)
            { const int64 nb = (int64) r->tbytes * r->rec[0];
              if (r->ttop + nb > r->tcap)
                { r->tcap = r->ttop + nb + r->tcap / 4 + 4096;
                  r->tbuf = (unsigned char *) damar_grow(r->tbuf, (size_t) r->tcap, "piles");
                }
              if (nb > 0)
                memcpy(r->tbuf + r->ttop, r->rtrace, (size_t) nb);
              r->toff[n] = r->ttop;
              r->tlen[n] = r->rec[0];
              r->ttop += nb;
            }
          r->col[0][n] = r->rec[2];  r->col[1][n] = r->rec[4];      /* abpos aepos */
          r->col[2][n] = r->rec[3];  r->col[3][n] = r->rec[5];      /* bbpos bepos */
          r->col[4][n] = r->rec[8];  r->col[5][n] = r->rec[6];      /* bread flags */
          r->col[6][n] = r->rec[1];  r->col[7][n] = r->rec[9];      /* diffs, the word behind bread */
          r->col[8][n] = r->rec[0];
          n += 1;
          got = next_record(r);
          if (got < 0)
            { fprintf(stderr, "damar: .las file ends before the %lld records of its header\n", (long long) r->novl);
              return -1;
            }
          r->have = got;
        }
      while (r->have && r->rec[7] == a);
      if (start > 0 && (n > r->bound || (r->traces && r->ttop > r->tbound)))
        { r->pstart = start;  r->pend = n - start;  r->pend_aread = a;
          n = start;
          break;
        }
      if (np + 2 >= r->pcap)
        { r->pcap = r->pcap + r->pcap / 4 + 256;
          r->pile_off   = (int64 *) damar_grow(r->pile_off, sizeof(int64) * (size_t) (r->pcap + 1), "piles");
          r->pile_aread = (int *) damar_grow(r->pile_aread, sizeof(int) * (size_t) r->pcap, "piles");
        }
      r->pile_off[np] = start;
      r->pile_aread[np] = a;
      np += 1;
      r->pile_off[np] = n;
    }
  if (np == 0)
    return 0;
  b->npiles = np;  b->nrec = n;
  b->pile_off = r->pile_off;  b->pile_aread = r->pile_aread;
  b->abpos = r->col[0];  b->aepos = r->col[1];  b->bbpos = r->col[2];  b->bepos = r->col[3];
  b->bread = r->col[4];  b->flags = r->col[5];
  return 1;
}

int damar_piles_next(damar_pile_reader *r, damar_pile_batch *b)
{ if (r->traces)
    { fprintf(stderr, "damar: this pile reader carries traces: damar_piles_next_traces reads it\n");
      return -1;
    }
  return piles_next(r, b);
}

/* what a batch's records hold beside the columns of damar_pile_batch, for a tool that writes records back (LAtrim): their
   differences and the unused word that ends the 40 bytes of a record in the file */
void damar_piles_rest(const damar_pile_reader *r, const int **diffs, const int **last_word)
{ *diffs = r->col[6];
  *last_word = r->col[7];
}

/* the trace values of a batch's records, with or without the traces themselves: with tbytes (1 for a trace spacing of 125
   or less, else 2) what tells where in the file a record lies (OGbuild's progress lines) */
const int *damar_piles_tlen(const damar_pile_reader *r) { return r->col[8]; }

/* the next batch with its traces: record i's tlen[i] values of tbytes bytes begin at trace + trace_off[i] */
int damar_piles_next_traces(damar_pile_reader *r, damar_trace_batch *t)
{ int got;
  memset(t, 0, sizeof(*t));
  if (!r->traces)
    { fprintf(stderr, "damar: this pile reader was opened without traces\n");
      return -1;
    }
  if ((got = piles_next(r, &t->p)) <= 0)
    return got;
  t->trace = r->tbuf;  t->trace_off = r->toff;  t->tlen = r->tlen;
  t->trace_bytes = (r->pend > 0) ? r->toff[r->pstart] : r->ttop;
  t->tbytes = r->tbytes;  t->tspace = r->tspace;
  return 1;
}

/***** the sweeps, one pile at a time ***********************************************************/

static int cmp_int(const void *x, const void *y)
{ int a = *(const int *) x, b = *(const int *) y;
  return (a > b) - (a < b);
}

/* order of the repeat events: by coordinate, an end before a start on the same one (LArepeat.c:107-120) */
static int cmp_event(const void *x, const void *y)
{ int a = *(const int *) x, b = *(const int *) y;
  int c = abs(a) - abs(b);
  return c ? c : (a > b) - (a < b);
}

int damar_host_pile_coverage(const damar_pile_batch *b, const damar_repeat_params *p, int64 *histo, int64 *bases, int64 *inactive)
{ int64 pi, i, cap = 0;
  int  *ev = NULL;
  for (pi = 0; pi < b->npiles; pi++)
    { const int64 lo = b->pile_off[pi], hi = b->pile_off[pi + 1];
      const int a = b->pile_aread[pi], alen = b->read_len[a];
      int64 sum = 0, active = 0, cov;
      int   n = 0, depth = 0;
      if (2 * (hi - lo) > cap)
        { cap = 2 * (hi - lo) + 64;
          ev = (int *) damar_grow(ev, sizeof(int) * (size_t) cap, "piles");
        }
      for (i = lo; i < hi; i++)
        { if (!(b->read_flags[b->bread[i]] & DB_BEST) || (b->flags[i] & OVL_DISCARD) || b->bread[i] == a ||
              b->aepos[i] - b->abpos[i] < p->min_aln_len)
            continue;
          sum += b->aepos[i] - b->abpos[i];
          ev[n++] = 2 * b->abpos[i] + 1;            /* union of [abpos, aepos): any order on one coordinate gives the same length */
          ev[n++] = 2 * b->aepos[i];
        }
      qsort(ev, (size_t) n, sizeof(int), cmp_int);
      for (i = 0; i < n; i++)
        { depth += (ev[i] & 1) ? 1 : -1;
          if (depth > 0 && i + 1 < n)
            active += (ev[i + 1] >> 1) - (ev[i] >> 1);
        }
      cov = active > 0 ? sum / active : 0;
      if (cov < p->max_cov)
        histo[cov] += 1;
      *bases += alen;
      *inactive += alen - active;
    }
  free(ev);
  return 0;
}

int damar_host_pile_repeats(const damar_pile_batch *b, const damar_repeat_params *p, damar_pile_track *out)
{ const int enter = (int) (p->cov * p->xcov_enter), leave = (int) (p->cov * p->xcov_leave);
  const int width = 2 + (p->inccov ? 1 : 0);
  int64 pi, i, j, cap = 0, dcap = 1024, top = 0;
  int  *ev = NULL, *data = (int *) damar_grow(NULL, sizeof(int) * (size_t) dcap, "piles");
  out->merged = out->repeat_bases = 0;
  for (pi = 0; pi < b->npiles; pi++)
    { const int64 lo = b->pile_off[pi], hi = b->pile_off[pi + 1], base = top;
      const int a = b->pile_aread[pi], alen = b->read_len[a];
      int n = 0, k, span = 0, inside = 0, peak = 0;
      if (2 * (hi - lo) > cap)
        { cap = 2 * (hi - lo) + 64;
          ev = (int *) damar_grow(ev, sizeof(int) * (size_t) cap, "piles");
        }
      for (i = lo; i < hi; i++)
        { if ((b->flags[i] & OVL_DISCARD) || (!p->inc_identity && b->bread[i] == a) ||
              b->aepos[i] - b->abpos[i] < p->min_aln_len)
            continue;
          ev[n++] = b->abpos[i];
          ev[n++] = -(b->aepos[i] - 1);
        }
      k = n / 2;
      qsort(ev, (size_t) n, sizeof(int), cmp_event);
      if (top + 3 * (int64) k + 8 > dcap)
        { dcap = dcap + dcap / 4 + 3 * (int64) k + 8;
          data = (int *) damar_grow(data, sizeof(int) * (size_t) dcap, "piles");
        }
      /* a region is open from the event that lifts the depth above `enter` to the one that drops it below `leave`; the
         value kept with -C is the highest depth a start reached strictly after the opening event (:340-352, 405) and, over
         a merge, the predecessor's stored value (:397) */
      for (i = 0; i < n; i++)
        { if (ev[i] < 0) span -= 1;
          else
            { span += 1;
              if (span > peak) peak = span;
            }
          if (inside && span < leave)
            { data[top++] = -ev[i];
              out->repeat_bases += data[top - 1] - data[top - 2];
              if (p->inccov) data[top++] = peak;
              inside = 0;
            }
          else if (!inside && span > enter)
            { if (top - base >= width && ev[i] - data[top - (width - 1)] < p->merge_dist)
                { peak = p->inccov ? data[top - 1] : 0;
                  top -= width - 1;                          /* the predecessor's end (and value) go, its begin stays */
                  out->merged += 1;
                }
              else
                { peak = 0;
                  data[top++] = ev[i];
                }
              inside = 1;
            }
        }
      /* edge extension (:439-487): the reference counts support over the first k records of the UNFILTERED pile.  A region
         left open at the pile's end has no end coordinate (the reference reads a stale one there): it is not extended. */
      for (j = base; j < (inside ? top - 1 : top); j += width)
        { const int rb = data[j], re = data[j + 1];
          int support;
          if (rb > 0 && rb < EDGE_DIST && re < alen - EDGE_DIST)
            { support = 0;
              for (i = lo; i < lo + k; i++)
                if (b->aepos[i] > re - EDGE_FUZZ && b->aepos[i] < re + EDGE_FUZZ && b->abpos[i] == 0)
                  support += 1;
              if (support > 2) data[j] = 0;
            }
          if (re < alen - 1 && re > alen - EDGE_DIST && rb > EDGE_DIST)
            { support = 0;
              for (i = lo; i < lo + k; i++)
                if (b->abpos[i] > rb - EDGE_FUZZ && b->abpos[i] < rb + EDGE_FUZZ && b->aepos[i] == alen)
                  support += 1;
              if (support > 2) data[j + 1] = alen;
            }
        }
      out->count[pi] = (int) (top - base);
    }
  free(ev);
  out->data = data;
  out->ndata = top;
  return 0;
}

int damar_host_pile_tandem(const damar_pile_batch *b, int min_len, damar_pile_track *out)
{ int64 pi, i, cap = 0, dcap = 1024, top = 0;
  int  *ev = NULL, *data = (int *) damar_grow(NULL, sizeof(int) * (size_t) dcap, "piles");
  out->merged = out->repeat_bases = 0;
  for (pi = 0; pi < b->npiles; pi++)
    { const int64 lo = b->pile_off[pi], hi = b->pile_off[pi + 1], base = top;
      int n = 0, depth = 0;
      if (2 * (hi - lo) > cap)
        { cap = 2 * (hi - lo) + 64;
          ev = (int *) damar_grow(ev, sizeof(int) * (size_t) cap, "piles");
        }
      for (i = lo; i < hi; i++)
        if (b->abpos[i] - b->bepos[i] <= SEP_FUZZ && b->aepos[i] - b->bbpos[i] > min_len)
          { ev[n++] = 2 * b->bbpos[i];              /* a start sorts before an end on its coordinate: touching intervals fuse */
            ev[n++] = 2 * b->aepos[i] + 1;
          }
      qsort(ev, (size_t) n, sizeof(int), cmp_int);
      if (top + n + 8 > dcap)
        { dcap = dcap + dcap / 4 + n + 8;
          data = (int *) damar_grow(data, sizeof(int) * (size_t) dcap, "piles");
        }
      for (i = 0; i < n; i++)
        if (ev[i] & 1)
          { if (--depth == 0) data[top++] = ev[i] >> 1; }
        else
          { if (depth++ == 0) data[top++] = ev[i] >> 1; }
      out->count[pi] = (int) (top - base);
    }
  free(ev);
  out->data = data;
  out->ndata = top;
  return 0;
}

/***** track writers ****************************************************************************/

/* lib/compression.c:15-77: runs of {u64 n, n bytes of one zlib stream}, a stream per 8 MiB of input */
static int write_chunks(FILE *f, const void *buf, uint64 len, uint64 *written)
{ const unsigned char *in = (const unsigned char *) buf;
  const uint64 chunk = 8u << 20;
  *written = 0;
  while (len > 0)
    { const uint64 n = len < chunk ? len : chunk;
      uLongf  clen = compressBound((uLong) n);
      unsigned char *o = (unsigned char *) damar_grow(NULL, clen, "piles");
      uint64  c64;
      if (compress(o, &clen, in, (uLong) n) != Z_OK)
        { free(o);
          return -1;
        }
      c64 = clen;
      if (fwrite(&c64, 8, 1, f) != 1 || fwrite(o, clen, 1, f) != 1)
        { free(o);
          return -1;
        }
      free(o);
      *written += 8 + c64;
      in += n;
      len -= n;
    }
  return 0;
}

/* <path>[.<block>].<track>.a2 / .d2; anno = u64 byte offsets for the nreads + 1 reads of the whole database */
int damar_track_write_a2(const char *dbpath, const char *track, int block, int nreads, const uint64 *anno, const int *data, int64 ndata)
{ struct { uint16 version, size; uint32 pad; uint64 len, clen, cdlen, r1, r2, r3, r4; } h;
  char  name[4400], path[4500];
  FILE *af, *df;
  int   rc = -1;
  if (block > 0) snprintf(name, sizeof(name), "%s.%d.%s", dbpath, block, track);
  else           snprintf(name, sizeof(name), "%s.%s", dbpath, track);
  snprintf(path, sizeof(path), "%s.a2", name);
  if ((af = fopen(path, "w")) == NULL)
    { fprintf(stderr, "failed to open %s\n", path);
      return -1;
    }
  snprintf(path, sizeof(path), "%s.d2", name);
  if ((df = fopen(path, "w")) == NULL)
    { fprintf(stderr, "failed to open %s\n", path);
      fclose(af);
      return -1;
    }
  memset(&h, 0, sizeof(h));
  h.version = 2;
  h.size = 8;
  h.len = (uint64) nreads;
  if (fwrite(&h, sizeof(h), 1, af) == 1 &&
      write_chunks(af, anno, 8 * (uint64) (nreads + 1), &h.clen) == 0 &&
      write_chunks(df, data, 4 * (uint64) ndata, &h.cdlen) == 0)
    { rewind(af);
      rc = (fwrite(&h, sizeof(h), 1, af) == 1) ? 0 : -1;
    }
  if (rc)
    fprintf(stderr, "failed to write track %s\n", name);
  fclose(af);
  fclose(df);
  return rc;
}

/* <path>[.<block>].<track>.anno = int len, int 8, int64 offs[len + 1] (bytes); .data = the ints */
int damar_track_write_anno(const char *dbpath, const char *track, int block, int len, const int64 *offs, const int *data)
{ char  name[4400], path[4500];
  FILE *af, *df;
  int   size = 8, rc;
  if (block > 0) snprintf(name, sizeof(name), "%s.%d.%s", dbpath, block, track);
  else           snprintf(name, sizeof(name), "%s.%s", dbpath, track);
  snprintf(path, sizeof(path), "%s.anno", name);
  af = fopen(path, "w");
  snprintf(path, sizeof(path), "%s.data", name);
  df = fopen(path, "w");
  if (af == NULL || df == NULL)
    { fprintf(stderr, "damar: cannot open track files %s.anno / .data for writing\n", name);
      if (af) fclose(af);
      if (df) fclose(df);
      return -1;
    }
  rc = fwrite(&len, sizeof(int), 1, af) == 1 && fwrite(&size, sizeof(int), 1, af) == 1 &&
       fwrite(offs, sizeof(int64), (size_t) (len + 1), af) == (size_t) (len + 1) &&
       (offs[len] == 0 || fwrite(data, 1, (size_t) offs[len], df) == (size_t) offs[len]);
  fclose(af);
  fclose(df);
  return rc ? 0 : -1;
}
