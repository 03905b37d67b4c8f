/* quality.c -- LAq (scrub/LAq.c) as calls: the q track, a quality value per trace-spacing segment ("tile") of every A read
 * from the difference counts its overlaps' traces hold, and the trim track derived from it.
 *   - damar_host_pile_quality: the plain histogram of one pile at a time, as the reference's handler_annotate
 *     (DAMAR_PILES=host; the second opinion for kernels/pile_quality.hip),
 *   - damar_trim_from_q: the 5-tile window walk from both ends (trim_q_offsets), shared by both passes,
 *   - damar_q_track: the annotate pass over a file, batch by batch through damar_pile_quality (the GPU unless
 *     DAMAR_PILES=host); the walk stays here: it is sequential per read, O(tiles), and the q values come back anyway,
 *   - damar_trim_update: -u, record headers plus the two tracks at hand.
 * Nothing here touches the GPU runtime. */
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>

#include "damar_hip.h"
#include "damar_host.h"

#define TRIM_WINDOW 5                     /* LAq.c:36 */

int damar_trace_batch_valid(const damar_trace_batch *t, int64 *ntiles_out)
{ const damar_pile_batch *b = &t->p;
  int64 i, tiles = 0, segs = 0;
  const char *why = "malformed batch";
  if (b->npiles < 0 || b->nrec < 0 || b->npiles > 0x7fffffff || b->nrec > 0x7fffffff || b->nreads <= 0)
    goto bad;
  if (t->tspace <= 0 || t->tspace > 65535 || (t->tbytes != 1 && t->tbytes != 2) || t->trace_bytes < 0)
    { why = "trace spacing or width out of range";
      goto bad;
    }
  if (b->npiles == 0 ? b->nrec != 0 : (b->pile_off[0] != 0 || b->pile_off[b->npiles] != b->nrec))
    goto bad;
  for (i = 0; i < b->npiles; i++)
    { if (b->pile_off[i] > b->pile_off[i + 1] || b->pile_aread[i] < 0 || b->pile_aread[i] >= b->nreads ||
          b->read_len[b->pile_aread[i]] < 0)
        goto bad;
      tiles += (b->read_len[b->pile_aread[i]] + t->tspace - 1) / t->tspace;
    }
  for (i = 0; i < b->nrec; i++)
    { if (t->tlen[i] < 0 || t->trace_off[i] < 0 || t->trace_off[i] + (int64) t->tbytes * t->tlen[i] > t->trace_bytes)
        { why = "a record's trace lies outside the batch's trace bytes";
          goto bad;
        }
      if (b->abpos[i] < 0)
        { why = "a record begins before its read";
          goto bad;
        }
      segs += t->tlen[i] / 2;
    }
  if (tiles > 0x7fffffff || segs > 0x7fffffff)
    { fprintf(stderr, "damar: quality: %lld segments and %lld tiles in one batch, 2^31 - 1 is the most of either\n",
              (long long) segs, (long long) tiles);
      return 0;
    }
  *ntiles_out = tiles;
  return 1;
bad:
  fprintf(stderr, "damar: quality: %s\n", why);
  return 0;
}

/* handler_annotate (LAq.c:312-409).  The reference's histogram is flat, q_histo[2 * tw * tile + 2 * q + comp], so a segment
   of q >= tw differences counts in tile + q / tw at q % tw; what would land beyond the read's tiles is dropped (the reference
   writes it where it is never read).  A record of tlen < 4 makes the reference read past the trace: here the first
   segment's rule applies from tlen 2, the last one's from tlen 4. */
int damar_host_pile_quality(const damar_trace_batch *t, const damar_q_params *p, int *q_out)
{ const damar_pile_batch *b = &t->p;
  const int tw = t->tspace;
  const uint32 segmax = (uint32) p->segmax;
  uint32 *histo = NULL;
  int64   pi, i, hcap = 0, top = 0;
  for (pi = 0; pi < b->npiles; pi++)
    { const int a = b->pile_aread[pi], alen = b->read_len[a];
      const int64 ntiles = (alen + tw - 1) / tw;
      int64 tile;
      if (ntiles * tw > hcap)
        { hcap = ntiles * tw;
          histo = (uint32 *) damar_grow(histo, sizeof(uint32) * (size_t) hcap, "quality");
        }
      memset(histo, 0, sizeof(uint32) * (size_t) (ntiles * tw));
      for (i = b->pile_off[pi]; i < b->pile_off[pi + 1]; i++)
        { const int nseg = t->tlen[i] / 2;
          int s;
          if (b->bread[i] == a)
            continue;
          for (s = 0; s < nseg; s++)
            { int q;
              if (s == 0)
                { if (b->abpos[i] % tw != 0) continue; }
              else if (s == nseg - 1)
                { if (b->aepos[i] % tw != 0 && b->aepos[i] != alen) continue; }
              q = damar_trace_value(t, i, 2 * s);
              tile = (int64) b->abpos[i] / tw + s + q / tw;
              if (tile < ntiles)
                histo[tile * tw + q % tw] += 1;
            }
        }
      for (tile = 0; tile < ntiles; tile++)
        { const uint32 *h = histo + tile * tw;
          uint64 sum = 0;
          uint32 count = 0;
          int    q;
          for (q = 0; q < tw && count != segmax; q++)
            { const uint32 has = h[q] < segmax - count ? h[q] : segmax - count;
              count += has;
              sum += (uint64) has * (uint64) q;
            }
          if (count < (uint32) p->segmin)
            q = p->ccs ? 25 : 0;
          else
            { if (sum == 0)
                sum = count;
              q = (int) ((2 * sum + count) / (2 * (uint64) count));       /* (int) ((float) sum / count + 0.5) */
            }
          q_out[top++] = q;
        }
    }
  free(histo);
  return 0;
}

/* trim_q_offsets (LAq.c:96-202) as written: a value of 0 is bad unless ccs, the window's mean is sum / 5 in ints, the right
   walk takes dataq[oe] off its sum (the value after its window), and neither walk stops at its own read's values. */
int damar_trim_from_q(const int *dataq, int64 ndata, int64 ob, int64 oe, int rlen, int tw, int trim_q, int min_len, int ccs,
                      int *trim_b, int *trim_e)
{ const int64 base = ob;
  const int   ntiles = (rlen + tw - 1) / tw;
  const int   left = *trim_b ? *trim_b / tw : 0, right = *trim_e ? *trim_e / tw : ntiles;
  int64 w;
  int   sum, q, tb, te;
#define QAT(k) ((k) >= 0 && (k) < ndata ? dataq[k] : 0)
  if (ob >= oe)
    { *trim_b = *trim_e = 0;
      return 0;
    }
  ob += left;
  oe -= ntiles - right;
  sum = 0;
  for (w = ob; w - ob <= TRIM_WINDOW && ob < oe; w++)
    { q = QAT(w);
      if (q >= trim_q || (!ccs && q == 0))
        { ob = w + 1;
          sum = 0;
          continue;
        }
      if (w - ob == TRIM_WINDOW && sum / TRIM_WINDOW >= trim_q)
        { sum -= QAT(ob);
          ob++;
        }
      sum += q;
    }
  sum = 0;
  for (w = oe; oe - w <= TRIM_WINDOW && ob < oe; w--)
    { q = QAT(w - 1);
      if (q >= trim_q || (!ccs && q == 0))
        { oe = w - 1;
          sum = 0;
          continue;
        }
      if (oe - w == TRIM_WINDOW && sum / TRIM_WINDOW >= trim_q)
        { sum -= QAT(oe);
          oe--;
        }
      sum += q;
    }
#undef QAT
  tb = (ob - base) * tw < rlen ? (int) ((ob - base) * tw) : rlen;
  te = (oe - base) * tw < rlen ? (int) ((oe - base) * tw) : rlen;
  if (te - tb < min_len)
    tb = te = 0;
  *trim_b = tb;
  *trim_e = te;
  return 1;
}

void damar_q_result_free(damar_q_result *res)
{ free(res->q_anno);  free(res->q_data);  free(res->trim_anno);  free(res->trim_data);
  memset(res, 0, sizeof(*res));
}

int damar_q_track(const damar_dbinfo *db, const char *las, const damar_q_params *p, int trim_q, int min_len, damar_q_result *res)
{ damar_pile_reader *r;
  damar_trace_batch  t;
  int64 qcap = 0, i;
  int   got, rc = 1, a;

  memset(res, 0, sizeof(*res));
  if ((r = damar_piles_open_traces(las, 0, 0)) == NULL)
    return 1;
  res->q_anno = (uint64 *) calloc((size_t) db->nreads + 2, sizeof(uint64));
  res->trim_anno = (uint64 *) calloc((size_t) db->nreads + 2, sizeof(uint64));
  res->q_data = (int *) damar_grow(NULL, 8, "quality");
  res->trim_data = (int *) damar_grow(NULL, sizeof(int) * 2 * ((size_t) db->nreads + 1), "quality");
  while ((got = damar_piles_next_traces(r, &t)) > 0)
    { int64 ntiles = 0;
      if (damar_batch_bind(&t.p, db, las, DAMAR_BIND_A) || damar_pile_quality(&t, p, NULL, &ntiles))
        goto done;
      if (res->nq + ntiles > qcap)
        { qcap = res->nq + ntiles + qcap / 4 + 1024;
          res->q_data = (int *) damar_grow(res->q_data, sizeof(int) * (size_t) qcap, "quality");
        }
      if (damar_pile_quality(&t, p, res->q_data + res->nq, &ntiles))
        goto done;
      res->nq += ntiles;
      for (i = 0; i < t.p.npiles; i++)                         /* LAq.c:405 */
        res->q_anno[t.p.pile_aread[i]] += sizeof(int) * (uint64) ((db->read_len[t.p.pile_aread[i]] + t.tspace - 1) / t.tspace);
    }
  if (got < 0)
    goto done;
  damar_counts_to_offsets(res->q_anno, db->nreads);                  /* post_annotate, calculate_trim */
  for (a = 0; a < db->nreads; a++)
    { int tb = 0, te = 0;
      if (damar_trim_from_q(res->q_data, res->nq, (int64) (res->q_anno[a] / sizeof(int)), (int64) (res->q_anno[a + 1] / sizeof(int)),
                            db->read_len[a], damar_piles_tspace(r), trim_q, min_len, p->ccs, &tb, &te))
        { res->trim_data[res->ntrim++] = tb;
          res->trim_data[res->ntrim++] = te;
          res->trim_anno[a] += 2 * sizeof(int);
        }
    }
  damar_counts_to_offsets(res->trim_anno, db->nreads);
  rc = 0;
done:
  if (rc)
    damar_q_result_free(res);
  damar_piles_close(r);
  return rc;
}

/* handler_update_anno (LAq.c:464-544) */
int damar_trim_update(const damar_dbinfo *db, const char *las, const uint64 *q_anno, const int *q_data, int64 nq,
                      const uint64 *trim_anno, const int *trim_data, int trim_q, int min_len, int ccs, damar_q_result *res)
{ damar_pile_reader *r;
  damar_pile_batch   b;
  int64 cap = 0, pi, i;
  int   got, rc = 1, tw;

  memset(res, 0, sizeof(*res));
  if ((r = damar_piles_open(las, 0)) == NULL)
    return 1;
  tw = damar_piles_tspace(r);
  res->trim_anno = (uint64 *) calloc((size_t) db->nreads + 2, sizeof(uint64));
  res->trim_data = (int *) damar_grow(NULL, 8, "quality");
  while ((got = damar_piles_next(r, &b)) > 0)
    { if (damar_batch_bind(&b, db, las, DAMAR_BIND_A))
        goto done;
      if (res->ntrim + 2 * b.npiles > cap)
        { cap = res->ntrim + 2 * b.npiles + cap / 4 + 1024;
          res->trim_data = (int *) damar_grow(res->trim_data, sizeof(int) * (size_t) cap, "quality");
        }
      for (pi = 0; pi < b.npiles; pi++)
        { const int a = b.pile_aread[pi];
          const uint64 at = trim_anno[a] / sizeof(int);
          int ab_min = INT_MAX, ae_max = 0, tb, te;
          if (at + 2 != trim_anno[a + 1] / sizeof(int))        /* the reference asserts it */
            { fprintf(stderr, "damar: read %d has overlaps in %s and no entry in the trim track\n", a, las);
              goto done;
            }
          for (i = b.pile_off[pi]; i < b.pile_off[pi + 1]; i++)
            { if ((b.flags[i] & OVL_DISCARD) || b.bread[i] == a)
                continue;
              if (b.abpos[i] < ab_min) ab_min = b.abpos[i];
              if (b.aepos[i] > ae_max) ae_max = b.aepos[i];
            }
          tb = trim_data[at];
          te = trim_data[at + 1];
          if (tb < ab_min || te > ae_max)                      /* tighten */
            { if (ab_min == INT_MAX)
                tb = te = 0;
              else
                { tb = ab_min + tw - 1;
                  te = ae_max;
                  damar_trim_from_q(q_data, nq, (int64) (q_anno[a] / sizeof(int)), (int64) (q_anno[a + 1] / sizeof(int)),
                                    db->read_len[a], tw, trim_q, min_len, ccs, &tb, &te);
                }
            }
          res->trim_data[res->ntrim++] = tb;
          res->trim_data[res->ntrim++] = te;
          res->trim_anno[a] += 2 * sizeof(int);
        }
    }
  if (got < 0)
    goto done;
  damar_counts_to_offsets(res->trim_anno, db->nreads);
  rc = 0;
done:
  if (rc)
    damar_q_result_free(res);
  damar_piles_close(r);
  return rc;
}

/***** reading a track back (lib/tracks.c:20-132, lib/compression.c:79-125) *********************/

/* runs of {u64 n, n bytes of one zlib stream} into out[want] */
static int read_chunks(const unsigned char *in, uint64 clen, unsigned char *out, uint64 want)
{ uint64 at = 0, top = 0;
  while (at + 8 <= clen)
    { uint64 n;
      uLongf got = (uLongf) (want - top);
      memcpy(&n, in + at, 8);
      at += 8;
      if (n > clen - at || uncompress(out + top, &got, in + at, (uLong) n) != Z_OK)
        return -1;
      top += got;
      at += n;
    }
  return top == want ? 0 : -1;
}

static unsigned char *slurp(const char *path, uint64 skip, uint64 len)
{ FILE *f = fopen(path, "r");
  unsigned char *buf;
  if (f == NULL)
    return NULL;
  buf = (unsigned char *) damar_grow(NULL, (size_t) len, "quality");
  if (fseeko(f, (off_t) skip, SEEK_SET) != 0 || (len > 0 && fread(buf, (size_t) len, 1, f) != 1))
    { free(buf);
      buf = NULL;
    }
  fclose(f);
  return buf;
}

int damar_track_read_a2(const char *dbpath, const char *track, int nreads, uint64 **anno_out, int **data_out, int64 *ndata)
{ struct { uint16 version, size; uint32 pad; uint64 len, clen, cdlen, r1, r2, r3, r4; } h;
  char   path[4500];
  FILE  *f;
  unsigned char *ca = NULL, *cd = NULL;
  uint64 *anno = NULL, total;
  int   *data = NULL, rc = 1, j;
  snprintf(path, sizeof(path), "%s.%s.a2", dbpath, track);
  if ((f = fopen(path, "r")) == NULL)
    return 1;
  if (fread(&h, sizeof(h), 1, f) != 1 || h.size != 8 || h.len != (uint64) nreads)
    { fclose(f);
      return 1;
    }
  fclose(f);
  anno = (uint64 *) damar_grow(NULL, 8 * ((size_t) nreads + 1), "quality");
  if ((ca = slurp(path, sizeof(h), h.clen)) == NULL || read_chunks(ca, h.clen, (unsigned char *) anno, 8 * ((uint64) nreads + 1)))
    goto done;
  total = anno[nreads];
  for (j = 0; j < nreads; j++)
    if (anno[j] > anno[j + 1] || anno[j] % 4)
      goto done;
  if (total % 4)
    goto done;
  snprintf(path, sizeof(path), "%s.%s.d2", dbpath, track);
  data = (int *) damar_grow(NULL, (size_t) total, "quality");
  if ((cd = slurp(path, 0, h.cdlen)) == NULL || read_chunks(cd, h.cdlen, (unsigned char *) data, total))
    goto done;
  *anno_out = anno;
  *data_out = data;
  *ndata = (int64) (total / 4);
  anno = NULL;
  data = NULL;
  rc = 0;
done:
  free(ca);  free(cd);  free(anno);  free(data);
  return rc;
}

/* the uncompressed form (db/DB.c Load_Track): int len, int size, len + 1 offsets of `size` bytes; the data file */
static int read_anno_data(const damar_dbinfo *db, const char *track, uint64 **anno_out, int **data_out, int64 *ndata_out)
{ char    path[4500];
  FILE   *af, *df = NULL;
  uint64 *anno = NULL;
  int    *data = NULL;
  int64   ndata;
  int     len, size, j, rc = 1;
  snprintf(path, sizeof(path), "%s.%s.anno", db->path, track);
  if ((af = fopen(path, "r")) == NULL)
    return 1;
  snprintf(path, sizeof(path), "%s.%s.data", db->path, track);
  if (fread(&len, sizeof(int), 1, af) != 1 || fread(&size, sizeof(int), 1, af) != 1 || (size != 4 && size != 8) ||
      len != db->nreads || (df = fopen(path, "r")) == NULL)
    goto done;
  anno = (uint64 *) damar_grow(NULL, sizeof(uint64) * ((size_t) db->nreads + 1), "track");
  for (j = 0; j <= db->nreads; j++)
    { int64 v8 = 0;
      int   v4 = 0;
      if (fread(size == 4 ? (void *) &v4 : (void *) &v8, (size_t) size, 1, af) != 1)
        goto done;
      anno[j] = (uint64) (size == 4 ? v4 : v8);
    }
  ndata = (int64) (anno[db->nreads] / sizeof(int));
  data = (int *) damar_grow(NULL, sizeof(int) * (size_t) ndata, "track");
  if (ndata > 0 && fread(data, sizeof(int), (size_t) ndata, df) != (size_t) ndata)
    goto done;
  *anno_out = anno;  *data_out = data;  *ndata_out = ndata;
  anno = NULL;
  data = NULL;
  rc = 0;
done:
  fclose(af);
  if (df) fclose(df);
  free(anno);  free(data);
  return rc;
}

int damar_track_read_any(const damar_dbinfo *db, const char *track, uint64 **anno, int **data, int64 *ndata)
{ return damar_track_read_a2(db->path, track, db->nreads, anno, data, ndata) && read_anno_data(db, track, anno, data, ndata);
}
