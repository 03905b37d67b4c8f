/* homogenize.c -- TKhomogenize (scrub/TKhomogenize.c) as calls: the repeat intervals of every A read carried through its
 * overlaps' trace points onto the B reads, the union per read written as a track.
 *   - damar_host_homog_*: the plain routine, one bit array per read like the reference's (DAMAR_PILES=host; the second
 *     opinion for kernels/homogenize.hip), behind the session calls of include/damar_hip.h,
 *   - damar_homog_inputs_valid: what both paths index with,
 *   - damar_homogenize_track: the pass over a file, batch by batch through the session (the GPU unless DAMAR_PILES=host).
 * Nothing here touches the GPU runtime. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "damar_hip.h"
#include "damar_host.h"

#define MIN_INT_LEN 500                   /* TKhomogenize.c:49 */
/* ba_assign_range(arr, beg, end, 1) (lib.ext/bitarr.c:263-284): bits beg .. end inclusive, the single bit beg when
   end < beg; bit j is bit j % 8 of byte j / 8.  Held to the nbits bits of the array. */
void damar_bits_set_range(unsigned char *bits, int64 nbits, int64 beg, int64 end)
{ int64 b0, b1;
  if (end < beg) end = beg;
  if (beg < 0 || beg >= nbits) return;
  if (end >= nbits) end = nbits - 1;
  b0 = beg >> 3;
  b1 = end >> 3;
  if (b0 == b1)
    { bits[b0] |= (unsigned char) ((0xff << (beg & 7)) & (0xff >> (7 - (end & 7))));
      return;
    }
  bits[b0] |= (unsigned char) (0xff << (beg & 7));
  bits[b1] |= (unsigned char) (0xff >> (7 - (end & 7)));
  if (b1 - b0 > 1)
    memset(bits + b0 + 1, 0xff, (size_t) (b1 - b0 - 1));
}

/* get_trim (lib/utils.c:258-284) for every read: no entry, or an empty or inverted one, is (0, 0).  1: a read with
   something else than one pair (the reference asserts it). */
int damar_trim_pairs(const uint64 *anno, const int *data, int nreads, int *pairs)
{ int r;
  for (r = 0; r < nreads; r++)
    { const uint64 ob = anno[r] / sizeof(int), oe = anno[r + 1] / sizeof(int);
      int b = 0, e = 0;
      if (oe != ob && oe - ob != 2)
        return 1;
      if (oe != ob && data[ob] < data[ob + 1])
        { b = data[ob];
          e = data[ob + 1];
        }
      pairs[2 * r] = b;
      pairs[2 * r + 1] = e;
    }
  return 0;
}

static int track_valid(const uint64 *anno, int64 ndata, int nreads, const char *what)
{ int r;
  if (anno == NULL || ndata < 0 || anno[0] % 8 || anno[nreads] > 4 * (uint64) ndata)
    goto bad;
  for (r = 0; r < nreads; r++)
    if (anno[r] > anno[r + 1] || anno[r + 1] % 8)                /* {begin, end} pairs of ints */
      goto bad;
  return 1;
bad:
  fprintf(stderr, "damar: homogenize: the %s track is not pairs of ints for %d reads\n", what, nreads);
  return 0;
}

/* the seeded track's long intervals lie inside their reads (the reference would write outside its bit arrays) */
int damar_homog_seed_valid(const int *read_len, int nreads, const uint64 *anno, const int *data, int64 ndata)
{ int r;
  if (!track_valid(anno, ndata, nreads, "interval") || (ndata > 0 && data == NULL))
    return 0;
  for (r = 0; r < nreads; r++)
    { uint64 k;
      for (k = anno[r] / 4; k < anno[r + 1] / 4; k += 2)
        if ((int64) data[k + 1] - data[k] >= MIN_INT_LEN && (data[k] < 0 || data[k + 1] > read_len[r]))
          { fprintf(stderr, "damar: homogenize: interval %d..%d lies outside read %d of %d bases\n", data[k], data[k + 1], r, read_len[r]);
            return 0;
          }
    }
  return 1;
}

int damar_homog_inputs_valid(const damar_trace_batch *t, int nreads, const int *read_len, const uint64 *anno, const int *data,
                             int64 ndata, int ends, const int *trim)
{ const damar_pile_batch *b = &t->p;
  const char *why = "malformed batch";
  int64 i;
  if (b->npiles < 0 || b->nrec < 0 || b->npiles > 0x7fffffff || b->nrec > 0x7fffffff || b->nreads != nreads)
    goto bad;
  if (t->tspace <= 0 || t->tspace > 65535 || (t->tbytes != 1 && t->tbytes != 2) || t->trace_bytes < 0)
    { why = "trace spacing or width out of range";
      goto bad;
    }
  if (b->npiles == 0 ? b->nrec != 0 : (b->pile_off[0] != 0 || b->pile_off[b->npiles] != b->nrec))
    goto bad;
  if (ends == 0 || ends < -1 || (ends != -1 && trim == NULL))
    { why = "ends is -1 or positive, and needs the trim pairs";
      goto bad;
    }
  if (!track_valid(anno, ndata, nreads, "interval") || (ndata > 0 && data == NULL))
    return 0;
  for (i = 0; i < b->npiles; i++)
    if (b->pile_off[i] > b->pile_off[i + 1] || b->pile_aread[i] < 0 || b->pile_aread[i] >= nreads)
      goto bad;
  for (i = 0; i < b->nrec; i++)
    { if (t->tlen[i] < 0 || t->trace_off[i] < 0 || t->trace_off[i] + (int64) t->tbytes * t->tlen[i] > t->trace_bytes)
        { why = "a record's trace lies outside the batch's trace bytes";
          goto bad;
        }
      if (b->bread[i] < 0 || b->bread[i] >= nreads)
        { why = "a record's B read is not in the database";
          goto bad;
        }
      if (b->abpos[i] < 0 || b->aepos[i] < b->abpos[i] || b->bbpos[i] < 0 || b->bepos[i] < b->bbpos[i] ||
          b->bepos[i] > read_len[b->bread[i]])
        { why = "a record's coordinates lie outside its reads";
          goto bad;
        }
    }
  return 1;
bad:
  fprintf(stderr, "damar: homogenize: %s\n", why);
  return 0;
}

/***** the plain routine ************************************************************************/

struct damar_host_homog
{ int    nreads, res;
  int   *rlen;                 /* [nreads] */
  int64 *boff;                 /* [nreads + 1] byte offsets: a read's bits begin on a byte, as in the reference */
  unsigned char *bits;
  int64  cnt[3];               /* records seen by add, ranges set, intervals read out */
};

static int bits_of(int rlen, int res)       /* the bits read back; one spare bit follows */
{ return res > 1 ? (rlen + res - 1) / res : rlen; }

damar_host_homog *damar_host_homog_open(const int *read_len, int nreads, int res)
{ damar_host_homog *h = (damar_host_homog *) calloc(1, sizeof(*h));
  int r;
  if (h == NULL)
    return NULL;
  h->nreads = nreads;
  h->res = res;
  h->rlen = (int *) damar_grow(NULL, sizeof(int) * (size_t) nreads, "homogenize");
  h->boff = (int64 *) damar_grow(NULL, sizeof(int64) * ((size_t) nreads + 1), "homogenize");
  h->boff[0] = 0;
  for (r = 0; r < nreads; r++)
    { h->rlen[r] = read_len[r];
      h->boff[r + 1] = h->boff[r] + (bits_of(read_len[r], res) + 1 + 7) / 8;
    }
  h->bits = (unsigned char *) calloc((size_t) h->boff[nreads] + 1, 1);
  if (h->bits == NULL)
    { fprintf(stderr, "damar: homogenize: no memory for a mask of %lld bytes\n", (long long) h->boff[nreads]);
      damar_host_homog_close(h);
      return NULL;
    }
  return h;
}

void damar_host_homog_close(damar_host_homog *h)
{ if (h == NULL)
    return;
  free(h->rlen);  free(h->boff);  free(h->bits);
  free(h);
}

void damar_host_homog_counts(const damar_host_homog *h, int64 *cnt)
{ cnt[0] = h->cnt[0];  cnt[1] = h->cnt[1];  cnt[2] = h->cnt[2]; }

static void set_range(damar_host_homog *h, int r, int beg, int end)
{ damar_bits_set_range(h->bits + h->boff[r], (int64) bits_of(h->rlen[r], h->res) + 1, beg, end);
  h->cnt[1] += 1;
}

/* TKhomogenize.c:193-226 */
int damar_host_homog_seed(damar_host_homog *h, const uint64 *anno, const int *data)
{ const int res = h->res;
  int r;
  for (r = 0; r < h->nreads; r++)
    { uint64 k;
      for (k = anno[r] / 4; k < anno[r + 1] / 4; k += 2)
        { const int beg = data[k], end = data[k + 1];
          if ((int64) end - beg < MIN_INT_LEN)
            continue;
          set_range(h, r, (beg + res - 1) / res, end / res);
        }
    }
  return 0;
}

static int trace_b(const damar_trace_batch *t, int64 rec, int seg)
{ return damar_trace_value(t, rec, 2 * seg + 1);
}

/* handler_homogenize (TKhomogenize.c:346-546), the walk as written */
int damar_host_homog_add(damar_host_homog *h, const damar_trace_batch *t, const uint64 *anno, const int *data, int ends, const int *trim)
{ const damar_pile_batch *b = &t->p;
  const int tw = t->tspace, res = h->res;
  int64 pi, i;
  for (pi = 0; pi < b->npiles; pi++)
    { const int a = b->pile_aread[pi];
      for (i = b->pile_off[pi]; i < b->pile_off[pi + 1]; i++)
        { const int br = b->bread[i], blen = h->rlen[br];
          const int ab = b->abpos[i], ae = b->aepos[i], bepos = b->bepos[i], nseg = t->tlen[i] / 2;
          const int trim_b = trim != NULL ? trim[2 * br] : 0, trim_e = trim != NULL ? trim[2 * br + 1] : blen;
          uint64 ob = anno[a] / 4;
          const uint64 oe = anno[a + 1] / 4;
          h->cnt[0] += 1;
          if (a == br)
            continue;
          while (ob < oe)
            { const int beg = data[ob], end = data[ob + 1];
              int iab, iae, ibb = -1, ibe = -1, aoff = ab, boff = b->bbpos[i], j;
              ob += 2;
              if ((int64) end - beg < MIN_INT_LEN)
                continue;
              if (beg > ae)
                break;
              iab = beg > ab ? beg : ab;
              iae = end < ae ? end : ae;
              if (iab >= iae)
                continue;
              for (j = 0; j < nseg; j++)
                { const int bl = trace_b(t, i, j);
                  if (ibb == -1)
                    { if (aoff + tw >= iab)
                        { const int   adiff = iab - aoff;
                          const float ratio = 1.0 * tw / bl;
                          const int   v = boff + (int) (adiff / ratio);
                          ibb = v < bepos ? v : bepos;
                        }
                      else if (j == nseg - 1)
                        ibb = boff < bepos ? boff : bepos;
                    }
                  if (aoff + tw >= iae && ibe == -1)
                    { const int   adiff = iae - aoff;
                      const float ratio = 1.0 * tw / bl;
                      const int   v = boff + (int) (adiff / ratio);
                      if (ibb == -1)
                        ibb = boff < bepos ? boff : bepos;
                      ibe = v < bepos ? v : bepos;
                      break;
                    }
                  aoff = ((aoff + tw) / tw) * tw;
                  boff += bl;
                }
              if (ibb == -1 || ibe == -1)
                continue;
              if (b->flags[i] & OVL_COMP)
                { const int x = ibb;
                  ibb = blen - ibe;
                  ibe = blen - x;
                }
              if (ends != -1)
                { if (ibb < ends + trim_b)
                    { const int cut = ends + trim_b < ibe ? ends + trim_b : ibe;
                      set_range(h, br, (ibb + res - 1) / res, cut / res);
                    }
                  if (ibe > trim_e - ends)
                    { const int from = trim_e - ends > ibb ? trim_e - ends : ibb;
                      set_range(h, br, (from + res - 1) / res, ibe / res);
                    }
                }
              else
                set_range(h, br, (ibb + res - 1) / res, ibe / res);
            }
        }
    }
  return 0;
}

/* post_homogenize (TKhomogenize.c:230-321): anno receives byte offsets */
int damar_host_homog_finish(damar_host_homog *h, uint64 *anno, int **data_out, int64 *ndata, int64 *tagged)
{ const int res = h->res;
  int  *data = (int *) damar_grow(NULL, 8, "homogenize");
  int64 cap = 0, top = 0, k;
  uint64 off = 0;
  int   r;
  for (r = 0; r < h->nreads; r++)
    { const unsigned char *bits = h->bits + h->boff[r];
      const int rlen = h->rlen[r], alen = bits_of(rlen, res);
      int j, beg = -1;
      anno[r] = 0;
      for (j = 0; j <= alen; j++)
        { const int val = j < alen && (bits[j >> 3] >> (j & 7) & 1);
          if (val && beg == -1)
            beg = j;
          else if (!val && beg != -1)
            { if (top + 2 > cap)
                { cap = cap + cap / 4 + 1024;
                  data = (int *) damar_grow(data, sizeof(int) * (size_t) cap, "homogenize");
                }
              data[top++] = beg * res;
              if (j == alen)                                     /* the run reaches the last bit */
                data[top++] = rlen - 1;
              else
                data[top++] = (int64) (j - 1) * res < rlen ? (j - 1) * res : rlen;
              anno[r] += 2 * sizeof(int);
              beg = -1;
            }
        }
    }
  anno[h->nreads] = 0;
  for (r = 0; r <= h->nreads; r++)
    { const uint64 c = anno[r];
      anno[r] = off;
      off += c;
    }
  *tagged = 0;
  for (k = 0; k < top; k += 2)
    *tagged += data[k + 1] - data[k];
  h->cnt[2] = top / 2;
  *data_out = data;
  *ndata = top;
  return 0;
}

/***** the pass over a file *********************************************************************/

void damar_homog_result_free(damar_homog_result *res)
{ free(res->anno);  free(res->data);
  memset(res, 0, sizeof(*res));
}

int damar_homogenize_track(const damar_dbinfo *db, const char *las, const damar_homog_params *p, damar_homog_result *res)
{ damar_pile_reader *r = NULL;
  damar_homog       *h = NULL;
  damar_trace_batch  t;
  int   *pairs = NULL;
  int    got, rc = 1;

  memset(res, 0, sizeof(*res));
  if (p->res < 1 || p->ends == 0 || p->ends < -1 || p->iv_anno == NULL)
    { fprintf(stderr, "damar: homogenize: res %d, ends %d\n", p->res, p->ends);
      return 1;
    }
  if (p->ends != -1)
    { pairs = (int *) damar_grow(NULL, sizeof(int) * 2 * ((size_t) db->nreads + 1), "homogenize");
      if (p->trim_anno == NULL || damar_trim_pairs(p->trim_anno, p->trim_data, db->nreads, pairs))
        { fprintf(stderr, "damar: homogenize: the trim track does not hold one interval per read at most\n");
          goto done;
        }
    }
  if ((r = damar_piles_open_traces(las, 0, 0)) == NULL)
    goto done;
  if ((h = damar_homog_open(db->read_len, db->nreads, p->res)) == NULL)
    goto done;
  if (p->merge && damar_homog_seed(h, p->iv_anno, p->iv_data, p->iv_ndata))
    goto done;
  while ((got = damar_piles_next_traces(r, &t)) > 0)
    { if (damar_batch_bind(&t.p, db, las, DAMAR_BIND_A))
        goto done;
      if (damar_homog_add(h, &t, p->iv_anno, p->iv_data, p->iv_ndata, p->ends, pairs))
        goto done;
    }
  if (got < 0)
    goto done;
  res->anno = (uint64 *) damar_grow(NULL, sizeof(uint64) * ((size_t) db->nreads + 2), "homogenize");
  if (damar_homog_finish(h, res->anno, &res->data, &res->ndata, &res->tagged))
    goto done;
  rc = 0;
done:
  if (rc)
    damar_homog_result_free(res);
  damar_homog_close(h);
  if (r != NULL)
    damar_piles_close(r);
  free(pairs);
  return rc;
}
