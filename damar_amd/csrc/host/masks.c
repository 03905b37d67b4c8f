/* masks.c -- LArepeat and TANmask as calls: a .las file goes through the pile reader (piles.c) batch by batch, every batch
 * through the C-ABI (damar_pile_coverage / damar_pile_repeats / damar_pile_tandem, the GPU unless DAMAR_PILES=host), and the
 * per-pile counts become the offsets of a track.  The commands (larepeat_main.c, tanmask_main.c) and the Python interface
 * are argument handling around these two calls. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "damar_hip.h"
#include "damar_host.h"

void damar_repeat_result_free(damar_repeat_result *res)
{ free(res->histo);  free(res->anno);  free(res->data);
  memset(res, 0, sizeof(*res));
}

int damar_repeat_track(const damar_dbinfo *db, const char *las, const damar_repeat_params *p0, int max_areads, int cov_only,
                       damar_repeat_result *res)
{ damar_repeat_params p = *p0;
  damar_pile_reader *r;
  damar_pile_batch   b;
  int    got = 0, rc = 1;
  int   *count = NULL;
  int64  ccap = 0, dcap = 0, i;

  memset(res, 0, sizeof(*res));
  if ((r = damar_piles_open(las, 0)) == NULL)
    return 1;
  if (max_areads < 0)
    max_areads = db->nreads;
  if (p.cov <= 0 || cov_only)
    { /* LArepeat.c:168-233: the pass ends after max_areads + 1 piles */
      int64 left = (int64) max_areads + 1, sum_len = 0, piles = 0;
      int   j, best = 0;
      res->histo = (int64 *) calloc((size_t) p.max_cov, sizeof(int64));
      while (left > 0 && (got = damar_piles_next(r, &b)) > 0)
        { if (damar_batch_bind(&b, db, las, DAMAR_BIND_AB))
            goto done;
          if (b.npiles > left)
            { b.npiles = left;
              b.nrec = b.pile_off[left];
            }
          if (damar_pile_coverage(&b, &p, res->histo, &res->cov_bases, &res->cov_inactive))
            goto done;
          for (i = 0; i < b.npiles; i++)
            sum_len += db->read_len[b.pile_aread[i]];
          piles += b.npiles;
          left -= b.npiles;
        }
      if (got < 0)
        goto done;
      for (j = 1; j < p.max_cov; j++)                        /* :142-149: the first strict maximum */
        if (res->histo[j] > res->histo[best])
          best = j;
      res->cov_max = best;
      res->avg_rlen = piles > 0 ? (int) (sum_len / piles) : 0;
      p.cov = best;
      damar_piles_rewind(r);
    }
  res->cov = p.cov;
  if (p.cov <= 0)
    { rc = 2;                                                /* the caller prints the reference's two lines */
      goto done;
    }
  if (!cov_only)
    { res->anno = (uint64 *) calloc((size_t) db->nreads + 2, sizeof(uint64));
      while ((got = damar_piles_next(r, &b)) > 0)
        { damar_pile_track t;
          if (damar_batch_bind(&b, db, las, DAMAR_BIND_AB))
            goto done;
          count = (int *) damar_reserve(count, &ccap, b.npiles, sizeof(int), 64, "masks");
          memset(&t, 0, sizeof(t));
          t.count = count;
          if (damar_pile_repeats(&b, &p, &t))
            goto done;
          if (res->ndata + t.ndata > dcap)
            { dcap = res->ndata + t.ndata + dcap / 4 + 1024;
              res->data = (int *) damar_grow(res->data, sizeof(int) * (size_t) dcap, "masks");
            }
          if (t.ndata > 0)
            memcpy(res->data + res->ndata, t.data, sizeof(int) * (size_t) t.ndata);
          free(t.data);
          res->ndata += t.ndata;
          res->merged += t.merged;
          res->bases_repeat += t.repeat_bases;
          for (i = 0; i < b.npiles; i++)
            { res->anno[b.pile_aread[i]] += sizeof(int) * (uint64) count[i];
              res->bases_total += db->read_len[b.pile_aread[i]];
            }
        }
      if (got < 0)
        goto done;
      damar_counts_to_offsets(res->anno, db->nreads);       /* :256-263 */
      if (res->data == NULL)
        res->data = (int *) damar_grow(NULL, 8, "masks");
    }
  rc = 0;
done:
  free(count);
  damar_piles_close(r);
  return rc;
}

int damar_tan_track(const damar_dbinfo *db, const char *las, int first, int last, int min_len, int64 **offs_out, int **data_out,
                    int64 *nmasks, int64 *masked)
{ damar_pile_reader *r;
  damar_pile_batch   b;
  int    got, rc = 1, next = first;
  int   *count = NULL, *data = NULL;
  int64  ccap = 0, dcap = 0, ndata = 0, i, j;
  int64 *offs = (int64 *) calloc((size_t) (last - first) + 2, sizeof(int64));

  *nmasks = *masked = 0;
  if ((r = damar_piles_open(las, 0)) == NULL)
    { free(offs);
      return 1;
    }
  while ((got = damar_piles_next(r, &b)) > 0)
    { damar_pile_track t;
      damar_batch_bind(&b, db, las, DAMAR_BIND_ONLY);
      for (i = 0; i < b.npiles; i++)                          /* TANmask.c:259-263, 318-322: ascending, inside the block */
        { if (b.pile_aread[i] < next || b.pile_aread[i] >= last)
            { rc = 2;
              goto done;
            }
          next = b.pile_aread[i] + 1;
        }
      count = (int *) damar_reserve(count, &ccap, b.npiles, sizeof(int), 64, "masks");
      memset(&t, 0, sizeof(t));
      t.count = count;
      if (damar_pile_tandem(&b, min_len, &t))
        goto done;
      if (ndata + t.ndata > dcap)
        { dcap = ndata + t.ndata + dcap / 4 + 1024;
          data = (int *) damar_grow(data, sizeof(int) * (size_t) dcap, "masks");
        }
      if (t.ndata > 0)
        memcpy(data + ndata, t.data, sizeof(int) * (size_t) t.ndata);
      for (j = 0; j + 1 < t.ndata; j += 2)
        { *masked += t.data[j + 1] - t.data[j];
          *nmasks += 1;
        }
      free(t.data);
      ndata += t.ndata;
      for (i = 0; i < b.npiles; i++)
        offs[b.pile_aread[i] - first + 1] = (int64) sizeof(int) * count[i];
    }
  if (got < 0)
    goto done;
  for (i = 1; i <= last - first; i++)
    offs[i] += offs[i - 1];
  if (data == NULL)
    data = (int *) damar_grow(NULL, 8, "masks");
  *offs_out = offs;
  *data_out = data;
  offs = NULL;
  data = NULL;
  rc = 0;
done:
  free(count);  free(offs);  free(data);
  damar_piles_close(r);
  return rc;
}
