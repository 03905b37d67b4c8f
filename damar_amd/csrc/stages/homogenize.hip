/* stages/homogenize.hip -- the C-ABI of the homogenized repeat mask: damar_homog_open .. damar_homog_close */
#include <vector>

#include "stage.h"

/***** TKhomogenize's mask of the whole database, kept in HBM across batches of piles (kernels/homogenize.hip) ****************/

struct damar_homog
{ int   nreads, res;
  damar_host_homog *hs;          /* DAMAR_PILES=host: the plain routine's state, nothing below is used */
  std::vector<int> rlen;
  u32  *d_words;                 /* the mask, nwords of them */
  u64  *d_woff, *d_cnt;          /* [nreads + 1] word offsets; [0] ranges set */
  int  *d_rlen;
  u64   nwords;
  struct : PileStage             /* the handle's buffers; the events and the figures are HM's */
  { DBuf ianno{*this}, idata{*this}, trim{*this}, count{*this}, doff{*this}, scan{*this}, out{*this};
  } S;
};
static DevStage HM;              /* the figures outlive the handle.  ms of the last session so far: upload, mark, read-out, download;
                                    cnt: records seen by add, ranges set, intervals read out */

extern "C" void damar_homog_last(double *ms, int64 *cnt) { HM.last(ms, cnt, 3); }

extern "C" void damar_homog_close(damar_homog *h)
{ if (h == NULL)
    return;
  if (h->hs != NULL)
    damar_host_homog_close(h->hs);
  else
    { h->S.release();
      HM.release();
      void *own[] = { h->d_words, h->d_woff, h->d_cnt, h->d_rlen };
      for (void *p : own)
        if (p != NULL) HIP_CHECK(hipFree(p));
    }
  delete h;
}

extern "C" damar_homog *damar_homog_open(const int *read_len, int nreads, int res)
{ if (read_len == NULL || nreads <= 0 || res < 1)
    { fprintf(stderr, "damar: homogenize: %d reads at resolution %d\n", nreads, res);
      return NULL;
    }
  for (int r = 0; r < nreads; r++)
    if (read_len[r] < 0)
      { fprintf(stderr, "damar: homogenize: read %d has length %d\n", r, read_len[r]);
        return NULL;
      }
  damar_homog *h = new damar_homog();
  h->nreads = nreads;  h->res = res;  h->hs = NULL;
  h->d_words = NULL;  h->d_woff = NULL;  h->d_cnt = NULL;  h->d_rlen = NULL;
  for (int i = 0; i < 4; i++) HM.ms[i] = 0;
  for (int i = 0; i < 3; i++) HM.cnt[i] = 0;
  h->rlen.assign(read_len, read_len + nreads);
  if (damar_piles_on_host())
    { if ((h->hs = damar_host_homog_open(read_len, nreads, res)) == NULL)
        { delete h;
          return NULL;
        }
      return h;
    }
  HM.device();
  std::vector<u64> woff((size_t) nreads + 1);
  woff[0] = 0;
  for (int r = 0; r < nreads; r++)
    { const u64 bits = (u64) (res > 1 ? (read_len[r] + res - 1) / res : read_len[r]) + 1;
      woff[(size_t) r + 1] = woff[r] + (bits + 31) / 32;
    }
  h->nwords = woff[nreads];
  const hipError_t e = hipMalloc((void **) &h->d_words, sizeof(u32) * (size_t) h->nwords + 64);
  if (e != hipSuccess)             /* no smaller mask would do, and there is no other path */
    { (void) hipGetLastError();
      fprintf(stderr, "damar: homogenize: no device memory for a mask of %llu bytes (%s)\n", (unsigned long long) (4 * h->nwords),
              hipGetErrorString(e));
      h->d_words = NULL;
      damar_homog_close(h);
      return NULL;
    }
  HIP_CHECK(hipMalloc((void **) &h->d_woff, sizeof(u64) * ((size_t) nreads + 1)));
  HIP_CHECK(hipMalloc((void **) &h->d_rlen, sizeof(int) * (size_t) nreads));
  HIP_CHECK(hipMalloc((void **) &h->d_cnt, 64));
  HM.mark(0);
  HIP_CHECK(hipMemsetAsync(h->d_words, 0, sizeof(u32) * (size_t) h->nwords + 64, G_st));
  HIP_CHECK(hipMemsetAsync(h->d_cnt, 0, 64, G_st));
  HIP_CHECK(hipMemcpyAsync(h->d_woff, woff.data(), sizeof(u64) * ((size_t) nreads + 1), hipMemcpyHostToDevice, G_st));
  HIP_CHECK(hipMemcpyAsync(h->d_rlen, read_len, sizeof(int) * (size_t) nreads, hipMemcpyHostToDevice, G_st));
  HM.mark(1);
  HIP_CHECK(hipStreamSynchronize(G_st));
  HM.laps_add(0, 1);
  return h;
}

/* the interval track goes up with every call: a few ints per read, next to a batch's trace bytes it does not count */
static void homog_track_up(damar_homog *h, HomArgs *a, const uint64 *anno, const int *data, int64 ndata)
{ const DevTrack iv = up_track(h->S.ianno, h->S.idata, anno, (size_t) h->nreads, data, ndata);
  memset(a, 0, sizeof(*a));
  a->nreads = (u32) h->nreads;  a->res = h->res;  a->ends = -1;
  a->iv_anno = iv.anno;  a->iv_data = iv.data;
  a->read_len = h->d_rlen;  a->woff = h->d_woff;  a->words = h->d_words;  a->nranges = h->d_cnt;
}

static void homog_marked(damar_homog *h)           /* after the kernel: its time and the running count of ranges */
{ u64 ranges = 0;
  HIP_CHECK(hipMemcpyAsync(&ranges, h->d_cnt, sizeof(u64), hipMemcpyDeviceToHost, G_st));
  HIP_CHECK(hipStreamSynchronize(G_st));
  HM.cnt[1] = (int64) ranges;
  HM.laps_add(0, 2);
}

extern "C" int damar_homog_seed(damar_homog *h, const uint64 *anno, const int *data, int64 ndata)
{ if (h == NULL)
    return 1;
  if (!damar_homog_seed_valid(h->rlen.data(), h->nreads, anno, data, ndata))
    return 1;
  if (h->hs != NULL)
    { if (damar_host_homog_seed(h->hs, anno, data))
        return 1;
      damar_host_homog_counts(h->hs, HM.cnt);
      return 0;
    }
  HomArgs a;
  HM.mark(0);
  homog_track_up(h, &a, anno, data, ndata);
  HM.mark(1);
  damar_launch_hom_seed(&a, G_st);
  HM.mark(2);
  homog_marked(h);
  return 0;
}

extern "C" int damar_homog_add(damar_homog *h, const damar_trace_batch *t, const uint64 *anno, const int *data, int64 ndata, int ends,
                               const int *trim)
{ if (h == NULL || t == NULL)
    return 1;
  if (!damar_homog_inputs_valid(t, h->nreads, h->rlen.data(), anno, data, ndata, ends, trim))
    return 1;
  if (h->hs != NULL)
    { if (damar_host_homog_add(h->hs, t, anno, data, ends, trim))
        return 1;
      damar_host_homog_counts(h->hs, HM.cnt);
      return 0;
    }
  const damar_pile_batch *b = &t->p;
  HM.cnt[0] += b->nrec;
  if (b->nrec == 0)
    return 0;
  HomArgs a;
  HM.mark(0);
  homog_track_up(h, &a, anno, data, ndata);
  a.npiles = (u32) b->npiles;  a.nrec = (u32) b->nrec;  a.tspace = t->tspace;  a.tbytes = t->tbytes;  a.ends = ends;
  const PileDev d = pile_up(h->S, b, t, { b->abpos, b->aepos, b->bbpos, b->bepos, b->bread, b->flags, t->tlen });
  if (ends != -1)
    a.trim = up(h->S.trim, trim, 2 * (size_t) h->nreads);
  HM.mark(1);
  a.pile_off = d.off;  a.pile_aread = d.aread;
  a.abpos = d.col[0];  a.aepos = d.col[1];  a.bbpos = d.col[2];  a.bepos = d.col[3];  a.bread = d.col[4];  a.flags = d.col[5];
  a.tlen = d.col[6];  a.trace_off = d.toff;  a.trace = d.trace;
  damar_launch_hom_mark(&a, G_st);
  HM.mark(2);
  homog_marked(h);
  return 0;
}

extern "C" int damar_homog_finish(damar_homog *h, uint64 *anno, int **data, int64 *ndata, int64 *tagged)
{ if (h == NULL || anno == NULL || data == NULL || ndata == NULL || tagged == NULL)
    return 1;
  if (h->hs != NULL)
    { if (damar_host_homog_finish(h->hs, anno, data, ndata, tagged))
        return 1;
      damar_host_homog_counts(h->hs, HM.cnt);
      return 0;
    }
  const size_t nr = (size_t) h->nreads;
  HomArgs a;
  memset(&a, 0, sizeof(a));
  a.nreads = (u32) h->nreads;  a.res = h->res;
  a.read_len = h->d_rlen;  a.woff = h->d_woff;  a.words = h->d_words;
  u32 *d_count = (u32 *) h->S.count.need(sizeof(u32) * nr), *d_doff = (u32 *) h->S.doff.need(sizeof(u32) * nr);
  void *d_scan = h->S.scan.need(damar_scan_workspace_bytes(nr));
  a.count = d_count;  a.off = d_doff;
  HM.mark(2);
  damar_launch_hom_count(&a, G_st);
  damar_exclusive_scan_u32(d_count, d_doff, nr, d_scan, h->d_cnt + 1, G_st);
  u64 total = 0;
  HIP_CHECK(hipMemcpyAsync(&total, h->d_cnt + 1, sizeof(u64), hipMemcpyDeviceToHost, G_st));
  HIP_CHECK(hipStreamSynchronize(G_st));
  if (total >= ((u64) 1 << 30))
    { fprintf(stderr, "damar: homogenize: %llu intervals, 2^30 - 1 is the most a track of ints holds here\n", (unsigned long long) total);
      return 1;
    }
  a.out = (int *) h->S.out.need(sizeof(int) * 2 * (size_t) total + 16);
  damar_launch_hom_emit(&a, G_st);
  HM.mark(3);
  std::vector<u32> cnt(nr);
  int *out = (int *) malloc(sizeof(int) * 2 * (size_t) total + 8);
  if (out == NULL)
    { fprintf(stderr, "damar: out of memory (homogenize)\n");
      return 1;
    }
  HIP_CHECK(hipMemcpyAsync(cnt.data(), d_count, sizeof(u32) * nr, hipMemcpyDeviceToHost, G_st));
  if (total > 0)
    HIP_CHECK(hipMemcpyAsync(out, a.out, sizeof(int) * 2 * (size_t) total, hipMemcpyDeviceToHost, G_st));
  HM.mark(4);
  HIP_CHECK(hipStreamSynchronize(G_st));
  uint64 off = 0;
  for (size_t r = 0; r < nr; r++)
    { anno[r] = off;
      off += 2 * sizeof(int) * (uint64) cnt[r];
    }
  anno[nr] = off;
  int64 sum = 0;
  for (u64 k = 0; k < total; k++)
    sum += out[2 * k + 1] - out[2 * k];
  *data = out;  *ndata = (int64) (2 * total);  *tagged = sum;
  HM.cnt[2] = (int64) total;
  HM.laps_add(2, 2);
  return 0;
}
