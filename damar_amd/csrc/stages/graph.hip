/* stages/graph.hip -- the C-ABI of OGbuild's edges: damar_graph_open .. damar_graph_close */
#include <vector>

#include "stage.h"
#include "damar_graph.h"

/***** the statuses, the symmetric-discard tables and the candidate edges of a file, kept in HBM across its batches of piles
       (kernels/graph_edges.hip) ***********************************************************************************************/

struct damar_graph
{ int   nreads;
  damar_host_graph *hs;          /* DAMAR_PILES=host: the plain routine's state, nothing below is used */
  u32  *d_status;
  int  *d_minfirst, *d_hasfirst, *d_rlen, *d_trim;
  u64  *d_ctr;
  int  *d_cand;   u64 cand_cap, ncand;
  u64  *d_probe;  u64 probe_cap, nprobe;
  u64   rec_end;                 /* behind the last record of any batch: what the file-order key of the first sort holds */
  struct : PileStage
  { DBuf diffs{*this}, k0{*this}, k1{*this}, v0{*this}, v1{*this}, sortw{*this}, scan{*this}, beg{*this}, keep{*this}, pos{*this},
         kcount{*this}, hostread{*this}, out{*this};
  } S;
};
static DevStage GR;              /* ms of the last session so far: upload, pile kernel, finishing kernels, download;
                                    cnt: records, candidate edges, reads the host routine finished, edges kept */

extern "C" void damar_graph_last(double *ms, int64 *cnt) { GR.last(ms, cnt, 4); }

extern "C" int damar_graph_maxdeg(void) { return test_limit("DAMAR_TEST_GRAPH_MAXDEG", DAMAR_GRAPH_MAXDEG, 1); }

extern "C" void damar_graph_close(damar_graph *g)
{ if (g == NULL)
    return;
  if (g->hs != NULL)
    damar_host_graph_close(g->hs);
  else
    { g->S.release();
      GR.release();
      void *own[] = { g->d_status, g->d_minfirst, g->d_hasfirst, g->d_rlen, g->d_trim, g->d_ctr, g->d_cand, g->d_probe };
      for (void *p : own)
        if (p != NULL) HIP_CHECK(hipFree(p));
    }
  delete g;
}

extern "C" damar_graph *damar_graph_open(const int *read_len, int nreads, const int *trim)
{ if (read_len == NULL || trim == NULL || nreads <= 0)
    { fprintf(stderr, "damar: graph: %d reads\n", nreads);
      return NULL;
    }
  damar_graph *g = new damar_graph();
  g->nreads = nreads;  g->hs = NULL;
  g->d_status = NULL;  g->d_minfirst = g->d_hasfirst = g->d_rlen = g->d_trim = NULL;  g->d_ctr = NULL;
  g->d_cand = NULL;  g->d_probe = NULL;  g->cand_cap = g->probe_cap = g->ncand = g->nprobe = 0;  g->rec_end = 0;
  for (int i = 0; i < 4; i++) { GR.ms[i] = 0;  GR.cnt[i] = 0; }
  if (damar_piles_on_host())
    { if ((g->hs = damar_host_graph_open(read_len, nreads, trim)) == NULL)
        { delete g;
          return NULL;
        }
      return g;
    }
  GR.device();
  const size_t nr = (size_t) nreads;
  HIP_CHECK(hipMalloc((void **) &g->d_status, sizeof(u32) * nr));
  HIP_CHECK(hipMalloc((void **) &g->d_minfirst, sizeof(int) * nr));
  HIP_CHECK(hipMalloc((void **) &g->d_hasfirst, sizeof(int) * nr));
  HIP_CHECK(hipMalloc((void **) &g->d_rlen, sizeof(int) * nr));
  HIP_CHECK(hipMalloc((void **) &g->d_trim, sizeof(int) * 2 * nr));
  HIP_CHECK(hipMalloc((void **) &g->d_ctr, sizeof(u64) * 16));
  u64 ctr[16];
  memset(ctr, 0, sizeof(ctr));
  ctr[GC_NEG] = ~0ull;
  GR.mark(0);
  HIP_CHECK(hipMemsetAsync(g->d_status, 0, sizeof(u32) * nr, G_st));
  HIP_CHECK(hipMemsetAsync(g->d_minfirst, 0x7f, sizeof(int) * nr, G_st));        /* 0x7f7f7f7f: above every read number */
  HIP_CHECK(hipMemsetAsync(g->d_hasfirst, 0, sizeof(int) * nr, G_st));
  HIP_CHECK(hipMemcpyAsync(g->d_rlen, read_len, sizeof(int) * nr, hipMemcpyHostToDevice, G_st));
  HIP_CHECK(hipMemcpyAsync(g->d_trim, trim, sizeof(int) * 2 * nr, hipMemcpyHostToDevice, G_st));
  HIP_CHECK(hipMemcpyAsync(g->d_ctr, ctr, sizeof(ctr), hipMemcpyHostToDevice, G_st));
  GR.mark(1);
  HIP_CHECK(hipStreamSynchronize(G_st));
  GR.laps_add(0, 1);
  return g;
}

/* a resident list grown to hold `need` items of `size` bytes, what it holds kept */
static void grow_resident(void **p, u64 *cap, u64 used, u64 need, size_t size)
{ if (need <= *cap)
    return;
  const u64 c = need + need / 2 + 4096;
  void *q = NULL;
  HIP_CHECK(hipMalloc(&q, size * (size_t) c + 64));
  if (*p != NULL)
    { if (used > 0)
        HIP_CHECK(hipMemcpyAsync(q, *p, size * (size_t) used, hipMemcpyDeviceToDevice, G_st));
      HIP_CHECK(hipStreamSynchronize(G_st));
      HIP_CHECK(hipFree(*p));
    }
  *p = q;
  *cap = c;
}

static void graph_args(const damar_graph *g, GraphArgs *a)
{ memset(a, 0, sizeof(*a));
  a->nreads = (u32) g->nreads;
  a->read_len = g->d_rlen;  a->trim = g->d_trim;
  a->status = g->d_status;  a->minfirst = g->d_minfirst;  a->hasfirst = g->d_hasfirst;
  a->cand = g->d_cand;  a->cand_cap = g->cand_cap;  a->probe = g->d_probe;  a->probe_cap = g->probe_cap;
  a->ctr = g->d_ctr;
  a->ncand = g->ncand;  a->nprobe = g->nprobe;
}

extern "C" int damar_graph_batch(damar_graph *g, const damar_pile_batch *b, const int *diffs, int64 first_rec)
{ if (g == NULL || first_rec < 0)
    return 1;
  if (g->hs != NULL)
    return damar_host_graph_batch(g->hs, b, diffs, first_rec);
  if (!damar_graph_inputs_valid(b, diffs, g->nreads))
    return 1;
  GR.cnt[0] += b->nrec;
  if (b->nrec == 0)
    return 0;
  if ((u64) first_rec + (u64) b->nrec > g->rec_end)
    g->rec_end = (u64) first_rec + (u64) b->nrec;
  if (g->rec_end >= ((u64) 1 << 61))
    { fprintf(stderr, "damar: graph: record %llu is more than the sort's key holds\n", (unsigned long long) g->rec_end);
      return 1;
    }
  GraphArgs a;
  GR.mark(0);
  const PileDev d = pile_up(g->S, b, NULL, { b->abpos, b->aepos, b->bbpos, b->bepos, b->bread, b->flags });
  const int *d_diffs = up(g->S.diffs, diffs, (size_t) b->nrec);
  GR.mark(1);
  graph_args(g, &a);
  a.npiles = (u32) b->npiles;  a.nrec = (u32) b->nrec;  a.first_rec = (u64) first_rec;
  a.pile_off = d.off;  a.pile_aread = d.aread;
  a.abpos = d.col[0];  a.aepos = d.col[1];  a.bbpos = d.col[2];  a.bepos = d.col[3];  a.bread = d.col[4];  a.flags = d.col[5];
  a.diffs = d_diffs;
  damar_launch_graph_count(&a, G_st);
  u64 ctr[2];
  HIP_CHECK(hipMemcpyAsync(ctr, g->d_ctr, sizeof(ctr), hipMemcpyDeviceToHost, G_st));
  HIP_CHECK(hipStreamSynchronize(G_st));
  if (ctr[GC_NCAND] >= 0xffffffffull)
    { fprintf(stderr, "damar: graph: %llu candidate edges, 2^32 - 2 is the most the sort's values number\n", (unsigned long long) ctr[GC_NCAND]);
      return 1;
    }
  grow_resident((void **) &g->d_cand, &g->cand_cap, g->ncand, ctr[GC_NCAND], sizeof(int) * GE_INTS);
  grow_resident((void **) &g->d_probe, &g->probe_cap, g->nprobe, ctr[GC_NPROBE], sizeof(u64));
  const u64 fill[2] = { g->ncand, g->nprobe };
  HIP_CHECK(hipMemcpyAsync(g->d_ctr, fill, sizeof(fill), hipMemcpyHostToDevice, G_st));
  graph_args(g, &a);                               /* the lists may have moved */
  a.npiles = (u32) b->npiles;  a.nrec = (u32) b->nrec;  a.first_rec = (u64) first_rec;
  a.pile_off = d.off;  a.pile_aread = d.aread;
  a.abpos = d.col[0];  a.aepos = d.col[1];  a.bbpos = d.col[2];  a.bepos = d.col[3];  a.bread = d.col[4];  a.flags = d.col[5];
  a.diffs = d_diffs;
  damar_launch_graph_emit(&a, G_st);
  GR.mark(2);
  HIP_CHECK(hipStreamSynchronize(G_st));           /* `fill` is read by the copy until here */
  g->ncand = ctr[GC_NCAND];  g->nprobe = ctr[GC_NPROBE];
  GR.cnt[1] = (int64) g->ncand;
  GR.laps_add(0, 2);
  return 0;
}

static int bits_of(u64 v)         /* bits that hold every value below v */
{ int n = 1;
  while (n < 64 && ((u64) 1 << n) < v) n += 1;
  return n;
}

extern "C" int damar_graph_finish(damar_graph *g, damar_graph_result *res)
{ if (g == NULL || res == NULL)
    return 1;
  if (g->hs != NULL)
    return damar_host_graph_finish(g->hs, res);
  memset(res, 0, sizeof(*res));
  const size_t nr = (size_t) g->nreads;
  const u64 n = g->ncand;
  GraphArgs a;
  graph_args(g, &a);
  u64 *k0 = (u64 *) g->S.k0.need(sizeof(u64) * (size_t) n + 64), *k1 = (u64 *) g->S.k1.need(sizeof(u64) * (size_t) n + 64);
  u32 *v0 = (u32 *) g->S.v0.need(sizeof(u32) * (size_t) n + 64), *v1 = (u32 *) g->S.v1.need(sizeof(u32) * (size_t) n + 64);
  void *sortw = g->S.sortw.need(damar_sort_workspace_bytes(n > 0 ? n : 1));
  void *scanw = g->S.scan.need(damar_scan_workspace_bytes(n > 0 ? n : 1));
  u32 *d_beg = (u32 *) g->S.beg.need(sizeof(u32) * 4 * nr), *d_end = d_beg + 2 * nr;
  u32 *d_keep = (u32 *) g->S.keep.need(sizeof(u32) * (size_t) n + 64), *d_pos = (u32 *) g->S.pos.need(sizeof(u32) * (size_t) n + 64);
  u32 *d_kcount = (u32 *) g->S.kcount.need(sizeof(u32) * 2 * nr), *d_host = (u32 *) g->S.hostread.need(sizeof(u32) * nr);
  u64 *d_total = g->d_ctr + 12;
  GR.mark(2);
  HIP_CHECK(hipMemsetAsync(d_beg, 0, sizeof(u32) * 4 * nr, G_st));
  HIP_CHECK(hipMemsetAsync(d_kcount, 0, sizeof(u32) * 2 * nr, G_st));
  HIP_CHECK(hipMemsetAsync(d_host, 0, sizeof(u32) * nr, G_st));
  HIP_CHECK(hipMemsetAsync(d_total, 0, sizeof(u64), G_st));
  a.key = k0;  a.val = v0;
  damar_launch_graph_settle(&a, G_st);
  u32 h_serr[2] = { 0, 0 };
  u64 total = 0;
  if (n > 0)
    { /* ties keep the order the reference fills a list in: the record's place in the file, A's own edge before the mirrored one */
      int side = damar_radix_sort_u64(k0, v0, k1, v1, n, bits_of((g->rec_end + 1) << 2), sortw, G_st);
      HIP_CHECK(hipMemcpyAsync(&h_serr[0], damar_sort_error_word(sortw), sizeof(u32), hipMemcpyDeviceToHost, G_st));
      a.val_in = side ? v1 : v0;
      a.key = side ? k0 : k1;  a.val = side ? v0 : v1;
      a.rbits = bits_of((u64) nr);
      damar_launch_graph_keys(&a, G_st);
      u64 *ka = a.key, *kb = side ? k1 : k0;
      u32 *va = a.val, *vb = side ? v1 : v0;
      side = damar_radix_sort_u64(ka, va, kb, vb, n, 2 * a.rbits + 2, sortw, G_st);
      HIP_CHECK(hipMemcpyAsync(&h_serr[1], damar_sort_error_word(sortw), sizeof(u32), hipMemcpyDeviceToHost, G_st));
      a.key = side ? kb : ka;  a.val = side ? vb : va;
      a.beg = d_beg;  a.end = d_end;  a.keep = d_keep;  a.pos = d_pos;  a.kcount = d_kcount;  a.hostread = d_host;
      a.maxdeg = damar_graph_maxdeg();
      damar_launch_graph_bounds(&a, G_st);
      damar_launch_graph_reads(&a, G_st);
      damar_exclusive_scan_u32(d_keep, d_pos, n, scanw, d_total, G_st);
      HIP_CHECK(hipMemcpyAsync(&total, d_total, sizeof(u64), hipMemcpyDeviceToHost, G_st));
      HIP_CHECK(hipStreamSynchronize(G_st));
      if (h_serr[0] != 0 || h_serr[1] != 0)
        { fprintf(stderr, "damar: graph: the radix sort gave up on a look-back\n");
          return 1;
        }
      a.out = (int *) g->S.out.need(sizeof(int) * 9 * (size_t) total + 64);
      damar_launch_graph_gather(&a, G_st);
    }
  GR.mark(3);
  u64 ctr[GC_COUNT];
  std::vector<u32> kcount(2 * nr), status(nr), hostread(nr);
  int *edges = (int *) malloc(sizeof(int) * 9 * (size_t) total + 64);
  res->loff = (int64 *) malloc(sizeof(int64) * (nr + 1));  res->roff = (int64 *) malloc(sizeof(int64) * (nr + 1));
  res->status = (unsigned char *) malloc(nr + 1);
  if (edges == NULL || res->loff == NULL || res->roff == NULL || res->status == NULL)
    { fprintf(stderr, "damar: out of memory (graph)\n");
      free(edges);
      damar_graph_result_free(res);
      return 1;
    }
  HIP_CHECK(hipMemcpyAsync(ctr, g->d_ctr, sizeof(ctr), hipMemcpyDeviceToHost, G_st));
  HIP_CHECK(hipMemcpyAsync(kcount.data(), d_kcount, sizeof(u32) * 2 * nr, hipMemcpyDeviceToHost, G_st));
  HIP_CHECK(hipMemcpyAsync(status.data(), g->d_status, sizeof(u32) * nr, hipMemcpyDeviceToHost, G_st));
  HIP_CHECK(hipMemcpyAsync(hostread.data(), d_host, sizeof(u32) * nr, hipMemcpyDeviceToHost, G_st));
  if (total > 0)
    HIP_CHECK(hipMemcpyAsync(edges, a.out, sizeof(int) * 9 * (size_t) total, hipMemcpyDeviceToHost, G_st));
  GR.mark(4);
  HIP_CHECK(hipStreamSynchronize(G_st));
  GR.laps_add(2, 2);

  res->nreads = g->nreads;
  int64 lsum = 0, rsum = 0;
  for (size_t r = 0; r < nr; r++)
    { res->loff[r] = lsum;  res->roff[r] = rsum;
      lsum += kcount[r];  rsum += kcount[nr + r];
      res->status[r] = (status[r] & DAMAR_OG_CONTAINED) ? DAMAR_OG_CONTAINED : (status[r] & DAMAR_OG_PROPER) ? DAMAR_OG_PROPER : DAMAR_OG_WIDOW;
    }
  res->loff[nr] = lsum;  res->roff[nr] = rsum;
  /* the kept edges lie list by list: the left lists of all reads, then the right lists */
  res->left = edges;
  res->right = (int *) malloc(sizeof(int) * 9 * (size_t) rsum + 64);
  if (res->right == NULL)
    { fprintf(stderr, "damar: out of memory (graph)\n");
      damar_graph_result_free(res);
      return 1;
    }
  memcpy(res->right, edges + 9 * (size_t) lsum, sizeof(int) * 9 * (size_t) rsum);
  res->cnt_left = (int64) ctr[GC_LEFT];  res->cnt_right = (int64) (n - ctr[GC_LEFT]);
  res->edges = (int64) ctr[GC_EDGES];  res->redges = (int64) ctr[GC_REDGES];  res->symdiscard = (int64) ctr[GC_SYM];
  res->parallel = (int64) ctr[GC_PARALLEL];
  res->neg_rec = ctr[GC_NEG] == ~0ull ? -1 : (int64) ctr[GC_NEG];
  /* a read with a side over the limit came back with all its edges, in order: the host routine finishes it */
  int64 nhost = 0;
  for (size_t r = 0; r < nr; r++)
    if (hostread[r])
      { res->parallel += damar_host_graph_dedupe(res->left + 9 * res->loff[r], res->loff[r + 1] - res->loff[r],
                                                 res->right + 9 * res->roff[r], res->roff[r + 1] - res->roff[r]);
        nhost += 1;
      }
  if (nhost > 0)
    { damar_host_graph_compress(res->left, res->loff, g->nreads);
      damar_host_graph_compress(res->right, res->roff, g->nreads);
    }
  res->removed = (int64) n - res->loff[nr] - res->roff[nr];
  GR.cnt[1] = (int64) n;  GR.cnt[2] = nhost;  GR.cnt[3] = res->loff[nr] + res->roff[nr];
  return 0;
}
