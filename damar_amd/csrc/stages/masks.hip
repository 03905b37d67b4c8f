/* stages/masks.hip -- the C-ABI of the pile sweep: damar_pile_coverage, damar_pile_repeats, damar_pile_tandem */
#include <vector>

#include "stage.h"

/***** mask tracks from piles of overlaps: scrub/LArepeat.c and scrub/TANmask.c (kernels/pile_sweep.hip) **********/

static struct : PileStage       /* ms of the last call: upload, sort, sweep, download; cnt: events sorted, regions (TANDEM: intervals) written */
{ DBuf rlen{*this}, rflags{*this}, k0{*this}, k1{*this}, kept{*this}, koff{*this}, scan{*this}, sortw{*this}, bases{*this}, active{*this},
       rb{*this}, re{*this}, rc{*this}, out{*this}, count{*this}, doff{*this}, dst{*this}, misc{*this};
  std::vector<u64> hsum;         /* COVER's per-pile results on the host: grown, kept */
  std::vector<int> hact;
} PL;

extern "C" void damar_pile_release(void)
{ PL.release();
  std::vector<u64>().swap(PL.hsum);
  std::vector<int>().swap(PL.hact);
}

extern "C" void damar_pile_last(double *ms, int64 *cnt) { PL.last(ms, cnt, 2); }

static int bits_for(u64 v)      /* bits that hold the value v */
{ int b = 1;
  while (b < 63 && (v >> b) != 0) b += 1;
  return b;
}

/* what the kernels index with: checked here, once, on the host.  The kernels hold record offsets and three ints of data per
   kept record in 32 bits, so a batch holds fewer than 2^29 records (the reader's batches hold 2^23). */
static int pile_batch_valid(const damar_pile_batch *b)
{ if (b->npiles < 0 || b->nrec < 0 || b->npiles > 0x7fffffff || b->nrec > 0x1fffffff || b->nreads <= 0 || b->maxlen < 0)
    return 0;
  if (b->npiles == 0)
    return b->nrec == 0;
  if (b->pile_off[0] != 0 || b->pile_off[b->npiles] != b->nrec)
    return 0;
  for (int64 i = 0; i < b->npiles; i++)
    if (b->pile_off[i] > b->pile_off[i + 1] || b->pile_aread[i] < 0 || b->pile_aread[i] >= b->nreads)
      return 0;
  for (int64 i = 0; i < b->nrec; i++)
    if (b->bread[i] < 0 || b->bread[i] >= b->nreads)
      return 0;
  return 1;
}

/* One batch through the device.  COVER: bases_out / active_out [npiles].  REPEAT, TANDEM: out. */
static int pile_device(int mode, const damar_pile_batch *b, const damar_repeat_params *p, int min_len,
                       u64 *bases_out, int *active_out, damar_pile_track *out)
{ ensure_init();
  const u32 np = (u32) b->npiles;
  const u64 nrec = (u64) b->nrec, nkeys = 2 * nrec;
  int pbits = bits_for((u64) (b->maxlen > 0 ? b->maxlen : 1));
  if (pbits > 30)
    { fprintf(stderr, "damar: piles: reads of %d bases are beyond the event key\n", b->maxlen);
      return 1;
    }
  const int hibit = pbits + 1 + bits_for(np);

  PileArgs a;
  memset(&a, 0, sizeof(a));
  a.npiles = np;  a.mode = mode;  a.pbits = pbits;
  a.min_len = (mode == DAMAR_PILE_TANDEM) ? min_len : p->min_aln_len;
  if (mode != DAMAR_PILE_TANDEM)
    { a.inc_identity = p->inc_identity;  a.inccov = p->inccov ? 1 : 0;
      a.enter = (int) (p->cov * p->xcov_enter);  a.leave = (int) (p->cov * p->xcov_leave);     /* LArepeat.c:328-329 */
      a.merge_dist = p->merge_dist;
    }
  u64 *k0 = (u64 *) PL.k0.need(sizeof(u64) * (size_t) nkeys + 64), *k1 = (u64 *) PL.k1.need(sizeof(u64) * (size_t) nkeys + 64);
  u32 *d_kept = (u32 *) PL.kept.need(sizeof(u32) * (size_t) np), *d_koff = (u32 *) PL.koff.need(sizeof(u32) * (size_t) np);
  u32 *d_count = (u32 *) PL.count.need(sizeof(u32) * (size_t) np), *d_doff = (u32 *) PL.doff.need(sizeof(u32) * (size_t) np);
  void *d_scan = PL.scan.need(damar_scan_workspace_bytes(np));
  void *d_sortw = PL.sortw.need(damar_sort_workspace_bytes(nkeys));
  u64 *d_misc = (u64 *) PL.misc.need(256);          /* [0] total kept, [1] total data, [2..3] stats, [4] error word */

  PL.mark(0);
  const PileDev d = pile_up(PL, b, NULL, { b->abpos, b->aepos, b->bbpos, b->bepos, b->bread, b->flags });
  a.read_len = up(PL.rlen, b->read_len, (size_t) b->nreads);
  a.read_flags = up(PL.rflags, b->read_flags, (size_t) b->nreads);
  HIP_CHECK(hipMemsetAsync(d_misc, 0, 256, G_st));
  PL.mark(1);

  a.pile_off = d.off;  a.pile_aread = d.aread;
  a.abpos = d.col[0];  a.aepos = d.col[1];  a.bbpos = d.col[2];  a.bepos = d.col[3];  a.bread = d.col[4];  a.flags = d.col[5];
  a.keys = k0;  a.kept = d_kept;  a.koff = d_koff;
  a.stats = d_misc + 2;  a.err = (u32 *) (d_misc + 4);
  a.count = d_count;
  if (mode == DAMAR_PILE_COVER)
    { a.bases = (u64 *) PL.bases.need(sizeof(u64) * (size_t) np);
      a.active = (int *) PL.active.need(sizeof(int) * (size_t) np);
    }
  damar_launch_pile_events(&a, G_st);
  damar_exclusive_scan_u32(d_kept, d_koff, np, d_scan, d_misc, G_st);
  const int side = damar_radix_sort_keys_u64(k0, k1, nkeys, 0, hibit, d_sortw, G_st);
  a.keys = side ? k1 : k0;
  u64 h_misc[5];
  u32 h_serr = 0;
  HIP_CHECK(hipMemcpyAsync(h_misc, d_misc, sizeof(h_misc), hipMemcpyDeviceToHost, G_st));
  HIP_CHECK(hipMemcpyAsync(&h_serr, damar_sort_error_word(d_sortw), sizeof(u32), hipMemcpyDeviceToHost, G_st));
  PL.mark(2);
  HIP_CHECK(hipStreamSynchronize(G_st));
  if (h_serr != 0)
    { fprintf(stderr, "damar: piles: the radix sort's look-back timed out\n");
      return 1;
    }
  if ((u32) h_misc[4] & DAMAR_PILE_ERR_RANGE)
    { fprintf(stderr, "damar: piles: a record's coordinates lie outside its read (longest read %d)\n", b->maxlen);
      return 1;
    }
  const u64 nkept = h_misc[0];
  PL.cnt[0] = (int64) (2 * nkept);
  if (mode == DAMAR_PILE_REPEAT)
    { a.rb = (int *) PL.rb.need(sizeof(int) * (size_t) nkept + 16);
      a.re = (int *) PL.re.need(sizeof(int) * (size_t) nkept + 16);
      a.rc = (int *) PL.rc.need(sizeof(int) * (size_t) nkept + 16);
    }
  if (mode != DAMAR_PILE_COVER)
    a.out = (int *) PL.out.need(sizeof(int) * 3 * (size_t) nkept + 16);
  damar_launch_pile_sweep(&a, G_st);
  if (mode == DAMAR_PILE_COVER)
    { PL.mark(3);
      HIP_CHECK(hipMemcpyAsync(bases_out, a.bases, sizeof(u64) * (size_t) np, hipMemcpyDeviceToHost, G_st));
      HIP_CHECK(hipMemcpyAsync(active_out, a.active, sizeof(int) * (size_t) np, hipMemcpyDeviceToHost, G_st));
      PL.cnt[1] = 0;
    }
  else
    { damar_exclusive_scan_u32(d_count, d_doff, np, d_scan, d_misc + 1, G_st);
      HIP_CHECK(hipMemcpyAsync(h_misc, d_misc, sizeof(h_misc), hipMemcpyDeviceToHost, G_st));
      HIP_CHECK(hipStreamSynchronize(G_st));
      const u64 ndata = h_misc[1];
      int *d_dst = (int *) PL.dst.need(sizeof(int) * (size_t) ndata + 16);
      damar_launch_pile_gather(a.out, d_koff, d_count, d_doff, np, d_dst, G_st);
      PL.mark(3);
      out->data = (int *) malloc(sizeof(int) * (size_t) ndata + 8);
      if (out->data == NULL)
        { fprintf(stderr, "damar: out of memory (piles)\n");
          return 1;
        }
      out->ndata = (int64) ndata;
      out->merged = (int64) h_misc[2];
      out->repeat_bases = (int64) h_misc[3];
      if (ndata > 0)
        HIP_CHECK(hipMemcpyAsync(out->data, d_dst, sizeof(int) * (size_t) ndata, hipMemcpyDeviceToHost, G_st));
      HIP_CHECK(hipMemcpyAsync(out->count, d_count, sizeof(int) * (size_t) np, hipMemcpyDeviceToHost, G_st));
    }
  PL.mark(4);
  PL.sync_laps(0, 4);
  if (mode != DAMAR_PILE_COVER)
    { const int width = (mode == DAMAR_PILE_REPEAT && a.inccov) ? 3 : 2;       /* a region left open holds its begin alone */
      int64 regions = 0;
      for (u32 i = 0; i < np; i++)
        regions += (out->count[i] + width - 1) / width;
      PL.cnt[1] = regions;
    }
  return 0;
}

static void pile_empty(damar_pile_track *out)
{ out->data = (int *) malloc(8);
  out->ndata = out->merged = out->repeat_bases = 0;
}

extern "C" int damar_pile_coverage(const damar_pile_batch *b, const damar_repeat_params *p, int64 *histo, int64 *bases, int64 *inactive)
{ if (!pile_batch_valid(b) || p->max_cov <= 0)
    { fprintf(stderr, "damar: piles: malformed batch\n");
      return 1;
    }
  if (damar_piles_on_host())
    return damar_host_pile_coverage(b, p, histo, bases, inactive);
  if (b->npiles == 0)
    return 0;
  std::vector<u64> &sum = PL.hsum;
  std::vector<int> &act = PL.hact;
  sum.assign((size_t) b->npiles, 0);
  act.assign((size_t) b->npiles, 0);
  if (b->nrec > 0)
    { if (pile_device(DAMAR_PILE_COVER, b, p, 0, sum.data(), act.data(), NULL))
        return 1;
    }
  for (int64 i = 0; i < b->npiles; i++)         /* LArepeat.c:208-223 */
    { const int   alen = b->read_len[b->pile_aread[i]];
      const int64 cov = act[i] > 0 ? (int64) sum[i] / act[i] : 0;
      if (cov < p->max_cov)
        histo[cov] += 1;
      *bases += alen;
      *inactive += alen - act[i];
    }
  return 0;
}

extern "C" int damar_pile_repeats(const damar_pile_batch *b, const damar_repeat_params *p, damar_pile_track *out)
{ if (!pile_batch_valid(b) || out == NULL || (b->npiles > 0 && out->count == NULL))
    { fprintf(stderr, "damar: piles: malformed batch\n");
      return 1;
    }
  /* the state after an event is the last setting event's only while span_enter >= span_leave (LArepeat.c:609-613 refuses
     low > high); below that the device's scan and a sequential walk would part ways */
  if (p->xcov_enter < p->xcov_leave || (int) (p->cov * p->xcov_enter) < (int) (p->cov * p->xcov_leave))
    { fprintf(stderr, "damar: piles: coverage %d with enter %.2f below leave %.2f\n", p->cov, p->xcov_enter, p->xcov_leave);
      return 1;
    }
  if (damar_piles_on_host())
    return damar_host_pile_repeats(b, p, out);
  if (b->nrec == 0)
    { for (int64 i = 0; i < b->npiles; i++) out->count[i] = 0;
      pile_empty(out);
      return 0;
    }
  return pile_device(DAMAR_PILE_REPEAT, b, p, 0, NULL, NULL, out);
}

extern "C" int damar_pile_tandem(const damar_pile_batch *b, int min_len, damar_pile_track *out)
{ if (!pile_batch_valid(b) || out == NULL || (b->npiles > 0 && out->count == NULL))
    { fprintf(stderr, "damar: piles: malformed batch\n");
      return 1;
    }
  if (damar_piles_on_host())
    return damar_host_pile_tandem(b, min_len, out);
  if (b->nrec == 0)
    { for (int64 i = 0; i < b->npiles; i++) out->count[i] = 0;
      pile_empty(out);
      return 0;
    }
  return pile_device(DAMAR_PILE_TANDEM, b, NULL, min_len, NULL, NULL, out);
}
