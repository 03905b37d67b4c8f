/* stages/quality.hip -- the C-ABI of the piles' quality values: damar_pile_quality */
#include <vector>

#include "stage.h"

/***** LAq's per-tile quality from the traces of piles: scrub/LAq.c handler_annotate (kernels/pile_quality.hip) **********/

static struct : PileStage       /* ms of the last device call: upload, count + scan, scatter + select, download; cnt: segments counted, tiles */
{ DBuf alen{*this}, tile0{*this}, depth{*this}, run{*this}, vals{*this}, q{*this}, scan{*this}, misc{*this};
  std::vector<int> halen;        /* per pile: the read's length and where its tiles begin (host arithmetic, kept) */
  std::vector<u32> htile0;
} LQ;

extern "C" void damar_q_release(void)
{ LQ.release();
  std::vector<int>().swap(LQ.halen);
  std::vector<u32>().swap(LQ.htile0);
}

extern "C" void damar_q_last(double *ms, int64 *cnt) { LQ.last(ms, cnt, 2); }

extern "C" int damar_pile_quality(const damar_trace_batch *t, const damar_q_params *p, int *q_out, int64 *ntiles_out)
{ int64 ntiles = 0;
  if (t == NULL || p == NULL || ntiles_out == NULL || !damar_trace_batch_valid(t, &ntiles))
    return 1;
  if (p->segmin < 1 || p->segmax < p->segmin)
    { fprintf(stderr, "damar: quality: segmin %d and segmax %d: 1 <= segmin <= segmax is needed\n", p->segmin, p->segmax);
      return 1;
    }
  *ntiles_out = ntiles;
  if (q_out == NULL || ntiles == 0)
    return 0;
  if (damar_piles_on_host())
    return damar_host_pile_quality(t, p, q_out);

  ensure_init();
  const damar_pile_batch *b = &t->p;
  const u32 np = (u32) b->npiles, nt = (u32) ntiles;
  const size_t nrec = (size_t) b->nrec;
  u64 segs = 0;                                    /* what the runs hold at most: every segment of every trace */
  for (size_t i = 0; i < nrec; i++) segs += (u64) (t->tlen[i] / 2);
  LQ.halen.resize(np);
  LQ.htile0.resize((size_t) np + 1);
  LQ.htile0[0] = 0;
  for (u32 i = 0; i < np; i++)
    { LQ.halen[i] = b->read_len[b->pile_aread[i]];
      LQ.htile0[i + 1] = LQ.htile0[i] + (u32) ((LQ.halen[i] + t->tspace - 1) / t->tspace);
    }

  QArgs a;
  memset(&a, 0, sizeof(a));
  a.npiles = np;  a.nrec = (u32) nrec;  a.ntiles = nt;
  a.tspace = t->tspace;  a.tbytes = t->tbytes;
  a.segmin = (u32) p->segmin;  a.segmax = (u32) p->segmax;  a.ccs = p->ccs ? 1 : 0;
  u32 *d_depth = (u32 *) LQ.depth.need(sizeof(u32) * ((size_t) nt + 1));
  u32 *d_run = (u32 *) LQ.run.need(sizeof(u32) * ((size_t) nt + 1));
  u16 *d_vals = (u16 *) LQ.vals.need(sizeof(u16) * (size_t) segs + 16);
  int *d_q = (int *) LQ.q.need(sizeof(int) * (size_t) nt);
  void *d_scan = LQ.scan.need(damar_scan_workspace_bytes((u64) nt + 1));
  u64 *d_misc = (u64 *) LQ.misc.need(64);

  LQ.mark(0);
  a.pile_alen = up(LQ.alen, LQ.halen.data(), (size_t) np);
  a.pile_tile0 = up(LQ.tile0, LQ.htile0.data(), (size_t) np + 1);
  const PileDev d = pile_up(LQ, b, t, { b->abpos, b->aepos, b->bread, t->tlen });
  HIP_CHECK(hipMemsetAsync(d_depth, 0, sizeof(u32) * ((size_t) nt + 1), G_st));
  LQ.mark(1);

  a.pile_off = d.off;  a.pile_aread = d.aread;
  a.abpos = d.col[0];  a.aepos = d.col[1];  a.bread = d.col[2];  a.tlen = d.col[3];
  a.trace_off = d.toff;  a.trace = d.trace;
  a.depth = d_depth;  a.off = d_run;  a.vals = d_vals;  a.q = d_q;
  damar_launch_q_count(&a, G_st);
  damar_exclusive_scan_u32(d_depth, d_run, (u64) nt + 1, d_scan, d_misc, G_st);       /* d_run[nt] = d_misc[0] = segments counted */
  LQ.mark(2);
  damar_launch_q_scatter(&a, G_st);
  damar_launch_q_select(&a, G_st);
  LQ.mark(3);
  u64 h_total = 0;
  HIP_CHECK(hipMemcpyAsync(q_out, d_q, sizeof(int) * (size_t) nt, hipMemcpyDeviceToHost, G_st));
  HIP_CHECK(hipMemcpyAsync(&h_total, d_misc, sizeof(u64), hipMemcpyDeviceToHost, G_st));
  LQ.mark(4);
  LQ.sync_laps(0, 4);
  LQ.cnt[0] = (int64) h_total;  LQ.cnt[1] = ntiles;
  return 0;
}
