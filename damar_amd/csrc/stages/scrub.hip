/* stages/scrub.hip -- the C-ABI of the per-pile scrubbing kernels: damar_pile_gaps, damar_pile_filter, damar_pile_patches */
#include <vector>
#include <limits.h>

#include "stage.h"

/***** LAgap's containments, gaps and breaks per pile: scrub/LAgap.c (kernels/pile_gaps.hip) ******************************/

static struct : PileStage       /* ms of the last call: upload, kernel, download (HIP events), whole call (wall);
                                   cnt: piles, piles the host routine did beside the kernel, break events */
{ DBuf rlen{*this}, xanno{*this}, xdata{*this}, skip{*this}, flags{*this}, status{*this}, nev{*this}, evs{*this}, pcnt{*this};
} GP;

extern "C" void damar_gap_release(void) { GP.release(); }

extern "C" void damar_gap_limits(int *bins, int *events)
{ *bins = DAMAR_GAP_MAXBINS;
  *events = DAMAR_GAP_MAXEVENTS;
}

extern "C" void damar_gap_last(double *ms, int64 *cnt) { GP.last(ms, cnt, 3); }

extern "C" int damar_pile_gaps(const damar_pile_batch *b, const damar_gap_params *p, int *flags_out, damar_gap_events *ev)
{ GP.begin();
  if (ev == NULL || !damar_gap_inputs_valid(b, p) || (b->nrec > 0 && flags_out == NULL) || (b->npiles > 0 && ev->count == NULL))
    return 1;
  const size_t np = (size_t) b->npiles, nrec = (size_t) b->nrec;
  const bool host = damar_piles_on_host() != 0;
  damar_gap_list L = { NULL, 0, 0 };
  int64 cnt[3] = { 0, 0, 0 }, fallback = 0;

  std::vector<u8>  skip(np + 1, 0);
  std::vector<int> status(np + 1, 1), nev(np + 1, 0), evs, pcnt;
  if (!host && np > 0)
    { /* the kernel takes the records of one B read for a run.  The reference's containment loop skips a discarded record
         before it looks at its B read, so where the B reads do not ascend it can pair records across another read's:
         such a pile is the host routine's */
      for (size_t q = 0; q < np; q++)
        for (int64 i = b->pile_off[q] + 1; i < b->pile_off[q + 1]; i++)
          if (b->bread[i] < b->bread[i - 1])
            { skip[q] = 1;
              break;
            }
      GP.device();
      GapArgs a;
      memset(&a, 0, sizeof(a));
      a.npiles = (u32) np;
      a.maxbins = test_limit("DAMAR_TEST_GAP_BINS", DAMAR_GAP_MAXBINS, INT_MIN);
      a.maxev = DAMAR_GAP_MAXEVENTS;  a.stitch = p->stitch;
      const size_t evints = np * DAMAR_GAP_MAXEVENTS * DAMAR_GAP_EVENT_INTS;
      int *d_flags = (int *) GP.flags.need(sizeof(int) * nrec + 16);
      int *d_status = (int *) GP.status.need(sizeof(int) * np + 16), *d_nev = (int *) GP.nev.need(sizeof(int) * np + 16);
      int *d_ev = (int *) GP.evs.need(sizeof(int) * evints + 16), *d_cnt = (int *) GP.pcnt.need(sizeof(int) * 3 * np + 16);
      GP.mark(0);
      if (p->ex_anno != NULL)
        { const DevTrack ex = up_track(GP.xanno, GP.xdata, p->ex_anno, (size_t) b->nreads, p->ex_data, p->ex_ndata);
          a.ex_anno = ex.anno;  a.ex_data = ex.data;
        }
      a.skip = up(GP.skip, skip.data(), np);
      const PileDev d = pile_up(GP, b, NULL, { b->abpos, b->aepos, b->bbpos, b->bepos, b->bread, b->flags });
      a.read_len = up(GP.rlen, b->read_len, (size_t) b->nreads);
      HIP_CHECK(hipMemsetAsync(d_nev, 0, sizeof(int) * np, G_st));
      GP.mark(1);
      a.pile_off = d.off;  a.pile_aread = d.aread;
      a.abpos = d.col[0];  a.aepos = d.col[1];  a.bbpos = d.col[2];  a.bepos = d.col[3];  a.bread = d.col[4];  a.flags = d.col[5];
      a.flags_out = d_flags;  a.status = d_status;  a.nev = d_nev;  a.ev = d_ev;  a.cnt = d_cnt;
      damar_launch_pile_gaps(&a, (u32) test_limit("DAMAR_TEST_GAP_GRID", (int) damar_pile_gaps_grid(), 1), G_st);
      HIP_CHECK(hipGetLastError());
      GP.mark(2);
      evs.resize(evints + 1);
      pcnt.resize(3 * np + 1);
      if (nrec > 0)
        HIP_CHECK(hipMemcpyAsync(flags_out, d_flags, sizeof(int) * nrec, hipMemcpyDeviceToHost, G_st));
      HIP_CHECK(hipMemcpyAsync(status.data(), d_status, sizeof(int) * np, hipMemcpyDeviceToHost, G_st));
      HIP_CHECK(hipMemcpyAsync(nev.data(), d_nev, sizeof(int) * np, hipMemcpyDeviceToHost, G_st));
      HIP_CHECK(hipMemcpyAsync(evs.data(), d_ev, sizeof(int) * evints, hipMemcpyDeviceToHost, G_st));
      HIP_CHECK(hipMemcpyAsync(pcnt.data(), d_cnt, sizeof(int) * 3 * np, hipMemcpyDeviceToHost, G_st));
      GP.mark(3);
      GP.sync_laps(0, 3);
    }
  /* the events in pile order; what the kernel left (all piles with DAMAR_PILES=host) is the plain routine's */
  for (size_t q = 0; q < np; q++)
    { const int64 before = L.n;
      if (status[q] != 0)
        { damar_host_gap_pile(b, (int64) q, p, flags_out, &L, cnt);
          fallback += host ? 0 : 1;
        }
      else
        { if (nev[q] < 0 || nev[q] > DAMAR_GAP_MAXEVENTS)
            { fprintf(stderr, "damar: gaps: pile %zu came back with %d events\n", q, nev[q]);
              free(L.ev);
              return 1;
            }
          if (list_append(&L.ev, &L.n, &L.cap, DAMAR_GAP_EVENT_INTS, evs.data() + q * DAMAR_GAP_MAXEVENTS * DAMAR_GAP_EVENT_INTS, nev[q], "gaps"))
            return 1;
          for (int i = 0; i < 3; i++) cnt[i] += pcnt[3 * q + i];
        }
      ev->count[q] = (int) (L.n - before);
    }
  if (L.ev == NULL && (L.ev = (int *) malloc(sizeof(int) * DAMAR_GAP_EVENT_INTS)) == NULL)       /* no event: still the caller's to free */
    { fprintf(stderr, "damar: out of memory (gaps)\n");
      return 1;
    }
  ev->ev = L.ev;
  ev->nev = L.n;
  ev->contained = cnt[0];  ev->breaks = cnt[1];  ev->dropped = cnt[2];
  GP.end(b->npiles, fallback, L.n);
  return 0;
}

/***** LAfilter's screens per pile: scrub/LAfilter.c filter_handler (kernels/pile_filter.hip) *****************************/

static struct : PileStage       /* ms of the last call: upload, kernel, download (HIP events), whole call (wall);
                                   cnt: piles, piles the host routine did beside the kernel, records that left discarded */
{ DBuf rlen{*this}, trim{*this}, ranno{*this}, rdata{*this}, soff{*this}, slen{*this}, sdata{*this}, state{*this},
       out[7] = { *this, *this, *this, *this, *this, *this, *this }, status{*this}, pcnt{*this};
} FL;

extern "C" void damar_filter_release(void) { FL.release(); }

extern "C" void damar_filter_limits(int *group, int *len)
{ *group = DAMAR_FILTER_MAXGROUP;
  *len = DAMAR_FILTER_MAXLEN;
}

extern "C" void damar_filter_last(double *ms, int64 *cnt) { FL.last(ms, cnt, 3); }

extern "C" int damar_pile_filter(const damar_trace_batch *t, const int *diffs, const damar_filter_params *p, damar_filter_out *out)
{ FL.begin();
  if (!damar_filter_inputs_valid(t, diffs, p, out))
    return 1;
  const damar_pile_batch *b = &t->p;
  const size_t np = (size_t) b->npiles, nrec = (size_t) b->nrec, nreads = (size_t) b->nreads;
  const bool host = damar_piles_on_host() != 0;
  int64 fallback = 0, gone = 0;

  std::vector<int> status(np + 1, 1);
  if (!host && np > 0)
    { FL.device();
      FilterArgs a;
      memset(&a, 0, sizeof(a));
      a.npiles = (u32) np;
      a.steps = p->steps;
      a.maxgroup = test_limit("DAMAR_TEST_FILTER_GROUP", DAMAR_FILTER_MAXGROUP, 1);
      a.maxlen = test_limit("DAMAR_TEST_FILTER_LEN", DAMAR_FILTER_MAXLEN, 1);
      if ((p->steps & DAMAR_FILTER_MAIN) && p->lowcov && p->max_unaligned != -1)
        { int longest = 0;           /* the coverage bits: room for the longest A read of the batch that the kernel takes */
          for (size_t q = 0; q < np; q++)
            { const int alen = b->read_len[b->pile_aread[q]];
              if (alen <= a.maxlen && alen > longest) longest = alen;
            }
          a.mask_words = (longest + 31) / 32 + 2;
        }
      a.downsample = p->downsample;  a.max_rid = (int) (p->downsample * b->nreads / 100.0);  a.seg_rate = p->seg_rate;
      a.stitch = p->stitch;  a.stitch_aggr = p->stitch_aggr;  a.min_rlen = p->min_rlen;  a.min_olen = p->min_olen;
      a.max_unaligned = p->max_unaligned;  a.min_nonrep = p->min_nonrep;  a.max_diffs = p->max_diffs;  a.merge_tips = p->merge_tips;
      a.multi = p->multi;  a.lowcov = p->lowcov;  a.remove = p->remove;  a.include = p->include;  a.tbytes = t->tbytes;
      int *d_out[7];
      for (int i = 0; i < 7; i++) d_out[i] = (int *) FL.out[i].need(sizeof(int) * nrec + 16);
      int *d_status = (int *) FL.status.need(sizeof(int) * np + 16);
      int *d_cnt = (int *) FL.pcnt.need(sizeof(int) * DAMAR_FC_COUNT * np + 16);
      FL.mark(0);
      if (p->trim != NULL)
        a.trim = up(FL.trim, p->trim, 2 * nreads);
      if (p->min_nonrep != -1)
        { const DevTrack rep = up_track(FL.ranno, FL.rdata, p->rep_anno, nreads, p->rep_data, p->rep_ndata);
          a.rep_anno = rep.anno;  a.rep_data = rep.data;
        }
      if (p->sym_off != NULL)
        { a.sym_off = up(FL.soff, p->sym_off, nreads + 1);
          a.sym_len = up(FL.slen, p->sym_len, nreads + 1);
          a.sym_data = up(FL.sdata, p->sym_data, (size_t) p->sym_ndata);
        }
      if (p->read_state != NULL)
        a.read_state = up(FL.state, p->read_state, nreads);
      const PileDev d = pile_up(FL, b, t, { b->abpos, b->aepos, b->bbpos, b->bepos, b->bread, b->flags, diffs, t->tlen });
      a.read_len = up(FL.rlen, b->read_len, nreads);
      FL.mark(1);
      a.pile_off = d.off;  a.pile_aread = d.aread;
      a.abpos = d.col[0];  a.aepos = d.col[1];  a.bbpos = d.col[2];  a.bepos = d.col[3];  a.bread = d.col[4];  a.flags = d.col[5];
      a.diffs = d.col[6];  a.tlen = d.col[7];  a.trace_off = d.toff;  a.trace = d.trace;
      a.o_flags = d_out[0];  a.o_ae = d_out[1];  a.o_be = d_out[2];  a.o_df = d_out[3];  a.o_tl = d_out[4];  a.o_why = d_out[5];  a.o_by = d_out[6];
      a.status = d_status;  a.cnt = d_cnt;
      damar_launch_pile_filter(&a, (u32) test_limit("DAMAR_TEST_FILTER_GRID", (int) damar_pile_filter_grid(), 1), G_st);
      HIP_CHECK(hipGetLastError());
      FL.mark(2);
      int *dst[7] = { out->flags, out->aepos, out->bepos, out->diffs, out->tlen, out->reason, out->cont_by };
      if (nrec > 0)
        for (int i = 0; i < 7; i++)
          HIP_CHECK(hipMemcpyAsync(dst[i], d_out[i], sizeof(int) * nrec, hipMemcpyDeviceToHost, G_st));
      HIP_CHECK(hipMemcpyAsync(status.data(), d_status, sizeof(int) * np, hipMemcpyDeviceToHost, G_st));
      HIP_CHECK(hipMemcpyAsync(out->cnt, d_cnt, sizeof(int) * DAMAR_FC_COUNT * np, hipMemcpyDeviceToHost, G_st));
      FL.mark(3);
      FL.sync_laps(0, 3);
    }
  /* what the kernel left (all piles with DAMAR_PILES=host) is the plain routine's */
  for (size_t q = 0; q < np; q++)
    if (status[q] != 0)
      { damar_host_filter_pile(t, diffs, (int64) q, p, out);
        fallback += host ? 0 : 1;
      }
  for (size_t i = 0; i < nrec; i++)
    gone += (out->flags[i] & 0x2) != 0;
  FL.end(b->npiles, fallback, gone);
  return 0;
}

/***** LAfix's breaks and weak segments per pile: scrub/LAfix.c fix_process (kernels/pile_patch.hip) **********************/

static struct : PileStage       /* ms of the last call: upload, kernel, download (HIP events), whole call (wall);
                                   cnt: piles, piles the host routine did beside the kernel, repairs */
{ DBuf trim{*this}, rlen{*this}, qanno{*this}, qdata{*this}, ranno{*this}, rdata{*this}, skip{*this}, slot{*this}, gaps{*this}, status{*this},
       ngaps{*this};
} FX;

extern "C" void damar_fix_release(void) { FX.release(); }

extern "C" void damar_fix_limits(int *segs, int *cands)
{ *segs = DAMAR_FIX_MAXSEGS;
  *cands = DAMAR_FIX_MAXCAND;
}

extern "C" void damar_fix_last(double *ms, int64 *cnt) { FX.last(ms, cnt, 3); }

extern "C" int damar_pile_patches(const damar_trace_batch *t, const damar_fix_params *p, const int *trim, damar_fix_gaps *out)
{ FX.begin();
  if (out == NULL || !damar_fix_inputs_valid(t, p, trim) || (t->p.npiles > 0 && out->count == NULL))
    return 1;
  static_assert(sizeof(damar_fix_gap) == 8 * sizeof(int), "the kernel writes a repair as eight ints");
  const damar_pile_batch *b = &t->p;
  const size_t np = (size_t) b->npiles, nrec = (size_t) b->nrec;
  const bool host = damar_piles_on_host() != 0;
  const int tw = t->tspace;
  damar_fix_list L = { NULL, 0, 0 };
  int64 fallback = 0;

  std::vector<u8>  skip(np + 1, 0);
  std::vector<int> status(np + 1, 1), ngaps(np + 1, 0);
  std::vector<long long> slot(np + 1, 0);
  std::vector<damar_fix_gap> got;
  if (!host && np > 0)
    { /* per pile: whether its B reads ascend (a pile where they do not is the host routine's), and the room its repairs
         need at the most -- a repair is a pair of neighbouring records of one B read or a bad segment inside the trim */
      for (size_t q = 0; q < np; q++)
        { const int aread = b->pile_aread[q], tb = trim[2 * q], te = trim[2 * q + 1];
          long long room = 0;
          if (tb < te)
            { for (int64 i = b->pile_off[q] + 1; i < b->pile_off[q + 1]; i++)
                { if (b->bread[i] < b->bread[i - 1])
                    skip[q] = 1;
                  if (b->bread[i] == b->bread[i - 1] && b->aepos[i - 1] < b->abpos[i])
                    room += 1;
                }
              const int64 qa = (int64) (p->q_anno[aread] / 4);
              for (int s = tb / tw; s < te / tw; s++)
                { const int v = (qa + s < p->q_ndata) ? p->q_data[qa + s] : 0;
                  room += (v == 0 || v >= p->lowq) ? 1 : 0;
                }
              if (room > DAMAR_FIX_MAXREP)
                room = DAMAR_FIX_MAXREP;
            }
          slot[q + 1] = slot[q] + room;
        }
      const size_t nslot = (size_t) slot[np];
      FX.device();
      FixArgs a;
      memset(&a, 0, sizeof(a));
      a.npiles = (u32) np;
      a.maxsegs = test_limit("DAMAR_TEST_FIX_SEGS", DAMAR_FIX_MAXSEGS, INT_MIN);
      a.tspace = tw;  a.tbytes = t->tbytes;
      a.lowq = p->lowq;  a.maxgap = p->maxgap;  a.maxspanners = p->maxspanners;  a.minsupport = p->minsupport;
      a.q_ndata = p->q_ndata;
      const size_t nreads = (size_t) b->nreads;
      int *d_gaps = (int *) FX.gaps.need(sizeof(damar_fix_gap) * nslot + 16);
      int *d_status = (int *) FX.status.need(sizeof(int) * np + 16), *d_ngaps = (int *) FX.ngaps.need(sizeof(int) * np + 16);
      FX.mark(0);
      if (p->rep_anno != NULL)
        { const DevTrack rep = up_track(FX.ranno, FX.rdata, p->rep_anno, nreads, p->rep_data, p->rep_ndata);
          a.rep_anno = rep.anno;  a.rep_data = rep.data;
        }
      a.trim = up(FX.trim, trim, 2 * np);
      a.skip = up(FX.skip, skip.data(), np);
      a.slot_off = up(FX.slot, slot.data(), np + 1);
      const PileDev d = pile_up(FX, b, t, { b->abpos, b->aepos, b->bbpos, b->bepos, b->bread, b->flags, t->tlen });
      a.read_len = up(FX.rlen, b->read_len, nreads);
      const DevTrack q = up_track(FX.qanno, FX.qdata, p->q_anno, nreads, p->q_data, p->q_ndata);
      HIP_CHECK(hipMemsetAsync(d_ngaps, 0, sizeof(int) * np, G_st));
      FX.mark(1);
      a.pile_off = d.off;  a.pile_aread = d.aread;
      a.abpos = d.col[0];  a.aepos = d.col[1];  a.bbpos = d.col[2];  a.bepos = d.col[3];  a.bread = d.col[4];  a.flags = d.col[5];
      a.tlen = d.col[6];  a.trace_off = d.toff;  a.trace = d.trace;
      a.q_anno = q.anno;  a.q_data = q.data;
      a.gaps = d_gaps;  a.status = d_status;  a.ngaps = d_ngaps;
      damar_launch_pile_patch(&a, G_st);
      HIP_CHECK(hipGetLastError());
      FX.mark(2);
      got.resize(nslot + 1);
      HIP_CHECK(hipMemcpyAsync(status.data(), d_status, sizeof(int) * np, hipMemcpyDeviceToHost, G_st));
      HIP_CHECK(hipMemcpyAsync(ngaps.data(), d_ngaps, sizeof(int) * np, hipMemcpyDeviceToHost, G_st));
      if (nslot > 0)
        HIP_CHECK(hipMemcpyAsync(got.data(), d_gaps, sizeof(damar_fix_gap) * nslot, hipMemcpyDeviceToHost, G_st));
      FX.mark(3);
      FX.sync_laps(0, 3);
    }
  /* the repairs in pile order; what the kernel left (all piles with DAMAR_PILES=host) is the plain routine's */
  for (size_t q = 0; q < np; q++)
    { const int64 before = L.n;
      if (status[q] != 0)
        { damar_host_fix_pile(t, (int64) q, p, trim[2 * q], trim[2 * q + 1], &L);
          fallback += (host || trim[2 * q] >= trim[2 * q + 1]) ? 0 : 1;
        }
      else
        { if (ngaps[q] < 0 || ngaps[q] > slot[q + 1] - slot[q])
            { fprintf(stderr, "damar: fix: pile %zu came back with %d repairs\n", q, ngaps[q]);
              free(L.g);
              return 1;
            }
          if (list_append(&L.g, &L.n, &L.cap, 1, got.data() + slot[q], ngaps[q], "fix"))
            return 1;
        }
      out->count[q] = (int) (L.n - before);
    }
  if (L.g == NULL && (L.g = (damar_fix_gap *) malloc(sizeof(damar_fix_gap))) == NULL)       /* no repair: still the caller's to free */
    { fprintf(stderr, "damar: out of memory (fix)\n");
      return 1;
    }
  out->gaps = L.g;
  out->ngaps = L.n;
  FX.end(b->npiles, fallback, L.n);
  return 0;
}
