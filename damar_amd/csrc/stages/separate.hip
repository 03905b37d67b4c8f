/* stages/separate.hip -- the C-ABI of LAseparate's chains per group: damar_pile_chains (kernels/pile_chains.hip) */
#include <vector>

#include "stage.h"

static struct : PileStage       /* ms of the last call: upload, kernels, download (HIP events), whole call (wall);
                                   cnt: groups, groups the host routine did beside the kernel, groups of more than one record */
{ DBuf rlen{*this}, ranno{*this}, rdata{*this}, arep{*this}, brep{*this}, out[5] = { *this, *this, *this, *this, *this }, status{*this};
} SP;

extern "C" void damar_separate_release(void) { SP.release(); }

extern "C" void damar_separate_limits(int *group, int *chains)
{ *group = DAMAR_SEPARATE_MAXGROUP;
  *chains = DAMAR_SEPARATE_MAXCHAINS;
}

extern "C" void damar_separate_last(double *ms, int64 *cnt) { SP.last(ms, cnt, 3); }

extern "C" int damar_pile_chains(const damar_pile_batch *b, const damar_separate_params *p, damar_chain_out *out)
{ SP.begin();
  if (!damar_separate_inputs_valid(b, p, out))
    return 1;
  const size_t np = (size_t) b->npiles, nrec = (size_t) b->nrec, nreads = (size_t) b->nreads;
  const bool host = damar_piles_on_host() != 0;
  int64 groups = 0, multi = 0, fallback = 0;

  std::vector<int> status(nrec + 1, 1);
  if (!host && nrec > 0)
    { SP.device();
      ChainArgs a;
      memset(&a, 0, sizeof(a));
      a.npiles = (u32) np;
      a.kind = p->kind;  a.twidth = p->twidth;
      a.maxgroup = test_limit("DAMAR_TEST_SEPARATE_GROUP", DAMAR_SEPARATE_MAXGROUP, 2);
      a.maxchains = test_limit("DAMAR_TEST_SEPARATE_CHAINS", DAMAR_SEPARATE_MAXCHAINS, 1);
      int *d_out[5];
      for (int i = 0; i < 5; i++) d_out[i] = (int *) SP.out[i].need(sizeof(int) * nrec + 16);
      int *d_status = (int *) SP.status.need(sizeof(int) * nrec + 16);
      a.arep = (int *) SP.arep.need(sizeof(int) * nrec + 16);
      a.brep = (int *) SP.brep.need(sizeof(int) * nrec + 16);
      SP.mark(0);
      if (p->rep_anno != NULL)
        { const DevTrack rep = up_track(SP.ranno, SP.rdata, p->rep_anno, nreads, p->rep_data, p->rep_ndata);
          a.rep_anno = rep.anno;  a.rep_data = rep.data;
        }
      const PileDev d = pile_up(SP, b, NULL, { b->abpos, b->aepos, b->bbpos, b->bepos, b->bread, b->flags });
      a.read_len = up(SP.rlen, b->read_len, nreads);
      SP.mark(1);
      a.pile_off = d.off;  a.pile_aread = d.aread;
      a.abpos = d.col[0];  a.aepos = d.col[1];  a.bbpos = d.col[2];  a.bepos = d.col[3];  a.bread = d.col[4];  a.flags = d.col[5];
      a.o_flags = d_out[0];  a.o_nchains = d_out[1];  a.o_proper = d_out[2];  a.o_nbest = d_out[3];  a.o_best = d_out[4];
      a.status = d_status;
      damar_launch_pile_chains(&a, (u32) test_limit("DAMAR_TEST_SEPARATE_GRID", (int) damar_pile_chains_grid(), 1), G_st);
      HIP_CHECK(hipGetLastError());
      SP.mark(2);
      int *dst[5] = { out->flags, out->nchains, out->proper, out->nbest, out->best };
      for (int i = 0; i < 5; i++)
        HIP_CHECK(hipMemcpyAsync(dst[i], d_out[i], sizeof(int) * nrec, hipMemcpyDeviceToHost, G_st));
      HIP_CHECK(hipMemcpyAsync(status.data(), d_status, sizeof(int) * nrec, hipMemcpyDeviceToHost, G_st));
      SP.mark(3);
      SP.sync_laps(0, 3);
    }
  /* what the kernel left (all groups with DAMAR_PILES=host) is the plain routine's */
  for (size_t q = 0; q < np; q++)
    for (int64 g0 = b->pile_off[q], i = g0; i < b->pile_off[q + 1]; i++)
      if (i + 1 == b->pile_off[q + 1] || b->bread[i + 1] != b->bread[g0])
        { groups += 1;
          multi += i > g0;
          if (status[(size_t) g0] != 0)
            { damar_host_chain_group(b, (int64) q, g0, (int) (i - g0 + 1), p, out);
              fallback += host ? 0 : 1;
            }
          g0 = i + 1;
        }
  SP.end(groups, fallback, multi);
  return 0;
}
