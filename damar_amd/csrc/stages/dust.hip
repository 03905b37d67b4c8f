/* stages/dust.hip -- the C-ABI of the low-complexity mask: damar_dust_reads */
#include <vector>
#include <limits.h>
#include <math.h>

#include "stage.h"

/***** DBdust's low-complexity mask of reads: db/DBdust.c (kernels/dust.hip) **********************************************/

static struct : DevStage        /* ms of the last call: upload, kernels, download (HIP events), whole call (wall);
                                   cnt: reads, reads the host routine did beside the kernel, intervals written */
{ DBuf bases{*this}, roff{*this}, pread{*this}, pfirst{*this}, rpiece{*this}, cand{*this}, ncand{*this}, nint{*this},
       steps{*this}, ooff{*this}, out{*this};
  int64 stepped[2] = { 0, 0 };
} DU;

extern "C" void damar_dust_release(void) { DU.release(); }

extern "C" void damar_dust_limits(int *piece, int *halo, int *stripe, int *window)
{ *piece = DAMAR_DUST_PIECE;
  *halo = DAMAR_DUST_HALO;
  *stripe = DAMAR_DUST_STRIPE;
  *window = DAMAR_DUST_MAXWINDOW;
}

extern "C" void damar_dust_last(double *ms, int64 *cnt) { DU.last(ms, cnt, 3); }

extern "C" void damar_dust_steps(int64 *steps) { steps[0] = DU.stepped[0];  steps[1] = DU.stepped[1]; }

extern "C" int damar_dust_reads(const unsigned char *bases, const int64 *read_off, int64 nreads, const damar_dust_params *p,
                                int64 *out_off, int **out)
{ DU.begin();
  if (!damar_dust_params_valid(p) || nreads < 0 || out_off == NULL || out == NULL || (nreads > 0 && (bases == NULL || read_off == NULL)))
    return 1;
  const size_t nr = (size_t) nreads;
  for (size_t i = 0; i < nr; i++)
    if (read_off[i + 1] < read_off[i] || read_off[i + 1] - read_off[i] > INT_MAX - 8)
      { fprintf(stderr, "damar: dust: read %zu has no length\n", i);
        return 1;
      }
  DU.stepped[0] = DU.stepped[1] = 0;
  *out = NULL;

  /* what the kernel does not do: the doubles of -b, a window its lanes do not hold */
  const bool host = damar_dust_on_host() != 0;
  const bool device = !host && !p->biased && p->window >= 3 && p->window <= DAMAR_DUST_MAXWINDOW && nr > 0;
  std::vector<int> nint(nr + 1, -1), dev_iv;
  std::vector<u32> rpiece(nr + 1, 0);
  int64 fallback = 0;
  if (device)
    { std::vector<u32> pread;
      std::vector<int> pfirst;
      for (size_t i = 0; i < nr; i++)
        { const int ntri = (int) (read_off[i + 1] - read_off[i]) - 2;
          rpiece[i] = (u32) pread.size();
          for (int a = 0; a < ntri; a += DAMAR_DUST_PIECE)
            { pread.push_back((u32) i);
              pfirst.push_back(a);
            }
        }
      rpiece[nr] = (u32) pread.size();
      const size_t np = pread.size();
      DU.device();
      DustArgs a;
      memset(&a, 0, sizeof(a));
      a.npieces = (u32) np;  a.nreads = (u32) nr;
      a.window = p->window;  a.thresh = p->thresh;  a.thresh2i = (int) ceil(2. * p->thresh);  a.minlen = p->minlen;
      a.stripe = test_limit("DAMAR_TEST_DUST_STRIPE", DAMAR_DUST_STRIPE, 1);
      a.cand = (int *) DU.cand.need(sizeof(int) * 2 * (size_t) a.stripe * np + 16);
      a.ncand = (int *) DU.ncand.need(sizeof(int) * np + 16);
      a.nint = (int *) DU.nint.need(sizeof(int) * nr + 16);
      a.steps = (u64 *) DU.steps.need(sizeof(u64) * 2);
      DU.mark(0);
      a.bases = up(DU.bases, bases, (size_t) read_off[nr]);
      a.read_off = (const long long *) up(DU.roff, read_off, nr + 1);
      a.piece_read = up(DU.pread, pread.data(), np);
      a.piece_first = up(DU.pfirst, pfirst.data(), np);
      a.read_piece = up(DU.rpiece, rpiece.data(), nr + 1);
      HIP_CHECK(hipMemsetAsync(a.steps, 0, sizeof(u64) * 2, G_st));
      DU.mark(1);
      damar_launch_dust_pieces(&a, G_st);
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipMemcpyAsync(nint.data(), a.nint, sizeof(int) * nr, hipMemcpyDeviceToHost, G_st));
      HIP_CHECK(hipStreamSynchronize(G_st));
      /* where the kernel's reads lie among themselves; the host's reads are put between them below */
      std::vector<long long> doff(nr + 1, 0);
      for (size_t i = 0; i < nr; i++)
        { if (nint[i] > (int) (rpiece[i + 1] - rpiece[i]) * a.stripe)
            { fprintf(stderr, "damar: dust: read %zu came back with %d intervals\n", i, nint[i]);
              return 1;
            }
          doff[i + 1] = doff[i] + (nint[i] > 0 ? 2 * (long long) nint[i] : 0);
        }
      a.out_off = up(DU.ooff, doff.data(), nr);
      a.out = (int *) DU.out.need(sizeof(int) * (size_t) doff[nr] + 16);
      damar_launch_dust_gather(&a, G_st);
      HIP_CHECK(hipGetLastError());
      DU.mark(2);
      dev_iv.resize((size_t) doff[nr] + 1);
      u64 st[2] = { 0, 0 };
      if (doff[nr] > 0)
        HIP_CHECK(hipMemcpyAsync(dev_iv.data(), a.out, sizeof(int) * (size_t) doff[nr], hipMemcpyDeviceToHost, G_st));
      HIP_CHECK(hipMemcpyAsync(st, a.steps, sizeof(st), hipMemcpyDeviceToHost, G_st));
      DU.mark(3);
      DU.sync_laps(0, 3);
      DU.stepped[0] = (int64) st[0];  DU.stepped[1] = (int64) st[1];
    }

  /* the reads in order; what the kernel left (all reads with DAMAR_DUST=host) is the plain routine's */
  int64 n = 0, cap = 0, got = 0;
  int  *all = NULL;
  damar_dust_list work = { NULL, 0, 0 };
  for (size_t i = 0; i < nr; i++)
    { const int len = (int) (read_off[i + 1] - read_off[i]);
      const int64 need = nint[i] >= 0 ? 2 * (int64) nint[i] : 2 * (int64) len;
      out_off[i] = n;
      if (damar_room(&cap, n + need, 4096))
        all = (int *) damar_grow(all, sizeof(int) * (size_t) cap, "dust intervals");
      if (nint[i] >= 0)
        { if (need > 0)
            memcpy(all + n, dev_iv.data() + got, sizeof(int) * (size_t) need);
          got += need;
          n += need;
        }
      else
        { n += 2 * damar_host_dust_read(bases + read_off[i], len, p, 0, 0, all + n, &work, DU.stepped);
          fallback += host ? 0 : 1;
        }
    }
  out_off[nr] = n;
  free(work.iv);
  if (all == NULL)
    all = (int *) damar_grow(NULL, sizeof(int), "dust intervals");      /* no interval: still the caller's to free */
  *out = all;
  DU.end(nreads, fallback, n / 2);
  return 0;
}
