/* stages/correct.hip -- the C-ABI of the tiles' consensus: damar_tile_consensus */
#include <algorithm>
#include <vector>

#include "stage.h"

/***** LAcorrect's consensus per tile: corrector/consensus.c (kernels/tile_consensus.hip) ************************************/

#define TCN_MAXLANES 32768u    /* stripes of the work area: 512 wavefronts */
#define TCN_CHUNK    131072u   /* tasks per launch: bounds the staging of the called bases */

static struct : DevStage        /* ms of the last call: upload, kernel, download (HIP events), whole call (wall);
                                   cnt: tiles, tiles the host routine did beside the kernel, bases called */
{ DBuf order{*this}, eoff{*this}, soff{*this}, slen{*this}, bases{*this}, work{*this}, out{*this}, status{*this}, len{*this};
} TCN;

extern "C" void damar_correct_release(void) { TCN.release(); }

extern "C" void damar_correct_limits(int *seg, int *cols, int *cells)
{ *seg = DAMAR_CORRECT_MAXSEG;
  *cols = DAMAR_CORRECT_MAXCOLS;
  *cells = DAMAR_CORRECT_CELLS;
}

extern "C" void damar_correct_last(double *ms, int64 *cnt) { TCN.last(ms, cnt, 3); }

extern "C" int damar_tile_consensus(const damar_tile_batch *b, int64 *cons_off, unsigned char **cons, int *added)
{ TCN.begin();
  if (cons_off == NULL || cons == NULL || !damar_tile_batch_valid(b) || (b->ntiles > 0 && added == NULL))
    return 1;
  static_assert(sizeof(int64) == sizeof(long long), "offsets go to the device as they are");
  const size_t nt = (size_t) b->ntiles;
  const bool host = damar_piles_on_host() != 0;
  int64 fallback = 0;
  for (int i = 0; i < 3; i++) TCN.cnt[i] = 0;       /* a call that fails leaves zeros, not a mixture */
  if (nt >= ((size_t) 1 << 31))
    { fprintf(stderr, "damar: correct: %zu tiles in one call (below 2^31 are taken)\n", nt);
      return 1;
    }

  /* per tile: where its result lies among the device's (-1: the host routine does it, -2: empty) */
  std::vector<long long> task_of(nt + 1, -1), comp_off;
  std::vector<u32> order;
  std::vector<u8>  compact;
  for (size_t t = 0; t < nt; t++)
    { const int64 e0 = b->ent_off[t], e1 = b->ent_off[t + 1];
      added[t] = (int) (e1 - e0);
      if (e1 == e0)
        { task_of[t] = -2;
          continue;
        }
      if (host)
        continue;
      bool fits = true;
      for (int64 e = e0; e < e1; e++)
        fits = fits && b->seq_len[e] <= DAMAR_CORRECT_MAXSEG;
      if (fits)
        order.push_back((u32) t);
    }
  if (!order.empty())
    { const int maxcols = test_limit("DAMAR_TEST_CORRECT_COLS", DAMAR_CORRECT_MAXCOLS, 2) & ~1;
      auto weight = [&](u32 t) -> long long
        { if (b->weight != NULL) return b->weight[t];
          const int64 e0 = b->ent_off[t], e1 = b->ent_off[t + 1];
          return (long long) (e1 - e0) * (long long) (b->seq_off[e1 - 1] + b->seq_len[e1 - 1] - b->seq_off[e0]);
        };
      std::stable_sort(order.begin(), order.end(), [&](u32 x, u32 y) { return weight(x) > weight(y); });
      const size_t ntask = order.size(), nent = (size_t) b->ent_off[nt];
      TCN.device();
      TileArgs a;
      memset(&a, 0, sizeof(a));
      a.maxcols = maxcols;
      a.maxscript = maxcols + DAMAR_CORRECT_MAXSEG;
      a.cells = DAMAR_CORRECT_CELLS;
      a.stripe = ((size_t) 6 * maxcols + 2 * (size_t) a.maxscript + 3 * (size_t) a.cells + 15) & ~(size_t) 15;
      const u32 lanes = (u32) std::min<size_t>((ntask + 63) / 64 * 64, TCN_MAXLANES);
      a.blocks = lanes / 64;
      const size_t chunk = std::min<size_t>(ntask, TCN_CHUNK);
      u8  *d_out = (u8 *) TCN.out.need(chunk * (size_t) maxcols);
      int *d_status = (int *) TCN.status.need(sizeof(int) * chunk), *d_len = (int *) TCN.len.need(sizeof(int) * chunk);
      a.work = (u8 *) TCN.work.need((size_t) lanes * a.stripe);
      TCN.mark(0);
      a.ent_off = (const long long *) up(TCN.eoff, b->ent_off, nt + 1);
      a.seq_off = (const long long *) up(TCN.soff, b->seq_off, nent);
      a.seq_len = up(TCN.slen, b->seq_len, nent);
      a.bases = up(TCN.bases, b->bases, (size_t) b->nbases);
      const u32 *d_order = up(TCN.order, order.data(), ntask);
      TCN.mark(1);
      TCN.sync_laps(0, 1);
      a.out = d_out;  a.status = d_status;  a.len = d_len;
      std::vector<int> status(chunk), len(chunk);
      std::vector<u8>  got(chunk * (size_t) maxcols);
      comp_off.assign(ntask + 1, 0);
      for (size_t c0 = 0; c0 < ntask; c0 += chunk)
        { const size_t n = std::min(chunk, ntask - c0);
          a.ntasks = (u32) n;
          a.order = d_order + c0;
          TCN.mark(1);
          damar_launch_tile_consensus(&a, G_st);
          HIP_CHECK(hipGetLastError());
          TCN.mark(2);
          HIP_CHECK(hipMemcpyAsync(status.data(), d_status, sizeof(int) * n, hipMemcpyDeviceToHost, G_st));
          HIP_CHECK(hipMemcpyAsync(len.data(), d_len, sizeof(int) * n, hipMemcpyDeviceToHost, G_st));
          HIP_CHECK(hipMemcpyAsync(got.data(), d_out, n * (size_t) maxcols, hipMemcpyDeviceToHost, G_st));
          TCN.mark(3);
          HIP_CHECK(hipStreamSynchronize(G_st));
          TCN.laps_add(1, 2);
          for (size_t i = 0; i < n; i++)
            { const size_t it = c0 + i;
              comp_off[it + 1] = comp_off[it];
              if (status[i] != 0)
                continue;
              if (len[i] < 0 || len[i] > maxcols)
                { fprintf(stderr, "damar: correct: tile %u came back with %d bases\n", order[it], len[i]);
                  for (int k = 0; k < 4; k++) TCN.ms[k] = 0;
                  return 1;
                }
              task_of[order[it]] = (long long) it;
              compact.insert(compact.end(), got.begin() + i * (size_t) maxcols, got.begin() + i * (size_t) maxcols + len[i]);
              comp_off[it + 1] += len[i];
            }
        }
    }

  /* the calls in tile order; what the kernel left (all tiles with DAMAR_PILES=host) is the plain routine's */
  unsigned char *all = NULL, *one = NULL;
  int64 cap = 0, n = 0, onecap = 0;
  for (size_t t = 0; t < nt; t++)
    { const unsigned char *src = NULL;
      int64 len = 0;
      cons_off[t] = n;
      if (task_of[t] >= 0)
        { len = comp_off[task_of[t] + 1] - comp_off[task_of[t]];
          src = compact.data() + comp_off[task_of[t]];
        }
      else if (task_of[t] == -1)
        { const int got = damar_host_tile(b, (int64) t, &one, &onecap);
          if (got < 0)
            { free(all);  free(one);
              return 1;
            }
          len = got;
          src = one;
          fallback += host ? 0 : 1;
        }
      if (n + len > cap)
        { cap = n + len + cap / 4 + 4096;
          unsigned char *grown = (unsigned char *) realloc(all, (size_t) cap);
          if (grown == NULL)
            { fprintf(stderr, "damar: out of memory (correct)\n");
              free(all);  free(one);
              return 1;
            }
          all = grown;
        }
      if (len > 0)
        memcpy(all + n, src, (size_t) len);
      n += len;
    }
  cons_off[nt] = n;
  free(one);
  if (all == NULL && (all = (unsigned char *) malloc(1)) == NULL)
    { fprintf(stderr, "damar: out of memory (correct)\n");
      return 1;
    }
  *cons = all;
  TCN.end(b->ntiles, fallback, n);
  return 0;
}
