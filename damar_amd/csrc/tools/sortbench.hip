/* sortbench.hip -- the radix sort of kernels/radix_sort.hip on its own: checks every entry point against
 * std::stable_sort on the host (small n, ragged sizes, every digit count) and times the two sorts of the
 * path at their config-2 sizes (k-mer index: 135 M packed u64 on bits 32..60; seed pairs: 61 M u64 on 43 bits).
 * Built per variant: hipcc -DOS_THREADS=.. -DOS_ITEMS=.. -DOS_MINW=.. (scripts/gpu_sortbench.sh).
 *
 *   sortbench check          correctness sweep, exit 1 on the first difference
 *   sortbench time [reps]    timings; prints GB/s against the ALGORITHMIC bytes of SURVEY 8(d)
 *                            (16-byte records, one read + one write per 8-bit digit) and the bytes moved here
 *   sortbench index [reps]   the packed k-mer index of one config-2 block (135 Mbp of 10 kb reads, k = 14) both ways:
 *                            kmer_tuples + sort over its keys, and the sort that makes its keys (KmerKeys); ms and bytes
 *                            moved.  Both results are compared first, there and on a block of reads of k - 1 .. k + 6 bases.
 *   sortbench order [reps]   the ordering of the kept runs behind the seed sort over the read pair only (kernels/seed_merge.hip
 *                            damar_launch_order_runs) against the one it replaced, a workgroup per run: 45 000 runs of 8 seeds,
 *                            of 100, and a mix with a tail up to 2048; both checked against std::stable_sort; ms and runs per second
 */
#include "../kernels/radix_sort.hip"
#include "../kernels/kmer_index.hip"
#include "../kernels/sort_scan.hip"          /* (the scans seed_merge.hip's launchers call) */
#include "../kernels/seed_merge.hip"
#include <vector>
#include <algorithm>
#include <numeric>
#include <string.h>

static u64 rng_state = 88172645463325252ull;
static u64 rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

template <typename T> static T *dev(size_t n) { void *p; HIP_CHECK(hipMalloc(&p, sizeof(T) * (n ? n : 1))); return (T *) p; }

static int check_err(void *ws)
{ u32 e = 0;
  HIP_CHECK(hipMemcpy(&e, damar_sort_error_word(ws), 4, hipMemcpyDeviceToHost));
  return e != 0;
}

/* kind 0: u32 key + u32 val; 1: u32 keys; 2: u64 key + u32 val; 3: u64 keys on [lo,hi); 4: split */
static int check_one(int kind, u64 n, int lo, int hi, int skew)
{ std::vector<u64> hk(n);
  std::vector<u32> hv(n);
  for (u64 i = 0; i < n; i++)
    { u64 x = rnd();
      if (skew == 1) x &= 0x0303030303030303ull;            /* few distinct digits: long runs */
      if (skew == 2) x = (x & 0xff) * 0x0101010101010101ull;
      if (kind < 2) x &= 0xffffffffull;
      hk[i] = x;
      hv[i] = (u32) i;
    }
  std::vector<u32> ord(n);
  std::iota(ord.begin(), ord.end(), 0u);
  const u64 m = (hi - lo >= 64) ? ~0ull : (((1ull << (hi - lo)) - 1) << lo);
  std::stable_sort(ord.begin(), ord.end(), [&](u32 a, u32 b) { return (hk[a] & m) < (hk[b] & m); });
  void *ws = dev<char>(damar_sort_workspace_bytes(n));
  int bad = 0;
  if (kind < 2)
    { std::vector<u32> h32(n);
      for (u64 i = 0; i < n; i++) h32[i] = (u32) hk[i];
      u32 *k0 = dev<u32>(n), *k1 = dev<u32>(n), *v0 = dev<u32>(n), *v1 = dev<u32>(n);
      HIP_CHECK(hipMemcpy(k0, h32.data(), 4 * n, hipMemcpyHostToDevice));
      HIP_CHECK(hipMemcpy(v0, hv.data(), 4 * n, hipMemcpyHostToDevice));
      int side = kind == 0 ? damar_radix_sort_u32(k0, v0, k1, v1, n, hi, ws, 0) : damar_radix_sort_keys_u32(k0, k1, n, hi, ws, 0);
      HIP_CHECK(hipDeviceSynchronize());
      std::vector<u32> ok(n), ov(n);
      HIP_CHECK(hipMemcpy(ok.data(), side ? k1 : k0, 4 * n, hipMemcpyDeviceToHost));
      HIP_CHECK(hipMemcpy(ov.data(), side ? v1 : v0, 4 * n, hipMemcpyDeviceToHost));
      for (u64 i = 0; i < n && !bad; i++)
        if (ok[i] != h32[ord[i]] || (kind == 0 && ov[i] != ord[i]))
          { fprintf(stderr, "kind %d n %llu bits %d: item %llu differs\n", kind, (unsigned long long) n, hi, (unsigned long long) i); bad = 1; }
      hipFree(k0); hipFree(k1); hipFree(v0); hipFree(v1);
    }
  else
    { u64 *k0 = dev<u64>(n), *k1 = dev<u64>(n);
      u32 *v0 = dev<u32>(n), *v1 = dev<u32>(n), *oh = dev<u32>(n), *ol = dev<u32>(n);
      HIP_CHECK(hipMemcpy(k0, hk.data(), 8 * n, hipMemcpyHostToDevice));
      HIP_CHECK(hipMemcpy(v0, hv.data(), 4 * n, hipMemcpyHostToDevice));
      int side = 0;
      if (kind == 2) side = damar_radix_sort_u64(k0, v0, k1, v1, n, hi, ws, 0);
      else if (kind == 3) side = damar_radix_sort_keys_u64(k0, k1, n, lo, hi, ws, 0);
      else damar_radix_sort_split_u64(k0, k1, n, lo, hi, oh, ol, ws, 0);
      HIP_CHECK(hipDeviceSynchronize());
      std::vector<u64> ok(n);
      std::vector<u32> ov(n), h1(n), h2(n);
      HIP_CHECK(hipMemcpy(ok.data(), side ? k1 : k0, 8 * n, hipMemcpyDeviceToHost));
      HIP_CHECK(hipMemcpy(ov.data(), side ? v1 : v0, 4 * n, hipMemcpyDeviceToHost));
      HIP_CHECK(hipMemcpy(h1.data(), oh, 4 * n, hipMemcpyDeviceToHost));
      HIP_CHECK(hipMemcpy(h2.data(), ol, 4 * n, hipMemcpyDeviceToHost));
      for (u64 i = 0; i < n && !bad; i++)
        { const u64 want = hk[ord[i]];
          bool good = (kind == 4) ? (h1[i] == (u32) (want >> 32) && h2[i] == (u32) want)
                                  : (ok[i] == want && (kind != 2 || ov[i] == ord[i]));
          if (!good)
            { fprintf(stderr, "kind %d n %llu bits [%d,%d): item %llu differs\n", kind, (unsigned long long) n, lo, hi, (unsigned long long) i); bad = 1; }
        }
      hipFree(k0); hipFree(k1); hipFree(v0); hipFree(v1); hipFree(oh); hipFree(ol);
    }
  if (check_err(ws))
    { fprintf(stderr, "kind %d n %llu: look-back timeout flagged\n", kind, (unsigned long long) n); bad = 1; }
  hipFree(ws);
  return bad;
}

static int do_check(void)
{ const u64 sizes[] = { 1, 2, 63, 64, 65, 255, 4095, 4096, 4097, 8191, 8193, 100000, 1000003, 5000011 };
  int nbad = 0, ncase = 0;
  for (u64 n : sizes)
    for (int skew = 0; skew < 3; skew++)
      { if (n > 200000 && skew == 2) continue;
        nbad += check_one(0, n, 0, 28, skew);  ncase++;
        nbad += check_one(0, n, 0, 13, skew);  ncase++;
        nbad += check_one(1, n, 0, 32, skew);  ncase++;
        nbad += check_one(2, n, 0, 43, skew);  ncase++;
        nbad += check_one(2, n, 0, 64, skew);  ncase++;
        nbad += check_one(3, n, 15, 58, skew); ncase++;
        nbad += check_one(3, n, 3, 8, skew);   ncase++;
        nbad += check_one(4, n, 32, 60, skew); ncase++;
        nbad += check_one(4, n, 32, 40, skew); ncase++;
        if (nbad) { printf("FAILED after %d cases\n", ncase); return 1; }
      }
  printf("check ok: %d cases (threads %d, items %d)\n", ncase, sort_threads(), sort_threads() == 1024 ? 8 : 16);
  return 0;
}

/* time one sort shape; returns ms per sort */
static double time_sort(int kind, u64 n, int lo, int hi, int reps)
{ std::vector<u64> hk(n);
  for (u64 i = 0; i < n; i++) hk[i] = rnd();
  void *ws = dev<char>(damar_sort_workspace_bytes(n));
  u64 *src = dev<u64>(n), *k0 = dev<u64>(n), *k1 = dev<u64>(n);
  u32 *v0 = dev<u32>(n), *v1 = dev<u32>(n);
  HIP_CHECK(hipMemcpy(src, hk.data(), 8 * n, hipMemcpyHostToDevice));
  hipEvent_t e0, e1;
  hipEventCreate(&e0); hipEventCreate(&e1);
  double tot = 0;
  for (int r = 0; r < reps + 1; r++)
    { HIP_CHECK(hipMemcpyAsync(k0, src, (kind == 0 ? 4 : 8) * n, hipMemcpyDeviceToDevice, 0));
      hipEventRecord(e0, 0);
      if (kind == 0) damar_radix_sort_u32((u32 *) k0, v0, (u32 *) k1, v1, n, hi, ws, 0);
      else if (kind == 2) damar_radix_sort_u64(k0, v0, k1, v1, n, hi, ws, 0);
      else if (kind == 3) damar_radix_sort_keys_u64(k0, k1, n, lo, hi, ws, 0);
      else damar_radix_sort_split_u64(k0, k1, n, lo, hi, v0, v1, ws, 0);
      hipEventRecord(e1, 0);
      HIP_CHECK(hipEventSynchronize(e1));
      float ms; hipEventElapsedTime(&ms, e0, e1);
      if (r > 0) tot += ms;
    }
  if (check_err(ws)) { fprintf(stderr, "look-back timeout flagged\n"); exit(1); }
#ifdef OS_STATS
  { u32 e[4];
    HIP_CHECK(hipMemcpy(e, damar_sort_error_word(ws), 16, hipMemcpyDeviceToHost));
    printf("   look-back of digit 0, last sort: %.2f steps and %.2f empty polls per tile (%u tiles)\n", e[1] / (double) e[3], e[2] / (double) e[3], e[3]);
  }
#endif
  hipFree(ws); hipFree(src); hipFree(k0); hipFree(k1); hipFree(v0); hipFree(v1);
  return tot / reps;
}

static void report(const char *name, int kind, u64 n, int lo, int hi, int reps)
{ const int P = (hi - lo + 7) / 8;
  const double ms = time_sort(kind, n, lo, hi, reps);
  const double item = (kind == 0) ? 8 : (kind == 2 ? 12 : 8);                   /* bytes per item as laid out here */
  const double keyb = (kind == 0) ? 4 : 8;
  const double moved = (double) n * (keyb + 2 * item * P);
  const double algo  = (double) n * 32.0 * P;                                    /* 16 B read + 16 B written per digit */
  printf("%-34s n=%9llu P=%d  %7.3f ms   algorithmic %6.0f GB/s   moved %6.0f GB/s\n", name, (unsigned long long) n, P, ms,
         algo / ms * 1e-6, moved / ms * 1e-6);
}

/* a block of random reads in HBM as shim.hip lays it out (boff, coarse, bases with their 4s, 2-bit copy, position words) */
struct BenchBlock { DevBlock d;  u8 *bases;  u32 *pk, *boff, *coarse;  u32 nk; };

static BenchBlock make_block(const std::vector<u32> &lens, int kmer)
{ BenchBlock b;
  const u32 n = (u32) lens.size();
  std::vector<u32> boff(n + 1);
  u32 total = 0, maxlen = 0;
  for (u32 i = 0; i < n; i++)
    { boff[i] = total;  total += lens[i] + 1;  maxlen = std::max(maxlen, lens[i]); }
  boff[n] = total;
  std::vector<u8> hb((size_t) total + 192, 4);
  for (u32 i = 0; i < n; i++)
    { u64 x = 0;
      for (u32 j = 0; j < lens[i]; j++)
        { if ((j & 31) == 0) x = rnd();
          hb[64 + boff[i] + j] = (u8) (x & 3);  x >>= 2;
        }
    }
  const size_t nq = ((size_t) total >> COARSE_SHIFT) + 2;
  std::vector<u32> coarse(nq);
  for (size_t q = 0, r = 0; q < nq; q++)
    { while (r + 1 < n && (u64) boff[r + 1] <= ((u64) q << COARSE_SHIFT)) r += 1;
      coarse[q] = (u32) r;
    }
  b.bases = dev<u8>(hb.size());  b.boff = dev<u32>(n + 1);  b.coarse = dev<u32>(nq);
  b.pk = dev<u32>(2 * (size_t) damar_pack_words(total));
  HIP_CHECK(hipMemcpy(b.bases, hb.data(), hb.size(), hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(b.boff, boff.data(), 4 * (size_t) (n + 1), hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(b.coarse, coarse.data(), 4 * nq, hipMemcpyHostToDevice));
  damar_launch_pack_bases(b.bases + 64, total, b.pk + PK_PAD, 0);
  HIP_CHECK(hipDeviceSynchronize());
  memset(&b.d, 0, sizeof(b.d));
  b.d.bases = b.bases + 64;  b.d.pk = b.pk + PK_PAD;  b.d.boff = b.boff;  b.d.coarse = b.coarse;
  b.d.nreads = n;  b.d.total = total;  b.d.maxlen = (int) maxlen;
  int pb = 1;
  while ((1u << pb) < maxlen + 1) pb += 1;
  b.d.rpbits = pb;
  b.nk = total - (u32) kmer * n;
  return b;
}

/* both index sorts of a block; ms[0]: kmer_tuples + sort, ms[1]: the sort that makes its keys; 1 if the results differ */
static int index_both(const BenchBlock &b, int kmer, int reps, double ms[2])
{ const u64 n = b.nk;
  void *ws = dev<char>(damar_sort_workspace_bytes(n));
  u64 *k0 = dev<u64>(n), *k1 = dev<u64>(n);
  u32 *oh[2] = { dev<u32>(n), dev<u32>(n) }, *ol[2] = { dev<u32>(n), dev<u32>(n) };
  KmerKeys src;
  src.blk = b.d;  src.kmer = kmer;
  hipEvent_t e0, e1;
  hipEventCreate(&e0); hipEventCreate(&e1);
  for (int way = 0; way < 2; way++)
    { double tot = 0;
      for (int r = 0; r < reps + 1; r++)
        { hipEventRecord(e0, 0);
          if (way == 0)
            { damar_launch_kmer_tuples(&b.d, kmer, (u32) n, k0, 0, NULL, 0);
              damar_radix_sort_split_u64(k0, k1, n, 32, 32 + 2 * kmer, oh[0], ol[0], ws, 0);
            }
          else
            damar_radix_sort_split_kmers(&src, k0, k1, n, oh[1], ol[1], ws, 0);
          hipEventRecord(e1, 0);
          HIP_CHECK(hipEventSynchronize(e1));
          float t; hipEventElapsedTime(&t, e0, e1);
          if (r > 0) tot += t;
          if (check_err(ws)) { fprintf(stderr, "look-back timeout flagged\n"); exit(1); }
        }
      ms[way] = reps > 0 ? tot / reps : 0;
    }
  int bad = 0;
  { std::vector<u32> a(n), c(n);
    for (int h = 0; h < 2 && !bad; h++)
      { HIP_CHECK(hipMemcpy(a.data(), h ? ol[0] : oh[0], 4 * n, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(c.data(), h ? ol[1] : oh[1], 4 * n, hipMemcpyDeviceToHost));
        bad = memcmp(a.data(), c.data(), 4 * n) != 0;
      }
  }
  hipFree(ws); hipFree(k0); hipFree(k1); hipFree(oh[0]); hipFree(oh[1]); hipFree(ol[0]); hipFree(ol[1]);
  return bad;
}

static void free_block(BenchBlock &b) { hipFree(b.bases); hipFree(b.pk); hipFree(b.boff); hipFree(b.coarse); }

static int do_index(int reps)
{ const int kmer = 14;
  double ms[2];
  { /* reads of k - 1 bases (no k-mer), k (one) ... k + 6: read borders in every round of 64 slots */
    std::vector<u32> lens(40000);
    for (auto &x : lens) x = (u32) (kmer - 1 + rnd() % 8);
    BenchBlock b = make_block(lens, kmer);
    const int bad = index_both(b, kmer, 0, ms);
    free_block(b);
    if (bad) { printf("index FAILED: short reads, made keys differ from kmer_tuples\n"); return 1; }
  }
  std::vector<u32> lens(13500);
  for (auto &x : lens) x = (u32) (6000 + rnd() % 8000);
  BenchBlock b = make_block(lens, kmer);
  if (index_both(b, kmer, reps, ms))
    { printf("index FAILED: made keys differ from kmer_tuples\n"); return 1; }
  const int    P  = (2 * kmer + 7) / 8;
  const double nk = b.nk, pkb = b.d.total / 4.0;
  const double moved[2] = { pkb + 8 * nk + 8 * nk + P * 16 * nk, pkb + (pkb + 8 * nk) + (P - 1) * 16 * nk };
  const char  *name[2]  = { "index build, kmer_tuples + sort", "index build, sort makes its keys" };
  for (int w = 0; w < 2; w++)
    printf("%-34s n=%9u P=%d  %7.3f ms   moved %6.2f GB = %6.0f GB/s\n", name[w], b.nk, P, ms[w], moved[w] * 1e-9, moved[w] / ms[w] * 1e-6);
  free_block(b);
  return 0;
}

/* the ordering before order_waves / order_long, for the comparison: a workgroup of 256 threads per work item whatever its
   length, every wavefront finds the length for itself, the sort in LDS with a barrier per step */
__global__ __launch_bounds__(256)
void order_sort_old(u64 *__restrict__ keys, u64 nhits, int ppos, int dbits, const u32 *__restrict__ work, u32 nwork)
{ __shared__ u64 rk[OR_MAX];
  __shared__ u32 ck[OR_MAX];
  const int  l = lane_id();
  const u64  pmask = (1ull << ppos) - 1;
  if (blockIdx.x >= nwork)
    return;
  const u64 i = work[blockIdx.x];
  const u32 n = run_length(keys, nhits, i, ppos + dbits, OR_MAX, l, keys[i] >> (ppos + dbits));
  if (n < 2 || n > OR_MAX)
    return;
  u32 P = 2;
  while (P < n)
    P <<= 1;
  for (u32 j = threadIdx.x; j < P; j += 256)
    { if (j < n)
        { const u64 k = keys[i + j];
          rk[j] = k;
          ck[j] = ((u32) ((k >> dbits) & pmask) << 11) | j;
        }
      else
        ck[j] = 0xffffffffu;
    }
  __syncthreads();
  for (u32 k2 = 2; k2 <= P; k2 <<= 1)
    for (u32 jj = k2 >> 1; jj > 0; jj >>= 1)
      { for (u32 t = threadIdx.x; t < (P >> 1); t += 256)
          { const u32 ix = ((t & ~(jj - 1)) << 1) | (t & (jj - 1)), px = ix | jj;
            const bool up = (ix & k2) == 0;
            const u32 a = ck[ix], c = ck[px];
            if ((a > c) == up)
              { ck[ix] = c;  ck[px] = a; }
          }
        __syncthreads();
      }
  for (u32 j = threadIdx.x; j < n; j += 256)
    keys[i + j] = rk[ck[j] & 2047u];
}

/* shape 0: runs of 8 seeds, 1: of 100, 2: 80 % of 4 .. 64, 19 % of 65 .. 512, 1 % of 513 .. 2048 */
static int order_shape(int shape, int reps)
{ const int ppos = 15, dbits = 15;
  const u32 nruns = 45000;
  std::vector<u64> hk;
  std::vector<u32> hw(nruns);
  for (u32 r = 0; r < nruns; r++)
    { u32 n = shape == 0 ? 8 : 100;
      if (shape == 2)
        { const u32 x = (u32) (rnd() % 100);
          n = x < 80 ? 4 + (u32) (rnd() % 61) : (x < 99 ? 65 + (u32) (rnd() % 448) : 513 + (u32) (rnd() % 1536));
          if (r == 7) n = 2048;
        }
      hw[r] = (u32) hk.size();
      for (u32 j = 0; j < n; j++)
        hk.push_back(((u64) r << (ppos + dbits)) | (rnd() & ((1ull << (ppos + dbits)) - 1)));
    }
  const u64 nhits = hk.size();
  std::vector<u64> want(hk);
  for (u32 r = 0; r < nruns; r++)
    std::stable_sort(want.begin() + hw[r], want.begin() + (r + 1 < nruns ? hw[r + 1] : nhits),
                     [&](u64 a, u64 b) { return ((a >> dbits) & 0x7fff) < ((b >> dbits) & 0x7fff); });
  u64 *src = dev<u64>(nhits), *k = dev<u64>(nhits);
  u32 *w = dev<u32>(nruns);
  void *sc = dev<char>(damar_order_runs_scratch_bytes(nhits));
  HIP_CHECK(hipMemcpy(src, hk.data(), 8 * nhits, hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(w, hw.data(), 4 * nruns, hipMemcpyHostToDevice));
  hipEvent_t e0, e1;
  hipEventCreate(&e0); hipEventCreate(&e1);
  const char *shapes[3] = { "runs of 8", "runs of 100", "mixed, tail to 2048" };
  int bad = 0;
  for (int way = 0; way < 2 && !bad; way++)
    { double tot = 0;
      for (int r = 0; r < reps + 1; r++)
        { HIP_CHECK(hipMemcpyAsync(k, src, 8 * nhits, hipMemcpyDeviceToDevice, 0));
          hipEventRecord(e0, 0);
          if (way == 0)
            hipLaunchKernelGGL(order_sort_old, dim3(nruns), dim3(256), 0, 0, k, nhits, ppos, dbits, (const u32 *) w, nruns);
          else
            damar_launch_order_runs(k, nhits, ppos, dbits, w, nruns, sc, 0);
          hipEventRecord(e1, 0);
          HIP_CHECK(hipEventSynchronize(e1));
          float t; hipEventElapsedTime(&t, e0, e1);
          if (r > 0) tot += t;
        }
      std::vector<u64> got(nhits);
      HIP_CHECK(hipMemcpy(got.data(), k, 8 * nhits, hipMemcpyDeviceToHost));
      bad = memcmp(got.data(), want.data(), 8 * nhits) != 0;
      const double ms = reps > 0 ? tot / reps : 0;
      printf("order %-20s %5u runs, %8llu seeds  %-22s %7.3f ms  %7.1f M runs/s%s\n", shapes[shape], nruns, (unsigned long long) nhits,
             way ? "order_waves+order_long" : "workgroup per run", ms, ms > 0 ? nruns / ms * 1e-3 : 0., bad ? "  WRONG ORDER" : "");
    }
  hipFree(src); hipFree(k); hipFree(w); hipFree(sc);
  return bad;
}

static int do_order(int reps)
{ int bad = 0;
  for (int shape = 0; shape < 3; shape++)
    bad |= order_shape(shape, reps);
  return bad;
}

int main(int argc, char **argv)
{ if (argc > 1 && strcmp(argv[1], "check") == 0)
    return do_check();
  if (argc > 1 && strcmp(argv[1], "order") == 0)
    return do_order(argc > 2 ? atoi(argv[2]) : 20);
  if (argc > 1 && strcmp(argv[1], "index") == 0)
    return do_index(argc > 2 ? atoi(argv[2]) : 10);
  const int reps = argc > 2 ? atoi(argv[2]) : 10;
  printf("variant: shape %d (1024: threads x 8 keys, 512 / 256: threads x 16 keys), minw %d\n", sort_threads(), OS_MINW);
  report("kmer index, packed u64 split", 4, 135000000ull, 32, 60, reps);
  report("kmer index, u32 + u32",        0, 135000000ull, 0, 28, reps);
  report("seed pairs, packed u64",       3, 61000000ull, 15, 58, reps);
  report("seed pairs, u64 + u32",        2, 61000000ull, 0, 43, reps);
  report("seed pairs, packed u64 (c4)",  3, 6000000ull, 16, 58, reps);
  return 0;
}
