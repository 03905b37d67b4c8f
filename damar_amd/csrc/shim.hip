/* shim.hip -- the C-ABI of libdamar_hip.so: the reference's three-function filter
 * interface (dalign/filter.h:64-70) implemented on one MI355X.
 *
 *   Set_Filter_Params  filter.c:171-201
 *   Sort_Kmers         filter.c:753-994   -> damar_block_upload + damar_index_build
 *   Match_Filter       filter.c:2519-2929 -> damar_match (+ ownership of btable)
 *
 * Everything compute-heavy is a HIP kernel (kernels/ *.hip); this file owns device
 * memory, orders the launches on one stream, copies the alignment records back and
 * hands them to the per-read-pair host tail (host/tail.cpp -> host/redundancy.c -> host/las.c).  There is no CPU
 * fallback: without a HIP device every entry point fails loudly.
 */
#include <algorithm>
#include <vector>
#include <deque>
#include <string>
#include <thread>
#include <atomic>
#include <mutex>
#include <condition_variable>
#include <functional>
#include <string.h>
#include <unistd.h>
#include <limits.h>

#include "kernels/dev_common.h"
#include <ctype.h>
#include "kernels/kernels.h"

extern "C" {
#include "damar_filter.h"
#include "damar_hip.h"
#include "host/damar_host.h"
}
#include "shim_internal.h"     /* what of this file the tool stages (stages/ *.hip) share */

#define MAXGRAM 10000          /* filter.c:71 */

/***** globals shared with the caller (filter.h:54-62 / daligner.c:131-140) *****************/

extern "C" {
int    BIASED    = 0;
int    VERBOSE   = 0;
int    MINOVER   = 2000;       /* 2 * (-l 1000), daligner.c:695, 861 */
int    HGAP_MIN  = 0;
int    SYMMETRIC = 1;
int    IDENTITY  = 0;
uint64 MEM_LIMIT    = ~0ull;   /* replaced by the physical memory size at first use */
uint64 MEM_PHYSICAL = ~0ull;
}

static int P_kmer = 14, P_hitmin = 35, P_binshift = 6, P_suppress = 0, P_nshift = 2;
static u32 P_bread_lo = 0, P_bread_hi = 0xffffffffu;      /* damar_set_bread_range */

/* Restrict the following damar_match / Match_Filter calls to the read pairs whose B read (block-local
 * index) lies in [lo, hi): the index merge and the seed sort still see the whole block pair, so the seed
 * list, the reference's thread slices (filter.c:2804-2816) and with them every record of the range are
 * exactly those of the unrestricted call.  A multi-GPU scheduler splits one block pair over several GPUs
 * this way; the parts' files merge into the unsplit files.  hi < 0 lifts the restriction. */
extern "C" void damar_set_bread_range(int lo, int hi)
{ P_bread_lo = lo < 0 ? 0u : (u32) lo;
  P_bread_hi = hi < 0 ? 0xffffffffu : (u32) hi;
}

extern "C" int Set_Filter_Params(int kmer, int binshift, int suppress, int hitmin, int nthreads)
{ if (kmer <= 1)
    return 1;
  P_kmer = kmer;  P_binshift = binshift;  P_suppress = suppress;  P_hitmin = hitmin;
  P_nshift = 0;
  while ((2 << P_nshift) <= nthreads)
    P_nshift += 1;
  return 0;
}

/***** device state ***************************************************************************/

static int          G_ready = 0;
hipStream_t         G_st;                   /* the seed stream (shim_internal.h) */
static hipStream_t   G_copy;                /* record downloads of the asynchronous mode */
static hipStream_t   G_rep;                 /* report launches of the asynchronous mode: beside the next comparisons' seed stages */
static hipStream_t   G_ctl;                 /* small downloads (a launch's counters) that must not queue behind anything */
static std::thread  *G_late = NULL;         /* creates G_copy, G_rep, G_ctl behind damar_hip_init (see there) */
static std::mutex    G_late_mu;
static std::atomic<int> G_late_pending(0);
static hipStream_t preload_stream(void);
void late_streams(void)                     /* before the first use of G_copy / G_rep / G_ctl */
{ if (G_late_pending.load(std::memory_order_acquire) == 0)
    return;
  std::lock_guard<std::mutex> lk(G_late_mu);
  if (G_late != NULL)
    { G_late->join();
      delete G_late;
      G_late = NULL;
      G_late_pending.store(0, std::memory_order_release);
    }
}
/* The helper threads of this library (the start-up thread above, the allocation of the second landing buffer) are inside
   HIP calls; a process that leaves through exit() -- an error path of the caller, a plan with nothing to compare -- would
   run the runtime's exit-time teardown beside them.  Registered with atexit by damar_hip_init and called by
   damar_set_async(0): they are joined first. */
static void helpers_join(void);
static hipEvent_t    G_front_done;          /* the seed stages a report launch reads from are complete */
static hipEvent_t    G_rep_done;            /* the report launch in flight is complete (DAMAR_OVERLAP=2) */
static hipEvent_t    G_report_done;
static hipEvent_t    G_set_d2h[2];
static hipEvent_t    G_last_d2h[2] = { NULL, NULL };   /* per set of record buffers: the download the next kernel that writes
                                                          into the set must not overtake */
hipDeviceProp_t G_prop;
static hipEvent_t   G_ev[24];
static double       G_ms[DAMAR_T_COUNT];
static int          G_limit = 0;          /* the mutual-count cap the last Match_Filter used */
static double       H_ms[8];              /* host wall clock per phase (DAMAR_HOSTPROF=1 prints them at drain) */
static const char  *H_name[8] = { "index_build", "match:front", "match:order", "match:report", "match:d2h",
                                  "match:submit", "match:total", "final_drain" };
static int    ilog2_ceil(u64 n);

/* The filter parameters and option globals a comparison was set up under (filter.h:54-62).  A report launch may be made --
   or made again after an overflow -- during a LATER call, after the caller has moved on to other options: launches and
   host tails use this snapshot, taken when the comparison's seed stage ran, never the globals of the moment. */
struct JobParams
{ int kmer, hitmin, binshift, symmetric, minover, hgap_min; };

static JobParams params_now(void)
{ JobParams p;
  p.kmer = P_kmer;  p.hitmin = P_hitmin;  p.binshift = P_binshift;
  p.symmetric = SYMMETRIC;  p.minover = MINOVER;  p.hgap_min = HGAP_MIN;
  return p;
}


static int64        G_cnt[8];

struct Arena { char *base; size_t cap, top; };
static Arena G_work = { NULL, 0, 0 };       /* per-call temporaries, grow-only */
static Arena G_hitsJ[DAMAR_MAX_JOBS];       /* sorted seed pairs of the comparisons of the current report launch, one arena each
                                               (12 B per seed pair: what the report kernel reads) */
static Arena G_ordJ[DAMAR_MAX_JOBS];        /* their work lists and processing orders   */
static Arena G_tmp2 = { NULL, 0, 0 };       /* the same for what is left after the early cut */
static Arena G_tmp  = { NULL, 0, 0 };       /* sort ping-pong partner, flags, scan space of the seed stage: shared by the
                                               comparisons (the stream orders them), 20 B per seed pair */

static void *dmalloc(size_t n)
{ void *p = NULL;
  static int prof = -1;
  if (prof < 0)
    prof = getenv("DAMAR_HOSTPROF") != NULL;
  const double t0 = prof ? now_ms() : 0.;
  HIP_CHECK(hipMalloc(&p, n ? n : 16));
  if (prof && now_ms() - t0 > 50.)            /* the driver's occasional multi-second allocations */
    fprintf(stderr, "damar: hipMalloc of %.3f GB took %.0f ms\n", n / 1073741824., now_ms() - t0);
  return p;
}

/* The k-mer index arrays (8 B per k-mer) come and go with every index:
 * hipMalloc / hipFree of such sizes costs tens of milliseconds each and synchronises the device,
 * so released buffers are parked here and handed out again (best fit within 25 % slack).  The
 * pool is bounded; what does not fit is really freed. */
struct PoolBuf { void *p; size_t n; };
static std::vector<PoolBuf> &DP_free = *new std::vector<PoolBuf>();
static size_t DP_bytes = 0;
static const size_t DP_LIMIT = (size_t) 48 << 30;

static void *dpool_get(size_t n, size_t *got)
{ int best = -1;
  for (size_t i = 0; i < DP_free.size(); i++)
    if (DP_free[i].n >= n && DP_free[i].n <= n + (n >> 2) + (1 << 20) && (best < 0 || DP_free[i].n < DP_free[best].n))
      best = (int) i;
  if (best >= 0)
    { PoolBuf b = DP_free[best];
      DP_free.erase(DP_free.begin() + best);
      DP_bytes -= b.n;
      *got = b.n;
      return b.p;
    }
  *got = n;
  return dmalloc(n);
}

static void dpool_put(void *p, size_t n)
{ if (p == NULL)
    return;
  if (DP_bytes + n > DP_LIMIT || DP_free.size() >= 64)
    { HIP_CHECK(hipFree(p));
      return;
    }
  PoolBuf b = { p, n };
  DP_free.push_back(b);
  DP_bytes += n;
}

static void arena_reserve(Arena *a, size_t need)
{ if (need <= a->cap)
    { a->top = 0;
      return;
    }
  if (a->base)
    { HIP_CHECK(hipStreamSynchronize(G_st));
      HIP_CHECK(hipFree(a->base));
    }
  a->cap  = need + (need >> 3) + (1u << 20);
  a->base = (char *) dmalloc(a->cap);
  a->top  = 0;
}

static void *arena_take(Arena *a, size_t n)
{ size_t at = (a->top + 255) & ~(size_t) 255;
  if (at + n > a->cap)
    { fprintf(stderr, "damar: internal error, device arena overflow (%zu + %zu > %zu)\n", at, n, a->cap);
      die();
    }
  a->top = at + n;
  return a->base + at;
}

static size_t pad256(size_t n) { return (n + 511) & ~(size_t) 255; }
/* one bit per seed in whole tiles of DAMAR_SCAN_TILE (pair_heads_mark / pair_work_mark write all 64 words of a tile) */
static size_t bit_words_bytes(u64 n) { return (size_t) ((n + DAMAR_SCAN_TILE - 1) / DAMAR_SCAN_TILE) * (DAMAR_SCAN_TILE / 8); }

static int G_device = 0;      /* the device of this process; threads that touch HIP select it first */

/* NUMA node of the host memory next to GPU `device` (its PCI function's numa_node in sysfs), or -1 when the host says
   nothing.  Makes the HIP runtime start but allocates nothing: a node worker calls it BEFORE damar_hip_init, binds its
   threads and its memory policy to that node, and only then lets the library create streams and pinned landing buffers. */
extern "C" int damar_hip_numa_node(int device)
{ int ndev = 0;
  char bus[64] = "", path[160];
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
    return -1;
  if (hipDeviceGetPCIBusId(bus, (int) sizeof(bus), device) != hipSuccess || bus[0] == 0)
    return -1;
  for (char *c = bus; *c; c++)
    *c = (char) tolower(*c);
  snprintf(path, sizeof(path), "/sys/bus/pci/devices/%s/numa_node", bus);
  FILE *f = fopen(path, "r");
  int node = -1;
  if (f != NULL)
    { if (fscanf(f, "%d", &node) != 1)
        node = -1;
      fclose(f);
    }
  return node;
}

extern "C" int damar_hip_init(int device)
{ int ndev = 0;
  const bool iprof = getenv("DAMAR_INITPROF") != NULL;      /* where the bring-up time goes, on stderr */
  const double ip0 = now_ms();
#define INIT_MARK(what) do { if (iprof) fprintf(stderr, "init: +%.1f ms %s\n", now_ms() - ip0, what); } while (0)
  hipError_t e = hipGetDeviceCount(&ndev);
  INIT_MARK("hipGetDeviceCount");
  if (e != hipSuccess || ndev <= 0)
    { fprintf(stderr, "damar: FATAL: no HIP device visible (%s); libdamar_hip has no CPU fallback\n",
              hipGetErrorString(e));
      die();
    }
  if (device < 0 || device >= ndev)
    { fprintf(stderr, "damar: FATAL: device %d requested, %d present\n", device, ndev);
      die();
    }
  if (G_ready && device != G_device)
    { /* the streams, events and every pooled buffer of this process live on the first device: a second one
         would launch on streams of the first with memory of the second */
      fprintf(stderr, "damar: FATAL: device %d requested after the library was initialised on device %d "
                      "(one GPU per process)\n", device, G_device);
      die();
    }
  HIP_CHECK(hipSetDevice(device));
  G_device = device;
  HIP_CHECK(hipGetDeviceProperties(&G_prop, device));
  INIT_MARK("hipSetDevice + hipGetDeviceProperties");
  if (!G_ready)
    { if (strncmp(G_prop.gcnArchName, "gfx950", 6) != 0 && getenv("DAMAR_ANY_ARCH") == NULL)
        { fprintf(stderr, "damar: FATAL: device %d is %s; the kernels of this library are built for gfx950 (MI355X)\n",
                  device, G_prop.gcnArchName);
          die();
        }
      /* A stream costs 10 - 20 ms to create (a hardware queue each), a file's code object 4 - 10 ms to load, the first
         host-to-device copy of a process another 10 - 15 ms (tools/startup.hip, scripts/gpu_hiptrace.sh,
         profiles/r05_startup.txt) -- and a cold command is 0.25 s of kernels.  A start-up thread does, while this one
         creates the main stream and returns to its caller: the preload stream the block readers are waiting for and a
         first small copy on it, the seed side's code objects in the order a job needs them, the copy / report /
         control streams (first used when the first report launch is due: late_streams() joins the thread), the
         report kernel's code object. */
      G_late_pending.store(1, std::memory_order_release);
      G_late = new std::thread([device]()
        { const double t0 = now_ms();
          HIP_CHECK(hipSetDevice(device));
          { hipStream_t ps = preload_stream();
            void *d = NULL;
            static char warm[4096];
            HIP_CHECK(hipMalloc(&d, sizeof(warm)));
            HIP_CHECK(hipMemcpyAsync(d, warm, sizeof(warm), hipMemcpyHostToDevice, ps));
            HIP_CHECK(hipStreamSynchronize(ps));
            HIP_CHECK(hipFree(d));
          }
          const double t1 = now_ms();
          damar_preload_index();
          damar_preload_sort();
          damar_preload_merge();
          damar_preload_scan();
          const double t2 = now_ms();
          HIP_CHECK(hipStreamCreate(&G_copy));
          { /* EXPERIMENT (profiles/r06_sweeps.txt): the report stream on DAMAR_REPORT_CUS of the 256 CUs, so
               that the one-wavefront-per-tile kernels of the seed stream do not queue for wave slots behind a report launch.
               DAMAR_REPORT_CUPAT=1 spreads the CUs left out over the mask instead of taking them off its end. */
            const char *e = getenv("DAMAR_REPORT_CUS");
            const int ncu = G_prop.multiProcessorCount, want = e ? atoi(e) : 0;
            if (want > 0 && want < ncu)
              { const int pat = getenv("DAMAR_REPORT_CUPAT") ? atoi(getenv("DAMAR_REPORT_CUPAT")) : 0;
                std::vector<uint32_t> mask((size_t) (ncu + 31) / 32, 0u);
                for (int i = 0; i < ncu; i++)
                  { const bool on = pat ? ((long long) (i + 1) * want / ncu != (long long) i * want / ncu) : (i < want);
                    if (on)
                      mask[(size_t) i / 32] |= 1u << (i % 32);
                  }
                HIP_CHECK(hipExtStreamCreateWithCUMask(&G_rep, (uint32_t) mask.size(), mask.data()));
              }
            else
              HIP_CHECK(hipStreamCreate(&G_rep));
          }
          HIP_CHECK(hipStreamCreate(&G_ctl));
          const double t3 = now_ms();
          damar_preload_report();
          if (getenv("DAMAR_INITPROF") != NULL)
            fprintf(stderr, "init: start-up thread: preload stream + first copy %.1f ms, code objects of the seed side %.1f ms, three "
                            "streams %.1f ms, report code object %.1f ms\n", t1 - t0, t2 - t1, t3 - t2, now_ms() - t3);
        });
      HIP_CHECK(hipStreamCreate(&G_st));
      INIT_MARK("first stream");
      { /* which seed-side kernels raise their wave priority (kernels/kernels.h SEED_PRIO): 1 = sorts, 2 = merge and
           work list, 4 = k-mer tuples.  Config-2 step on three boxes (profiles/r03_sweeps.txt): none 398 / 415 / 434 ms,
           sorts only 403 / 405, all 409 / 413 / 408: the sorts (a chain of tiles through the look-back) are the kernels
           whose time beside a report launch varies threefold from box to box, and with priority it does not. */
        const char *e = getenv("DAMAR_SEED_PRIO");
        const int mask = e ? atoi(e) : 1;
        damar_sort_set_prio(mask & 1);
        damar_merge_set_prio((mask >> 1) & 1);
        damar_index_set_prio((mask >> 2) & 1);
      }
      HIP_CHECK(hipEventCreate(&G_front_done));
      HIP_CHECK(hipEventCreateWithFlags(&G_rep_done, hipEventDisableTiming));
      HIP_CHECK(hipEventCreateWithFlags(&G_set_d2h[0], hipEventDisableTiming));
      HIP_CHECK(hipEventCreateWithFlags(&G_set_d2h[1], hipEventDisableTiming));
      HIP_CHECK(hipEventCreate(&G_report_done));
      for (int i = 0; i < 24; i++)
        HIP_CHECK(hipEventCreate(&G_ev[i]));
      if (MEM_PHYSICAL == ~0ull)
        { uint64 phys = (uint64) sysconf(_SC_PHYS_PAGES) * (uint64) sysconf(_SC_PAGESIZE);
          if (MEM_LIMIT == ~0ull)
            MEM_LIMIT = phys;
          MEM_PHYSICAL = phys;
        }
      G_ready = 1;
      atexit(helpers_join);
      INIT_MARK("events, done");
    }
#undef INIT_MARK
  return ndev;
}

static double Q_ms[4];      /* DAMAR_HOSTPROF: scratch_prepare, scratch_outputs, outside the library between two
                               damar_match_batch calls, from a report launch to the next comparison's first kernel */
static double Q_exit = 0, Q_flush = 0, Q_seg[4], Q_entry = 0;

static void hostprof_at_exit(void)
{ fprintf(stderr, "damar host wall ms (at exit):");
  for (int i = 0; i < 8; i++)
    fprintf(stderr, " %s=%.1f", H_name[i], H_ms[i]);
  fprintf(stderr, " | scratch_prepare=%.1f scratch_outputs=%.1f\n", Q_ms[0], Q_ms[1]);
}

void ensure_init(void)
{ if (!G_ready)
    { const char *d = getenv("DAMAR_DEVICE");
      damar_hip_init(d ? atoi(d) : 0);
      if (getenv("DAMAR_HOSTPROF"))
        atexit(hostprof_at_exit);
    }
}

static void finish_all(void);

extern "C" void damar_hip_sync(void)
{ ensure_init();
  finish_all();
  HIP_CHECK(hipDeviceSynchronize());
}

extern "C" const char *damar_hip_device_name(void)
{ static char name[400];
  ensure_init();
  snprintf(name, sizeof(name), "%s (%s, %d CUs)", G_prop.name[0] ? G_prop.name : "AMD GPU", G_prop.gcnArchName,
           G_prop.multiProcessorCount);
  return name;
}

/* A cold process pays ~25 ms per GB the first time its HBM footprint grows (the driver maps and clears new
 * memory; a buffer that is freed and allocated again is handed back at once: build/malloc_test.hip).  A command
 * that knows it will need tens of GB calls this early on a thread of its own, next to reading its input: the
 * footprint is grown and released there, and the allocations of the real work find it ready. */
extern "C" void damar_prewarm(int gigabytes)
{ ensure_init();
  HIP_CHECK(hipSetDevice(G_device));
  std::vector<void *> held;
  for (int g = 0; g < gigabytes; g += 2)
    { void *p = NULL;
      if (hipMalloc(&p, (size_t) 2 << 30) != hipSuccess)
        { (void) hipGetLastError();
          break;
        }
      held.push_back(p);
    }
  for (void *p : held)
    (void) hipFree(p);
}

static int G_debug = -1;
/* DAMAR_DEBUG=1: synchronise after every stage and name it on stderr, so that a device
 * fault can be attributed to the kernel that caused it. */
static void stage(const char *name)
{ if (G_debug < 0)
    G_debug = (getenv("DAMAR_DEBUG") != NULL);
  if (G_debug)
    { hipError_t e = hipStreamSynchronize(G_st);
      fprintf(stderr, "[damar] stage %-14s %s\n", name, hipGetErrorName(e));
      fflush(stderr);
    }
}
/* The host waits for a count from the device three times per comparison (seed pairs, work items, ...) with the stream's
   next kernels depending on it: hipStreamSynchronize sleeps until an interrupt wakes it, 30 - 45 us after the copy has
   landed (gaps on the seed stream in the kernel trace, config 4's first 24 blocks: 97 ms of 1 160).  DAMAR_SYNC_SPIN=1
   polls the stream instead: measured, config-4 lead leg 1.178 -> 1.153 s, config 2 and 3 unchanged (profiles/r06_sweeps.txt);
   not the default -- a polling thread per worker is a core less for the tails and writers of a node job. */
static void stream_wait(hipStream_t st)
{ static int spin = -1;
  if (spin < 0)
    { const char *e = getenv("DAMAR_SYNC_SPIN");
      spin = e ? atoi(e) : 0;
    }
  if (spin)
    { hipError_t q;
      while ((q = hipStreamQuery(st)) == hipErrorNotReady)
        __builtin_ia32_pause();
      HIP_CHECK(q);
      return;
    }
  HIP_CHECK(hipStreamSynchronize(st));
}

static void  tick(int i)            { HIP_CHECK(hipEventRecord(G_ev[i], G_st)); }
static void  tick_on(int i, hipStream_t st) { HIP_CHECK(hipEventRecord(G_ev[i], st)); }
static float lap(int i, int j)      { float ms = 0; HIP_CHECK(hipEventElapsedTime(&ms, G_ev[i], G_ev[j])); return ms; }
/* the four timer events of output set `oset` (G_ev[16 .. 23]): around its report kernel, around its download */
enum { SET_KERNEL_BEGIN = 0, SET_KERNEL_END = 1, SET_D2H_BEGIN = 2, SET_D2H_END = 3 };
static int   set_ev(int oset, int k) { return 16 + 4 * oset + k; }

extern "C" void damar_last_timings(double *ms)  { memcpy(ms, G_ms, sizeof(G_ms)); }
extern "C" void damar_last_counters(int64 *c)   { memcpy(c, G_cnt, sizeof(G_cnt)); }
extern "C" int  damar_last_limit(void)          { return G_limit; }
static int G_merge_flagged = -1;         /* tiles of the last COUNT sweep that the general kernel did; -1: not looked at */
extern "C" int  damar_last_merge_flagged(void)  { return G_merge_flagged; }

/***** blocks ************************************************************************************/

/* struct damar_dev_block: shim_internal.h */

static damar_dev_block *block_upload_on(const HITS_DB *block, hipStream_t st, const damar_packed *pk = NULL, int comp = 0);

extern "C" damar_dev_block *damar_block_upload(const HITS_DB *block)
{ ensure_init();
  return block_upload_on(block, G_st);
}

/* Blocks uploaded ahead of their Sort_Kmers call (the command-line driver prepares the next B block on a
   second thread): on their own stream, so the copy runs beside the kernels of the current block pair.
   Sort_Kmers takes a preloaded block by the address of its bases. */
static std::mutex PL_mu;
static std::vector<std::pair<const void *, damar_dev_block *>> PL_ready;
static hipStream_t PL_st = NULL;
static std::atomic<int> PL_state(0);         /* 0: nobody has asked for it, 1: being created (by the start-up thread of damar_hip_init or
                                                by the first caller), 2: there */
static hipStream_t preload_stream(void)
{ int s = PL_state.load(std::memory_order_acquire);
  if (s == 2)
    return PL_st;
  int zero = 0;
  if (s == 0 && PL_state.compare_exchange_strong(zero, 1))
    { HIP_CHECK(hipStreamCreateWithFlags(&PL_st, hipStreamNonBlocking));
      PL_state.store(2, std::memory_order_release);
      return PL_st;
    }
  while (PL_state.load(std::memory_order_acquire) != 2)
    usleep(50);
  return PL_st;
}

extern "C" void damar_block_preload(const HITS_DB *block)
{ ensure_init();
  HIP_CHECK(hipSetDevice(G_device));          /* the current device is a per-thread setting */
  (void) preload_stream();
  damar_dev_block *b = block_upload_on(block, PL_st);
  std::lock_guard<std::mutex> lk(PL_mu);
  PL_ready.push_back(std::make_pair((const void *) block->bases, b));
}

/* damar_block_upload on the preload stream, for a second host thread that prepares blocks ahead of the one that
 * launches the kernels (hipStreamSynchronize inside: the block is complete when this returns) */
extern "C" damar_dev_block *damar_block_upload_bg(const HITS_DB *block)
{ ensure_init();
  HIP_CHECK(hipSetDevice(G_device));          /* the current device is a per-thread setting */
  (void) preload_stream();
  return block_upload_on(block, PL_st);
}

/* A block that the host keeps packed (damar_read_block_packed: block->bases == NULL): the forward strand (comp 0) or the
 * reverse complement (comp 1) is unpacked on the device, on the preload stream like damar_block_upload_bg.  The host
 * tail needs the bases of a read pair only where two local alignments have to be bridged by a realignment (filter.c:1950
 * -2059, a few pairs in a thousand): it unpacks those reads out of the registered stretch (host_read). */
extern "C" damar_dev_block *damar_block_upload_packed(const HITS_DB *block, const damar_packed *pk, int comp)
{ ensure_init();
  HIP_CHECK(hipSetDevice(G_device));          /* the current device is a per-thread setting */
  (void) preload_stream();
  packed_register(block->reads, pk);
  return block_upload_on(block, PL_st, pk, comp);
}

/* the block is about to be closed: the tail must have drained (damar_async_drain) */
extern "C" void damar_packed_forget(const HITS_DB *block)
{ packed_forget(block->reads);
}

static damar_dev_block *take_preloaded(const HITS_DB *block)
{ std::lock_guard<std::mutex> lk(PL_mu);
  for (size_t i = 0; i < PL_ready.size(); i++)
    if (PL_ready[i].first == (const void *) block->bases)
      { damar_dev_block *b = PL_ready[i].second;
        PL_ready.erase(PL_ready.begin() + i);
        return b;
      }
  return NULL;
}

struct PackStage { u8 *raw; size_t nraw; u32 *foff; size_t nfoff; int64 holds; };
static thread_local PackStage TL_stage = { NULL, 0, NULL, 0, 0 };

/* pk != NULL: the block comes as its stretch of the .bps file and is unpacked (comp: into its reverse complement) on the
   device (kernels/kmer_index.hip unpack_bps); block->bases is not looked at then */
static damar_dev_block *block_upload_on(const HITS_DB *block, hipStream_t st, const damar_packed *pk, int comp)
{ damar_dev_block *b = (damar_dev_block *) calloc(1, sizeof(damar_dev_block));
  int    n = block->nreads;
  int64  total = block->reads[n].boff;
  if (total > 0x7fffffffll)
    { fprintf(stderr, "damar: Fatal error, DB blocks are greater than 2Gbp!\n");   /* filter.c:794-798 */
      die();
    }
  std::vector<u32> boff((size_t) n + 1);
  for (int i = 0; i <= n; i++)
    boff[i] = (u32) block->reads[i].boff;
  int minlen = 0x7fffffff;
  for (int i = 0; i < n; i++)
    minlen = std::min(minlen, (int) (boff[i + 1] - boff[i]) - 1);
  size_t nq = ((size_t) total >> COARSE_SHIFT) + 2;
  std::vector<u32> coarse(nq);
  { u32 r = 0;
    for (size_t q = 0; q < nq; q++)
      { u64 p = (u64) q << COARSE_SHIFT;
        while (r + 1 < (u32) n && (u64) boff[r + 1] <= p)
          r += 1;
        coarse[q] = r;
      }
  }
  b->bases_alloc = (u8 *) dmalloc((size_t) total + 192);      /* 64 B of padding on both sides */
  HIP_CHECK(hipMemsetAsync(b->bases_alloc, 4, (size_t) total + 192, st));
  b->boff   = (u32 *) dmalloc(sizeof(u32) * ((size_t) n + 1));
  b->coarse = (u32 *) dmalloc(sizeof(u32) * nq);
  if (pk == NULL)
    HIP_CHECK(hipMemcpyAsync(b->bases_alloc + 63, ((const char *) block->bases) - 1, (size_t) total + 1,
                             hipMemcpyHostToDevice, st));
  HIP_CHECK(hipMemcpyAsync(b->boff, boff.data(), sizeof(u32) * ((size_t) n + 1), hipMemcpyHostToDevice, st));
  HIP_CHECK(hipMemcpyAsync(b->coarse, coarse.data(), sizeof(u32) * nq, hipMemcpyHostToDevice, st));
  if (pk != NULL)
    { /* the stretch goes up once per host thread and block: a block's two strands are unpacked out of the same copy
         (TL_stage remembers what it holds).  The staging buffers belong to the thread and are never freed: a hipFree
         waits for every stream of the device, i.e. for the kernels of the thread that computes */
      DevBlock tmp;
      memset(&tmp, 0, sizeof(tmp));
      tmp.boff = b->boff;  tmp.coarse = b->coarse;  tmp.total = (u32) total;  tmp.nreads = (u32) n;
      if (TL_stage.holds != pk->serial)
        { if (TL_stage.nraw < (size_t) pk->nraw + 64)
            { if (TL_stage.raw) HIP_CHECK(hipFree(TL_stage.raw));
              TL_stage.nraw = (size_t) pk->nraw + ((size_t) pk->nraw >> 3) + 4096;
              TL_stage.raw  = (u8 *) dmalloc(TL_stage.nraw);
            }
          if (TL_stage.nfoff < (size_t) n + 1)
            { if (TL_stage.foff) HIP_CHECK(hipFree(TL_stage.foff));
              TL_stage.nfoff = (size_t) n + ((size_t) n >> 3) + 1024;
              TL_stage.foff  = (u32 *) dmalloc(sizeof(u32) * TL_stage.nfoff);
            }
          HIP_CHECK(hipMemcpyAsync(TL_stage.raw, pk->raw, (size_t) pk->nraw, hipMemcpyHostToDevice, st));
          HIP_CHECK(hipMemcpyAsync(TL_stage.foff, pk->foff, sizeof(u32) * (size_t) n, hipMemcpyHostToDevice, st));
          TL_stage.holds = pk->serial;
        }
      damar_launch_unpack_bps(TL_stage.raw, TL_stage.foff, &tmp, comp, b->bases_alloc + 64, st);
    }
  HIP_CHECK(hipStreamSynchronize(st));
  b->d.bases  = b->bases_alloc + 64;
  b->pk_alloc = (u32 *) dmalloc(sizeof(u32) * 2 * (size_t) damar_pack_words((u32) total));      /* forward, then reversed */
  b->d.pk     = b->pk_alloc + PK_PAD;
  b->d.rbias  = (u32) (16 * damar_pack_words((u32) total) + 16 * PK_PAD);
  damar_launch_pack_bases(b->d.bases, (u32) total, b->pk_alloc + PK_PAD, st);
  HIP_CHECK(hipStreamSynchronize(st));
  b->d.boff   = b->boff;
  b->d.coarse = b->coarse;
  for (int i = 0; i < 4; i++)
    b->freq[i] = block->freq[i];
  b->minlen = minlen;
  b->d.nreads = (u32) n;
  b->d.total  = (u32) total;
  b->d.maxlen = block->maxlen;
  /* position words of this block's k-mer indexes: read << rpbits | offset in the read when both fit 32 bits (kernels.h) */
  { const int pb = std::max(1, ilog2_ceil((u64) block->maxlen + 1)), ab = std::max(1, ilog2_ceil((u64) n));
    static int rp_on = -1;
    if (rp_on < 0)
      { const char *e = getenv("DAMAR_PACK_POS");
        rp_on = e ? atoi(e) : 1;
      }
    b->d.rpbits = (rp_on && pb + ab <= 32 && pb < 32) ? pb : 0;
  }
  if (block->tracks != NULL)                  /* the merged mask track of daligner.c:442-497 */
    { const int64 *anno = (const int64 *) block->tracks->anno;
      const int   *data = (const int *) block->tracks->data;
      std::vector<u32> moff((size_t) n + 1);
      for (int i = 0; i <= n; i++)
        moff[i] = (u32) anno[i];
      b->moff = (u32 *) dmalloc(sizeof(u32) * ((size_t) n + 1));
      b->mdat = (int *) dmalloc(sizeof(int) * ((size_t) anno[n] + 2));
      HIP_CHECK(hipMemcpyAsync(b->moff, moff.data(), sizeof(u32) * ((size_t) n + 1), hipMemcpyHostToDevice, st));
      if (anno[n] > 0)
        HIP_CHECK(hipMemcpyAsync(b->mdat, data, sizeof(int) * (size_t) anno[n], hipMemcpyHostToDevice, st));
      HIP_CHECK(hipStreamSynchronize(st));
      b->d.moff = b->moff;
      b->d.mdat = b->mdat;
    }
  b->nreads   = n;
  return b;
}


extern "C" void damar_block_free(damar_dev_block *b)
{ if (b == NULL)
    return;
  finish_all();                                /* a report launch in flight (or held back) may still read the bases */
  HIP_CHECK(hipStreamSynchronize(G_st));
  HIP_CHECK(hipFree(b->bases_alloc));
  HIP_CHECK(hipFree(b->pk_alloc));
  if (b->moff) HIP_CHECK(hipFree(b->moff));
  if (b->mdat) HIP_CHECK(hipFree(b->mdat));
  HIP_CHECK(hipFree(b->boff));
  HIP_CHECK(hipFree(b->coarse));
  free(b);
}

/***** index **************************************************************************************/

struct damar_dev_index
{ size_t codes_bytes, pos_bytes;                   /* what the pool gave (dpool_get) */
  damar_dev_block *blk;
  int   own_block;
  void *codes;                 /* u32 per k-mer, u64 when wide (k > 16) */
  u32  *pos;
  u32   n;
  int   kbits, wide;
};

/* The radix sort's look-back is bounded; a timeout (never seen) raises a device word.  sort_check queues its copy
   behind the sort, sort_verify looks at the copies once the stream has been synchronised. */
static u32 *H_serr = NULL;
static int  H_nserr = 0;
static void sort_verify(void)
{ for (int i = 0; i < H_nserr; i++)
    if (H_serr[i] != 0)
      { fprintf(stderr, "damar: FATAL: the radix sort's look-back timed out\n");
        die();
      }
  H_nserr = 0;
}
void sort_check(const void *sw)
{ if (H_serr == NULL)
    HIP_CHECK(hipHostMalloc((void **) &H_serr, 64 * sizeof(u32), hipHostMallocDefault));
  if (H_nserr == 64)
    { HIP_CHECK(hipStreamSynchronize(G_st));
      sort_verify();
    }
  HIP_CHECK(hipMemcpyAsync(&H_serr[H_nserr++], damar_sort_error_word(sw), sizeof(u32), hipMemcpyDeviceToHost, G_st));
}

/* Tile shape of the radix sort (radix_sort.hip): 1024 threads x 8 keys -- the 8192-key tile of the 512 x 16 shape in half
   the registers, so that two workgroups of 16 wavefronts fill a CU (measured alone and beside a resident report launch:
   profiles/r04_sweeps.txt; the 256-thread shape of round 3 is the slowest of the three now that a report wavefront
   holds 64 registers).  DAMAR_SORT_THREADS overrides. */
static bool overlap_on(void);
static bool corun_on(void);
static void pick_sort_shape(void)
{ static int forced = -1;
  if (forced < 0)
    { const char *e = getenv("DAMAR_SORT_THREADS");
      forced = e ? atoi(e) : 0;
    }
  damar_sort_set_threads(forced ? forced : 1024);
}

static int ilog2_ceil(u64 n)
{ int b = 0;
  while ((1ull << b) < n)
    b += 1;
  return b;
}

static int  G_index_made = 0;            /* the last index build made its keys inside the sort (damar_index_last_made) */
extern "C" int damar_index_last_made(void) { return G_index_made; }

static int  B_have = 0, B_log[4];        /* -b log weights, fixed by the first biased Sort_Kmers of the process */

/* A new job in the same process (the in-process driver, tests): forget the -b weights, as a
 * fresh daligner process would. */
extern "C" void damar_bias_reset(void) { B_have = 0; }

static damar_dev_index *index_build_k(damar_dev_block *blk, int own_block, int *len, int K, int suppress, int use_bias)
{ ensure_init();
  pick_sort_shape();
  if (K > 32)
    { fprintf(stderr, "damar: FATAL: -k%d: a k-mer code holds at most 32 bases\n", K);
      die();
    }
  if (blk->nreads > 0 && blk->minlen < K)      /* daligner.c:499-504: the k-mer slots assume rlen >= k */
    { fprintf(stderr, "[ERROR] - daligner: Block contains reads < %dbp long !  Run DBsplit.\n", K);
      die();
    }
  int64 nk64 = (int64) blk->d.total - (int64) K * blk->nreads;
  if (nk64 <= 0)
    { *len = 0;
      if (own_block)
        damar_block_free(blk);
      return NULL;
    }
  u32 nk = (u32) nk64;
  const int kbits = 2 * K;
  const int wide = K > 16;                  /* codes as u64 (filter.c's KmerPos.code is 64 bits wide) */
  const size_t cs = wide ? sizeof(u64) : sizeof(u32);
  const bool masked = blk->d.moff != NULL;
  const bool biased = use_bias != 0;
  /* -b (filter.c:774-789): the log weights are set by the FIRST block a process sorts and then
     kept (the reference tests a static pointer), also for complemented and other blocks */
  if (biased && !B_have)
    { const double scale = -10000. / log(4.);
      for (int i = 0; i < 4; i++)
        B_log[i] = (int) ceil(scale * log((double) blk->freq[i]));
      B_have = 1;
    }
  const u32 cap = biased ? blk->d.total : nk;          /* -b can leave one k-mer per base */
  const int npass = (kbits + 7) / 8;
  damar_dev_index *ix = (damar_dev_index *) calloc(1, sizeof(damar_dev_index));
  ix->blk = blk;  ix->own_block = own_block;  ix->kbits = kbits;  ix->wide = wide;
  /* k <= 16: the sort runs on ONE u64 per k-mer, code << 32 | pos, on the code bits only (radix_sort.hip), and its
     last pass writes the two halves apart: codes[] and pos[] share one buffer of 8 bytes per k-mer.
     k > 16: u64 codes and u32 positions as key and payload. */
  if (wide)
    { ix->codes = dpool_get(cs * (size_t) cap, &ix->codes_bytes);
      ix->pos   = (u32 *) dpool_get(sizeof(u32) * (size_t) cap, &ix->pos_bytes);
    }
  else
    { ix->codes = dpool_get(2 * sizeof(u32) * (size_t) cap, &ix->codes_bytes);
      ix->pos   = (u32 *) ix->codes + cap;
    }

  size_t swb = damar_sort_workspace_bytes(cap);
  arena_reserve(&G_work, pad256(sizeof(u64) * (size_t) cap) + 3 * pad256(sizeof(u32) * (size_t) cap) + pad256(swb) +
                         pad256(damar_scan_workspace_bytes(cap)) + (1 << 16));
  void *tk = arena_take(&G_work, sizeof(u64) * (size_t) cap);
  u32 *tv = (u32 *) arena_take(&G_work, sizeof(u32) * (size_t) cap);
  void *sw = arena_take(&G_work, swb);
  u32 *keep = NULL, *off = NULL;
  void *scw = NULL;
  u64 *tot = NULL;
  if (masked || biased || suppress > 0)
    { keep = (u32 *) arena_take(&G_work, sizeof(u32) * (size_t) cap);
      off  = (u32 *) arena_take(&G_work, sizeof(u32) * (size_t) cap);
      scw  = arena_take(&G_work, damar_scan_workspace_bytes(cap));
      tot  = (u64 *) arena_take(&G_work, 64);
    }

  /* the sort ping-pongs: start on the side that makes it end in the index's own arrays (wide), resp. that makes
     its last pass READ the temporary, so that it can write the index's buffer (packed) */
  void *k0, *k1;
  u32  *v0, *v1;
  if (wide)
    { k0 = (npass & 1) ? tk : ix->codes;  k1 = (npass & 1) ? ix->codes : tk;
      v0 = (npass & 1) ? tv : ix->pos;    v1 = (npass & 1) ? ix->pos : tv;
    }
  else
    { k0 = (npass & 1) ? tk : ix->codes;  k1 = (npass & 1) ? ix->codes : tk;
      v0 = v1 = NULL;
    }

  /* The plain packed build with position words (k <= 16, no mask, no -b: what a daligner run does all day) never has its
     unsorted keys in HBM: the sort's histogram and first pass make them from the 2-bit bases (radix_sort.hip,
     damar_radix_sort_split_kmers), so the `tuples` phase below is empty.  DAMAR_INDEX_GEN=0: kmer_tuples writes them
     and the sort reads them, as every other build does. */
  static int gen_on = -1;
  if (gen_on < 0)
    { const char *e = getenv("DAMAR_INDEX_GEN");
      gen_on = e ? atoi(e) : 1;
    }
  const bool made = gen_on && !wide && !masked && !biased && blk->d.rpbits > 0;
  G_index_made = made;

  tick(0);
  if (biased || masked)
    { /* filter.c:474-526 / 549-688 + the filler squeeze of :855-888: only k-mers inside one
         unmasked stretch (resp. the windows the -b walk yields) enter the index; dropping the rest
         before the sort leaves the same sorted list.  The candidates sit in the sort's other buffer. */
      void *k9 = k1;
      u32  *v9 = wide ? ((v0 == tv) ? ix->pos : tv) : (u32 *) k1 + cap;
      u64   kept = 0;
      u32   nin = nk;
      if (biased)
        { nin = cap;
          HIP_CHECK(hipMemsetAsync(keep, 0, sizeof(u32) * (size_t) cap, G_st));
          damar_launch_biased_tuples(&blk->d, K, B_log, k9, wide, v9, keep, G_st);
        }
      else
        { damar_launch_kmer_tuples(&blk->d, K, nk, k9, wide, v9, G_st);
          damar_launch_mask_flags(&blk->d, K, v9, nk, keep, G_st);
        }
      damar_exclusive_scan_u32(keep, off, nin, scw, tot, G_st);
      damar_launch_compact_pairs(k9, wide, v9, keep, off, nin, k0, v0, G_st);      /* v0 == NULL: packed into k0 */
      HIP_CHECK(hipMemcpyAsync(&kept, tot, sizeof(u64), hipMemcpyDeviceToHost, G_st));
      HIP_CHECK(hipStreamSynchronize(G_st));
      nk = (u32) kept;
      if (nk == 0)
        { damar_index_free(ix);
          *len = 0;
          return NULL;
        }
      if (VERBOSE && biased)
        printf("\n   Revised kmer count = %u\n", nk);
    }
  else if (!made)
    damar_launch_kmer_tuples(&blk->d, K, nk, k0, wide, v0, G_st);                   /* v0 == NULL: packed */
  tick(1);
  if (wide)
    { int side = damar_radix_sort_u64((u64 *) k0, v0, (u64 *) k1, v1, nk, kbits, sw, G_st);
      if ((side ? k1 : k0) != ix->codes)
        { fprintf(stderr, "damar: internal error, sort ended on the wrong side\n");
          die();
        }
    }
  else if (made)
    { KmerKeys src;
      src.blk  = blk->d;
      src.kmer = K;
      damar_radix_sort_split_kmers(&src, (u64 *) k0, (u64 *) k1, nk, (u32 *) ix->codes, ix->pos, sw, G_st);
    }
  else
    damar_radix_sort_split_u64((u64 *) k0, (u64 *) k1, nk, 32, 32 + kbits, (u32 *) ix->codes, ix->pos, sw, G_st);
  sort_check(sw);
  tick(2);
  u32 n = nk;
  if (suppress > 0)                         /* filter.c:890-939 */
    { u64  kept = 0;
      damar_launch_suppress_flags(ix->codes, wide, n, suppress, keep, G_st);
      damar_exclusive_scan_u32(keep, off, n, scw, tot, G_st);
      damar_launch_compact_pairs(ix->codes, wide, ix->pos, keep, off, n, tk, tv, G_st);
      HIP_CHECK(hipMemcpyAsync(&kept, tot, sizeof(u64), hipMemcpyDeviceToHost, G_st));
      HIP_CHECK(hipStreamSynchronize(G_st));
      n = (u32) kept;
      HIP_CHECK(hipMemcpyAsync(ix->codes, tk, cs * (size_t) n, hipMemcpyDeviceToDevice, G_st));
      HIP_CHECK(hipMemcpyAsync(ix->pos, tv, sizeof(u32) * (size_t) n, hipMemcpyDeviceToDevice, G_st));
    }
  tick(3);
  HIP_CHECK(hipStreamSynchronize(G_st));
  sort_verify();
  G_ms[DAMAR_T_TUPLES] = lap(0, 1);
  G_ms[DAMAR_T_KSORT]  = lap(1, 2);
  G_ms[DAMAR_T_TABLE]  = lap(2, 3);
  ix->n = n;
  if (VERBOSE)
    { printf("\n   Kmer count = %u\n   Index occupies %.2fGb of HBM\n", n, ((cs + 4.) * n) / 1073741824.);
      fflush(stdout);
    }
  if (n == 0)
    { damar_index_free(ix);
      *len = 0;
      return NULL;
    }
  *len = (int) n;
  return ix;
}

extern "C" damar_dev_index *damar_index_build(damar_dev_block *blk, int own_block, int *len)
{ double t0 = now_ms();
  damar_dev_index *ix = index_build_k(blk, own_block, len, P_kmer, P_suppress, BIASED);
  H_ms[0] += now_ms() - t0;
  return ix;
}

extern "C" void damar_index_free(damar_dev_index *ix)
{ if (ix == NULL)
    return;
  HIP_CHECK(hipStreamSynchronize(G_st));
  dpool_put(ix->codes, ix->codes_bytes);       /* (the stream was synchronised above: nothing reads them any more) */
  if (ix->pos_bytes)                           /* (k <= 16: the positions live in the codes' buffer) */
    dpool_put(ix->pos, ix->pos_bytes);
  if (ix->own_block)
    damar_block_free(ix->blk);
  free(ix);
}

/* Residency figures for a scheduler that keeps blocks and indexes in HBM (daligner -P, driver.Plan): free and total bytes
   of the device, the bytes one resident block holds, and a way to hand the pool of parked index buffers back. */
extern "C" void damar_hbm_info(uint64_t *free_bytes, uint64_t *total_bytes)
{ ensure_init();
  size_t f = 0, t = 0;
  HIP_CHECK(hipMemGetInfo(&f, &t));
  if (free_bytes)  *free_bytes = (uint64_t) f + (uint64_t) DP_bytes;       /* (parked buffers are as good as free) */
  if (total_bytes) *total_bytes = (uint64_t) t;
}

extern "C" uint64_t damar_block_bytes(const damar_dev_block *b)
{ if (b == NULL)
    return 0;
  const uint64_t tot = b->d.total;
  return tot + 128 + (tot >> 2) + 64 + sizeof(u32) * ((uint64_t) b->nreads + 1) + sizeof(u32) * ((tot >> COARSE_SHIFT) + 2);
}

extern "C" void damar_pool_trim(void)
{ finish_all();
  HIP_CHECK(hipStreamSynchronize(G_st));
  for (size_t i = 0; i < DP_free.size(); i++)
    HIP_CHECK(hipFree(DP_free[i].p));
  DP_free.clear();
  DP_bytes = 0;
}

/* HBM held by one index (what its buffers took from the pool): lets a scheduler bound residency */
extern "C" uint64_t damar_index_bytes(const damar_dev_index *ix)
{ return ix == NULL ? 0 : (uint64_t) (ix->codes_bytes + ix->pos_bytes); }

extern "C" void damar_index_download(const damar_dev_index *ix, void *out)
{ struct KP { uint64 code; int rpos; int read; } *kp = (KP *) out;
  std::vector<u32> pos(ix->n), boff((size_t) ix->blk->nreads + 1);
  std::vector<u64> codes(ix->n);
  if (ix->wide)
    HIP_CHECK(hipMemcpy(codes.data(), ix->codes, sizeof(u64) * (size_t) ix->n, hipMemcpyDeviceToHost));
  else
    { std::vector<u32> c32(ix->n);
      HIP_CHECK(hipMemcpy(c32.data(), ix->codes, sizeof(u32) * (size_t) ix->n, hipMemcpyDeviceToHost));
      for (u32 i = 0; i < ix->n; i++)
        codes[i] = c32[i];
    }
  HIP_CHECK(hipMemcpy(pos.data(), ix->pos, sizeof(u32) * (size_t) ix->n, hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(boff.data(), ix->blk->boff, sizeof(u32) * boff.size(), hipMemcpyDeviceToHost));
  const int rp = ix->blk->d.rpbits;
  for (u32 i = 0; i < ix->n; i++)
    { kp[i].code = codes[i];
      if (rp)                                   /* packed position word: read << rpbits | offset in the read */
        { kp[i].rpos = (int) (pos[i] & ((1u << rp) - 1u));
          kp[i].read = (int) (pos[i] >> rp);
        }
      else
        { u32 r = (u32) (std::upper_bound(boff.begin(), boff.end(), pos[i]) - boff.begin()) - 1;
          kp[i].rpos = (int) (pos[i] - boff[r]);
          kp[i].read = (int) r;
        }
    }
}

extern "C" void *Sort_Kmers(HITS_DB *block, int *len)
{ /* block->tracks, if any, is the merged mask of daligner.c:442-497: it travels with the block */
  damar_dev_block *b = take_preloaded(block);
  if (b == NULL)
    b = damar_block_upload(block);
  return (void *) damar_index_build(b, 1, len);
}

/***** report scratch ******************************************************************************/

struct ReportScratch
{ int nslots_wanted; int   nslots, span, bwidth;
  u32   cell_cap;
  u32   ttmp_stride;
  void *state;  int *marks;  void *cells;  int *buckets;  u16 *ttmp;
  u64   state_stride, marks_stride, bucket_stride;
  short *tables;             /* SCORE then TABLE */
  const void *tables_of;     /* host spec they were copied from */
  u32  *counters;
  LaRecord *recs;  u32 rec_cap;      /* the record / trace buffers and the counters of set `cur` */
  u16  *tpool;     u32 tpool_cap;
  u32  *ctr;
  /* two sets of record / trace buffers and counters: a launch writes into one set while the records of the launch before
     it are still on their way to the host out of the other (measured: a launch waited 1.4 - 2.2 ms for that download),
     and the next launch can be queued behind a running one */
  LaRecord *recs_set[2];  u16 *tpool_set[2];  u32 rec_cap_set[2], tpool_cap_set[2];  int cur;
  u32  *widemap[2];  u32 widemap_cap[2];          /* per output set: one bit per work item of the launch's jobs (ReportArgs.widemap) */
  void *wcells;  u32 wcell_cap;  int wslots;      /* the wide kernel's 16-byte pebbles (allocated when a launch first needs them) */
};
static ReportScratch RS = {};   /* (nslots_wanted: the slot count asked for when nslots was last sized) */

static int default_slots(void)
{ const char *e = getenv("DAMAR_SLOTS");
  if (e && atoi(e) > 0)
    return atoi(e);
  /* (rounds 2-3: a report launch that shares the machine with the next comparisons' seed stages left them a fifth of the
     register file, 4 of the 5 wavefronts per SIMD the round-3 kernel was compiled for.  report_packed.h's kernel now needs 64
     VGPRs and a launch now takes every wave slot: measured per config-2 step 298 / 300 / 293 / 298 / 286 ms at 4 / 5 / 6 /
     7 / 8 report wavefronts per SIMD, profiles/r04_sweeps.txt -- the seed kernels then run in the gaps the report
     wavefronts leave as they retire, and nothing is gained by reserving registers for them) */
  /* (DAMAR_REPORT_WPS: report wavefronts per SIMD of a launch, for sweeps) */
  if (const char *w = getenv("DAMAR_REPORT_WPS"))
    if (atoi(w) > 0)
      return G_prop.multiProcessorCount * 4 * damar_report2_slots_per_wave() * std::min(atoi(w), damar_report2_waves_per_simd());
  if (corun_on())
    return G_prop.multiProcessorCount * 4 * damar_report2_slots_per_wave() * (damar_report2_waves_per_simd() >= 8 ? 8 : std::min(4, damar_report2_waves_per_simd()));
  /* every wave slot of the chip: one scratch slot per wavefront of the one-pair kernel, two per wavefront of the packed one */
  return G_prop.multiProcessorCount * 4 * std::max(damar_report_waves_per_simd(), damar_report2_slots_per_wave() * damar_report2_waves_per_simd());
}

static int G_ring = 0;
/* pebbles per slot to start with: an alignment drops about 200 per kb and direction; a pool that overflows is
   quadrupled and the launch repeated.  Kept small because the driver clears what it hands out: an 8 GB pool
   (65536 cells x 8192 slots) cost every process 0.25 - 0.8 s in hipMalloc, and the 6.6 GB of 12288 slots with
   16384 cells and rings of 4096 diagonals 0.2 - 0.7 s. */
#define DEFAULT_CELLS (1u << 13)

/* the pebble pool of a slot after an overflow: a chain head holds 18 bits of pebble index (report.hip PK_HBITS) */
static u32 max_cells(void)                  /* (DAMAR_TEST_MAX_CELLS: a test hook that sends ordinary read pairs through the wide kernel) */
{ static u32 m = 0;
  if (m == 0)
    { const char *e = getenv("DAMAR_TEST_MAX_CELLS");
      m = (e && atoi(e) >= 16) ? std::min<u32>((u32) atoi(e), DAMAR_MAX_CELLS) : DAMAR_MAX_CELLS;
    }
  return m;
}

/* Blocks of a wide-kernel launch.  RS.wslots is sized when the wide pebbles are first allocated; block b of that launch also
   takes slot b of the ordinary scratch (band state, marks, trace buffers: slot_scratch), which holds RS.nslots slots and may
   have been rebuilt with fewer since (DAMAR_SLOTS, less free memory): never more blocks than either has. */
static int wide_slots(void)
{ return std::min(RS.wslots, RS.nslots); }

/* The wide kernel's pebble pool: 16 bytes x RS.wcell_cap pebbles x RS.wslots slots, allocated when a launch first needs
   it (wide_pool_ensure).  When the wide kernel itself raises DAMAR_ERR_CELLS the pool gets four times the pebbles over
   half the slots, and the caller repeats everything (wide_pool_grow; nothing may be running on the old pool: the
   caller has synchronised). */
static void wide_pool_ensure(void)
{ if (RS.wcells != NULL)
    return;
  RS.wslots = std::min(RS.nslots, 64);
  RS.wcell_cap = 1u << 21;
  RS.wcells = dmalloc((size_t) 16 * RS.wcell_cap * (size_t) RS.wslots);
}
static void wide_pool_grow(void)
{ if (RS.wcell_cap >= (1u << 26))
    { fprintf(stderr, "damar: FATAL: an alignment needs more than %u trace pebbles even in the wide format\n", RS.wcell_cap);
      die();
    }
  HIP_CHECK(hipFree(RS.wcells));
  RS.wcell_cap *= 4;
  RS.wslots = std::max(8, RS.wslots / 2);
  RS.wcells = dmalloc((size_t) 16 * RS.wcell_cap * (size_t) RS.wslots);
}

static u32 grow_cells(u32 cell_cap)
{ if (cell_cap >= max_cells())
    { fprintf(stderr, "damar: FATAL: an alignment needs more than %u trace pebbles; use a larger trace spacing (-s)\n", max_cells());
      die();
    }
  return std::min(cell_cap * 4, max_cells());
}

/* one read pair per wavefront with 8-byte pebbles (DAMAR_PACKED=0): no wide kernel runs behind that path, its limit stays loud */
static void marks_must_fit(int amax, int bmax, int tspace)
{ if (tspace > 0 && std::max(amax, bmax) / tspace + 8 > DAMAR_MAX_MARKS)
    { fprintf(stderr, "damar: FATAL: reads of %d bases need a trace spacing (-s) of at least %d here\n", std::max(amax, bmax),
              std::max(amax, bmax) / (DAMAR_MAX_MARKS - 8) + 1);
      die();
    }
}

static void scratch_prepare(int amax, int bmax, int binshift, int tspace, u32 cell_cap, hipStream_t st)
{ if (tspace <= 0)
    { fprintf(stderr, "damar: FATAL: trace spacing %d\n", tspace);
      die();
    }
  /* (reads of more than DAMAR_MAX_MARKS trace spacings -- 14 bits of trace-grid index in a packed chain head -- are the wide
     kernel's: report_launch, kernels/report.hip report_wide_kernel) */
  if (tspace > DAMAR_MAX_TSPACE)                  /* pebbles carry diagonal and wave number modulo 2^16 (kernels/report.hip: struct Cell) */
    { fprintf(stderr, "damar: FATAL: a trace spacing (-s) above %d is not supported by this build\n", DAMAR_MAX_TSPACE);
      die();
    }
  if (G_last_d2h[RS.cur] != NULL)  /* whatever is launched next overwrites the record buffers of this set */
    { HIP_CHECK(hipStreamWaitEvent(st, G_last_d2h[RS.cur], 0));
      G_last_d2h[RS.cur] = NULL;
    }
  /* The band state of a slot (used only while a band is wider than the 64 lanes) is a ring of G_ring
     diagonals, not one entry per diagonal of the pair: 1024 instead of alen + blen keeps the scratch of
     12288 slots at 2.5 GB (the driver stalls for seconds whenever a process first grows past ~24 GB).
     A band that outgrows the ring raises DAMAR_ERR_WIDE and the launch is repeated with a larger one. */
  if (G_ring == 0)
    { const char *e = getenv("DAMAR_RING");
      G_ring = e ? atoi(e) : 1024;
      if (G_ring < 128) G_ring = 128;
      while (G_ring & (G_ring - 1)) G_ring += G_ring & -G_ring;      /* next power of two */
    }
  int span = 128;
  while (span < amax + bmax + 72) span *= 2;
  if (span > G_ring) span = G_ring;
  int bwidth = (amax >> binshift) - ((-bmax) >> binshift) + 1;
  int mtp    = 2 * (std::max(amax, bmax) / tspace + 2) + 8;
  u32 tstr   = (u32) (4 * mtp + 32);
  /* the longest reads differ a little from block to block: sizes are taken with a quarter of headroom so
     that a plan line does not rebuild the scratch for every B block */
  if (RS.bwidth < bwidth)      bwidth = ((bwidth + bwidth / 4) + 255) & ~255;
  if (RS.ttmp_stride < tstr)   tstr   = ((tstr + tstr / 4) + 255u) & ~255u;
  int nslots = default_slots();
  bool grow = RS.span < span || RS.bwidth < bwidth || RS.cell_cap < cell_cap || RS.ttmp_stride < tstr;
  if (grow || (RS.nslots != nslots && RS.nslots_wanted != nslots))
    { const double g0 = now_ms();
      HIP_CHECK(hipStreamSynchronize(G_st));
      late_streams();
      HIP_CHECK(hipStreamSynchronize(G_rep));
      if (RS.state)   { HIP_CHECK(hipFree(RS.state)); HIP_CHECK(hipFree(RS.marks)); HIP_CHECK(hipFree(RS.cells));
                        HIP_CHECK(hipFree(RS.buckets)); HIP_CHECK(hipFree(RS.ttmp)); RS.state = NULL; }
      /* the scratch of all wave slots must fit what is left of HBM (very long reads: the
         per-slot band buffers grow with alen + blen): fewer resident alignments then, never a
         failed allocation in the middle of a run */
      RS.nslots_wanted = nslots;
      { size_t freeb = 0, totb = 0;
        const u64 nspan = (u64) std::max(RS.span, span), ncell = std::max(RS.cell_cap, cell_cap);
        const u64 per = damar_report_state_stride((int) nspan) + 4ull * 2 * nspan + 8ull * ncell +
                        4ull * (3ull * std::max(RS.bwidth, bwidth) + 16) + 2ull * std::max(RS.ttmp_stride, tstr);
        const double g1 = now_ms();
        HIP_CHECK(hipMemGetInfo(&freeb, &totb));
        if (getenv("DAMAR_HOSTPROF")) fprintf(stderr, "damar: scratch grow: sync+free %.1f ms, hipMemGetInfo %.1f ms\n", g1 - g0, now_ms() - g1);
        const u64 budget = (u64) (freeb * 0.6);
        if ((u64) nslots * per > budget)
          { int fit = (int) (budget / per);
            if (fit < 64)
              { fprintf(stderr, "damar: FATAL: not enough device memory for the alignment scratch (%.1f MB per wave slot, %.1f GB free)\n",
                        per / 1048576., freeb / 1073741824.);
                die();
              }
            if (VERBOSE)
              fprintf(stderr, "damar: %d instead of %d resident alignments (%.1f MB of scratch each)\n", fit, nslots, per / 1048576.);
            nslots = fit - fit % damar_report2_slots_per_wave();      /* (a wavefront of the packed kernel holds that many slots) */
          }
      }
      RS.nslots = nslots;
      RS.span   = std::max(RS.span, span);
      RS.bwidth = std::max(RS.bwidth, bwidth);
      RS.cell_cap = std::max(RS.cell_cap, cell_cap);
      RS.ttmp_stride = std::max(RS.ttmp_stride, tstr);
      RS.state_stride  = damar_report_state_stride(RS.span);
      RS.marks_stride  = (u64) 2 * RS.span;
      RS.bucket_stride = (u64) 3 * RS.bwidth + 16;
      const double g2 = now_ms();
      RS.state   = dmalloc((size_t) RS.state_stride * nslots);
      RS.marks   = (int *) dmalloc(sizeof(int) * (size_t) RS.marks_stride * nslots);
      RS.cells   = dmalloc((size_t) 8 * RS.cell_cap * nslots);                /* 8-byte pebbles (kernels/report.hip: struct Cell) */
      RS.buckets = (int *) dmalloc(sizeof(int) * (size_t) RS.bucket_stride * nslots);
      RS.ttmp    = (u16 *) dmalloc(sizeof(u16) * (size_t) RS.ttmp_stride * nslots);
      HIP_CHECK(hipMemsetAsync(RS.state, 0, (size_t) RS.state_stride * nslots, st));
      HIP_CHECK(hipMemsetAsync(RS.marks, 0, sizeof(int) * (size_t) RS.marks_stride * nslots, st));
      if (getenv("DAMAR_HOSTPROF"))
        fprintf(stderr, "damar: scratch grow: 5 allocations of %.2f GB in all %.1f ms (span %d bwidth %d cells %u)\n",
                ((double) RS.state_stride + 4. * RS.marks_stride + 8. * RS.cell_cap + 4. * RS.bucket_stride + 2. * RS.ttmp_stride) * nslots / 1073741824.,
                now_ms() - g2, RS.span, RS.bwidth, RS.cell_cap);
    }
  if (RS.counters == NULL)
    { RS.counters = (u32 *) dmalloc(sizeof(u32) * DAMAR_COUNTER_WORDS * 2);
      RS.tables   = (short *) dmalloc(sizeof(short) * 65536 * DAMAR_MAX_JOBS);
    }
  HIP_CHECK(hipMemsetAsync(RS.buckets, 0, sizeof(int) * (size_t) RS.bucket_stride * RS.nslots, st));
}

/* the record / trace buffers of set RS.cur hold at least this much (nothing is in flight on that set: its last launch has
   been completed; its download may still run) */
static void scratch_outputs(u32 rec_cap, u32 tpool_cap)
{ const int c = RS.cur;
  if (RS.rec_cap_set[c] < rec_cap || RS.tpool_cap_set[c] < tpool_cap)
    { late_streams();
      HIP_CHECK(hipStreamSynchronize(G_copy));
      G_last_d2h[c] = NULL;
      if (RS.rec_cap_set[c] < rec_cap)
        { RS.rec_cap_set[c] = rec_cap + (rec_cap >> 2);
          if (RS.recs_set[c]) HIP_CHECK(hipFree(RS.recs_set[c]));
          RS.recs_set[c] = (LaRecord *) dmalloc(sizeof(LaRecord) * (size_t) RS.rec_cap_set[c]);
        }
      if (RS.tpool_cap_set[c] < tpool_cap)
        { RS.tpool_cap_set[c] = tpool_cap + (tpool_cap >> 2);
          if (RS.tpool_set[c]) HIP_CHECK(hipFree(RS.tpool_set[c]));
          RS.tpool_set[c] = (u16 *) dmalloc(sizeof(u16) * (size_t) RS.tpool_cap_set[c]);
        }
    }
  RS.recs  = RS.recs_set[c];   RS.rec_cap   = RS.rec_cap_set[c];
  RS.tpool = RS.tpool_set[c];  RS.tpool_cap = RS.tpool_cap_set[c];
  RS.ctr   = RS.counters + (size_t) c * DAMAR_COUNTER_WORDS;
}

static void fill_report_args(ReportArgs *ra, const damar_dev_block *ab, const damar_dev_block *bb,
                             int comp, int self, Align_Spec *spec, hipStream_t st, int job, int tslot, const JobParams &jp)
{ memset(ra, 0, sizeof(*ra));
  ra->job = job;
  ra->ablk = ab->d;  ra->bblk = bb->d;
  ra->kmer = jp.kmer;  ra->hitmin = jp.hitmin;  ra->binshift = jp.binshift;
  ra->minhit = (jp.hitmin - 1) / jp.kmer + 1;
  ra->comp = comp;  ra->self = self;  ra->symmetric = jp.symmetric;
  ra->minover = jp.minover;  ra->hgap_min = jp.hgap_min;
  ra->tspace = Trace_Spacing(spec);
  ra->ave_path = damar_spec_ave_path(spec);
  ra->reach = Overlap_If_Possible(spec);
  /* SCORE/TABLE of this Align_Spec, every time (128 KB): remembering "the tables of spec X are
     already up" by X's address went wrong when a freed spec's address came back for a new one
     with another -e */
  { /* ... but only when the slot does not hold these very values already (a host copy of what is up there is compared):
       the copy comes out of pageable memory, and behind the download of the previous launch's records it held the
       launch back by 1.4 - 7 ms (scripts/gpu_gaps_api.sh) */
    static short *shadow = NULL;
    static bool   valid[DAMAR_MAX_JOBS];
    if (shadow == NULL)
      shadow = (short *) malloc(sizeof(short) * 65536 * DAMAR_MAX_JOBS);
    short *mine = shadow + (size_t) tslot * 65536;
    if (shadow == NULL || !valid[tslot] || memcmp(mine, damar_spec_score_table(spec), sizeof(short) * 65536) != 0)
      { HIP_CHECK(hipMemcpyAsync(RS.tables + (size_t) tslot * 65536, damar_spec_score_table(spec), sizeof(short) * 65536,
                                 hipMemcpyHostToDevice, st));
        if (shadow != NULL)
          { memcpy(mine, damar_spec_score_table(spec), sizeof(short) * 65536);
            valid[tslot] = true;
            HIP_CHECK(hipStreamSynchronize(st));        /* (a later launch on another stream may find the slot "up") */
          }
      }
  }
  ra->score = RS.tables + (size_t) tslot * 65536;
  ra->table = ra->score + 32768;
  { const int16 *sc = damar_spec_score_table(spec);          /* SCORE[x] = matches * mscore - (15 - matches) * dscore */
    ra->mscore = sc[32767] / 15;
    ra->dscore = -sc[0] / 15;
  }
  ra->state = RS.state;  ra->state_stride = RS.state_stride;  ra->span = RS.span;
  ra->marks = RS.marks;  ra->marks_stride = RS.marks_stride;
  ra->cells = RS.cells;  ra->cell_cap = RS.cell_cap;
  ra->buckets = RS.buckets;  ra->bucket_stride = RS.bucket_stride;  ra->bwidth = RS.bwidth;
  ra->bucket_bits = ilog2_ceil((u64) RS.bwidth + 2);
  ra->ttmp = RS.ttmp;  ra->ttmp_stride = RS.ttmp_stride;
  ra->recs = RS.recs;  ra->rec_cap = RS.rec_cap;
  ra->tpool = RS.tpool;  ra->tpool_cap = RS.tpool_cap;
  ra->t8 = 0;                                   /* (the pipeline's launches set it: report_launch) */
  ra->widemap = NULL;  ra->wcells = NULL;  ra->wcell_cap = 0;  ra->cell_max = DAMAR_MAX_CELLS;
  { static int lim = -1;                        /* test hook: a lower limit makes the 16-bit re-launch happen (tests/test_gpu_configs.py) */
    if (lim < 0)
      lim = getenv("DAMAR_TEST_T8_LIMIT") ? atoi(getenv("DAMAR_TEST_T8_LIMIT")) : 255;
    ra->t8max = lim;
  }
  ra->counters = RS.ctr;
  ra->cursor = RS.ctr + DAMAR_CNT_CURSOR + job;
  ra->nfilt  = RS.ctr + DAMAR_CNT_NFILT + job;
}


/* Two read pairs per wavefront (kernels/report_packed.h) unless DAMAR_PACKED=0.  Measured on config 2 (profiles/r02_*):
 * identical output, 356 ms of report kernel per step against 366 ms for one pair per wavefront (357 ms at the end of
 * round 1).  Both kernels are bound by how long ONE wavefront takes for a wave step (~4500-6000 cycles of serial issue;
 * the scalar unit is 86 % busy in the one-pair kernel), not by HBM; the packed one advances two alignments per such
 * step but fits 4 instead of 8 wavefronts per SIMD (its wave loop needs ~100 VGPRs). */
static bool use_packed(const ReportArgs *ra, int amax, int bmax)
{ static int want = -1;
  if (want < 0)
    { const char *e = getenv("DAMAR_PACKED");
      want = e ? atoi(e) : 1;
    }
  if (!want || (RS.nslots % damar_report2_slots_per_wave()) || ra->tspace <= 0)
    return false;
  if (ra->mscore * 8 > 32000 || ra->dscore * 8 > 32000)
    return false;
  return true;
}

/***** the landing buffers of the host tail (host/tail.cpp) and the asynchronous mode's thin callers *******/

struct RecOrder                                /* (damar_local_alignment_batch_opts lays its traces out in this order) */
{ bool operator()(const LaRecord &x, const LaRecord &y) const
  { return (x.item != y.item) ? (x.item < y.item) : (x.seq < y.seq); }
};

/* Page-locked landing buffers for the records and trace points of one report launch, recycled
 * through a small pool: the download runs at PCIe speed and nothing is allocated or touched
 * for the first time inside the timed loop. */
static bool   A_on = false;                   /* the asynchronous host pipeline is running (damar_set_async) */
/* what the tail reads of a buffer is the plain part (host/tail.h); the rest is how it gets there */
struct HostBuf : damar_tail_buf
{ size_t rec_cap, tp_cap, wmap_cap;
  hipEvent_t e0, e1;               /* around the download; e1 is what the tail thread waits for */
  bool      pending;
};
static std::mutex             &HB_mu   = *new std::mutex();
static std::vector<HostBuf *> &HB_free = *new std::vector<HostBuf *>();

/* Page-locking costs a millisecond per 4 - 5 MB (hipHostMalloc of 70 MB: 13 ms, a hipHostFree 5 ms: scripts/gpu_hiptrace.sh)
   and the thread that asks is the one that launches the kernels: in a cold four-line plan the two buffers, each
   allocated at its first launch and grown at its second (cross comparisons hold twice the records of the self
   comparison a plan starts with), were 60 ms of that thread's 490.  So a buffer is sized for 2.5 x what its first launch
   needs, and the first one brings a twin along, allocated by a thread of its own while the tail of the first launch
   runs. */
static void hostbuf_size(HostBuf *h, size_t nrec, size_t ntp, bool generous)
{ if (h->rec_cap < nrec)
    { if (h->recs) HIP_CHECK(hipHostFree(h->recs));
      h->rec_cap = generous ? nrec + nrec + (nrec >> 1) + 4096 : nrec + (nrec >> 2) + 4096;
      HIP_CHECK(hipHostMalloc((void **) &h->recs, sizeof(LaRecord) * h->rec_cap, hipHostMallocDefault));
    }
  if (h->tp_cap < ntp)
    { if (h->tpool) HIP_CHECK(hipHostFree(h->tpool));
      h->tp_cap = generous ? ntp + ntp + (ntp >> 1) + 65536 : ntp + (ntp >> 2) + 65536;
      HIP_CHECK(hipHostMalloc((void **) &h->tpool, sizeof(u16) * h->tp_cap, hipHostMallocDefault));
    }
}

static std::thread *HB_twin = NULL;           /* allocates the second landing buffer (hostbuf_get); joined by helpers_join() */
static void hostbuf_put(HostBuf *h)
{ std::lock_guard<std::mutex> lk(HB_mu);
  HB_free.push_back(h);
}

/* the pipeline's two ways back (host/tail.h): the tail thread waits for the download, the last tail returns the buffer */
static double hostbuf_landed(damar_tail_buf *b)
{ HostBuf *h = static_cast<HostBuf *>(b);
  float ms = 0;
  if (h->pending)
    { HIP_CHECK(hipSetDevice(G_device));          /* the current device is a per-thread setting */
      HIP_CHECK(hipEventSynchronize(h->e1));
      HIP_CHECK(hipEventElapsedTime(&ms, h->e0, h->e1));
      h->pending = false;                         /* (the other comparisons of the launch share the buffer) */
    }
  return ms;
}
static void hostbuf_release(damar_tail_buf *b) { hostbuf_put(static_cast<HostBuf *>(b)); }

static HostBuf *hostbuf_new(void)
{ HostBuf *h = new HostBuf();
  memset(h, 0, sizeof(*h));
  HIP_CHECK(hipEventCreate(&h->e0));
  HIP_CHECK(hipEventCreate(&h->e1));
  h->landed = hostbuf_landed;  h->release = hostbuf_release;
  return h;
}

static void helpers_join(void)
{ late_streams();
  tail_pool_join();
  std::thread *t = NULL;
  { std::lock_guard<std::mutex> lk(HB_mu);
    t = HB_twin;  HB_twin = NULL;
  }
  if (t != NULL)
    { t->join();
      delete t;
    }
}

static HostBuf *hostbuf_get(size_t nrec, size_t ntp)
{ HostBuf *h = NULL;
  static std::atomic<int> made(0);
  { std::lock_guard<std::mutex> lk(HB_mu);
    if (!HB_free.empty())
      { h = HB_free.back();
        HB_free.pop_back();
      }
  }
  if (h == NULL)
    h = hostbuf_new();
  h->pending = false;
  const bool first = (h->rec_cap == 0 && h->tp_cap == 0);
  hostbuf_size(h, nrec, ntp, first);
  if (first && made.fetch_add(1) == 0 && A_on)
    { /* the twin of the process's first buffer (asynchronous mode: a second launch's records land while the first
         one's are with the tail) */
      const size_t rc = h->rec_cap, tc = h->tp_cap;
      const int dev = G_device;
      HB_twin = new std::thread([rc, tc, dev]()
        { HIP_CHECK(hipSetDevice(dev));
          HostBuf *t = hostbuf_new();
          t->rec_cap = rc;  t->tp_cap = tc;
          HIP_CHECK(hipHostMalloc((void **) &t->recs, sizeof(LaRecord) * rc, hipHostMallocDefault));
          HIP_CHECK(hipHostMalloc((void **) &t->tpool, sizeof(u16) * tc, hipHostMallocDefault));
          std::lock_guard<std::mutex> lk(HB_mu);
          HB_free.push_back(t);
        });
    }
  h->nrec = nrec;  h->ntp = ntp;
  return h;
}

/* Asynchronous mode (damar_set_async(1)): the host side runs as a two-stage pipeline behind the GPU (host/tail.cpp):
 * tails in submission order, then the sort and write of the files.  damar_async_drain() must be called before the
 * blocks or the Align_Spec involved are released, and before the counters are read. */
static bool G_tail_reports = false;          /* a tail job writes its number of confirmed hits into the caller's job struct (damar_match with -v) */
extern "C" void damar_async_drain(void)
{ if (!A_on)
    return;
  finish_all();
  tail_drain();
}

extern "C" void damar_set_async(int on)
{ if (on && !A_on)
    { tail_start();
      A_on = true;
    }
  else if (!on && A_on)
    { damar_async_drain();
      tail_stop();
      A_on = false;
      helpers_join();
    }
}

/* totals since the last call: confirmed records, tail ms, write ms (drains first) */
extern "C" void damar_async_totals(int64 *ncheck, double *tail_ms, double *write_ms)
{ const double d0 = now_ms();
  damar_async_drain();
  H_ms[7] += now_ms() - d0;
  if (getenv("DAMAR_HOSTPROF"))
    { fprintf(stderr, "damar host wall ms:");
      for (int i = 0; i < 8; i++)
        { fprintf(stderr, " %s=%.1f", H_name[i], H_ms[i]);
          H_ms[i] = 0;
        }
      fprintf(stderr, " | between calls=%.1f launch->next front=%.1f flush->exit=%.1f entry->front=%.1f front->tick0=%.1f\n",
              Q_ms[2], Q_ms[3], Q_seg[0], Q_seg[2], Q_seg[3]);
      Q_ms[2] = Q_ms[3] = 0;  Q_exit = 0;  Q_seg[0] = Q_seg[2] = Q_seg[3] = 0;
    }
  tail_totals(ncheck, tail_ms, write_ms);
}

/* milliseconds the downloads of the asynchronous mode took since the last call (drains first) */
extern "C" double damar_async_d2h_ms(void)
{ damar_async_drain();
  return tail_d2h_ms();
}

/***** Match_Filter **********************************************************************************/

static std::vector<u64> G_seed_keys;
static std::vector<u32> G_seed_vals;
static int  G_seed_pbits = 0, G_seed_abits = 0, G_seed_dbits = 0;
static int  G_keep_seeds = 0;

static int64 sizeof_db(const HITS_DB *db)      /* db/DB.c:726 sizeof_DB without tracks */
{ return (int64) sizeof(HITS_DB) + (int64) sizeof(HITS_READ) * (db->nreads + 2) + db->totlen + db->nreads + 4 +
         (db->path ? (int64) strlen(db->path) + 1 : 0);
}


/* A comparison with more seed pairs than the seed arrays can hold is run in SLABS: consecutive ranges of B reads, each
   with its own merge, seed sort, work list and place in a report launch.  The seed key is bread-major and the report
   work is independent per (bread, aread) run (filter.c:2210-2241), so the slabs' sorted lists one after the other are
   the list of the whole comparison; the reference's thread slices are placed from the whole list's figures (`off`,
   `total`; kernels/seed_merge.hip slice_ends). */
struct SlabPlan
{ int  n;                        /* slabs (1: the comparison in one piece) */
  bool mem_bound;                /* cap comes from the free device memory: the slabs run one at a time in one slot */
  std::vector<int>   b_lo;       /* [n + 1] slab s holds the B reads [b_lo[s], b_lo[s + 1]) */
  std::vector<int64> hits;       /* [n] its seed pairs */
  std::vector<u64>   off;        /* [n] seed pairs of the slabs before it */
  u64  total, cap;
  u32  limit;                    /* the cap on mutual matches of the whole comparison */
};
static SlabPlan &G_plan = *new SlabPlan();
static int64 G_slab_tot[2] = { 0, 0 };      /* seed stages run, comparisons split (damar_slab_totals) */

/* The greedy cut: a slab takes B reads while its seed pairs stay <= cap, and always at least one.  b_lo[0 .. n] and
   sums[0 .. n-1] for up to max_slabs slabs; returns n, -(r + 1) when read r alone has more than cap seed pairs, or 0
   when max_slabs is too small. */
extern "C" int damar_slab_cut(const uint64_t *hits, int nreads, uint64_t cap, int *b_lo, int64 *sums, int max_slabs)
{ int n = 0;
  uint64_t acc = 0;
  if (max_slabs < 1)
    return 0;
  b_lo[0] = 0;
  for (int r = 0; r < nreads; r++)
    { if (hits[r] > cap)
        return -(r + 1);
      if (r > b_lo[n] && acc + hits[r] > cap)
        { sums[n++] = (int64) acc;
          if (n >= max_slabs)
            return 0;
          b_lo[n] = r;
          acc = 0;
        }
      acc += hits[r];
    }
  sums[n++] = (int64) acc;
  b_lo[n] = nreads;
  return n;
}

/* What the seed stage of one comparison leaves on the device for the report launch. */
struct Front
{ const u64 *keys;  const u32 *vals;  u64 total;
  const u32 *work;  u32 nwork;
  const u32 *order;
  int pbits, abits, dbits;
  JobParams jp;                 /* parameters and options of the moment the seed stage ran */
  size_t bytes;                 /* of the two arenas that hold the above */
  double t_entry;
};

/* The switches of the seed stage.  Read from the environment once per process, by the first seed stage (front_opts). */
struct FrontOpts
{ int pack_seeds;   /* DAMAR_PACK_SEEDS (1): a seed is ONE u64 when position-in-B fits beside the sort key; 0 forces the
                       diagonal into a second array (front_setup) */
  int early_cut;    /* DAMAR_EARLY_CUT (0).  Measured on config 2: 38 % of the seed pairs belong to read pairs with >= 3 seeds
                       (76.4 M seeds, 42.9 M read pairs, 5.8 M of them with >= 3), so the cut saves 3.7 of the 6 sort passes
                       but costs a 4-pass sort of the pair ids and two more passes over the seeds: merge + sort + work list
                       203 -> 209 ms per step.  Off unless asked for; with a B-read range (a pair split over GPUs) it keeps
                       only that range's seeds. */
  int two_step;     /* DAMAR_WORK_TWOSTEP (0): 1 = heads, then their screen (rounds 1-5; tested) */
  int pair_sort;    /* DAMAR_SORT_PAIR (1): 0 = never sort over the read pair only (the sort over all the bits, rounds 1-6),
                       1 or unset: always (both tested; front_setup has the rule) */
  int order_mode;   /* DAMAR_ORDER (11): 0 = reference order, 1 = most seeds first, 2 = size classes, 9 = longest seed extent
                       first, 10 = longest geometric overlap first, 11 = the larger of the two (default: 356 ms of report
                       kernel per config-2 step against 370 for 1, 361 for 9, 411 for 10), other n = runs of >= n seeds first */
};
static const FrontOpts &front_opts(void)
{ static FrontOpts o;
  static bool filled = false;
  if (!filled)
    { const char *e;
      o.pack_seeds = (e = getenv("DAMAR_PACK_SEEDS")) ? atoi(e) : 1;
      o.early_cut  = (e = getenv("DAMAR_EARLY_CUT")) ? atoi(e) : 0;
      o.two_step   = ((e = getenv("DAMAR_WORK_TWOSTEP")) && atoi(e) > 0) ? 1 : 0;
      o.pair_sort  = (e = getenv("DAMAR_SORT_PAIR")) ? atoi(e) : 1;
      o.order_mode = (e = getenv("DAMAR_ORDER")) ? atoi(e) : 11;
      filled = true;
    }
  return o;
}

/* A seed stage in progress: what its steps hand to each other.  (Front, above, is what outlives the stage.) */
struct SeedStage
{ damar_match_job *job;
  int    slab;                   /* < 0: the whole comparison */
  Arena *hits, *ord;             /* the arenas of the job's slot: sorted seed pairs; work list and processing order */
  double t_entry;
  MergeArgs m;                   /* with the key widths pbits / abits / dbits and the cap on mutual matches */
  int    bbits, sbits, idbits;   /* bits of a B read; of the sort key (pbits + abits + bbits); of a read pair (abits + bbits) */
  int    minhit;                 /* seeds a run needs to be a work item */
  bool   cut;                    /* the early cut is on for this stage */
  size_t bmwords;                /* its bitmap over the pair ids */
  u32    mtiles;                 /* merge workspace (G_work): */
  void  *mw;  u32 *tcount;  u64 *tot;  void *mscw;
  u64    total;                  /* seed pairs (after the early cut: the survivors) */
  int64  nhits;                  /* seed pairs the merge counted */
  u64    s_off, s_all;           /* where this stage's seeds lie in the whole comparison's list */
  u64   *keys;  u32 *vals;       /* the sorted side (in *hits) */
  u64   *tk;                     /* the idle side */
  u32   *flags, *foff;  void *scw2;  u64 *sends;
  void  *resort_ws, *order_ws;   /* only where the sort over the read pair may need them */
  bool   psort;                  /* the seeds are sorted over the read pair only */
  int    hshift;                 /* slices of the reference's threads in the head test (-1: applied already) */
  u32   *work;  u32 nwork;
  const u32 *order;
};

/* From the job to the merge's arguments and the layout of the seed key: the 64-bit check, the rule for packed seeds, the
   slab's range of B reads and cap (G_plan), and which of the alternative paths this stage takes (cut, psort).  Resets
   *f, and for the whole comparison (slab < 0) the job's counts and G_plan.  Leaves s.m and the widths; false when an
   index is empty.  Host arithmetic only: no device work, no wait. */
static bool front_setup(SeedStage &s, damar_match_job *job, int slot, Front *f, int slab)
{ const HITS_DB *ablock = job->ablock, *bblock = job->bblock;
  const damar_dev_index *aidx = job->aidx, *bidx = job->bidx;
  const FrontOpts &o = front_opts();
  memset(&s, 0, sizeof(s));
  s.job = job;  s.slab = slab;
  s.hits = &G_hitsJ[slot];  s.ord = &G_ordJ[slot];
  s.t_entry = now_ms();
  pick_sort_shape();
  memset(f, 0, sizeof(*f));
  f->t_entry = s.t_entry;
  f->jp = params_now();
  if (slab < 0)
    { job->counts[0] = job->counts[1] = job->counts[2] = 0;
      G_plan.n = 1;  G_plan.mem_bound = false;  G_plan.total = 0;
      G_plan.b_lo.assign(2, 0);  G_plan.b_lo[1] = bblock->nreads;
      G_plan.hits.assign(1, 0);  G_plan.off.assign(1, 0);
    }
  if (aidx == NULL || bidx == NULL || aidx->n == 0 || bidx->n == 0)
    return false;
  if (aidx->kbits != bidx->kbits)
    { fprintf(stderr, "damar: internal error, index parameters differ\n");
      die();
    }
  MergeArgs &m = s.m;
  m.acode = aidx->codes;  m.apos = aidx->pos;  m.alen = aidx->n;
  m.bcode = bidx->codes;  m.bpos = bidx->pos;  m.blen = bidx->n;
  m.wide = aidx->wide;
  m.kbits = aidx->kbits;
  m.self = job->self;  m.comp = job->comp;  m.identity = IDENTITY;
  m.limit = (MEM_LIMIT > 0) ? MAXGRAM : 0x7fffffffu;      /* filter.c:2700-2702 */
  m.b_lo = 0;  m.b_hi = 0xffffffffu;
  if (slab >= 0)                                          /* the cap is the whole comparison's, the B reads the slab's */
    { m.limit = G_plan.limit;
      m.b_lo = (u32) G_plan.b_lo[slab];  m.b_hi = (u32) G_plan.b_lo[slab + 1];
    }
  m.ablk = aidx->blk->d;  m.bblk = bidx->blk->d;
  m.pbits = std::max(1, ilog2_ceil((u64) ablock->maxlen + 1));
  m.abits = std::max(1, ilog2_ceil((u64) ablock->nreads));
  s.bbits = std::max(1, ilog2_ceil((u64) bblock->nreads));
  s.sbits = m.pbits + m.abits + s.bbits;
  s.idbits = m.abits + s.bbits;                           /* a read pair as one number: bread << abits | aread */
  if (s.sbits > 64)
    { fprintf(stderr, "damar: FATAL: seed key needs %d bits (> 64)\n", s.sbits);
      die();
    }
  /* Packed seeds: when position-in-B fits beside the sort key, a seed is ONE u64 (pair | apos | bpos) and the sort moves
     8 bytes per seed instead of 12; otherwise the diagonal travels in a second array (DAMAR_PACK_SEEDS=0 forces that) */
  const int db = std::max(1, ilog2_ceil((u64) bblock->maxlen + 1));
  m.dbits = (o.pack_seeds && s.sbits + db <= 64) ? db : 0;

  s.minhit = (P_hitmin - 1) / P_kmer + 1;
  const bool ranged = P_bread_lo > 0 || P_bread_hi != 0xffffffffu;      /* one part of a block pair split over GPUs */
  s.cut = (o.early_cut || ranged) && !G_keep_seeds && s.idbits <= 32;
  s.bmwords = (((size_t) 1 << (s.idbits <= 32 ? s.idbits : 32)) + 31) / 32;
  /* The seed sort over the READ PAIR only (its abits + bbits of the key's sbits: 4 passes instead of 6).  The seeds of a
     pair then lie in index order; the screen of the run heads takes them in any order and the runs of the kept heads -- all
     the report kernel walks -- are put in order of their A positions where they lie (kernels/seed_merge.hip order_runs).
     Not when something else reads the seeds (the tests' seed list, the two-step work list), not for the unpacked layout,
     not for the early cut's survivors.
     The ordering goes by the length of a run (a wavefront's registers up to 512 seeds, a workgroup beyond), which made
     it cheap enough to be on for every shape -- profiles/order_runs.txt has config 2, config 3 and config 4's lead both
     ways; until then a rule by the seed pairs per work item kept it to config 4's shape. */
  s.psort = o.pair_sort != 0 && !s.cut && !o.two_step && !G_keep_seeds && m.dbits != 0 && m.pbits + 11 <= 32 && m.pbits >= 8;
  s.hshift = P_nshift;
  return true;
}

/* For the tests (only while damar_last_seeds keeps the seed list: a blocking copy): how many tiles of the COUNT sweep
   just completed were left to the general kernel -- those merge_fast did not mark as done (MergeTile.pad[2]). */
static void front_note_flagged(SeedStage &s)
{ G_merge_flagged = -1;
  if (!G_keep_seeds)
    return;
  std::vector<MergeTile> tl(s.mtiles);
  HIP_CHECK(hipMemcpy(tl.data(), s.mw, sizeof(MergeTile) * (size_t) s.mtiles, hipMemcpyDeviceToHost));
  G_merge_flagged = 0;
  for (const MergeTile &t : tl)
    G_merge_flagged += (t.pad[2] == 0);
}

/* The merge's COUNT sweep over s.m (for a slab: with merge_range behind it) and the scan of the tile totals.  Starts
   the stage's clock (the host-profile lines, tick(0)), takes the merge workspace from G_work and leaves mw / tcount /
   tot / mscw and s.total.  One host wait: stream_wait for the total. */
static void front_count(SeedStage &s)
{ MergeArgs &m = s.m;
  s.mtiles = damar_merge_tiles(m.alen);
  if (Q_flush > 0)
    { Q_ms[3] += now_ms() - Q_flush;  Q_flush = 0; }
  Q_seg[3] += now_ms() - s.t_entry;
  tick(0);
  arena_reserve(&G_work, pad256(damar_merge_workspace_bytes(m.alen)) + pad256(damar_scan_workspace_bytes(s.mtiles)) + 4096);
  s.mw = arena_take(&G_work, damar_merge_workspace_bytes(m.alen));
  s.tcount = damar_merge_tile_counts(s.mw, m.alen);
  s.tot = (u64 *) arena_take(&G_work, 64);
  s.mscw = arena_take(&G_work, damar_scan_workspace_bytes(s.mtiles));
  damar_launch_merge_count(&m, s.mw, NULL, 0, G_st);
  if (s.slab >= 0)
    damar_launch_merge_range(&m, s.mw, G_st);
  stage("merge_count");
  damar_exclusive_scan_u32(s.tcount, s.tcount, s.mtiles, s.mscw, s.tot, G_st);
  stage("merge_scan");
  HIP_CHECK(hipMemcpyAsync(&s.total, s.tot, sizeof(u64), hipMemcpyDeviceToHost, G_st));
  stream_wait(G_st);
  front_note_flagged(s);
}

/* The reference's words for too little memory (filter.c:2634-2699), behind `lead`. */
static void low_memory_text(const char *lead)
{ fputs(lead, stderr);
  if (MEM_LIMIT == MEM_PHYSICAL)
    fprintf(stderr, " physical memory (%.1fGb), reduce block size\n", (1. * MEM_LIMIT) / 0x40000000ll);
  else
    { fprintf(stderr, " memory allocation (%.1fGb),", (1. * MEM_LIMIT) / 0x40000000ll);
      fprintf(stderr, " reduce block size or increase allocation\n");
    }
  fflush(stderr);
}

/* The cap on mutual matches of a whole comparison (filter.c:2634-2699; a slab runs under the cap its comparison
   settled).  The counts of front_count keep every run below MAXGRAM; the reference lowers that cap to the first mutual
   count at which the kept seeds no longer fit `avail`.  That only happens under memory pressure, so the histogram is
   built only then: COUNT with the histogram and a wait, then COUNT and scan under the lower cap and a wait.  Reads
   s.total and the merge workspace; leaves G_limit, s.m.limit and s.total. */
static void front_adapt_limit(SeedStage &s)
{ MergeArgs &m = s.m;
  if (MEM_LIMIT <= 0)
    { G_limit = 0x7fffffff;
      return;
    }
  const damar_match_job *job = s.job;
  int   limit = MAXGRAM;
  int64 avail = (int64) (MEM_LIMIT - (uint64) (sizeof_db(job->ablock) + sizeof_db(job->bblock))) / 16;
  if (job->aidx == job->bidx || avail > (int64) m.alen + 2 * (int64) m.blen)
    avail = (avail - m.alen) / 2;
  else
    avail = avail - ((int64) m.alen + m.blen);
  avail = (int64) (avail * .98);
  if ((int64) s.total > avail)
    { std::vector<unsigned long long> histo(MAXGRAM);
      unsigned long long *dgram = (unsigned long long *) dmalloc(sizeof(unsigned long long) * MAXGRAM);
      HIP_CHECK(hipMemsetAsync(dgram, 0, sizeof(unsigned long long) * MAXGRAM, G_st));
      damar_launch_merge_count(&m, s.mw, dgram, MAXGRAM, G_st);          /* the same sweep, with the run histogram */
      HIP_CHECK(hipMemcpyAsync(histo.data(), dgram, sizeof(unsigned long long) * MAXGRAM, hipMemcpyDeviceToHost, G_st));
      HIP_CHECK(hipStreamSynchronize(G_st));
      HIP_CHECK(hipFree(dgram));
      int64 tom = 0;
      int   j;
      for (j = 0; j < MAXGRAM; j++)
        { tom += (int64) j * (int64) histo[j];
          if (tom > avail)
            break;
        }
      limit = j;
      if (limit <= 1)
        { low_memory_text("\nError: Insufficient ");
          exit(1);
        }
      if (limit < 10)
        low_memory_text("\nWarning: Sensitivity hampered by low ");
      /* count again with the lower cap */
      m.limit = (u32) limit;
      damar_launch_merge_count(&m, s.mw, NULL, 0, G_st);
      damar_exclusive_scan_u32(s.tcount, s.tcount, s.mtiles, s.mscw, s.tot, G_st);
      HIP_CHECK(hipMemcpyAsync(&s.total, s.tot, sizeof(u64), hipMemcpyDeviceToHost, G_st));
      HIP_CHECK(hipStreamSynchronize(G_st));
      front_note_flagged(s);
    }
  G_limit = limit;
  if (VERBOSE)
    printf("\n   Capping mutual k-mer matches over %d (effectively -t%d)\n", limit, (int) sqrt(1. * limit));
}

/* What the seed stage of `n` seed pairs reserves: in the comparison's own arena (front_hits_bytes), in the shared one
   (front_tmp_bytes), with the early cut -- whose survivors are at most n -- in the shared arenas of the cut
   (front_cut_bytes), and for the work list (front_ord_bytes).  The steps reserve by these expressions and the number of
   seed pairs a seed stage can hold (seed_cap) is derived from them; each stands above the step whose takes it covers. */
static size_t front_hits_bytes(u64 n);
static size_t front_tmp_bytes(u64 n);
static size_t front_cut_bytes(u64 n, int minhit, size_t bmwords);
static size_t front_ord_bytes(u64 n, int minhit);
/* what arena_reserve(a, need) would take from the device beyond what the arena holds */
static size_t arena_growth(const Arena &a, size_t need)
{ if (need <= a.cap)
    return 0;
  const size_t cap = need + (need >> 3) + (1u << 20);
  return cap - a.cap;
}
static size_t front_growth(u64 n, const Arena &hits, const Arena &ord, bool cut, int minhit, size_t bmwords)
{ const size_t own = arena_growth(hits, front_hits_bytes(n)) + arena_growth(ord, front_ord_bytes(n, minhit));
  if (!cut)
    return own + arena_growth(G_tmp, front_tmp_bytes(n));
  return own + arena_growth(G_tmp, front_cut_bytes(n, minhit, bmwords)) + arena_growth(G_tmp2, front_tmp_bytes(n));
}

/* The most seed pairs one seed stage may have: below the 32-bit seed index (work items, the tile scans), and no more
   than the arenas of ONE comparison slot (seed pairs, work list) and the shared seed-stage arenas can be grown to hold in
   HALF the device memory that is free now.  The other half is left to what follows a seed stage and cannot be sized
   before it has run: the report launch's record and trace buffers, which grow with the records found.  A comparison cut
   by this figure (*mem_bound) runs its slabs one at a time in that one slot -- each slab's launch is completed before
   the next slab's seed stage starts (damar_match_batch) -- so no second slot's arenas grow beside it and the figure
   holds for every slab, not only the first.
   The device is asked only when `total` seed pairs would make an arena grow -- a comparison that fits what the arenas
   hold costs nothing here.  Test hooks: DAMAR_TEST_SEED_CAP=<n> replaces the figure; DAMAR_TEST_FREE_BYTES=<n> stands
   for the free device memory (and the device is not asked). */
static u64 seed_cap(u64 total, const Arena &hits, const Arena &ord, bool cut, int minhit, size_t bmwords, bool *mem_bound)
{ const u64 index_cap = 0xfffffff0ull - 1;
  const char *e = getenv("DAMAR_TEST_SEED_CAP");
  *mem_bound = false;
  if (e != NULL && atoll(e) > 0)
    return (u64) atoll(e);
  const u64 top = std::min(total, index_cap);
  if (front_growth(top, hits, ord, cut, minhit, bmwords) == 0)
    return index_cap;
  size_t free_b = 0, total_b = 0;
  e = getenv("DAMAR_TEST_FREE_BYTES");
  if (e != NULL && atoll(e) > 0)
    free_b = (size_t) atoll(e);
  else
    HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
  free_b /= 2;
  if (front_growth(top, hits, ord, cut, minhit, bmwords) <= free_b)
    return index_cap;
  u64 lo = 0, hi = top;                        /* the largest n whose arenas fit (growth is monotone in n) */
  while (lo < hi)
    { const u64 mid = lo + (hi - lo + 1) / 2;
      if (front_growth(mid, hits, ord, cut, minhit, bmwords) <= free_b) lo = mid; else hi = mid - 1;
    }
  *mem_bound = true;
  return lo;
}

/* Hits known: does the stage hold them?  For the whole comparison: seed_cap, and when s.total is beyond it the seed
   pairs per B read from what the COUNT sweep left (merge_bread_hist, built only now, with tick(1) and a wait), the
   greedy cut into G_plan, the merge lap -- and true: FRONT_SPLIT.  For a slab: its count against the plan's.  Leaves
   s_off / s_all, and counts the stage in G_slab_tot[0] when it goes on. */
static bool front_plan_slabs(SeedStage &s)
{ const u64 total = s.total;
  const int slab = s.slab;
  s.s_off = 0;  s.s_all = total;
  if (slab < 0)
    { G_plan.total = total;  G_plan.hits[0] = s.nhits;  G_plan.limit = s.m.limit;
      const u64 cap = seed_cap(total, *s.hits, *s.ord, s.cut, s.minhit, s.bmwords, &G_plan.mem_bound);
      G_plan.cap = cap;
      if (total > cap)
        { const int nrb = s.job->bblock->nreads;
          std::vector<unsigned long long> hist((size_t) nrb);
          unsigned long long *dh = (unsigned long long *) dmalloc(sizeof(unsigned long long) * (size_t) nrb);
          HIP_CHECK(hipMemsetAsync(dh, 0, sizeof(unsigned long long) * (size_t) nrb, G_st));
          damar_launch_merge_bread_hist(&s.m, s.mw, dh, G_st);   /* (reads the entries' counts and B starts, which the scan has not touched) */
          HIP_CHECK(hipMemcpyAsync(hist.data(), dh, sizeof(unsigned long long) * (size_t) nrb, hipMemcpyDeviceToHost, G_st));
          tick(1);
          HIP_CHECK(hipStreamSynchronize(G_st));
          HIP_CHECK(hipFree(dh));
          stage("bread_hist");
          G_plan.b_lo.assign((size_t) nrb + 2, 0);  G_plan.hits.assign((size_t) nrb + 1, 0);
          const int ns = damar_slab_cut((const uint64_t *) hist.data(), nrb, cap, G_plan.b_lo.data(), G_plan.hits.data(), nrb + 1);
          if (ns < 0)
            { fprintf(stderr, "damar: FATAL: B read %d alone has %llu seed pairs, more than the %llu one seed stage holds\n",
                      -ns - 1, hist[(size_t) (-ns - 1)], (unsigned long long) cap);
              die();
            }
          G_plan.n = ns;
          G_plan.b_lo.resize((size_t) ns + 1);  G_plan.hits.resize((size_t) ns);
          G_plan.off.assign((size_t) ns, 0);
          u64 sum = 0;
          for (int x = 0; x < ns; x++)
            { G_plan.off[x] = sum;  sum += (u64) G_plan.hits[x]; }
          if (sum != total)
            { fprintf(stderr, "damar: internal error, %llu seed pairs by B read, %llu counted\n", (unsigned long long) sum,
                      (unsigned long long) total);
              die();
            }
          G_slab_tot[1] += 1;
          if (VERBOSE)
            { printf("   Seed stage in %d slabs of at most %llu hits\n", ns, (unsigned long long) cap);
              fflush(stdout);
            }
          G_ms[DAMAR_T_MERGE] += lap(0, 1);
          return true;
        }
    }
  else
    { if (total != (u64) G_plan.hits[slab])
        { fprintf(stderr, "damar: internal error, slab %d has %llu seed pairs, %lld expected\n", slab, (unsigned long long) total,
                  (long long) G_plan.hits[slab]);
          die();
        }
      s.s_off = G_plan.off[slab];  s.s_all = G_plan.total;
    }
  G_slab_tot[0] += 1;
  return false;
}

/* The stage's laps and counts: merge and sort laps, G_cnt[0], the job's counts[0]; and when the stage `worked` (it got
   as far as a work list) the work lap, G_cnt[1] and -- for the tests -- the download of the sorted seeds (a blocking
   copy).  The stream has been waited for when this is called: the events of tick(0..3) are complete. */
static void front_account(SeedStage &s, bool worked)
{ G_ms[DAMAR_T_MERGE] += lap(0, 1);
  G_ms[DAMAR_T_SSORT] += lap(1, 2);
  G_cnt[0] += s.nhits;
  s.job->counts[0] += s.nhits;
  if (!worked)
    return;
  G_ms[DAMAR_T_WORK] += lap(2, 3);
  G_cnt[1] += s.nwork;
  if (G_keep_seeds)
    { const size_t at = s.slab >= 0 ? G_seed_keys.size() : 0;   /* (a slab's seeds behind those of the slabs before it: damar_match_batch clears) */
      G_seed_keys.resize(at + s.total);  G_seed_vals.resize(at + s.total);
      HIP_CHECK(hipMemcpy(G_seed_keys.data() + at, s.keys, sizeof(u64) * (size_t) s.total, hipMemcpyDeviceToHost));
      if (s.vals != NULL)
        HIP_CHECK(hipMemcpy(G_seed_vals.data() + at, s.vals, sizeof(u32) * (size_t) s.total, hipMemcpyDeviceToHost));
      G_seed_pbits = s.m.pbits;  G_seed_abits = s.m.abits;  G_seed_dbits = s.m.dbits;
    }
}

/* The two sides of a seed sort: it starts on k0 / v0 and must end on `home`, in the comparison's own arena (NULL: either
   side will do). */
struct SortBufs { u64 *k0, *k1;  u32 *v0, *v1;  void *sw;  u64 *home; };

/* The arenas of a seed sort over n seed pairs and of the work list made from its result.  arena_take starts every take
   on a multiple of 256; pad256(x) >= x + 256 pays for that.
     front_hits_bytes, the own arena:  pad256(8 n)  pk, the sorted keys
                                       pad256(4 n)  pv, their values (the unpacked layout only)
                                       4096         spare
     front_tmp_bytes, the shared one:  pad256(8 n)  tk, the other side of the keys
                                       pad256(4 n)  tv, of the values (unpacked only); the packed layout takes order_ws in
                                                    its room, 8 (n / 513 + 1) bytes, as the last take (front_emit_sort_plain)
                                       pad256(sort) sw
                                       pad256(4 n)  flags
                                       pad256(4 n)  foff, also the heads' bit words: max(4 n, bit_words_bytes(n)), which is
                                                    beyond 4 n by less than 512 bytes, and only below 128 seed pairs
                                       pad256(scan) scw2
                                       8192         sends (512 and its 256), the 512 of foff */
static size_t front_hits_bytes(u64 n)
{ return pad256(sizeof(u64) * (size_t) n) + pad256(sizeof(u32) * (size_t) n) + 4096; }
static size_t front_tmp_bytes(u64 n)
{ return pad256(sizeof(u64) * (size_t) n) + 3 * pad256(sizeof(u32) * (size_t) n) +
         pad256(damar_sort_workspace_bytes(n)) + pad256(damar_scan_workspace_bytes(n)) + 8192;
}
/* Reserves both arenas and takes the ping-pong set of a sort of `passes` passes: it is started from the side that makes
   the result land in the own arena.  Leaves tk, flags, foff, scw2 and sends in s.  (Reserving may wait for the stream
   and free, when an arena has to grow.) */
static SortBufs take_sort_bufs(SeedStage &s, Arena &own, Arena &shared, u64 n, int passes)
{ const bool packed = s.m.dbits != 0;
  SortBufs b;
  arena_reserve(&own, front_hits_bytes(n));
  arena_reserve(&shared, front_tmp_bytes(n));
  u64 *pk = (u64 *) arena_take(&own, sizeof(u64) * (size_t) n);
  u32 *pv = packed ? NULL : (u32 *) arena_take(&own, sizeof(u32) * (size_t) n);
  s.tk = (u64 *) arena_take(&shared, sizeof(u64) * (size_t) n);
  u32 *tv = packed ? NULL : (u32 *) arena_take(&shared, sizeof(u32) * (size_t) n);
  b.k0 = (passes & 1) ? s.tk : pk;  b.k1 = (passes & 1) ? pk : s.tk;
  b.v0 = (passes & 1) ? tv : pv;    b.v1 = (passes & 1) ? pv : tv;
  b.sw = arena_take(&shared, damar_sort_workspace_bytes(n));
  b.home = pk;
  s.flags = (u32 *) arena_take(&shared, sizeof(u32) * (size_t) n);
  s.foff  = (u32 *) arena_take(&shared, std::max(sizeof(u32) * (size_t) n, bit_words_bytes(n)));   /* (also the heads' bit words) */
  s.scw2  = arena_take(&shared, damar_scan_workspace_bytes(n));
  s.sends = (u64 *) arena_take(&shared, 64 * sizeof(u64));
  return b;
}

/* The seed sort of n seeds from b.k0 / b.v0: over the read pair only (`pair_only`) or over all of the key; keys alone
   in the packed layout.  Queues the sort's error word (sort_check).  With b.home the result must lie there and becomes
   s.keys / s.vals.  Returns the side the result is on.  No wait. */
static int sort_seeds(SeedStage &s, const SortBufs &b, u64 n, bool pair_only)
{ const MergeArgs &m = s.m;
  const int side = m.dbits ? damar_radix_sort_keys_u64(b.k0, b.k1, n, m.dbits + (pair_only ? m.pbits : 0), m.dbits + s.sbits, b.sw, G_st)
                           : damar_radix_sort_u64(b.k0, b.v0, b.k1, b.v1, n, s.sbits, b.sw, G_st);
  sort_check(b.sw);
  if (b.home == NULL)
    return side;
  s.keys = side ? b.k1 : b.k0;
  s.vals = side ? b.v1 : b.v0;
  if (s.keys != b.home)
    { fprintf(stderr, "damar: internal error, the seed sort ended on the wrong side\n");
      die();
    }
  return side;
}

/* EMIT and the seed sort without the early cut: the sorted seed pairs stay in the comparison's own arena until the
   report launch, everything else lives in G_tmp, which the comparisons share.  Reads s.total and the merge workspace;
   leaves keys / vals and the buffers of take_sort_bufs, resort_ws, and with psort order_ws.  tick(1) behind the emit.
   No wait. */
static void front_emit_sort_plain(SeedStage &s)
{ const int passes = ((s.psort ? s.sbits - s.m.pbits : s.sbits) + 7) / 8;          /* sort_scan.hip: 8 bits per pass */
  const SortBufs b = take_sort_bufs(s, *s.hits, G_tmp, s.total, passes);
  s.resort_ws = b.sw;
  if (s.psort)                                             /* (in the room of tv: the packed layout has no values) */
    s.order_ws = arena_take(&G_tmp, damar_order_runs_scratch_bytes(s.total));
  damar_launch_merge_emit(&s.m, s.mw, s.total, b.k0, b.v0, NULL, G_st);
  stage("merge_emit");
  tick(1);
  sort_seeds(s, b, s.total, s.psort);
}

/* What the early cut takes from G_tmp for n seed pairs before its survivors are known, term by term:
     pad256(8 n)                   uk, the unsorted keys
     4 pad256(4 n)                 uv, their values; pid0 and pid1, the pair ids and the other side of their sort; hbit,
                                   the head bits (n / 8 bytes used)
     pad256(4 (n / minhit + 64))   hd, the heads
     pad256(sort), pad256(scan)    sw, scc
     pad256(4 bmwords)             bitmap
     16384                         snd (512 and its 256) */
static size_t front_cut_bytes(u64 n, int minhit, size_t bmwords)
{ return pad256(sizeof(u64) * (size_t) n) + 4 * pad256(sizeof(u32) * (size_t) n) +
         pad256(sizeof(u32) * ((size_t) n / minhit + 64)) +
         pad256(damar_sort_workspace_bytes(n)) + pad256(damar_scan_workspace_bytes(n)) +
         pad256(sizeof(u32) * bmwords) + 16384;
}
/* EMIT and the seed sort with the early cut (kernels/seed_merge.hip): only the seeds of the read pairs report_thread
   enters go through the seed sort.  The pair ids are sorted on their own (4 B per seed instead of 12, 4 passes instead
   of 6), the reference's head test runs on them, and the seeds of the surviving pairs -- a few per cent -- are compacted
   out of the unsorted seeds and sorted over all the bits (take_sort_bufs in G_tmp2).  Two waits: for the number of
   heads, for the number of survivors.  Leaves what front_emit_sort_plain leaves, with s.total the survivors and
   hshift = -1; false when nothing survives, and the stage's account is then closed here (no work lap). */
static bool front_emit_sort_cut(SeedStage &s)
{ const MergeArgs &m = s.m;
  const u64 total = s.total;
  arena_reserve(&G_tmp, front_cut_bytes(total, s.minhit, s.bmwords));
  u64 *uk   = (u64 *) arena_take(&G_tmp, sizeof(u64) * (size_t) total);
  u32 *uv   = (u32 *) arena_take(&G_tmp, sizeof(u32) * (size_t) total);
  u32 *pid0 = (u32 *) arena_take(&G_tmp, sizeof(u32) * (size_t) total);
  u32 *pid1 = (u32 *) arena_take(&G_tmp, sizeof(u32) * (size_t) total);
  u32 *hbit = (u32 *) arena_take(&G_tmp, sizeof(u32) * (size_t) total);          /* head bits: total / 8 bytes used */
  u32 *hd   = (u32 *) arena_take(&G_tmp, sizeof(u32) * ((size_t) total / s.minhit + 64));
  void *sw  = arena_take(&G_tmp, damar_sort_workspace_bytes(total));
  void *scc = arena_take(&G_tmp, damar_scan_workspace_bytes(total));
  u32 *bitmap = (u32 *) arena_take(&G_tmp, sizeof(u32) * s.bmwords);
  u64 *snd  = (u64 *) arena_take(&G_tmp, 64 * sizeof(u64));

  damar_launch_merge_emit(&m, s.mw, total, uk, uv, pid0, G_st);
  stage("merge_emit");
  tick(1);
  const u32 *spid = damar_radix_sort_keys_u32(pid0, pid1, total, s.idbits, sw, G_st) ? pid1 : pid0;
  sort_check(sw);
  u64 n64 = 0;
  damar_launch_pair_heads_ids(spid, total, s.s_off, s.s_all, m.abits, s.minhit, P_nshift, snd, (u64 *) hbit, scc, s.tot, hd, G_st);
  HIP_CHECK(hipMemsetAsync(bitmap, 0, sizeof(u32) * s.bmwords, G_st));
  HIP_CHECK(hipMemcpyAsync(&n64, s.tot, sizeof(u64), hipMemcpyDeviceToHost, G_st));
  HIP_CHECK(hipStreamSynchronize(G_st));
  damar_launch_pair_bitmap(spid, hd, (u32) n64, m.abits, P_bread_lo, P_bread_hi, bitmap, G_st);
  damar_launch_seed_cut_count(uk, total, m.pbits + m.dbits, bitmap, (u32 *) scc, s.tot, G_st);
  HIP_CHECK(hipMemcpyAsync(&n64, s.tot, sizeof(u64), hipMemcpyDeviceToHost, G_st));
  HIP_CHECK(hipStreamSynchronize(G_st));
  stage("early_cut");
  const u64 nsurv = n64;
  G_cnt[6] += (int64) nsurv;
  if (nsurv == 0)
    { tick(2);  tick(3);
      front_account(s, false);
      return false;
    }
  const SortBufs b = take_sort_bufs(s, *s.hits, G_tmp2, nsurv, (s.sbits + 7) / 8);
  damar_launch_seed_cut_scatter(uk, m.dbits ? NULL : uv, total, m.pbits + m.dbits, bitmap, (const u32 *) scc, b.k0, b.v0, G_st);
  sort_seeds(s, b, nsurv, false);
  s.total  = nsurv;              /* from here on: the seeds of the read pairs that are entered, nothing else */
  s.hshift = -1;                 /* (the slice rule of the head test has been applied on the pair ids) */
  return true;
}

/* The work list and its processing order (the comparison's second arena: they outlive the seed stage), for nw work
   items: pad256(4 nw) five times for `work` (nw + 1 words) and front_order's ok0, ov0, ok1, ov1; pad256(sort) for its
   osw; 8192 spare.  A work item is the head of a run of at least minhit seeds, so n seed pairs make at most n / minhit. */
static size_t work_list_bytes(u64 nw)
{ return 5 * pad256(sizeof(u32) * (size_t) nw) + pad256(damar_sort_workspace_bytes(nw)) + 8192; }
static size_t front_ord_bytes(u64 n, int minhit)
{ return work_list_bytes(n / (u64) minhit + 1); }

/* Heads and screen in one pass over the sorted seeds: a bit per seed (in foff), the work list expanded from the bits
   once its length is known.  tick(3) behind pair_work, then the comparison's last wait: nothing after it needs the host
   again.  When the seeds were sorted over the read pair only and a kept run is too long for order_runs (more than 2048
   seeds: a tandem array against itself, a satellite), the seeds are sorted over all the bits after all -- from where
   they lie, the order of equal keys has not changed -- and the work list is made again, with a second wait.  Leaves
   work / nwork in *s.ord, the kept runs in order of their A positions, and psort as it turned out. */
static void front_work_onepass(SeedStage &s)
{ const MergeArgs &m = s.m;
  u64 got[2] = { 0, 0 };                               /* work items; a run order_runs would not sort */
  damar_launch_pair_work(s.keys, s.vals, s.total, s.s_off, s.s_all, m.pbits, m.dbits, m.abits, s.minhit, s.hshift, s.sends,
                         (u64 *) s.foff /* bit words */, s.scw2, s.tot, P_binshift, P_kmer, P_hitmin, P_bread_lo, P_bread_hi,
                         s.psort ? 1 : 0, G_st);
  stage("run_heads");
  tick(3);                                             /* (the expansion of the bits behind it is 4 us: outside the clock) */
  HIP_CHECK(hipMemcpyAsync(got, s.tot, 2 * sizeof(u64), hipMemcpyDeviceToHost, G_st));
  stream_wait(G_st);
  if (s.psort && got[1] != 0)
    { G_cnt[7] += 1;
      if (s.keys == s.tk || s.resort_ws == NULL)
        { fprintf(stderr, "damar: internal error, no room to sort the seeds again\n");
          die();
        }
      const SortBufs again = { s.keys, s.tk, NULL, NULL, s.resort_ws, NULL };
      if (sort_seeds(s, again, s.total, false))
        HIP_CHECK(hipMemcpyAsync(s.keys, s.tk, sizeof(u64) * (size_t) s.total, hipMemcpyDeviceToDevice, G_st));
      damar_launch_pair_work(s.keys, s.vals, s.total, s.s_off, s.s_all, m.pbits, m.dbits, m.abits, s.minhit, s.hshift, s.sends,
                             (u64 *) s.foff, s.scw2, s.tot, P_binshift, P_kmer, P_hitmin, P_bread_lo, P_bread_hi, 0, G_st);
      HIP_CHECK(hipMemcpyAsync(got, s.tot, 2 * sizeof(u64), hipMemcpyDeviceToHost, G_st));
      stream_wait(G_st);
      s.psort = false;
    }
  const u64 nwork64 = got[0];
  arena_reserve(s.ord, work_list_bytes(nwork64));
  s.work = (u32 *) arena_take(s.ord, sizeof(u32) * ((size_t) nwork64 + 1));
  if (nwork64 > 0)
    { damar_launch_pair_work_expand((const u64 *) s.foff, s.scw2, s.total, s.work, G_st);
      if (s.psort)                                     /* the runs the report kernel will walk, in the order of their A positions */
        damar_launch_order_runs(s.keys, s.total, m.pbits, m.dbits, s.work, (u32) nwork64, s.order_ws, G_st);
    }
  stage("work_list");
  s.nwork = (u32) nwork64;
}

/* DAMAR_WORK_TWOSTEP=1: the run heads into the idle key buffer, then their screen (dense, one thread each) and the
   compaction of the survivors; flags / foff are reused.  Two waits: for the number of heads (the work list is reserved
   for that many), and behind tick(3) for the number of work items.  Leaves work / nwork in *s.ord. */
static void front_work_twostep(SeedStage &s)
{ const MergeArgs &m = s.m;
  u64 nwork64 = 0;
  u32 *heads = (u32 *) s.tk;
  damar_launch_pair_heads(s.keys, s.total, s.s_off, s.s_all, m.pbits + m.dbits, m.abits, s.minhit, s.hshift, s.sends,
                          (u64 *) s.foff /* bit words */, s.scw2, s.tot, heads, G_st);
  stage("run_heads");
  HIP_CHECK(hipMemcpyAsync(&nwork64, s.tot, sizeof(u64), hipMemcpyDeviceToHost, G_st));
  HIP_CHECK(hipStreamSynchronize(G_st));
  const u32 nheads = (u32) nwork64;
  arena_reserve(s.ord, work_list_bytes(nheads));
  s.work = (u32 *) arena_take(s.ord, sizeof(u32) * ((size_t) nheads + 1));
  nwork64 = 0;
  if (nheads > 0)
    { damar_launch_pair_screen(s.keys, s.vals, s.total, m.pbits, m.dbits, heads, nheads, s.minhit, P_binshift, P_kmer, P_hitmin,
                               m.abits, P_bread_lo, P_bread_hi, s.flags, G_st);
      damar_exclusive_scan_u32(s.flags, s.foff, nheads, s.scw2, s.tot, G_st);
      damar_launch_compact_u32(heads, s.flags, s.foff, nheads, s.work, G_st);
      stage("work_list");
      HIP_CHECK(hipMemcpyAsync(&nwork64, s.tot, sizeof(u64), hipMemcpyDeviceToHost, G_st));
    }
  tick(3);
  HIP_CHECK(hipStreamSynchronize(G_st));
  s.nwork = (u32) nwork64;
}

/* Largest pairs first (FrontOpts::order_mode; the order only schedules the kernel: records carry their work item's rank
   in the reference's order): a cost per work item, and the items sorted by it.  Takes its buffers from *s.ord behind
   the work list (front_ord_bytes covers them) and leaves s.order, NULL for the reference's order.  No wait. */
static void front_order(SeedStage &s)
{ const MergeArgs &m = s.m;
  const int order_mode = front_opts().order_mode;
  const u32 nwork = s.nwork;
  if (nwork <= 1 || order_mode <= 0)
    return;
  u32 *ok0 = (u32 *) arena_take(s.ord, sizeof(u32) * (size_t) nwork);
  u32 *ov0 = (u32 *) arena_take(s.ord, sizeof(u32) * (size_t) nwork);
  u32 *ok1 = (u32 *) arena_take(s.ord, sizeof(u32) * (size_t) nwork);
  u32 *ov1 = (u32 *) arena_take(s.ord, sizeof(u32) * (size_t) nwork);
  void *osw = arena_take(s.ord, damar_sort_workspace_bytes(nwork));
  const u32 cmode = order_mode == 2 ? 1u : order_mode == 9 ? 0xffffffffu : order_mode == 10 ? 0xfffffffeu :
                    order_mode == 11 ? 0xfffffffdu : order_mode == 12 ? 0xfffffffcu : (order_mode > 2 ? (u32) order_mode : 0u);
  damar_launch_work_cost(s.keys, s.vals, s.total, m.pbits, m.abits, m.dbits, m.ablk.boff, m.bblk.boff, s.work, nwork, cmode, ok0, ov0, G_st);
  s.order = damar_radix_sort_u32(ok0, ov0, ok1, ov1, nwork, WORK_COST_BITS, osw, G_st) ? ov1 : ov0;
  sort_check(osw);
  stage("work_order");
}

/* Seed stage of one comparison (filter.c:2603-2760): merge-count, scan, emit, seed sort, work list and its
   processing order, into the arenas of job slot `slot`.  Returns FRONT_NONE when there is nothing to report, FRONT_READY
   with *f filled, or -- called with slab < 0, for the whole comparison -- FRONT_SPLIT when the comparison has more seed
   pairs than one seed stage holds: G_plan then says how it is cut, and the caller runs the slabs (slab = 0, 1, ...),
   each an ordinary seed stage over its range of B reads. */
enum { FRONT_NONE = 0, FRONT_READY = 1, FRONT_SPLIT = 2 };
static int match_front(damar_match_job *job, int slot, Front *f, int slab)
{ SeedStage s;
  if (!front_setup(s, job, slot, f, slab))
    return FRONT_NONE;
  front_count(s);
  if (slab < 0)                                   /* (a slab: the whole comparison's call has settled the cap) */
    front_adapt_limit(s);
  s.nhits = (int64) s.total;
  if (VERBOSE && slab < 0)
    { printf("   Hit count = %lld\n", (long long) s.nhits);
      fflush(stdout);
    }
  if (s.total == 0)
    return FRONT_NONE;
  if (front_plan_slabs(s))
    return FRONT_SPLIT;
  if (!s.cut)
    front_emit_sort_plain(s);
  else if (!front_emit_sort_cut(s))
    return FRONT_NONE;
  stage("seed_sort");
  tick(2);
  if (front_opts().two_step)
    front_work_twostep(s);
  else
    front_work_onepass(s);
  sort_verify();
  front_account(s, true);
  front_order(s);

  f->keys = s.keys;  f->vals = s.vals;  f->total = s.total;
  f->work = s.work;  f->nwork = s.nwork;  f->order = s.order;
  f->pbits = s.m.pbits;  f->abits = s.m.abits;  f->dbits = s.m.dbits;
  f->bytes = s.hits->cap + s.ord->cap;
  return s.nwork > 0 ? FRONT_READY : FRONT_NONE;
}

/* A report launch over up to DAMAR_MAX_JOBS comparisons, in two halves.  In asynchronous mode the launch goes to its own
   stream and is completed only when the NEXT launch is due (or at a drain): the kernel is bound by instruction issue and
   dependent latency, the seed stage of the following comparisons by HBM, and the two share the machine (tools/corun.hip:
   a register-heavy persistent kernel and a streaming kernel finish together in 80 % of the time they take one after the
   other).  Up to two launches are in flight -- one running, one queued behind it on the stream, so that the device goes
   from one to the next without the host -- while the seed stages of later comparisons accumulate; every comparison holds
   one of DAMAR_MAX_JOBS slots (arenas of its sorted seeds and work list, its SCORE/TABLE copy) from its seed stage until
   its launch has been completed. */
struct Comparison
{ int  slot;
  damar_match_job  job;                           /* a copy: the caller's array may be gone when the launch completes */
  damar_match_job *orig;                          /* the caller's struct (counts) while its call is still running */
  Front fr;
  const damar_dev_block *ablk, *bblk;             /* (an index may be released before a re-launch) */
};
struct Pending
{ bool live;
  int  n;
  Comparison c[DAMAR_MAX_JOBS];
  int  amax, bmax, tsmin;
  u32  cell_cap, rec_cap, tp_cap;
  int  t8;                                        /* the launch's trace values leave the device as bytes (ReportArgs.t8) */
  bool wide_ok;                                   /* the two-pair kernel runs: pairs beyond the packed pebble format go to the wide kernel */
  bool wide_done;                                 /* the wide kernel has run behind this attempt's launch */
  u32  wm_off[DAMAR_MAX_JOBS + 1];                /* the jobs' bit maps in RS.widemap (words) */
  int  attempt;
  int  oset;                                      /* the set of record buffers, counters and timers this launch uses */
  hipEvent_t done;                                /* behind the kernel */
  hipStream_t st;
  double t_launch;
  ReportArgs ra[DAMAR_MAX_JOBS];                  /* what the launch was given (the upload is asynchronous) */
  std::vector<TailJob *> writes;                  /* damar_write_overlaps requests that wait for this launch's tails */
};
static Pending *PQ = new Pending[2]();               /* PQ[i] uses output set i */
static int      PQ_head = 0, PQ_n = 0;             /* the oldest launch in flight, how many there are */
static bool     G_slot_busy[DAMAR_MAX_JOBS];

/* Comparisons whose seed stages are done and whose report launch has not been made yet.  In asynchronous mode a launch is
   held back while it would be SMALL: a launch ends by waiting for its longest alignment (a 15 kb read pair is some 10 ms of
   serial wave steps), so a launch over two comparisons of a sparse block pair (config 4: ~1 600 alignments each) costs as
   much as one over sixteen.  The comparisons of later calls join it until it holds DAMAR_BATCH_WORK read pairs or its set of
   job arenas is full; the files of the block pairs in it wait with it (damar_write_overlaps). */
struct Accum
{ int    n;
  Comparison c[DAMAR_MAX_JOBS / 2];
  size_t bytes;
  u64    nwork;
  std::vector<TailJob *> writes;
};
static Accum &AC = *new Accum();

/* The switches of the report stage.  Read from the environment once per process, by the first use (report_opts). */
struct ReportOpts
{ long long adapt_ratio;  /* DAMAR_ADAPT_RATIO (4000): seed pairs per work item above which a co-running launch takes fewer
                             wavefronts per SIMD (report_slots); 0 = never */
  int  adapt_wps;         /* DAMAR_ADAPT_WPS (3, at least 1): that many */
  int  queue_depth;       /* DAMAR_LAUNCH_QUEUE (1; 2 = the next launch is queued behind the running one).  Two takes the host
                             out of the hand-over, but measured SLOWER on config 2: 434 - 445 ms per step against 398 - 410
                             with one.  With one, the host waits for the running launch before it makes the next, so the seed
                             stream is idle during the last third of every launch -- the phase in which the kernel works
                             through the many short read pairs, whose band filters hammer the bucket arrays; seed sorts that
                             run beside that phase take 180 instead of 100 ms per step. */
  int  device_t8;         /* DAMAR_DEVICE_T8 (1): trace values leave the device as bytes where every comparison of the launch
                             writes byte traces (launch_size); 0: 16-bit values, compressed by the host tail as until round 4 */
  int  batch;             /* DAMAR_BATCH (0 = by the mode: batch_limit; else 1 .. DAMAR_MAX_JOBS): comparisons per launch.
                             Report ms per config-2 step: 1 -> 357, 2 -> 340, 4 -> 335.5, 16 -> 335.3; every job in flight
                             keeps its sorted seed pairs (12 B each) in HBM, which a cold process pays for at ~25 ms per GB */
  long long batch_work;   /* DAMAR_BATCH_WORK (32768): read pairs a held-back launch waits for, four per wave slot */
  bool small_caps;        /* DAMAR_TEST_SMALL_CAPS, tests: the first launch starts far too small, so that the overflow flags
                             and the re-launch are exercised */
};
static const ReportOpts &report_opts(void)
{ static ReportOpts o;
  static bool filled = false;
  if (!filled)
    { const char *e;
      o.adapt_ratio = (e = getenv("DAMAR_ADAPT_RATIO")) ? atoll(e) : 4000;
      o.adapt_wps   = std::max(1, (e = getenv("DAMAR_ADAPT_WPS")) ? atoi(e) : 3);
      o.queue_depth = ((e = getenv("DAMAR_LAUNCH_QUEUE")) && atoi(e) == 2) ? 2 : 1;
      o.device_t8   = (e = getenv("DAMAR_DEVICE_T8")) ? atoi(e) : 1;
      o.batch       = (e = getenv("DAMAR_BATCH")) ? atoi(e) : 0;
      if (o.batch != 0)
        o.batch = std::min(std::max(o.batch, 1), DAMAR_MAX_JOBS);
      o.batch_work  = (e = getenv("DAMAR_BATCH_WORK")) ? atoll(e) : 32768;
      o.small_caps  = getenv("DAMAR_TEST_SMALL_CAPS") != NULL;
      filled = true;
    }
  return o;
}

static std::mutex &A_mu = *new std::mutex();      /* the four totals below (the tail keeps its own: host/tail.cpp) */
static int64   A_nfilt = 0;                        /* totals of the asynchronous mode (damar_async_counts) */
static int64   W_tot[3] = { 0, 0, 0 };             /* band cells, wave steps per pass, wave-loop iterations (damar_wave_totals) */
static double  A_report_ms = 0;
static int64   A_launches = 0;

/* How much of the machine a launch of the two-pair kernel takes (r6).  A launch that fills every wave slot keeps the seed
   stream's next kernel waiting until its wavefronts retire; where the seed stages are the longer side -- a plan of many
   sparse block pairs: config 4 has 9 000 seed pairs per read pair that reaches the kernel, config 2 1 300, config 3 300 --
   a co-running launch runs on DAMAR_ADAPT_WPS wavefronts per SIMD (3) instead of all 8: it takes a quarter longer and the
   seed kernels run beside it the whole time (first 300 block pairs of config 4: 1.69 -> 1.58 s, profiles/r06_sweeps.txt).
   DAMAR_ADAPT_RATIO = seed pairs per work item above which that happens (4 000; 0 = never).  Returns the launch's slots. */
static int report_slots(const Pending &pd)
{ const ReportOpts &o = report_opts();
  int nslots = RS.nslots;
  if (o.adapt_ratio > 0 && corun_on() && pd.st == G_rep)
    { u64 seeds = 0, work = 0;
      for (int j = 0; j < pd.n; j++)
        { seeds += pd.c[j].fr.total;  work += pd.c[j].fr.nwork; }
      const int low = G_prop.multiProcessorCount * 4 * damar_report2_slots_per_wave() * o.adapt_wps;
      if (work > 0 && seeds / work > (u64) o.adapt_ratio && low < nslots)
        nslots = low;
    }
  return nslots;
}

/* Launches pd's comparisons on pd.st with the caps of pd into output set pd.oset: scratch and output buffers (which may
   wait for that set's last download), the jobs' arguments, the zeroed wide map and counters, the kernel between the set's
   two kernel timers, pd.done behind it.  Leaves pd.ra, wm_off, wide_ok and pd.live.  No wait for the launch; the host
   waits only where a buffer has to grow (scratch_prepare, scratch_outputs, the wide map: allocations) and for a spec's
   tables when they changed (fill_report_args: upload and hipStreamSynchronize(st)). */
static void report_launch(Pending &pd)
{ ReportArgs *const ra = pd.ra;
  const hipStream_t st = pd.st;
  double q0 = now_ms();
  RS.cur = pd.oset;
  scratch_prepare(pd.amax, pd.bmax, pd.c[0].fr.jp.binshift, pd.tsmin, pd.cell_cap, st);
  double q1 = now_ms();
  scratch_outputs(pd.rec_cap, pd.tp_cap);
  double q2 = now_ms();
  Q_ms[0] += q1 - q0;  Q_ms[1] += q2 - q1;
  bool packed = true;
  for (int j = 0; j < pd.n; j++)
    { const Comparison &c = pd.c[j];
      const Front &fr = c.fr;
      fill_report_args(&ra[j], c.ablk, c.bblk, c.job.comp, c.job.self, c.job.spec, st, j, c.slot, fr.jp);
      ra[j].keys = fr.keys;  ra[j].vals = fr.vals;  ra[j].nhits = fr.total;
      ra[j].work = fr.work;  ra[j].nwork = fr.nwork;
      ra[j].pbits = fr.pbits;  ra[j].abits = fr.abits;  ra[j].dbits = fr.dbits;
      ra[j].order = fr.order;
      ra[j].t8 = pd.t8;
      ra[j].widemap = NULL;  ra[j].wcells = RS.wcells;  ra[j].wcell_cap = RS.wcell_cap;  ra[j].cell_max = max_cells();
      packed = packed && use_packed(&ra[j], pd.amax, pd.bmax);
      if (ra[j].mscore != ra[0].mscore || ra[j].dscore != ra[0].dscore)
        { fprintf(stderr, "damar: internal error, the comparisons of one report launch differ in their -e\n");
          die();
        }
    }
  pd.wide_ok = packed;  pd.wide_done = false;
  if (!packed && std::max(pd.amax, pd.bmax) / std::max(1, pd.tsmin) + 8 > DAMAR_MAX_MARKS)
    { fprintf(stderr, "damar: FATAL: reads of %d bases need a trace spacing (-s) of at least %d when one read pair per wavefront "
                      "is asked for (DAMAR_PACKED=0): the wide kernel runs behind the two-pair kernel only\n",
              std::max(pd.amax, pd.bmax), std::max(pd.amax, pd.bmax) / (DAMAR_MAX_MARKS - 8) + 1);
      die();
    }
  if (packed)
    { /* one bit per work item and job, zero at every launch: which read pairs are the wide kernel's (kernels/report.hip) */
      u32 words = 0;
      for (int j = 0; j < pd.n; j++)
        { pd.wm_off[j] = words;
          words += (ra[j].nwork + 31) / 32 + 1;
        }
      pd.wm_off[pd.n] = words;
      const int c = pd.oset;
      if (RS.widemap_cap[c] < words)
        { if (RS.widemap[c]) HIP_CHECK(hipFree(RS.widemap[c]));
          RS.widemap_cap[c] = words + (words >> 2) + 1024;
          RS.widemap[c] = (u32 *) dmalloc(sizeof(u32) * (size_t) RS.widemap_cap[c]);
        }
      HIP_CHECK(hipMemsetAsync(RS.widemap[c], 0, sizeof(u32) * (size_t) words, st));
      for (int j = 0; j < pd.n; j++)
        ra[j].widemap = RS.widemap[c] + pd.wm_off[j];
    }
  HIP_CHECK(hipMemsetAsync(RS.ctr, 0, sizeof(u32) * DAMAR_COUNTER_WORDS, st));
  tick_on(set_ev(pd.oset, SET_KERNEL_BEGIN), st);
  if (packed)
    damar_launch_report2(ra, pd.n, NULL, 0, report_slots(pd), st);
  else
    damar_launch_report(ra, pd.n, RS.nslots, st);
  tick_on(set_ev(pd.oset, SET_KERNEL_END), st);
  if (pd.done == NULL)
    HIP_CHECK(hipEventCreateWithFlags(&pd.done, hipEventDisableTiming));
  HIP_CHECK(hipEventRecord(pd.done, st));
  pd.live = true;
  pd.t_launch = now_ms();
}

/* The steps of report_finish, over the launch pd and the counters hc[DAMAR_COUNTER_WORDS] as last read behind it. */

/* Waits for pd.done -- this launch only: a younger one may be queued behind it on the same stream -- and fetches the
   set's counters into hc over G_ctl (a second, short wait).  Adds the kernel's lap to the report time and counts the
   launch. */
static void report_wait(Pending &pd, u32 *hc)
{ HIP_CHECK(hipEventSynchronize(pd.done));
  late_streams();
  HIP_CHECK(hipMemcpyAsync(hc, RS.counters + (size_t) pd.oset * DAMAR_COUNTER_WORDS, sizeof(u32) * DAMAR_COUNTER_WORDS, hipMemcpyDeviceToHost, G_ctl));
  HIP_CHECK(hipStreamSynchronize(G_ctl));
  HIP_CHECK(hipGetLastError());
  { const float ms = lap(set_ev(pd.oset, SET_KERNEL_BEGIN), set_ev(pd.oset, SET_KERNEL_END));
    G_ms[DAMAR_T_REPORT] += ms;
    if (A_on)
      { std::lock_guard<std::mutex> lk(A_mu);
        A_report_ms += ms;
        A_launches += 1;
      }
  }
  G_cnt[5] += 1;
}

/* Read pairs beyond the packed pebble format (reads of more than DAMAR_MAX_MARKS trace spacings; alignments that
   overflowed the pebble pool at its largest, 2^18): the wide kernel takes them, into the same record buffers, behind
   the launch that is otherwise complete.  Until round 5 both were fatal.  Reads hc; when the wide kernel is due and no
   other flag is up, zeroes the jobs' cursors and the flag word, launches it on pd.st, records pd.done behind it and
   returns true: the caller waits and reads the counters again.  No wait. */
static bool report_wide_pass(Pending &pd, const u32 *hc)
{ if (!pd.wide_ok || pd.wide_done || hc[DAMAR_CNT_WIDE] == 0)
    return false;
  u32 flags = hc[DAMAR_CNT_FLAGS];
  if (pd.cell_cap >= max_cells())
    flags &= ~DAMAR_ERR_CELLS;                             /* (those pairs are in the map: nothing to repeat for them) */
  if (flags != 0)
    return false;
  wide_pool_ensure();
  for (int j = 0; j < pd.n; j++)
    { pd.ra[j].wcells = RS.wcells;  pd.ra[j].wcell_cap = RS.wcell_cap; }
  if (VERBOSE)
    fprintf(stderr, "damar: %u read pair(s) beyond the packed pebble format: wide kernel\n", hc[DAMAR_CNT_WIDE]);
  u32 *const ctr = RS.counters + (size_t) pd.oset * DAMAR_COUNTER_WORDS;
  HIP_CHECK(hipMemsetAsync(ctr + DAMAR_CNT_CURSOR, 0, sizeof(u32) * DAMAR_MAX_JOBS, pd.st));      /* the work lists once more */
  HIP_CHECK(hipMemsetAsync(ctr + DAMAR_CNT_FLAGS, 0, sizeof(u32), pd.st));
  damar_launch_report_wide(pd.ra, pd.n, wide_slots(), pd.st);
  HIP_CHECK(hipEventRecord(pd.done, pd.st));
  pd.wide_done = true;
  return true;
}

/* From the flags in hc to the next attempt.  Returns false when the launch is complete.  Otherwise something ran over:
   the wide kernel's own pool (grown here, behind a wait for pd.st; nothing else changes and everything runs once more),
   or what the flags name -- pebbles, the ring, byte traces, records, trace values -- which grows in pd or G_ring; the
   launch is made again and true returned.  Fatal: a wave past its loop bound, the seventh attempt, 2^32 trace values. */
static bool report_retry(Pending &pd, const u32 *hc)
{ u32 flags = hc[DAMAR_CNT_FLAGS];
  bool repeat = false;                                     /* the launch is repeated though no flag may be left */
  if (pd.wide_done && (flags & DAMAR_ERR_CELLS))
    { HIP_CHECK(hipStreamSynchronize(pd.st));
      wide_pool_grow();
      flags &= ~DAMAR_ERR_CELLS;
      repeat = true;
    }
  else if (pd.wide_ok && pd.cell_cap >= max_cells() && hc[DAMAR_CNT_WIDE] > 0)
    flags &= ~DAMAR_ERR_CELLS;                             /* the packed kernel's overflows at 2^18 are the wide kernel's pairs */
  if (flags == 0 && !repeat)
    return false;
  if ((flags & DAMAR_ERR_BAND) && !(flags & (DAMAR_ERR_CELLS | DAMAR_ERR_WIDE)))
    { fprintf(stderr, "damar: FATAL: a Local_Alignment wave exceeded its loop bound (where=%u)\n", hc[DAMAR_CNT_WHERE]);
      die();
    }
  if (pd.attempt >= 6)
    { fprintf(stderr, "damar: FATAL: report kernel keeps overflowing its buffers (flags %u)\n", flags);
      die();
    }
  pd.attempt += 1;
  if (flags & DAMAR_ERR_CELLS) pd.cell_cap = grow_cells(pd.cell_cap);
  if (flags & DAMAR_ERR_WIDE)  G_ring *= 4;
  if (flags & DAMAR_ERR_T8)    pd.t8 = 0;         /* a value above 255: 16-bit values again, and the reference's check on what is written */
  if (flags & DAMAR_ERR_RECS)  pd.rec_cap = std::max(2 * pd.rec_cap, hc[DAMAR_CNT_RECS] + 1024);
  if (flags & DAMAR_ERR_TPOOL)
    { if (pd.tp_cap >= 0xe0000000u)
        { fprintf(stderr, "damar: FATAL: more than 2^32 trace values in one comparison, use smaller blocks\n");
          die();
        }
      pd.tp_cap = (u32) std::min<u64>(0xe0000000ull, std::max<u64>(2ull * pd.tp_cap, (u64) hc[DAMAR_CNT_TPOOL] + 65536));
    }
  if (VERBOSE)
    fprintf(stderr, "damar: report kernel overflow (flags %u), retrying with larger buffers\n", flags);
  report_launch(pd);
  return true;
}

/* Starts the download of the complete launch's records, trace values and -- when the wide kernel ran -- wide map into a
   host buffer, which it returns.  Asynchronous mode: on G_copy between the buffer's events, with the set's event
   behind it for whatever writes the set next; no wait (but for the wide map, copied synchronously).  Otherwise on pd.st,
   waited for here, with the d2h lap.  Then adds what was downloaded to the counts and the wave totals. */
static HostBuf *report_download(Pending &pd, const u32 *hc)
{ const hipStream_t st = pd.st;
  const int n = pd.n;
  const u32 nrec = hc[DAMAR_CNT_RECS], ntrace = hc[DAMAR_CNT_TPOOL];
  HostBuf *hb = hostbuf_get(nrec, ntrace);
  hb->users = n;
  late_streams();
  hipStream_t cs = A_on ? G_copy : st;
  if (A_on)
    HIP_CHECK(hipEventRecord(hb->e0, cs));       /* (the report kernel has completed: the host synced on it) */
  if (nrec > 0)
    { HIP_CHECK(hipMemcpyAsync(hb->recs, RS.recs_set[pd.oset], sizeof(LaRecord) * (size_t) nrec, hipMemcpyDeviceToHost, cs));
      HIP_CHECK(hipMemcpyAsync(hb->tpool, RS.tpool_set[pd.oset], (pd.t8 ? sizeof(u8) : sizeof(u16)) * (size_t) ntrace, hipMemcpyDeviceToHost, cs));
    }
  hb->t8 = pd.t8;
  hb->nwide = pd.wide_done ? hc[DAMAR_CNT_WIDE] : 0;
  if (hb->nwide > 0)
    { const u32 words = pd.wm_off[n];
      if (hb->wmap_cap < words)
        { free(hb->wmap);
          hb->wmap_cap = words + 1024;
          hb->wmap = (u32 *) malloc(sizeof(u32) * hb->wmap_cap);
        }
      memcpy(hb->wm_off, pd.wm_off, sizeof(hb->wm_off));
      HIP_CHECK(hipMemcpy(hb->wmap, RS.widemap[pd.oset], sizeof(u32) * (size_t) words, hipMemcpyDeviceToHost));
    }
  tick_on(set_ev(pd.oset, SET_D2H_END), st);
  if (A_on)
    { /* asynchronous mode: the download runs on its own stream beside the next comparison's merge and sorts; the
         tail thread waits for it, and so does the next report kernel (which would overwrite the device buffers) */
      HIP_CHECK(hipEventRecord(hb->e1, cs));
      hb->pending = true;
      /* (an event of the SET, not hb->e1: the host buffer is recycled, and a wait on its event would mean its next
         download -- the one out of the other set that has just been started) */
      HIP_CHECK(hipEventRecord(G_set_d2h[pd.oset], cs));
      G_last_d2h[pd.oset] = G_set_d2h[pd.oset];
    }
  else
    { HIP_CHECK(hipStreamSynchronize(st));
      G_ms[DAMAR_T_D2H] += lap(set_ev(pd.oset, SET_D2H_BEGIN), set_ev(pd.oset, SET_D2H_END));
    }
  G_cnt[3] += nrec;  G_cnt[4] += ntrace;
  { std::lock_guard<std::mutex> lk(A_mu);
    W_tot[0] += (int64) (((u64) hc[DAMAR_CNT_CELLS + 1] << 32) | hc[DAMAR_CNT_CELLS]);
    W_tot[1] += (int64) (((u64) hc[DAMAR_CNT_HALFSTEPS + 1] << 32) | hc[DAMAR_CNT_HALFSTEPS]);
    W_tot[2] += (int64) (((u64) hc[DAMAR_CNT_ITERS + 1] << 32) | hc[DAMAR_CNT_ITERS]);
  }
  return hb;
}

/* Hands the comparisons to the host tail in job order (filter.c:2442-2483 per read pair), each with its seed hits from
   hc added to the caller's counts: queued behind the download in asynchronous mode, run here otherwise (hb is complete
   then, and goes back when its last comparison is done).  Then queues the file writes that waited for these tails. */
static void report_hand_over(Pending &pd, const u32 *hc, HostBuf *hb)
{ const int n = pd.n;
  for (int j = 0; j < n; j++)
    { const Comparison &c = pd.c[j];
      const damar_match_job &jb = c.job;
      if (c.orig != NULL)
        c.orig->counts[1] += hc[DAMAR_CNT_NFILT + j];          /* (summed over a comparison's slabs) */
      G_cnt[2] += hc[DAMAR_CNT_NFILT + j];
      if (A_on)
        { { std::lock_guard<std::mutex> lk(A_mu);
            A_nfilt += hc[DAMAR_CNT_NFILT + j];
          }
          TailJob *tj = new TailJob();
          tj->kind = 0;
          tj->hb = hb;  tj->jobid = j;  tj->njobs = n;
          tj->ablock = *jb.ablock;  tj->bblock = *jb.bblock;
          tj->self = jb.self;  tj->comp = jb.comp;  tj->spec = jb.spec;
          tj->symmetric = c.fr.jp.symmetric;  tj->hgap_min = c.fr.jp.hgap_min;
          tj->got = (G_tail_reports && c.orig != NULL) ? &c.orig->counts[2] : NULL;   /* (only for a caller that drains before its job struct goes: damar_match) */
          tail_submit(tj);
        }
      else
        { double t0 = now_ms();
          const int64 got = damar_host_tail(hb->recs, hb->nrec, hb->tpool, hb->t8, hb->nwide ? hb->wmap + hb->wm_off[j] : (const u32 *) NULL, jb.ablock, jb.bblock,
                                            jb.self, jb.comp, jb.spec, c.fr.jp.symmetric, c.fr.jp.hgap_min, j, n, 0);
          if (c.orig != NULL)
            c.orig->counts[2] += got;
          if (--hb->users == 0)
            hostbuf_put(hb);
          G_ms[DAMAR_T_TAIL] += now_ms() - t0;
        }
    }
  for (TailJob *w : pd.writes)                   /* the files of these comparisons: behind their tails */
    tail_submit(w);
  pd.writes.clear();
}

/* Completes the launch in flight: waits for it, lets the wide kernel run behind it, re-launches with larger buffers after
   an overflow -- until an attempt leaves nothing to repeat -- then starts the download of the records and hands the
   comparisons to the host tail.  Host-profile laps: 3 to the complete launch, 4 the download, 5 the hand-over. */
static void report_finish(Pending &pd)
{ if (!pd.live)
    return;
  u32 hc[DAMAR_COUNTER_WORDS];
  const double h2 = now_ms();
  do
    report_wait(pd, hc);
  while (report_wide_pass(pd, hc) || report_retry(pd, hc));
  pd.live = false;
  tick_on(set_ev(pd.oset, SET_D2H_BEGIN), pd.st);
  const double h3 = now_ms();
  HostBuf *hb = report_download(pd, hc);
  const double h4 = now_ms();
  report_hand_over(pd, hc, hb);
  const double h5 = now_ms();
  H_ms[3] += h3 - h2;  H_ms[4] += h4 - h3;  H_ms[5] += h5 - h4;
}

/* completes the oldest launch in flight and releases its comparisons' slots */
static void finish_oldest(void)
{ if (PQ_n == 0)
    return;
  Pending &pd = PQ[PQ_head];
  report_finish(pd);
  for (int j = 0; j < pd.n; j++)
    G_slot_busy[pd.c[j].slot] = false;
  pd.n = 0;
  PQ_head ^= 1;
  PQ_n -= 1;
}

/* comparisons per launch where DAMAR_BATCH does not say */
static int batch_limit(void)
{ if (report_opts().batch != 0)
    return report_opts().batch;
  return corun_on() ? 2 : 4;                /* overlapped launches: short ones interleave better (548 against 590 ms) */
}

/* Write_Overlap_Buffer + Reset_Overlap_Buffer (daligner.c:1020-1021, 1055-1056), queued behind
 * the pending tails in asynchronous mode, immediate otherwise. */
extern "C" void damar_write_overlaps(Align_Spec *spec, const char *d1, const char *d2,
                                     const char *ablock, const char *bblock, int lastRead)
{ if (!A_on)
    { Write_Overlap_Buffer(spec, (char *) d1, (char *) d2, (char *) ablock, (char *) bblock, lastRead);
      Reset_Overlap_Buffer(spec);
      return;
    }
  TailJob *job = new TailJob();
  job->kind = 1;  job->spec = spec;
  job->has1 = d1 != NULL;  job->has2 = d2 != NULL;
  if (d1) job->d1 = d1;
  if (d2) job->d2 = d2;
  job->a = ablock;  job->b = bblock;  job->last = lastRead;
  for (int j = 0; j < AC.n; j++)                 /* comparisons of this spec are still waiting for their launch */
    if (AC.c[j].job.spec == spec)
      { AC.writes.push_back(job);
        return;
      }
  for (int q = PQ_n - 1; q >= 0; q--)            /* the tails of a launch in flight are not queued yet: behind them */
    { Pending &pd = PQ[(PQ_head + q) & 1];         /* (the youngest launch that holds the spec) */
      for (int j = 0; j < pd.n; j++)
        if (pd.c[j].job.spec == spec)
          { pd.writes.push_back(job);
            return;
          }
    }
  tail_submit(job);
}

/* SURVEY 8(d)'s secondary unit of K6, counted by the packed report kernel itself (scalar adds in its wave loop): band
   cells (diagonals computed, summed over all wave steps), wave steps counted per alignment pass (= per half-wavefront),
   and iterations of the wave loop (each steps one or two halves) -- totals since the last call (drains first) */
extern "C" void damar_wave_totals(int64 *cells, int64 *half_steps, int64 *iterations)
{ damar_async_drain();
  std::lock_guard<std::mutex> lk(A_mu);
  if (cells)      *cells = W_tot[0];
  if (half_steps) *half_steps = W_tot[1];
  if (iterations) *iterations = W_tot[2];
  W_tot[0] = W_tot[1] = W_tot[2] = 0;
}

/* totals of the asynchronous mode since the last call (drains first): seed hits (what damar_match's counts[1] reports in
   the synchronous mode) and the report kernel's milliseconds */
extern "C" void damar_async_counts(int64 *nfilt, double *report_ms, int64 *launches)
{ damar_async_drain();
  std::lock_guard<std::mutex> lk(A_mu);
  if (nfilt)     *nfilt = A_nfilt;
  if (report_ms) *report_ms = A_report_ms;
  if (launches)  *launches = A_launches;
  A_nfilt = 0;  A_report_ms = 0;  A_launches = 0;
}

/* DAMAR_OVERLAP: 1 = the report launch runs BESIDE the next comparisons' seed stages (its own stream, 4 of 5 wavefronts per
   SIMD); 2 = it runs on its own stream but the next seed stages wait for it on the device: the kernels follow each other
   as in mode 0, while the host (completion of the launch, download, tails) stays pipelined; 0 = launch, wait, tail. */
static int overlap_mode(void)
{ static int on = -1;
  if (on < 0)
    { const char *e = getenv("DAMAR_OVERLAP");
      on = e ? atoi(e) : 1;
    }
  /* only behind the asynchronous host tail (nobody reads the records at return), and not when the caller wants the
     per-comparison counts printed (-v) or the seeds kept */
  return (A_on && !VERBOSE && !G_keep_seeds) ? on : 0;
}
static bool overlap_on(void) { return overlap_mode() != 0; }
static bool corun_on(void)   { return overlap_mode() == 1; }

/* The steps of flush_accum: the comparisons held back become a launch. */

/* An entry of the launch queue, i.e. a set of output buffers, with AC's comparisons copied into it.  The oldest launch in
   flight is completed first while as many are in flight as may be (ReportOpts::queue_depth: it ran beside these seed
   stages), which waits for it.  Leaves pd.n, oset and c[]; the caller clears AC. */
static Pending &launch_take(void)
{ while (PQ_n >= report_opts().queue_depth)
    finish_oldest();
  Pending &pd = PQ[(PQ_head + PQ_n) & 1];
  pd.n = AC.n;
  pd.oset = (int) (&pd - PQ);
  for (int j = 0; j < pd.n; j++)
    pd.c[j] = AC.c[j];
  return pd;
}

/* What a launch over pd's comparisons, nwork read pairs in all, starts with:
     amax, bmax   the longest A and B read of any comparison;  tsmin  the smallest trace spacing
     cell_cap     pebbles per slot: what the scratch has (DEFAULT_CELLS at first), at most max_cells()
     rec_cap      records: what the launch's output set has, at least 2 nwork + 4096, at most 2^31 - 1
     tp_cap       trace values: what the set has, at least 256 per record, at most 0xe0000000
     t8           trace values as bytes off the device (align.c:3375-3396 Compress_TraceTo8, K8 of SURVEY 8a19):
                  ReportOpts::device_t8, and 0 unless every comparison of the launch writes byte traces (-s <= 125)
   (The set's own sizes: asking one set for the other's size plus headroom would grow both for ever.)  With
   ReportOpts::small_caps, while neither set has been sized: 64 pebbles, 16 records, 512 trace values.  Host arithmetic only. */
static void launch_size(Pending &pd, u64 nwork)
{ pd.amax = pd.bmax = 0;  pd.tsmin = 0x7fffffff;
  pd.t8 = report_opts().device_t8;
  for (int j = 0; j < pd.n; j++)
    { const damar_match_job &jb = pd.c[j].job;
      pd.amax = std::max(pd.amax, jb.ablock->maxlen);  pd.bmax = std::max(pd.bmax, jb.bblock->maxlen);
      pd.tsmin = std::min(pd.tsmin, Trace_Spacing(jb.spec));
      if (Trace_Spacing(jb.spec) > TRACE_XOVR)
        pd.t8 = 0;
    }
  const u32 rec_have = RS.rec_cap_set[pd.oset], tp_have = RS.tpool_cap_set[pd.oset];
  pd.cell_cap = std::min<u32>(RS.cell_cap ? RS.cell_cap : DEFAULT_CELLS, max_cells());
  pd.rec_cap  = (u32) std::min<u64>(0x7fffffffu, std::max<u64>(rec_have, 2 * nwork + 4096));
  pd.tp_cap   = (u32) std::min<u64>(0xe0000000ull, std::max<u64>(tp_have, (u64) pd.rec_cap * 256u));
  if (report_opts().small_caps && RS.rec_cap_set[0] == 0 && RS.rec_cap_set[1] == 0)
    { pd.cell_cap = 64;  pd.rec_cap = 16;  pd.tp_cap = 512; }
}

/* Launches the comparisons held back: takes a queue entry, sizes the launch, orders the streams and launches.  Behind
   the asynchronous tail (overlap_on) the launch goes to G_rep behind the seed stages on G_st (G_front_done), and at
   DAMAR_OVERLAP=2 the next seed stages go behind it (G_rep_done); otherwise it goes to G_st and is completed here. */
static void flush_accum(void)
{ if (AC.n == 0)
    return;
  const bool defer = overlap_on();
  Pending &pd = launch_take();
  launch_size(pd, AC.nwork);
  pd.attempt = 0;
  late_streams();
  pd.st = defer ? G_rep : G_st;
  for (TailJob *w : AC.writes)
    pd.writes.push_back(w);
  AC.writes.clear();
  if (defer)                                   /* the launch reads what the seed stages wrote on the other stream */
    { HIP_CHECK(hipEventRecord(G_front_done, G_st));
      HIP_CHECK(hipStreamWaitEvent(G_rep, G_front_done, 0));
    }
  PQ_n += 1;
  report_launch(pd);
  if (!defer)
    finish_oldest();
  else if (!corun_on())                        /* in order on the device: the next seed stages start behind this launch */
    { HIP_CHECK(hipEventRecord(G_rep_done, G_rep));
      HIP_CHECK(hipStreamWaitEvent(G_st, G_rep_done, 0));
    }
  AC.n = 0;  AC.bytes = 0;  AC.nwork = 0;
  Q_flush = now_ms();
}

/* everything this library still owes: the comparisons held back, then the launch in flight */
static void finish_all(void)
{ flush_accum();
  while (PQ_n > 0)
    finish_oldest();
}

/* a free comparison slot; when there is none, the oldest launch is completed (or, with nothing in flight, the comparisons
   held back are launched) */
static int slot_take(void)
{ for (;;)
    { for (int i = 0; i < DAMAR_MAX_JOBS; i++)
        if (!G_slot_busy[i])
          { G_slot_busy[i] = true;
            return i;
          }
      if (PQ_n > 0)
        finish_oldest();
      else
        flush_accum();
    }
}

/* Several comparisons with ONE report launch each time their seed stages are done (kernels.h: DAMAR_MAX_JOBS): the seed
   stages run one after the other, each into its own arena, then every wavefront of the report kernel works through all
   the work lists.  The output is that of damar_match called for jobs[0], jobs[1], ... in this order.  Launches are cut
   at DAMAR_BATCH jobs (default 4, at most DAMAR_MAX_JOBS) and whenever the seed arenas would pass a quarter of HBM. */
extern "C" void damar_match_batch(damar_match_job *jobs, int njobs)
{ ensure_init();
  const double h0 = now_ms();
  if (Q_exit > 0)
    Q_ms[2] += h0 - Q_exit;
  memset(G_cnt, 0, sizeof(G_cnt));
  G_slab_tot[0] = G_slab_tot[1] = 0;
  for (int i = DAMAR_T_MERGE; i < DAMAR_T_COUNT; i++)
    G_ms[i] = 0;
  const bool defer = overlap_on();
  if (!defer)
    finish_all();
  const size_t budget = G_prop.totalGlobalMem / 8;                        /* per launch; up to three groups of comparisons hold arenas */
  const int    hard = DAMAR_MAX_JOBS / 2;                                 /* two sets of job arenas */
  const int    soft = std::min(batch_limit(), hard);
  for (int i = 0; i < njobs; i++)
    { const double f0 = now_ms();
      /* one launch, one set of filter parameters and one scoring (the kernel's trim table): comparisons held back under
         other options go first */
      if (AC.n > 0)
        { const JobParams now = params_now();
          const JobParams &was = AC.c[0].fr.jp;
          const int16 *s0 = damar_spec_score_table(AC.c[0].job.spec), *s1 = damar_spec_score_table(jobs[i].spec);
          bool go = now.kmer != was.kmer || now.hitmin != was.hitmin || now.binshift != was.binshift ||
                    s0[32767] != s1[32767] || s0[0] != s1[0];
          /* an Align_Spec whose files are already asked for (damar_write_overlaps) belongs to a finished block pair: a
             new pair on the same spec must not reach its overlap buffers before that write has detached them */
          for (TailJob *w : AC.writes)
            go = go || w->spec == jobs[i].spec;
          if (go)
            flush_accum();
        }
      int slot = slot_take();                     /* (may complete a launch, or launch what is held back) */
      if (i == 0)
        Q_seg[2] += now_ms() - h0;
      /* a seed stage that has something to report joins the comparisons held back, and the rules that cut a launch apply */
      auto joined = [&](int got, int sl)
        { Comparison &c = AC.c[AC.n];               /* (c.fr is the seed stage's: match_front wrote it) */
          if (got != FRONT_READY)
            G_slot_busy[sl] = false;
          else
            { c.job = jobs[i];  c.orig = &jobs[i];  c.slot = sl;
              c.ablk = jobs[i].aidx->blk;  c.bblk = jobs[i].bidx->blk;
              AC.bytes += c.fr.bytes;
              AC.nwork += c.fr.nwork;
              AC.n += 1;
            }
          if (AC.n >= hard || AC.bytes > budget || (AC.n >= soft && (!defer || AC.nwork >= (u64) report_opts().batch_work)))
            flush_accum();
        };
      if (G_keep_seeds)                        /* (a comparison without seed pairs downloads nothing: not the list of an earlier one) */
        { G_seed_keys.clear();  G_seed_vals.clear(); }
      const int got = match_front(&jobs[i], slot, &AC.c[AC.n].fr, -1);
      if (got != FRONT_SPLIT)
        { H_ms[1] += now_ms() - f0;
          joined(got, slot);
          continue;
        }
      /* too many seed pairs for one seed stage: slab after slab, each a comparison of its own from here on.  Slabs
         without seeds, and those outside the caller's range of B reads (damar_set_bread_range), are not run. */
      const int slot0 = slot;
      bool first = true;
      for (int sb = 0; sb < G_plan.n; sb++)
        { if (G_plan.hits[sb] == 0)
            continue;
          if ((u32) G_plan.b_lo[sb + 1] <= P_bread_lo || (u32) G_plan.b_lo[sb] >= P_bread_hi)
            { jobs[i].counts[0] += G_plan.hits[sb];          /* (not run, but seed pairs of the comparison: counts[0] and */
              G_cnt[0] += G_plan.hits[sb];                   /*  counter 0 are the whole comparison's, as without slabs)  */
              continue;
            }
          if (slot < 0 && G_plan.mem_bound)
            { /* the figure holds for the arenas of one slot: what the slabs before this one owe is completed, and this
                 slab runs where they ran */
              finish_all();
              slot = slot0;
              G_slot_busy[slot] = true;
            }
          else if (slot < 0)
            slot = slot_take();
          if (G_keep_seeds && first)
            { G_seed_keys.clear();  G_seed_vals.clear(); }
          first = false;
          joined(match_front(&jobs[i], slot, &AC.c[AC.n].fr, sb), slot);
          slot = -1;
        }
      if (slot >= 0)
        G_slot_busy[slot] = false;
      H_ms[1] += now_ms() - f0;
    }
  if (!defer)
    flush_accum();
  for (int j = 0; j < DAMAR_MAX_JOBS; j++)         /* the caller's job structs end with this call */
    PQ[0].c[j].orig = PQ[1].c[j].orig = NULL;
  for (int j = 0; j < DAMAR_MAX_JOBS / 2; j++)
    AC.c[j].orig = NULL;
  Q_exit = now_ms();
  if (Q_flush > 0)
    Q_seg[0] += Q_exit - Q_flush;
  H_ms[6] += Q_exit - h0;
}

extern "C" void damar_match(const HITS_DB *ablock, const HITS_DB *bblock,
                            damar_dev_index *aidx, damar_dev_index *bidx,
                            int self, int comp, Align_Spec *spec, int64 *counts)
{ damar_match_job job;
  memset(&job, 0, sizeof(job));
  job.ablock = ablock;  job.bblock = bblock;  job.aidx = aidx;  job.bidx = bidx;
  job.self = self;  job.comp = comp;  job.spec = spec;
  G_tail_reports = VERBOSE != 0;                 /* -v: the confirmed hits are counted by the host tail, which may run behind this call */
  damar_match_batch(&job, 1);
  if (G_tail_reports)
    damar_async_drain();
  G_tail_reports = false;
  if (counts)
    { counts[0] = job.counts[0];  counts[1] = job.counts[1];  counts[2] = job.counts[2]; }
  if (VERBOSE)
    { printf("\n     %lld %d-mers\n     %lld seed hits\n     %lld confirmed hits\n",
             (long long) job.counts[0], P_kmer, (long long) job.counts[1], (long long) job.counts[2]);
      fflush(stdout);
    }
}

extern "C" void Match_Filter(char *aname, HITS_DB *ablock, char *bname, HITS_DB *bblock,
                             void *atable, int alen, void *btable, int blen, int comp, Align_Spec *asettings)
{ (void) alen;  (void) blen;
  if (VERBOSE)
    { if (comp) printf("\nComparing %s to c(%s)\n", aname, bname);
      else      printf("\nComparing %s to %s\n", aname, bname);
    }
  damar_match(ablock, bblock, (damar_dev_index *) atable, (damar_dev_index *) btable,
              aname == bname, comp, asettings, NULL);             /* filter.c:2603 pointer equality */
  if (atable != btable && btable != NULL)                         /* filter.c:2722-2731, 2880-2881 */
    damar_index_free((damar_dev_index *) btable);
}


/***** datander: Match_Self (scrub/tandem.c:1182-1428) ************************************************/

static int T_kmer = 12, T_binshift = 4, T_hitmin = 35, T_nshift = 2;

/* scrub/tandem.h:58 Set_Filter_Params(kmer, binshift, hitmin, nthreads): the 4-argument
 * variant of datander.  It cannot share a name with filter.h's 5-argument function inside one
 * library, so it is exported under this name; libdamar_tandem.so (csrc/tandem_abi.c) carries
 * the reference name for a datander.c that links against it. */
extern "C" int damar_tandem_set_params(int kmer, int binshift, int hitmin, int nthreads)
{ if (kmer <= 1)
    return 1;
  T_kmer = kmer;  T_binshift = binshift;  T_hitmin = hitmin;
  T_nshift = 0;
  while ((2 << T_nshift) <= nthreads)
    T_nshift += 1;
  return 0;
}

/* The wide kernel behind a two-pair launch of ONE job on G_st (datander: dist, the batch entry: tasks), for the reads /
   tasks that launch left to it (DAMAR_CNT_WIDE: reads of more than DAMAR_MAX_MARKS trace spacings, alignments that
   overflowed the pebble pool at its largest).  hc = the counters as read behind the launch, updated; a flag left in
   hc[DAMAR_CNT_FLAGS] means that the whole launch is to be repeated.  Returns whether the wide kernel ran (then the
   job's map says whose two-pair records are to be dropped). */
static bool wide_behind(ReportArgs &ra, u32 *hc, u32 cell_cap, const int *dist, const LaTask *tasks, u32 ntasks)
{ if (ra.widemap == NULL || hc[DAMAR_CNT_WIDE] == 0)
    return false;
  u32 flags = hc[DAMAR_CNT_FLAGS];
  if (cell_cap >= max_cells())
    flags &= ~DAMAR_ERR_CELLS;                     /* (those are in the map: nothing to repeat for them) */
  if (flags != 0)
    return false;                                  /* something else ran over: the caller grows it and repeats the launch */
  wide_pool_ensure();
  ra.wcells = RS.wcells;  ra.wcell_cap = RS.wcell_cap;
  if (VERBOSE || getenv("DAMAR_TEST_MAX_CELLS") != NULL)
    fprintf(stderr, "damar: %u read(s) / task(s) beyond the packed pebble format: wide kernel\n", hc[DAMAR_CNT_WIDE]);
  HIP_CHECK(hipMemsetAsync(RS.ctr + DAMAR_CNT_CURSOR, 0, sizeof(u32) * DAMAR_MAX_JOBS, G_st));
  HIP_CHECK(hipMemsetAsync(RS.ctr + DAMAR_CNT_FLAGS, 0, sizeof(u32), G_st));
  if (dist != NULL)
    damar_launch_tandem_report_wide(&ra, dist, wide_slots(), G_st);
  else
    damar_launch_la_batch_wide(&ra, tasks, ntasks, wide_slots(), G_st);
  HIP_CHECK(hipMemcpyAsync(hc, RS.ctr, sizeof(u32) * DAMAR_COUNTER_WORDS, hipMemcpyDeviceToHost, G_st));
  HIP_CHECK(hipStreamSynchronize(G_st));
  HIP_CHECK(hipGetLastError());
  if (hc[DAMAR_CNT_FLAGS] & DAMAR_ERR_CELLS)       /* the wide kernel's own pool: four times the pebbles, and everything once more */
    { wide_pool_grow();
      hc[DAMAR_CNT_FLAGS] = (hc[DAMAR_CNT_FLAGS] & ~DAMAR_ERR_CELLS) | 0x40000000u;
    }
  return true;
}

/* the records of a launch behind which the wide kernel ran: what the two-pair kernel wrote for a read / task before it
   gave it up goes, the wide kernel's records lose their mark */
static void wide_filter(std::vector<LaRecord> &recs, const u32 *dmap, u32 words)
{ std::vector<u32> wmap(words);
  HIP_CHECK(hipMemcpy(wmap.data(), dmap, sizeof(u32) * (size_t) words, hipMemcpyDeviceToHost));
  size_t n = 0;
  for (size_t q = 0; q < recs.size(); q++)
    { u32 it = recs[q].item;
      if (it & DAMAR_ITEM_WIDE)
        recs[q].item = it & ~DAMAR_ITEM_WIDE;
      else if ((wmap[it >> 5] >> (it & 31)) & 1u)
        continue;
      recs[n++] = recs[q];
    }
  recs.resize(n);
}

extern "C" void damar_match_self(const HITS_DB *ablock, damar_dev_block *blk, Align_Spec *spec, int64 *counts)
{ finish_all();
  ensure_init();
  int64 nfilt = 0, ncheck = 0;
  int   n = 0;
  if (counts)
    counts[0] = counts[1] = counts[2] = 0;
  memset(G_cnt, 0, sizeof(G_cnt));
  damar_dev_index *ix = index_build_k(blk, 0, &n, T_kmer, 0, 0);
  if (ix == NULL)
    return;
  const int ts = Trace_Spacing(spec);
  int *dist = (int *) dmalloc(sizeof(int) * (size_t) n);
  tick(0);
  damar_launch_tandem_links(&blk->d, T_kmer, ix->codes, ix->wide, ix->pos, (u32) n, dist, G_st);
  tick(1);

  std::vector<LaRecord> recs;
  std::vector<u16>      tpool;
  u32 hc[DAMAR_COUNTER_WORDS];
  u32 *wmap = NULL;
  const u32 wwords = ((u32) ablock->nreads + 31) / 32 + 1;
  bool wide_ran = false;
  { const int sk = P_kmer, sh = P_hitmin, sb = P_binshift;        /* the report args read the P_* set */
    P_kmer = T_kmer;  P_hitmin = T_hitmin;  P_binshift = T_binshift;
    u32 cell_cap = std::min<u32>(RS.cell_cap ? RS.cell_cap : DEFAULT_CELLS, max_cells());
    u32 rec_cap  = std::max(RS.rec_cap, (u32) (4 * ablock->nreads + 4096));
    u32 tp_cap   = std::max(RS.tpool_cap, rec_cap * 64u);
    for (int attempt = 0; ; attempt++)
      { ReportArgs ra;
        scratch_prepare(ablock->maxlen, ablock->maxlen, T_binshift, ts, cell_cap, G_st);
        scratch_outputs(rec_cap, tp_cap);
        fill_report_args(&ra, blk, blk, 0, 1, spec, G_st, 0, 0, params_now());
        ra.nwork = (u32) ablock->nreads;
        const bool packed = use_packed(&ra, ablock->maxlen, ablock->maxlen);
        if (!packed)
          marks_must_fit(ablock->maxlen, ablock->maxlen, ts);      /* (one read per wavefront, DAMAR_PACKED=0: no wide kernel behind it) */
        else
          { /* one bit per read: which are the wide kernel's (kernels/report.hip tandem_wide_kernel) */
            if (wmap == NULL)
              wmap = (u32 *) dmalloc(sizeof(u32) * (size_t) wwords);
            HIP_CHECK(hipMemsetAsync(wmap, 0, sizeof(u32) * (size_t) wwords, G_st));
            ra.widemap = wmap;  ra.wcells = RS.wcells;  ra.wcell_cap = RS.wcell_cap;  ra.cell_max = max_cells();
          }
        HIP_CHECK(hipMemsetAsync(RS.ctr, 0, sizeof(u32) * DAMAR_COUNTER_WORDS, G_st));
        tick(4);
        if (packed)
          damar_launch_tandem_report2(&ra, dist, RS.nslots, G_st);
        else
          damar_launch_tandem_report(&ra, dist, RS.nslots, G_st);
        tick(5);
        HIP_CHECK(hipMemcpyAsync(hc, RS.ctr, sizeof(hc), hipMemcpyDeviceToHost, G_st));
        HIP_CHECK(hipStreamSynchronize(G_st));
        HIP_CHECK(hipGetLastError());
        G_ms[DAMAR_T_REPORT] = lap(4, 5);
        wide_ran = packed && wide_behind(ra, hc, cell_cap, dist, NULL, 0);
        if (packed && !wide_ran && cell_cap >= max_cells() && hc[DAMAR_CNT_WIDE] > 0)
          hc[DAMAR_CNT_FLAGS] &= ~DAMAR_ERR_CELLS;
        if (hc[DAMAR_CNT_FLAGS] == 0)
          break;
        hc[DAMAR_CNT_FLAGS] &= ~0x40000000u;
        if (((hc[DAMAR_CNT_FLAGS] & DAMAR_ERR_BAND) && !(hc[DAMAR_CNT_FLAGS] & (DAMAR_ERR_CELLS | DAMAR_ERR_WIDE))) || attempt >= 6)
          { fprintf(stderr, "damar: FATAL: tandem report kernel failed (flags %u, where=%u)\n", hc[DAMAR_CNT_FLAGS], hc[DAMAR_CNT_WHERE]);
            die();
          }
        if (hc[DAMAR_CNT_FLAGS] & DAMAR_ERR_CELLS) cell_cap = grow_cells(cell_cap);
        if (hc[DAMAR_CNT_FLAGS] & DAMAR_ERR_WIDE)  G_ring *= 4;
        if (hc[DAMAR_CNT_FLAGS] & DAMAR_ERR_RECS)  rec_cap = std::max(2 * rec_cap, hc[DAMAR_CNT_RECS] + 1024);
        if (hc[DAMAR_CNT_FLAGS] & DAMAR_ERR_TPOOL) tp_cap  = std::max(2 * tp_cap, hc[DAMAR_CNT_TPOOL] + 65536);
      }
    P_kmer = sk;  P_hitmin = sh;  P_binshift = sb;
  }
  recs.resize(hc[DAMAR_CNT_RECS]);
  tpool.resize(hc[DAMAR_CNT_TPOOL]);
  if (hc[DAMAR_CNT_RECS] > 0)
    { HIP_CHECK(hipMemcpy(recs.data(), RS.recs, sizeof(LaRecord) * (size_t) hc[DAMAR_CNT_RECS], hipMemcpyDeviceToHost));
      HIP_CHECK(hipMemcpy(tpool.data(), RS.tpool, sizeof(u16) * (size_t) hc[DAMAR_CNT_TPOOL], hipMemcpyDeviceToHost));
    }
  nfilt = hc[DAMAR_CNT_NFILT];
  if (wide_ran)
    wide_filter(recs, wmap, wwords);
  if (wmap != NULL)
    HIP_CHECK(hipFree(wmap));
  HIP_CHECK(hipFree(dist));
  damar_index_free(ix);

  /* host tail: scrub/tandem.c:1140-1166 (fusion/containment only, A records only) */
  ncheck = damar_host_tail(recs.data(), recs.size(), tpool.data(), 0, NULL, ablock, ablock, 1, 0, spec, 0, 0, 0, 1, 1);
  G_cnt[0] = n;  G_cnt[2] = nfilt;  G_cnt[3] = hc[DAMAR_CNT_RECS];
  if (counts)
    { counts[0] = n;  counts[1] = nfilt;  counts[2] = ncheck; }
  if (VERBOSE)
    { printf("\n     %lld seed hits\n     %lld confirmed hits\n", (long long) nfilt, (long long) ncheck);
      fflush(stdout);
    }
}

extern "C" void Match_Self(char *aname, HITS_DB *ablock, Align_Spec *settings)
{ if (VERBOSE)
    printf("\nIndexing %s\n\nComparing %s to itself\n", aname, aname);
  damar_dev_block *b = damar_block_upload(ablock);
  damar_match_self(ablock, b, settings, NULL);
  damar_block_free(b);
}

/***** test hooks ***************************************************************************************/

/* slab table of the last damar_match: b_lo[0 .. n] and hits[0 .. n-1] for up to `cap` slabs; returns n (1: not split) */
extern "C" int damar_last_slabs(int *b_lo, int64 *hits, int cap)
{ const int n = G_plan.n;
  for (int i = 0; i < n && i < cap; i++)
    { if (b_lo) b_lo[i] = G_plan.b_lo[(size_t) i];
      if (hits) hits[i] = G_plan.hits[(size_t) i];
    }
  if (b_lo != NULL && n <= cap && (size_t) n < G_plan.b_lo.size())
    b_lo[n] = G_plan.b_lo[(size_t) n];
  return n;
}

/* of the last damar_match / damar_match_batch: seed stages run (slabs, summed over its comparisons), comparisons split */
extern "C" void damar_slab_totals(int64 *out)
{ out[0] = G_slab_tot[0];  out[1] = G_slab_tot[1]; }

/* Test hook: the ordering of the kept runs alone (kernels/seed_merge.hip damar_launch_order_runs) on a caller's packed seeds:
   keys[0 .. nhits) in place, work[0 .. nwork) = the heads of the runs to order, ascending.  Returns 0. */
extern "C" int damar_order_runs_test(uint64 *keys, int64 nhits, int ppos, int dbits, const uint32 *work, int nwork)
{ finish_all();
  ensure_init();
  if (nhits <= 0 || nwork <= 0)
    return 0;
  u64  *dk;
  u32  *dw;
  void *sc;
  HIP_CHECK(hipMalloc((void **) &dk, sizeof(u64) * (size_t) nhits));
  HIP_CHECK(hipMalloc((void **) &dw, sizeof(u32) * (size_t) nwork));
  HIP_CHECK(hipMalloc(&sc, damar_order_runs_scratch_bytes((u64) nhits)));
  HIP_CHECK(hipMemcpy(dk, keys, sizeof(u64) * (size_t) nhits, hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(dw, work, sizeof(u32) * (size_t) nwork, hipMemcpyHostToDevice));
  damar_launch_order_runs(dk, (u64) nhits, ppos, dbits, dw, (u32) nwork, sc, G_st);
  HIP_CHECK(hipStreamSynchronize(G_st));
  HIP_CHECK(hipMemcpy(keys, dk, sizeof(u64) * (size_t) nhits, hipMemcpyDeviceToHost));
  HIP_CHECK(hipFree(dk));  HIP_CHECK(hipFree(dw));  HIP_CHECK(hipFree(sc));
  return 0;
}

/* Test hook: the work list alone on a caller's seeds -- keys[0 .. nhits) is the stretch [off, off + nhits) of a sorted list of
   gtotal seeds, vals (the diagonals) is NULL unless dbits == 0.  mode 0: one pass over sorted seeds (damar_launch_pair_work,
   then damar_launch_pair_work_expand); mode 1: the same with the seeds of a read pair in no particular order, *flag_out =
   "a kept run is too long to order" (the ordering itself is not run: keys are never written); mode 2: the calls of
   front_work_twostep.  At most cap ascending seed indices go to work_out.  Returns the number of work items, -1 for
   arguments it refuses (mode 1 never sees dbits == 0: SeedStage sorts those comparisons over all the bits). */
extern "C" int64 damar_pair_work_test(const uint64 *keys, const uint32 *vals, int64 nhits, int64 off, int64 gtotal, int ppos,
                                      int dbits, int abits, int minhit, int nshift, int binshift, int kmer, int hitmin,
                                      uint32 b_lo, uint32 b_hi, int mode, uint32 *work_out, int64 cap, int64 *flag_out)
{ if (flag_out)
    *flag_out = 0;
  if (nhits < 0 || nhits > 0x7fffffffll || off < 0 || gtotal < off + nhits || mode < 0 || mode > 2 || cap < 0 ||
      (cap > 0 && work_out == NULL) || ppos < 1 || dbits < 0 || abits < 0 || ppos + dbits + abits > 63 || ppos > 31 ||
      minhit < 1 || kmer < 1 || hitmin < 1 || binshift < 0 || binshift > 31 || nshift > 6 ||
      (dbits == 0) != (vals != NULL) || (mode == 1 && dbits == 0) || (nhits > 0 && keys == NULL))
    return -1;
  finish_all();
  ensure_init();
  if (nhits == 0)
    return 0;
  const size_t n = (size_t) nhits, ntiles = (n + DAMAR_SCAN_TILE - 1) / DAMAR_SCAN_TILE;
  u64  *dk, *bits, *send, *tot;
  u32  *dv = NULL, *heads = NULL, *flags = NULL, *work = NULL;
  void *scw;
  HIP_CHECK(hipMalloc((void **) &dk, sizeof(u64) * n));
  HIP_CHECK(hipMalloc((void **) &bits, std::max(sizeof(u64) * 64 * ntiles, sizeof(u32) * n)));   /* (mode 2: foff after the heads) */
  HIP_CHECK(hipMalloc((void **) &send, sizeof(u64) * 64));
  HIP_CHECK(hipMalloc((void **) &tot, 64));
  HIP_CHECK(hipMalloc(&scw, damar_scan_workspace_bytes((u64) nhits)));
  HIP_CHECK(hipMemcpy(dk, keys, sizeof(u64) * n, hipMemcpyHostToDevice));
  if (vals != NULL)
    { HIP_CHECK(hipMalloc((void **) &dv, sizeof(u32) * n));
      HIP_CHECK(hipMemcpy(dv, vals, sizeof(u32) * n, hipMemcpyHostToDevice));
    }
  u64 got[2] = { 0, 0 };
  if (mode < 2)
    { damar_launch_pair_work(dk, dv, (u64) nhits, (u64) off, (u64) gtotal, ppos, dbits, abits, minhit, nshift, send, bits, scw, tot,
                             binshift, kmer, hitmin, b_lo, b_hi, mode, G_st);
      HIP_CHECK(hipMemcpyAsync(got, tot, 2 * sizeof(u64), hipMemcpyDeviceToHost, G_st));
      HIP_CHECK(hipStreamSynchronize(G_st));
      if (got[0] > 0)
        { HIP_CHECK(hipMalloc((void **) &work, sizeof(u32) * ((size_t) got[0] + 1)));
          damar_launch_pair_work_expand(bits, scw, (u64) nhits, work, G_st);
        }
    }
  else
    { HIP_CHECK(hipMalloc((void **) &heads, sizeof(u32) * n));
      HIP_CHECK(hipMalloc((void **) &flags, sizeof(u32) * n));
      damar_launch_pair_heads(dk, (u64) nhits, (u64) off, (u64) gtotal, ppos + dbits, abits, minhit, nshift, send, bits, scw, tot,
                              heads, G_st);
      HIP_CHECK(hipMemcpyAsync(got, tot, sizeof(u64), hipMemcpyDeviceToHost, G_st));
      HIP_CHECK(hipStreamSynchronize(G_st));
      const u32 nheads = (u32) got[0];
      got[0] = 0;
      if (nheads > 0)
        { HIP_CHECK(hipMalloc((void **) &work, sizeof(u32) * ((size_t) nheads + 1)));
          damar_launch_pair_screen(dk, dv, (u64) nhits, ppos, dbits, heads, nheads, minhit, binshift, kmer, hitmin, abits, b_lo, b_hi,
                                   flags, G_st);
          damar_exclusive_scan_u32(flags, (u32 *) bits, nheads, scw, tot, G_st);
          damar_launch_compact_u32(heads, flags, (const u32 *) bits, nheads, work, G_st);
          HIP_CHECK(hipMemcpyAsync(got, tot, sizeof(u64), hipMemcpyDeviceToHost, G_st));
        }
    }
  HIP_CHECK(hipStreamSynchronize(G_st));
  const u64 nw = got[0];
  if (nw > 0 && cap > 0)
    HIP_CHECK(hipMemcpy(work_out, work, sizeof(u32) * (size_t) std::min<u64>(nw, (u64) cap), hipMemcpyDeviceToHost));
  if (flag_out)
    *flag_out = (int64) got[1];
  HIP_CHECK(hipFree(dk));  HIP_CHECK(hipFree(bits));  HIP_CHECK(hipFree(send));  HIP_CHECK(hipFree(tot));  HIP_CHECK(hipFree(scw));
  if (dv)    HIP_CHECK(hipFree(dv));
  if (heads) HIP_CHECK(hipFree(heads));
  if (flags) HIP_CHECK(hipFree(flags));
  if (work)  HIP_CHECK(hipFree(work));
  return (int64) nw;
}

extern "C" int64 damar_last_seeds(void *out, int64 cap)
{ struct SP { int diag, apos, aread, bread; } *sp = (SP *) out;
  if (out == NULL)
    { G_keep_seeds = (cap != 0);
      return 0;
    }
  int64 n = (int64) G_seed_keys.size();
  for (int64 i = 0; i < n && i < cap; i++)
    { u64 k = G_seed_keys[(size_t) i];
      const int bpos = (int) (k & ((1ull << G_seed_dbits) - 1));
      k >>= G_seed_dbits;
      sp[i].apos  = (int) (k & ((1ull << G_seed_pbits) - 1));
      sp[i].aread = (int) ((k >> G_seed_pbits) & ((1ull << G_seed_abits) - 1));
      sp[i].bread = (int) (k >> (G_seed_pbits + G_seed_abits));
      sp[i].diag  = G_seed_dbits ? sp[i].apos - bpos : (int) G_seed_vals[(size_t) i];
    }
  return n;
}

/* t8: the launch writes its trace values as bytes where the spacing allows it (ReportArgs.t8, what report_launch does for the
   pipeline at -s <= 125); they are widened into `traces` here.  A value that does not fit (DAMAR_ERR_T8) repeats the launch
   with 16-bit values: *t8_fell_back says so.  *wide_tasks: the tasks the wide kernel answered (DAMAR_CNT_WIDE). */
extern "C" int damar_local_alignment_batch_opts(damar_dev_block *ablk, damar_dev_block *bblk, int comp,
                                                Align_Spec *spec, const int *tasks, int ntasks,
                                                int *paths, int64 *trace_off, uint16 *traces, int64 trace_cap,
                                                int t8, int *t8_fell_back, int *wide_tasks)
{ finish_all();
  ensure_init();
  if (t8_fell_back) *t8_fell_back = 0;
  if (wide_tasks)   *wide_tasks = 0;
  if (ntasks <= 0)
    return 0;
  const int ts = Trace_Spacing(spec);
  int use8 = (t8 != 0 && ts <= TRACE_XOVR);
  u32 cell_cap = std::min<u32>(RS.cell_cap ? RS.cell_cap : DEFAULT_CELLS, max_cells()), rec_cap = 2 * (u32) ntasks + 16,
      tp_cap = (u32) std::min<int64>(trace_cap + 1024, 0x7fffffff);
  LaTask *dt = (LaTask *) dmalloc(sizeof(LaTask) * (size_t) ntasks);
  HIP_CHECK(hipMemcpy(dt, tasks, sizeof(LaTask) * (size_t) ntasks, hipMemcpyHostToDevice));
  u32 hc[DAMAR_COUNTER_WORDS];
  u32 *wmap = NULL;
  const u32 wwords = ((u32) ntasks + 31) / 32 + 1;
  bool wide_ran = false;
  for (int attempt = 0; ; attempt++)
    { ReportArgs ra;
      scratch_prepare(ablk->d.maxlen, bblk->d.maxlen, P_binshift, ts, cell_cap, G_st);
      stage("la_scratch");
      scratch_outputs(rec_cap, tp_cap);
      fill_report_args(&ra, ablk, bblk, comp, 0, spec, G_st, 0, 0, params_now());
      ra.t8 = use8;
      const bool packed = use_packed(&ra, ablk->d.maxlen, bblk->d.maxlen);
      if (!packed)
        marks_must_fit(ablk->d.maxlen, bblk->d.maxlen, ts);
      else
        { if (wmap == NULL)
            wmap = (u32 *) dmalloc(sizeof(u32) * (size_t) wwords);
          HIP_CHECK(hipMemsetAsync(wmap, 0, sizeof(u32) * (size_t) wwords, G_st));
          ra.widemap = wmap;  ra.wcells = RS.wcells;  ra.wcell_cap = RS.wcell_cap;  ra.cell_max = max_cells();
        }
      HIP_CHECK(hipMemsetAsync(RS.ctr, 0, sizeof(u32) * DAMAR_COUNTER_WORDS, G_st));
      stage("la_setup");
      if (packed)
        damar_launch_report2(&ra, 1, dt, (u32) ntasks, RS.nslots, G_st);
      else
        damar_launch_la_batch(&ra, dt, (u32) ntasks, RS.nslots, G_st);
      stage("la_kernel");
      HIP_CHECK(hipMemcpyAsync(hc, RS.ctr, sizeof(hc), hipMemcpyDeviceToHost, G_st));
      HIP_CHECK(hipStreamSynchronize(G_st));
      HIP_CHECK(hipGetLastError());
      wide_ran = packed && wide_behind(ra, hc, cell_cap, NULL, dt, (u32) ntasks);
      if (packed && !wide_ran && cell_cap >= max_cells() && hc[DAMAR_CNT_WIDE] > 0)
        hc[DAMAR_CNT_FLAGS] &= ~DAMAR_ERR_CELLS;
      if (hc[DAMAR_CNT_FLAGS] == 0)
        break;
      hc[DAMAR_CNT_FLAGS] &= ~0x40000000u;
      if (((hc[DAMAR_CNT_FLAGS] & DAMAR_ERR_BAND) && !(hc[DAMAR_CNT_FLAGS] & (DAMAR_ERR_CELLS | DAMAR_ERR_WIDE))) || attempt >= 6)
        { fprintf(stderr, "damar: FATAL: batch Local_Alignment failed (flags %u, where=%u)\n", hc[DAMAR_CNT_FLAGS], hc[DAMAR_CNT_WHERE]);
          die();
        }
      if (hc[DAMAR_CNT_FLAGS] & DAMAR_ERR_CELLS) cell_cap = grow_cells(cell_cap);
      if (hc[DAMAR_CNT_FLAGS] & DAMAR_ERR_WIDE)  G_ring *= 4;
      if (hc[DAMAR_CNT_FLAGS] & DAMAR_ERR_RECS)
        rec_cap = std::max(2 * rec_cap, hc[DAMAR_CNT_RECS] + 1024);
      if (hc[DAMAR_CNT_FLAGS] & DAMAR_ERR_T8)                    /* a value above 255 (t8max): 16-bit values again, as report_launch does */
        { use8 = 0;
          if (t8_fell_back) *t8_fell_back = 1;
        }
      if (hc[DAMAR_CNT_FLAGS] & DAMAR_ERR_TPOOL)
        { HIP_CHECK(hipFree(dt));
          if (wmap != NULL)
            HIP_CHECK(hipFree(wmap));
          return -1;
        }
    }
  HIP_CHECK(hipFree(dt));
  std::vector<LaRecord> recs(hc[DAMAR_CNT_RECS]);
  std::vector<u16> tp(hc[DAMAR_CNT_TPOOL]);
  HIP_CHECK(hipMemcpy(recs.data(), RS.recs, sizeof(LaRecord) * (size_t) hc[DAMAR_CNT_RECS], hipMemcpyDeviceToHost));
  if (use8)
    { std::vector<u8> tp8(hc[DAMAR_CNT_TPOOL]);
      HIP_CHECK(hipMemcpy(tp8.data(), RS.tpool, sizeof(u8) * (size_t) hc[DAMAR_CNT_TPOOL], hipMemcpyDeviceToHost));
      for (size_t i = 0; i < tp8.size(); i++)
        tp[i] = tp8[i];
    }
  else
    HIP_CHECK(hipMemcpy(tp.data(), RS.tpool, sizeof(u16) * (size_t) hc[DAMAR_CNT_TPOOL], hipMemcpyDeviceToHost));
  if (wide_ran && wide_tasks)
    *wide_tasks = (int) hc[DAMAR_CNT_WIDE];
  if (wide_ran)
    wide_filter(recs, wmap, wwords);
  if (wmap != NULL)
    HIP_CHECK(hipFree(wmap));
  std::sort(recs.begin(), recs.end(), RecOrder());
  std::vector<u32> boffa((size_t) ablk->nreads + 1), boffb((size_t) bblk->nreads + 1);
  HIP_CHECK(hipMemcpy(boffa.data(), ablk->boff, sizeof(u32) * boffa.size(), hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(boffb.data(), bblk->boff, sizeof(u32) * boffb.size(), hipMemcpyDeviceToHost));
  int64 top = 0;
  for (size_t i = 0; i < recs.size(); i++)
    { const LaRecord &r = recs[i];
      int *p = paths + 12 * r.item;
      int  al = (int) (boffa[r.aread + 1] - boffa[r.aread] - 1), bl = (int) (boffb[r.bread + 1] - boffb[r.bread] - 1);
      p[0] = r.abpos;  p[1] = r.bbpos;  p[2] = r.aepos;  p[3] = r.bepos;  p[4] = r.diffs;  p[5] = r.atlen;
      if (comp)
        { p[6] = bl - r.bepos;  p[7] = al - r.aepos;  p[8] = bl - r.bbpos;  p[9] = al - r.abpos; }
      else
        { p[6] = r.bbpos;  p[7] = r.abpos;  p[8] = r.bepos;  p[9] = r.aepos; }
      p[10] = r.diffs;  p[11] = r.btlen;
      if (top + r.atlen + r.btlen > trace_cap)
        return -1;
      trace_off[2 * r.item] = top;
      memcpy(traces + top, tp.data() + r.toff, sizeof(u16) * (size_t) r.atlen);
      top += r.atlen;
      trace_off[2 * r.item + 1] = top;
      memcpy(traces + top, tp.data() + r.toff + r.atlen, sizeof(u16) * (size_t) r.btlen);
      top += r.btlen;
    }
  return 0;
}

extern "C" int damar_local_alignment_batch(damar_dev_block *ablk, damar_dev_block *bblk, int comp,
                                           Align_Spec *spec, const int *tasks, int ntasks,
                                           int *paths, int64 *trace_off, uint16 *traces, int64 trace_cap)
{ return damar_local_alignment_batch_opts(ablk, bblk, comp, spec, tasks, ntasks, paths, trace_off, traces, trace_cap, 0, NULL, NULL);
}

extern "C" double damar_bench_sort_u32(uint32_t n, int nbits, int reps, uint32_t seed)
{ ensure_init();
  std::vector<u32> h(n);
  u32 x = seed ? seed : 1u, mask = (nbits >= 32) ? 0xffffffffu : ((1u << nbits) - 1);
  for (u32 i = 0; i < n; i++)
    { x ^= x << 13;  x ^= x >> 17;  x ^= x << 5;
      h[i] = x & mask;
    }
  u32 *src = (u32 *) dmalloc(sizeof(u32) * (size_t) n);
  u32 *k0 = (u32 *) dmalloc(sizeof(u32) * (size_t) n), *v0 = (u32 *) dmalloc(sizeof(u32) * (size_t) n);
  u32 *k1 = (u32 *) dmalloc(sizeof(u32) * (size_t) n), *v1 = (u32 *) dmalloc(sizeof(u32) * (size_t) n);
  void *sw = dmalloc(damar_sort_workspace_bytes(n));
  HIP_CHECK(hipMemcpy(src, h.data(), sizeof(u32) * (size_t) n, hipMemcpyHostToDevice));
  double total = 0;
  for (int r = 0; r < reps + 1; r++)
    { HIP_CHECK(hipMemcpyAsync(k0, src, sizeof(u32) * (size_t) n, hipMemcpyDeviceToDevice, G_st));
      HIP_CHECK(hipMemcpyAsync(v0, src, sizeof(u32) * (size_t) n, hipMemcpyDeviceToDevice, G_st));
      tick(8);
      damar_radix_sort_u32(k0, v0, k1, v1, n, nbits, sw, G_st);
      tick(9);
      HIP_CHECK(hipStreamSynchronize(G_st));
      if (r > 0)
        total += lap(8, 9);
    }
  HIP_CHECK(hipFree(src));  HIP_CHECK(hipFree(k0));  HIP_CHECK(hipFree(v0));
  HIP_CHECK(hipFree(k1));   HIP_CHECK(hipFree(v1));  HIP_CHECK(hipFree(sw));
  return total / reps;
}

/***** align.h:223-259: Work_Data and the single-call Local_Alignment ***********************************/

/* struct WorkData: shim_internal.h (Compute_Trace_PTS and _MID, stages/trace.hip, fill its script) */

extern "C" Work_Data *New_Work_Data(void)             /* align.c:135-160 */
{ return (Work_Data *) new WorkData();
}

extern "C" void Free_Work_Data(Work_Data *work)       /* align.c:162-173 */
{ delete (WorkData *) work;
}

/* align.c:1904-2097 for one pair of sequences, computed by the same wave kernel as Match_Filter
 * (one task through the batch path: the two sequences travel to HBM and back per call, so this
 * entry point is for callers that need the reference's API, not for throughput).  Supported call
 * shape: the one filter.c:2316 uses, low == hgh (seed diagonal) and no borders (lbord, hbord < 0);
 * anything else exits as the reference's batch-mode errors do.  align->aseq/bseq follow the
 * block layout (a 4 before the first and after the last base). */
extern "C" Path *Local_Alignment(Alignment *align, Work_Data *work, Align_Spec *spec,
                                 int low, int hgh, int anti, int lbord, int hbord)
{ ensure_init();
  WorkData *w = (WorkData *) work;
  if (low != hgh || lbord >= 0 || hbord >= 0)
    { fprintf(stderr, "damar: Local_Alignment: only the seed-diagonal call shape (low == hgh, no borders) is built\n");
      exit(1);
    }
  HITS_DB   db[2];
  HITS_READ rd[2][2];
  std::vector<char> buf[2];
  const char *seq[2] = { align->aseq, align->bseq };
  const int   len[2] = { align->alen, align->blen };
  const int   same = (align->aseq == align->bseq);
  for (int i = 0; i < 2; i++)
    { memset(&db[i], 0, sizeof(HITS_DB));
      memset(rd[i], 0, sizeof(rd[i]));
      buf[i].assign((size_t) len[i] + 2, 4);
      memcpy(buf[i].data() + 1, seq[i], (size_t) len[i]);
      rd[i][0].rlen = len[i];  rd[i][0].boff = 0;  rd[i][1].boff = len[i] + 1;
      db[i].nreads = db[i].ureads = 1;  db[i].maxlen = len[i];  db[i].totlen = len[i];
      db[i].bases = buf[i].data() + 1;  db[i].reads = rd[i];
    }
  damar_dev_block *ab = damar_block_upload(&db[0]);
  damar_dev_block *bb = same ? ab : damar_block_upload(&db[1]);
  const int mtp = 2 * (std::max(len[0], len[1]) / Trace_Spacing(spec) + 2) + 8;
  std::vector<uint16> tr((size_t) 4 * mtp + 64);
  int   task[4] = { 0, 0, low, anti }, paths[12];
  int64 toff[2];
  if (damar_local_alignment_batch(ab, bb, (int) (align->flags & COMP_FLAG), spec, task, 1, paths, toff,
                                  tr.data(), (int64) tr.size()))
    { fprintf(stderr, "damar: Local_Alignment: trace buffer too small\n");
      exit(1);
    }
  damar_block_free(ab);
  if (!same)
    damar_block_free(bb);
  Path *ap = align->path;
  ap->abpos = paths[0];  ap->bbpos = paths[1];  ap->aepos = paths[2];  ap->bepos = paths[3];
  ap->diffs = paths[4];  ap->tlen = paths[5];
  w->atrace.assign(tr.begin() + toff[0], tr.begin() + toff[0] + paths[5]);
  ap->trace = w->atrace.data();
  w->bpath.abpos = paths[6];  w->bpath.bbpos = paths[7];  w->bpath.aepos = paths[8];  w->bpath.bepos = paths[9];
  w->bpath.diffs = paths[10];  w->bpath.tlen = paths[11];
  w->btrace.assign(tr.begin() + toff[1], tr.begin() + toff[1] + paths[11]);
  w->bpath.trace = w->btrace.data();
  return &w->bpath;
}
