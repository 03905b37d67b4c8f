/* tail.cpp -- the host tail of the overlap path (filter.c:2442-2483 per read pair) and its threads: the pool a tail
 * cuts its records over, and the two-stage pipeline that runs tails and file writes behind the caller.  Host only:
 * where the records come from is the caller's business (tail.h: two hooks on the landing buffer).
 */
#include <algorithm>
#include <vector>
#include <deque>
#include <thread>
#include <mutex>
#include <condition_variable>
#include <functional>
#include <string.h>
#include <stdlib.h>
#include <time.h>
#include <unistd.h>

#include "tail.h"

typedef unsigned long long u64;
typedef unsigned int       u32;
typedef unsigned short     u16;
typedef unsigned char      u8;

/* Fatal errors end the process like the reference's exit(1) (db/DB.h:84-86), but without
 * running atexit handlers: tearing the HIP runtime down from inside a failed call can hang
 * when the library is embedded (ctypes). */
void die(void)
{ fflush(NULL);
  _exit(1);
}

double now_ms(void)
{ struct timespec t;
  clock_gettime(CLOCK_MONOTONIC, &t);
  return t.tv_sec * 1e3 + t.tv_nsec * 1e-6;
}

/***** blocks that the host keeps packed ****************************************************************/

static std::mutex PK_mu;
static std::vector<std::pair<const HITS_READ *, const damar_packed *>> PK_reg;      /* by the read table: the tail works on COPIES of
                                                                                       the block records, and a block shares its
                                                                                       read table with its complement */

void packed_register(const HITS_READ *reads, const damar_packed *pk)
{ std::lock_guard<std::mutex> lk(PK_mu);
  bool have = false;
  for (auto &e : PK_reg)
    if (e.first == reads)
      { e.second = pk;  have = true; }
  if (!have)
    PK_reg.push_back(std::make_pair(reads, pk));
}

void packed_forget(const HITS_READ *reads)
{ std::lock_guard<std::mutex> lk(PK_mu);
  for (size_t i = 0; i < PK_reg.size(); i++)
    if (PK_reg[i].first == reads)
      { PK_reg.erase(PK_reg.begin() + i);
        break;
      }
}

/* read r of a host block, one byte per base with a 4 on either side: straight out of an unpacked block, or unpacked
   into buf out of a packed one (comp: the record is the block's reverse complement) */
static const char *host_read(const HITS_DB *block, int r, int comp, std::vector<char> &buf)
{ if (block->bases != NULL)
    return (const char *) block->bases + block->reads[r].boff;
  const damar_packed *pk = NULL;
  { std::lock_guard<std::mutex> lk(PK_mu);
    for (auto &e : PK_reg)
      if (e.first == block->reads)
        pk = e.second;
  }
  if (pk == NULL)
    { fprintf(stderr, "damar: internal error, a block without bases that was never uploaded packed\n");
      die();
    }
  buf.resize((size_t) block->reads[r].rlen + 2);
  damar_unpack_read(pk, block, r, comp, buf.data() + 1);
  return buf.data() + 1;
}

/***** the tail of one comparison ***********************************************************************/

/* byte trace values of the device (ReportArgs.t8) into the 16-bit pool the redundancy handling works on */
static int64 tpool_push8(damar_tpool *tp, const u8 *src, int n)
{ static thread_local std::vector<uint16> wide;
  wide.resize((size_t) n);
  for (int i = 0; i < n; i++)
    wide[i] = src[i];
  return damar_tpool_push(tp, wide.data(), n);
}

/* One of the two records a local alignment becomes (filter.c:2470-2483): a path whose trace is still an offset into
   the downloaded pool.  The A view is the record as stored; the B view has the reads exchanged, its trace behind A's. */
struct View
{ int    tlen, diffs, abpos, bbpos, aepos, bepos;
  size_t toff;
};

static inline View view_a(const LaRecord &r)
{ return View { r.atlen, r.diffs, r.abpos, r.bbpos, r.aepos, r.bepos, (size_t) r.toff }; }

static inline View view_b(const LaRecord &r, int comp, int al, int bl)
{ if (comp)                                          /* align.c:2039-2042 */
    return View { r.btlen, r.diffs, bl - r.bepos, al - r.aepos, bl - r.bbpos, al - r.abpos, (size_t) r.toff + r.atlen };
  return View { r.btlen, r.diffs, r.bbpos, r.abpos, r.bepos, r.aepos, (size_t) r.toff + r.atlen };      /* align.c:2059-2062 */
}

/* a pair's only alignment: the view written straight from the downloaded trace, which Compress_TraceTo8 may shorten in
   place (the landing buffer is this comparison's own) */
static inline void view_write(const View &v, int aread, int bread, int comp, const u16 *tpool, int t8, int ts, Overlap_IO_Buffer *obuf)
{ Overlap ovl;
  memset(&ovl, 0, sizeof(ovl));
  ovl.flags = (uint32) comp;
  ovl.aread = aread;  ovl.bread = bread;
  ovl.path.tlen = v.tlen;  ovl.path.diffs = v.diffs;
  ovl.path.abpos = v.abpos;  ovl.path.bbpos = v.bbpos;  ovl.path.aepos = v.aepos;  ovl.path.bepos = v.bepos;
  /* (t8: the device has compressed the values already -- and raised DAMAR_ERR_T8 had one not fitted) */
  ovl.path.trace = t8 ? (void *) ((const u8 *) tpool + v.toff) : (void *) (tpool + v.toff);
  if (ts <= TRACE_XOVR && !t8)
    Compress_TraceTo8(&ovl, 1);
  AddOverlapToBuffer(obuf, &ovl, (ts <= TRACE_XOVR) ? 1 : 2);
}

/* one of a pair's several alignments: the view as a path of the pair's own 16-bit pool, for Handle_Redundancies */
static inline void view_push(const View &v, const u16 *tpool, int t8, damar_tpool *tp, std::vector<damar_path> &to)
{ damar_path p;
  p.tlen = v.tlen;  p.diffs = v.diffs;
  p.abpos = v.abpos;  p.bbpos = v.bbpos;  p.aepos = v.aepos;  p.bepos = v.bepos;
  p.toff = t8 ? tpool_push8(tp, (const u8 *) tpool + v.toff, v.tlen) : damar_tpool_push(tp, tpool + v.toff, v.tlen);
  to.push_back(p);
}

/* One contiguous range [lo, hi) of the ordered records (whole read pairs): filter.c:2442-2483
 * per pair, results appended to obuf. */
static int64 tail_range(const LaRecord *recs, const u32 *ord, const u64 *okey, size_t lo, size_t hi, const u16 *tpool, int t8,
                        const HITS_DB *ablock, const HITS_DB *bblock, int self, int comp, int ts,
                        Overlap_IO_Buffer *obuf, int symmetric, int hgap_min, int no_bridge)
{ int64 ncheck = 0;
  std::vector<damar_path> am, bm;
  damar_tpool tp = { NULL, 0, 0 };
  std::vector<char> aread_buf, bread_buf;                       /* (packed host blocks: the reads of a pair that is bridged) */
  size_t i = lo;
  while (i < hi)
    { size_t j = i;
      /* the records arrive in completion order and are visited in item order: every record and every trace is a
         cache miss in 300 MB of landing buffer unless it is asked for ahead (records 16 ahead, their traces 8 ahead) */
      if (i + 16 < hi)
        __builtin_prefetch(&recs[ord[i + 16]]);
      if (i + 8 < hi)
        { const LaRecord &pr = recs[ord[i + 8]];
          const size_t vb = t8 ? sizeof(u8) : sizeof(u16);
          const char *pt = (const char *) tpool + vb * (size_t) pr.toff;
          const size_t nb = vb * (size_t) (pr.atlen + pr.btlen);
          for (size_t o = 0; o < nb; o += 64)
            __builtin_prefetch(pt + o);
        }
      while (j < hi && (okey[j] >> 32) == (okey[i] >> 32))          /* (the item sits in the key: no record is touched for this) */
        j += 1;
      const int ar = recs[ord[i]].aread, br = recs[ord[i]].bread;
      const int al = ablock->reads[ar].rlen, bl = bblock->reads[br].rlen;
      const int doA = (al >= hgap_min);
      const int doB = (symmetric && bl >= hgap_min && (ar != br || !self || !comp));   /* filter.c:2300-2301 */
      const int ua = ar + ablock->ufirst, ub = br + bblock->ufirst;
      if (j - i == 1)
        { /* one alignment for the pair -- the common case: nothing for Handle_Redundancies to look at, so the records
             (filter.c:2470-2483: the A view, then the B view) are written straight from the downloaded traces */
          const LaRecord &r = recs[ord[i]];
          if (doA)
            view_write(view_a(r), ua, ub, comp, tpool, t8, ts, obuf);
          if (doB)
            view_write(view_b(r, comp, al, bl), ub, ua, comp, tpool, t8, ts, obuf);
          ncheck += doA + doB;
          i = j;
          continue;
        }
      am.clear();  bm.clear();  tp.top = 0;
      for (size_t q = i; q < j; q++)
        { const LaRecord &r = recs[ord[q]];
          if (doA)
            view_push(view_a(r), tpool, t8, &tp, am);
          if (doB)
            view_push(view_b(r, comp, al, bl), tpool, t8, &tp, bm);
        }
      damar_bridge_ctx bctx;
      if (am.size() > 1 || bm.size() > 1)      /* (only Handle_Redundancies looks at the sequences) */
        { bctx.aseq = host_read(ablock, ar, 0, aread_buf);  bctx.bseq = host_read(bblock, br, comp, bread_buf); }
      else
        { bctx.aseq = NULL;  bctx.bseq = NULL; }
      bctx.alen = al;  bctx.blen = bl;
      damar_emit_pair(am.data(), (int) am.size(), bm.data(), (int) bm.size(), &tp, comp, ts, ua, ub,
                      no_bridge ? (const damar_bridge_ctx *) NULL : &bctx, obuf, &ncheck);
      i = j;
    }
  free(tp.val);
  damar_bridge_release();
  return ncheck;
}

static int tail_threads(void)
{ static int n = 0;
  if (n == 0)
    { const char *e = getenv("DAMAR_TAIL_THREADS");
      n = e ? atoi(e) : 4;
      if (n < 1) n = 1;
      if (n > 64) n = 64;
    }
  return n;
}

/* The threads of the tail are kept between calls: a comparison's tail is 0.8 ms of work and four threads created and joined
   for it were 0.15 ms of that (config 3: 306 tails).  tail_pool_run(n, fn) runs fn(0) .. fn(n - 1), fn(0) on the caller. */
static struct TailPool
{ std::mutex              mu, run_mu;
  std::condition_variable cv_work, cv_done;
  std::vector<std::thread> th;
  const std::function<void(int)> *fn = NULL;
  int      n = 0, left = 0;
  uint64_t gen = 0;
  bool     stop = false;
} TP;

static void tail_pool_worker(int w)
{ uint64_t seen = 0;
  for (;;)
    { const std::function<void(int)> *fn;
      { std::unique_lock<std::mutex> lk(TP.mu);
        TP.cv_work.wait(lk, [&] { return TP.stop || TP.gen != seen; });
        if (TP.stop)
          return;
        seen = TP.gen;
        if (w >= TP.n)
          continue;
        fn = TP.fn;
      }
      (*fn)(w);
      { std::lock_guard<std::mutex> lk(TP.mu);
        if (--TP.left == 0)
          TP.cv_done.notify_one();
      }
    }
}

static void tail_pool_run(int n, const std::function<void(int)> &fn)
{ std::lock_guard<std::mutex> one(TP.run_mu);
  { std::lock_guard<std::mutex> lk(TP.mu);
    while ((int) TP.th.size() < n - 1)
      { const int w = (int) TP.th.size() + 1;
        TP.th.emplace_back(tail_pool_worker, w);
      }
    TP.fn = &fn;  TP.n = n;  TP.left = n - 1;  TP.gen += 1;
  }
  TP.cv_work.notify_all();
  fn(0);
  std::unique_lock<std::mutex> lk(TP.mu);
  TP.cv_done.wait(lk, [&] { return TP.left == 0; });
  TP.fn = NULL;  TP.n = 0;
}

void tail_pool_join(void)
{ { std::lock_guard<std::mutex> lk(TP.mu);
    TP.stop = true;
  }
  TP.cv_work.notify_all();
  for (auto &t : TP.th)
    t.join();
  TP.th.clear();
  TP.stop = false;
}

extern "C" int64 damar_host_tail(LaRecord *recs, size_t nrecs_all, const void *tpool_, int t8, const u32 *wmap,
                                 const HITS_DB *ablock, const HITS_DB *bblock, int self, int comp, Align_Spec *spec,
                                 int symmetric, int hgap_min, int jobid, int njobs, int no_bridge)
{ const u16 *tpool = (const u16 *) tpool_;
  const int ts = Trace_Spacing(spec);
  /* (work item, sequence) order = the reference's order of read pairs and of the alignments inside one.  ONE pass over
     the records (of a launch over several comparisons: those of this one, top byte of seq) collects 8-byte keys
     item << 32 | seq; everything after that -- a counting sort on the item (a wave emits the records of its item in
     sequence order; the insertion pass only guards that), the pair boundaries, the thread cuts -- works on the keys,
     which stay in cache, instead of on 48-byte records scattered over the landing buffer */
  const bool tprof = getenv("DAMAR_HOSTPROF") != NULL;
  const double tp0 = tprof ? now_ms() : 0.;
  std::vector<u64> key;
  std::vector<u32> idx;
  key.reserve(nrecs_all);  idx.reserve(nrecs_all);
  u32 maxitem = 0;
  for (size_t q = 0; q < nrecs_all; q++)
    if (njobs <= 1 || (int) (recs[q].seq >> DAMAR_SEQ_BITS) == jobid)
      { u32 it = recs[q].item;
        if (it & DAMAR_ITEM_WIDE)                    /* the wide kernel's record */
          { it &= ~DAMAR_ITEM_WIDE;
            recs[q].item = it;
          }
        else if (wmap != NULL && ((wmap[it >> 5] >> (it & 31)) & 1u))
          continue;                                   /* what the two-pair kernel wrote for a pair before it gave it up */
        key.push_back(((u64) it << 32) | (u64) recs[q].seq);
        idx.push_back((u32) q);
        if (it > maxitem) maxitem = it;
      }
  const size_t nrecs = key.size();
  const double tp1 = tprof ? now_ms() : 0.;
  std::vector<u32> ord(nrecs);
  std::vector<u64> okey(nrecs);
  { std::vector<u32> first((size_t) maxitem + 2, 0);
    for (size_t q = 0; q < nrecs; q++)
      first[(size_t) (key[q] >> 32) + 1] += 1;
    for (size_t q = 1; q < first.size(); q++)
      first[q] += first[q - 1];
    for (size_t q = 0; q < nrecs; q++)
      { const u32 at = first[(size_t) (key[q] >> 32)]++;
        ord[at] = idx[q];  okey[at] = key[q];
      }
    for (size_t q = 1; q < nrecs; q++)
      { const u64 x = okey[q];
        const u32 xi = ord[q];
        size_t r = q;
        while (r > 0 && okey[r - 1] > x && (okey[r - 1] >> 32) == (x >> 32))
          { okey[r] = okey[r - 1];  ord[r] = ord[r - 1];  r -= 1; }
        okey[r] = x;  ord[r] = xi;
      }
  }
  const double tp2 = tprof ? now_ms() : 0.;
  Overlap_IO_Buffer *obuf = OVL_IO_Buffer(spec);
  static size_t tmin = 0;                  /* below this many records one thread does it (DAMAR_TAIL_MIN) */
  if (tmin == 0)
    { const char *e = getenv("DAMAR_TAIL_MIN");
      tmin = (e && atol(e) > 0) ? (size_t) atol(e) : 8192;
    }
  const int nthr = (nrecs >= tmin) ? tail_threads() : 1;
  if (nthr == 1)
    return tail_range(recs, ord.data(), okey.data(), 0, nrecs, tpool, t8, ablock, bblock, self, comp, ts, obuf, symmetric, hgap_min, no_bridge);

  /* Read pairs are independent: cut the ordered records into nthr ranges at pair boundaries,
     let each thread fill a private buffer, append the buffers in order. */
  std::vector<size_t> cut(nthr + 1, nrecs);
  cut[0] = 0;
  for (int t = 1; t < nthr; t++)
    { size_t c = std::max(cut[t - 1], nrecs * (size_t) t / nthr);
      while (c < nrecs && c > 0 && (okey[c] >> 32) == (okey[c - 1] >> 32))
        c += 1;
      cut[t] = c;
    }
  /* The Align_Spec holds one buffer per -j thread and the writer gathers them all and sorts (align.c:6166-6200), so tail
     thread t appends to buffer t: no private buffer to copy over afterwards (a read pair's records stay together in one
     buffer, which is all the sort's tie-break needs).  With fewer -j buffers than tail threads: private buffers, appended
     in order. */
  const bool direct = Num_Threads(spec) >= nthr;
  std::vector<Overlap_IO_Buffer *> part(nthr, (Overlap_IO_Buffer *) NULL);
  std::vector<int64> got(nthr, 0);
  for (int t = 0; t < nthr; t++)
    { if (direct)
        part[t] = obuf + t;
      else
        { part[t] = CreateOverlapBuffer(4 * nthr, obuf->tbytes ? obuf->tbytes : 1, obuf->no_trace);
          if (part[t] == NULL)
            die();
        }
    }
  tail_pool_run(nthr, [&](int t) { got[t] = tail_range(recs, ord.data(), okey.data(), cut[t], cut[t + 1], tpool, t8, ablock, bblock,
                                                       self, comp, ts, part[t], symmetric, hgap_min, no_bridge); });
  int64 ncheck = 0;
  for (int t = 0; t < nthr; t++)
    { if (!direct)
        { if (damar_append_overlap_buffer(obuf, part[t]))
            { fprintf(stderr, "damar: FATAL: out of memory appending overlaps\n");
              die();
            }
          free(part[t]->ovls);
          free(part[t]->trace);
          free(part[t]);
        }
      ncheck += got[t];
    }
  if (tprof)
    fprintf(stderr, "damar: tail of %zu records: keys %.2f ms, order %.2f ms, %d threads %.2f ms\n", nrecs, tp1 - tp0, tp2 - tp1, nthr, now_ms() - tp2);
  return ncheck;
}

/***** the pipeline *************************************************************************************/

/* The host side runs as a two-stage pipeline behind its caller.  Stage 1 (one thread) does the tail of each
 * comparison in submission order and, for a write request, detaches the filled overlap buffers from the
 * Align_Spec; stage 2 sorts and writes the detached buffers.  The overlap buffers of an Align_Spec are
 * touched by stage 1 only; tail_drain() must be called before the blocks or the Align_Spec involved are
 * released, and before the counters are read. */

/* Heap objects that are never destroyed: at process exit a worker may still be parked in
 * wait(), and destroying a condition variable with a waiter (static destructors) hangs. */
struct Stage
{ std::mutex              mu;
  std::condition_variable cv, idle;
  std::deque<TailJob *>   queue;
  int                     busy;              /* jobs taken off the queue and not finished yet */
  bool                    quit;
  std::vector<std::thread *> threads;
  Stage() : busy(0), quit(false) {}
};
static Stage &A_s1 = *new Stage();
static Stage &A_s2 = *new Stage();
static std::mutex &A_mu = *new std::mutex();            /* the totals below */
static int64  A_ncheck = 0;
static double A_tail_ms = 0, A_write_ms = 0, A_d2h_ms = 0;

static void stage_submit(Stage &st, TailJob *job)
{ { std::lock_guard<std::mutex> lk(st.mu);
    st.queue.push_back(job);
  }
  st.cv.notify_one();
}

static TailJob *stage_next(Stage &st)
{ std::unique_lock<std::mutex> lk(st.mu);
  st.cv.wait(lk, [&st] { return st.quit || !st.queue.empty(); });
  if (st.queue.empty())
    return NULL;
  TailJob *job = st.queue.front();
  st.queue.pop_front();
  st.busy += 1;
  return job;
}

static void stage_done(Stage &st)
{ { std::lock_guard<std::mutex> lk(st.mu);
    st.busy -= 1;
  }
  st.idle.notify_all();
}

static void stage_drain(Stage &st)
{ std::unique_lock<std::mutex> lk(st.mu);
  st.idle.wait(lk, [&st] { return st.queue.empty() && st.busy == 0; });
}

static void tail_worker(void)
{ for (;;)
    { TailJob *job = stage_next(A_s1);
      if (job == NULL)
        return;
      double t0 = now_ms();
      if (job->kind == 0)
        { damar_tail_buf *hb = job->hb;
          if (hb->landed != NULL)
            { const double ms = hb->landed(hb);           /* (the other comparisons of the launch share the buffer) */
              std::lock_guard<std::mutex> lk(A_mu);
              A_d2h_ms += ms;
              t0 = now_ms();
            }
          int64 n = damar_host_tail(hb->recs, hb->nrec, hb->tpool, hb->t8, hb->nwide ? hb->wmap + hb->wm_off[job->jobid] : (const u32 *) NULL,
                                    &job->ablock, &job->bblock, job->self, job->comp, job->spec, job->symmetric, job->hgap_min,
                                    job->jobid, job->njobs, 0);
          if (job->got != NULL)
            *job->got += n;                    /* (summed over a comparison's slabs) */
          if (--hb->users == 0 && hb->release != NULL)
            hb->release(hb);
          delete job;
          std::lock_guard<std::mutex> lk(A_mu);
          A_ncheck += n;
          A_tail_ms += now_ms() - t0;
        }
      else
        { job->bufs = damar_detach_overlap_buffers(job->spec, &job->wp);
          stage_submit(A_s2, job);
          std::lock_guard<std::mutex> lk(A_mu);
          A_tail_ms += now_ms() - t0;
        }
      stage_done(A_s1);
    }
}

static void write_worker(void)
{ for (;;)
    { TailJob *job = stage_next(A_s2);
      if (job == NULL)
        return;
      double t0 = now_ms();
      damar_write_detached(&job->wp, job->bufs, job->has1 ? job->d1.c_str() : NULL,
                           job->has2 ? job->d2.c_str() : NULL, job->a.c_str(), job->b.c_str(), job->last);
      delete job;
      { std::lock_guard<std::mutex> lk(A_mu);
        A_write_ms += now_ms() - t0;
      }
      stage_done(A_s2);
    }
}

void tail_submit(TailJob *job)
{ stage_submit(A_s1, job);
}

void tail_drain(void)
{ stage_drain(A_s1);           /* stage 1 feeds stage 2: drain in pipeline order */
  stage_drain(A_s2);
}

void tail_start(void)
{ A_s1.quit = A_s2.quit = false;
  A_s1.threads.push_back(new std::thread(tail_worker));      /* one: the tails append to the overlap buffers in order */
  /* the sort + write of a block pair's files is independent of every other pair's: two writers by default
     (DAMAR_WRITE_THREADS), so that the files of the last pairs are not written one after the other at the drain */
  const char *e = getenv("DAMAR_WRITE_THREADS");
  int n = e ? atoi(e) : 2;
  if (n < 1) n = 1;
  if (n > 16) n = 16;
  for (int i = 0; i < n; i++)
    A_s2.threads.push_back(new std::thread(write_worker));
}

void tail_stop(void)
{ Stage *st[2] = { &A_s1, &A_s2 };
  for (int i = 0; i < 2; i++)
    { { std::lock_guard<std::mutex> lk(st[i]->mu);
        st[i]->quit = true;
      }
      st[i]->cv.notify_all();
      for (std::thread *th : st[i]->threads)
        { th->join();
          delete th;
        }
      st[i]->threads.clear();
    }
}

void tail_totals(int64 *ncheck, double *tail_ms, double *write_ms)
{ std::lock_guard<std::mutex> lk(A_mu);
  if (ncheck)   *ncheck = A_ncheck;
  if (tail_ms)  *tail_ms = A_tail_ms;
  if (write_ms) *write_ms = A_write_ms;
  A_ncheck = 0;  A_tail_ms = 0;  A_write_ms = 0;
}

double tail_d2h_ms(void)
{ std::lock_guard<std::mutex> lk(A_mu);
  double v = A_d2h_ms;
  A_d2h_ms = 0;
  return v;
}
