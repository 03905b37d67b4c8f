/* hosttail.cpp -- ORACLE (test infrastructure): the driver that puts the product's whole host tail
 * (damar_amd/csrc/host/tail.cpp: ordering, job filter, wide map, views, thread pool, pipeline) behind the CPU front
 * of the *_hosttail binaries.  The front appends one LaRecord per alignment it keeps; a comparison's records are handed
 * to the tail the way a launch delivers them.  Knobs, all off by default (the environment):
 *   ORACLE_HT_SHUFFLE=seed    the records in a seeded random order (the device delivers them in completion order)
 *   ORACLE_HT_BYTES=1         the pool as bytes with t8 = 1 where the spacing is at most TRACE_XOVR and every value fits
 *   ORACLE_HT_JOBS=k          the records carry job k of k + 2 in the top byte of seq, beside records of the other jobs
 *   ORACLE_HT_WIDE=seed       a seeded third of the items is in a wide map: their records carry DAMAR_ITEM_WIDE and
 *                             stand beside unmarked junk for the same items, which the tail must drop
 *   ORACLE_HT_SPEC_THREADS=n  overlap buffers of the Align_Spec (against the tail's own DAMAR_TAIL_THREADS: at least as
 *                             many = it fills them directly, fewer = private buffers appended in order)
 *   ORACLE_HT_PIPELINE=1      tails and file writes go through the two-stage pipeline and are drained, instead of being
 *                             called inline; the "landed" hook sleeps a millisecond so that stage 1 really waits
 */
#include <algorithm>
#include <random>
#include <vector>
#include <stdlib.h>
#include <unistd.h>

#include "oracle.h"
#include "../damar_amd/csrc/host/tail.h"

static int knob(const char *name)
{ const char *e = getenv(name);
  return e ? atoi(e) : -1;
}

struct Launch : damar_tail_buf              /* the records of one comparison, and what keeps them alive */
{ std::vector<LaRecord>      r;
  std::vector<uint16>        p;
  std::vector<unsigned char> p8;
  std::vector<unsigned int>  wm;
};
static Launch *cur = NULL;
static bool    piped = false;

static double landed(damar_tail_buf *)      { usleep(1000);  return 0.; }
static void   release(damar_tail_buf *b)    { delete static_cast<Launch *>(b); }

static void finish(void)
{ if (piped)
    { tail_drain();
      tail_stop();
    }
  tail_pool_join();
}

extern "C" int oracle_ht_spec_threads(void)
{ const int n = knob("ORACLE_HT_SPEC_THREADS");
  return n > 0 ? n : 1;
}

extern "C" void oracle_ht_record(const Path *a, int btlen, const uint16 *atr, const uint16 *btr,
                                 int aread, int bread, unsigned int item, unsigned int seq)
{ if (cur == NULL)
    cur = new Launch();
  LaRecord r;
  r.abpos = a->abpos;  r.bbpos = a->bbpos;  r.aepos = a->aepos;  r.bepos = a->bepos;  r.diffs = a->diffs;
  r.atlen = a->tlen;  r.btlen = btlen;
  r.aread = aread;  r.bread = bread;
  r.item = item;  r.seq = seq;
  r.toff = (unsigned int) cur->p.size();
  cur->p.insert(cur->p.end(), atr, atr + a->tlen);
  cur->p.insert(cur->p.end(), btr, btr + btlen);
  cur->r.push_back(r);
}

extern "C" void oracle_ht_compare(const HITS_DB *ablock, const HITS_DB *bblock, int self, int comp, Align_Spec *spec,
                                  int symmetric, int hgap_min, int no_bridge, int64 *ncheck)
{ static bool first = true;
  if (first)
    { first = false;
      piped = knob("ORACLE_HT_PIPELINE") > 0;
      if (piped)
        tail_start();
      atexit(finish);
    }
  Launch *L = cur ? cur : new Launch();
  cur = NULL;
  std::vector<LaRecord> &r = L->r;
  const size_t n = r.size();
  int jobid = 0, njobs = 1;

  const int wseed = knob("ORACLE_HT_WIDE");
  if (wseed >= 0)
    { unsigned int top = 0;
      for (size_t i = 0; i < n; i++)
        top = std::max(top, r[i].item);
      L->wm.assign(top / 32 + 2, 0u);
      for (size_t i = 0; i < n; i++)
        if ((r[i].item * 2654435761u + (unsigned int) wseed * 40503u) % 3u == 0)
          { LaRecord junk = r[i];                      /* what the two-pair kernel left behind for the pair */
            junk.diffs += 7;  junk.aepos -= 1;
            r.push_back(junk);
            L->wm[r[i].item >> 5] |= 1u << (r[i].item & 31);
            r[i].item |= DAMAR_ITEM_WIDE;
          }
    }
  const int job = knob("ORACLE_HT_JOBS");
  if (job >= 0)
    { jobid = job;  njobs = job + 2;
      const size_t m = r.size();
      for (size_t i = 0; i < m; i++)
        { LaRecord other = r[i];                       /* another comparison of the same launch */
          other.seq |= (unsigned int) ((job + 1 + (int) (i % (size_t) (njobs - 1))) % njobs) << DAMAR_SEQ_BITS;
          other.diffs += 3;
          r[i].seq |= (unsigned int) job << DAMAR_SEQ_BITS;
          r.push_back(other);
        }
    }
  const int sseed = knob("ORACLE_HT_SHUFFLE");
  if (sseed >= 0)
    { std::mt19937 gen((unsigned int) sseed);
      for (size_t i = r.size(); i > 1; i--)            /* (spelled out: the order must not depend on the library) */
        std::swap(r[i - 1], r[gen() % i]);
    }
  L->t8 = 0;
  if (knob("ORACLE_HT_BYTES") > 0 && Trace_Spacing(spec) <= TRACE_XOVR)
    { bool fits = true;
      for (uint16 v : L->p)
        fits = fits && v <= 255;
      if (fits)                                        /* otherwise 16-bit, as the device's fallback */
        { L->p8.assign(L->p.begin(), L->p.end());
          L->t8 = 1;
        }
    }
  L->recs = r.data();  L->nrec = r.size();
  L->tpool = L->t8 ? (uint16 *) L->p8.data() : L->p.data();  L->ntp = L->p.size();
  L->wmap = L->wm.empty() ? NULL : L->wm.data();
  L->nwide = L->wm.empty() ? 0 : 1;
  for (int j = 0; j <= DAMAR_MAX_JOBS; j++)
    L->wm_off[j] = 0;
  L->users = 1;
  L->landed = landed;  L->release = release;
  if (ncheck)
    *ncheck = 0;
  if (piped)
    { TailJob *tj = new TailJob();
      tj->kind = 0;
      tj->hb = L;  tj->jobid = jobid;  tj->njobs = njobs;
      tj->ablock = *ablock;  tj->bblock = *bblock;
      tj->self = self;  tj->comp = comp;  tj->spec = spec;
      tj->symmetric = symmetric;  tj->hgap_min = hgap_min;
      tj->got = NULL;                                  /* (the count of a piped comparison is not reported) */
      if (no_bridge)                                   /* the pipeline runs the overlap path's tail only */
        { fprintf(stderr, "oracle: ORACLE_HT_PIPELINE has no datander form\n");
          exit(1);
        }
      tail_submit(tj);
      return;
    }
  const int64 got = damar_host_tail(L->recs, L->nrec, L->tpool, L->t8, L->wmap, ablock, bblock, self, comp, spec,
                                    symmetric, hgap_min, jobid, njobs, no_bridge);
  if (ncheck)
    *ncheck = got;
  delete L;
}

extern "C" void oracle_ht_write(Align_Spec *spec, char *d1, char *d2, char *aroot, char *broot, int last)
{ if (!piped)
    { Write_Overlap_Buffer(spec, d1, d2, aroot, broot, last);
      Reset_Overlap_Buffer(spec);
      return;
    }
  TailJob *job = new TailJob();
  job->kind = 1;  job->spec = spec;
  job->has1 = d1 != NULL;  job->has2 = d2 != NULL;
  if (d1) job->d1 = d1;
  if (d2) job->d2 = d2;
  job->a = aroot;  job->b = broot;  job->last = last;
  tail_submit(job);
}

extern "C" void oracle_ht_drain(void)
{ if (piped)
    tail_drain();
}
