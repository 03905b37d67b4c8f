/* tail.h -- the per-read-pair host tail of the overlap path (filter.c:2442-2483) and the threads around it (tail.cpp):
 * what stands between the records of a report launch and the overlap buffers of an Align_Spec, and nothing of it
 * knows that a GPU exists.  These names are shared inside libdamar_hip.so and are no part of its interface: hidden.
 */
#ifndef DAMAR_TAIL_H
#define DAMAR_TAIL_H

#include <stddef.h>

#include "../la_record.h"
#ifdef __cplusplus
#include <string>
extern "C" {
#endif
#include "damar_host.h"

#define DAMAR_INTERNAL __attribute__((visibility("hidden")))      /* shared by the library's sources, not exported */

/* The tail of one comparison: those of recs[0 .. nrec) that carry jobid in the top byte of seq (njobs > 1; all of them
 * otherwise), in (item, seq) order, read pair by read pair into the overlap buffers of spec.  tpool holds per record
 * the A trace at toff and the B trace behind it, as bytes where t8 is set; wmap != NULL: one bit per item, set for the
 * pairs of which only the records marked DAMAR_ITEM_WIDE count (the mark is cleared in recs).  no_bridge: datander's
 * rule, fusion and containment only (scrub/tandem.c:767-850).  Returns the number of records written. */
DAMAR_INTERNAL int64 damar_host_tail(LaRecord *recs, size_t nrec, const void *tpool, int t8, const unsigned int *wmap,
                                     const HITS_DB *ablock, const HITS_DB *bblock, int self, int comp, Align_Spec *spec,
                                     int symmetric, int hgap_min, int jobid, int njobs, int no_bridge);

/* What the tail reads of the landing buffer of one launch.  The two hooks are all the pipeline knows of where the
 * buffer comes from; either may be NULL. */
typedef struct damar_tail_buf
{ LaRecord *recs;
  uint16   *tpool;
  size_t    nrec, ntp;
  int       t8;                    /* the trace values are bytes (the launch compressed them: ReportArgs.t8) */
  unsigned int *wmap;              /* nwide > 0: the jobs' bit maps of the read pairs the wide kernel took over (job j from wm_off[j]) */
  unsigned int  nwide, wm_off[DAMAR_MAX_JOBS + 1];
  int       users;                 /* comparisons of the launch whose tails have not run yet */
  double  (*landed)(struct damar_tail_buf *);      /* may block until the download has landed; returns its milliseconds */
  void    (*release)(struct damar_tail_buf *);     /* the last comparison is done with the buffer */
} damar_tail_buf;

#ifdef __cplusplus
}

DAMAR_INTERNAL void   die(void);           /* a fatal error: the process ends without running atexit handlers */
DAMAR_INTERNAL double now_ms(void);        /* wall clock */

/* blocks the host keeps packed: the tail unpacks the reads of a pair that is bridged out of the registered stretch */
DAMAR_INTERNAL void packed_register(const HITS_READ *reads, const damar_packed *pk);
DAMAR_INTERNAL void packed_forget(const HITS_READ *reads);

struct TailJob
{ int kind;                                  /* 0 = tail of one Match_Filter, 1 = write + reset */
  damar_tail_buf *hb;
  int  jobid, njobs;                         /* which comparison of the launch whose records hb holds */
  HITS_DB ablock, bblock;                    /* copies of the block records: the caller may reuse its structs
                                                (the read tables and bases they point to must stay alive) */
  int  self, comp;
  int  symmetric, hgap_min;                  /* the options the comparison ran under */
  Align_Spec *spec;
  std::string d1, d2, a, b;
  bool has1, has2;
  int  last;
  damar_write_params wp;                     /* stage 2 */
  Overlap_IO_Buffer *bufs;
  int64 *got;                                /* kind 0, -v only: where the caller wants the number of confirmed hits (it drains before it reads) */
};

DAMAR_INTERNAL void   tail_start(void);                /* the worker threads of the two stages (DAMAR_WRITE_THREADS writers) */
DAMAR_INTERNAL void   tail_submit(TailJob *job);       /* to stage 1, which owns it from here */
DAMAR_INTERNAL void   tail_drain(void);                /* stage 1, then stage 2 */
DAMAR_INTERNAL void   tail_stop(void);                 /* (drained:) the workers joined */
DAMAR_INTERNAL void   tail_pool_join(void);            /* the threads a tail cuts its records over */
DAMAR_INTERNAL void   tail_totals(int64 *ncheck, double *tail_ms, double *write_ms);      /* since the last call */
DAMAR_INTERNAL double tail_d2h_ms(void);
#endif

#endif
