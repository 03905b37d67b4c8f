/* shim_internal.h -- what the tool stages (stage.h, stages/ *.hip) take from the core of the shim (shim.hip): the seed
 * stream, the device's properties, bring-up, the radix sort's error word, the layout of a block on the
 * device and of a Work_Data.  These names are shared inside libdamar_hip.so and are no part of its interface: they
 * are hidden.  Nothing else of shim.hip's file scope belongs here.
 */
#ifndef DAMAR_SHIM_INTERNAL_H
#define DAMAR_SHIM_INTERNAL_H

#include <vector>

#include "kernels/dev_common.h"
#include "kernels/kernels.h"

extern "C" {
#include "damar_filter.h"
#include "damar_hip.h"
#include "host/damar_host.h"
}
#include "host/tail.h"               /* DAMAR_INTERNAL, die(), now_ms() */

struct damar_dev_block
{ DevBlock d;
  float freq[4];           /* base frequencies of the block (-b) */
  int   minlen;            /* shortest read */
  u32 *pk_alloc;
  u32 *moff;
  int *mdat;
  u8  *bases_alloc;        /* d.bases = bases_alloc + 64; d.bases[-1] is the leading terminator */
  u32 *boff, *coarse;
  int  nreads;
};

struct WorkData                        /* what a Work_Data * points to */
{ Path   bpath;
  std::vector<uint16> atrace, btrace;
  std::vector<int>    script;          /* Compute_Trace_PTS */
};

DAMAR_INTERNAL extern hipStream_t     G_st;       /* the seed stream: every launch and copy of a tool stage is on it */
DAMAR_INTERNAL extern hipDeviceProp_t G_prop;

DAMAR_INTERNAL void   ensure_init(void);          /* the device brought up, once */
DAMAR_INTERNAL void   late_streams(void);         /* before the first use of G_copy / G_rep / G_ctl: the start-up thread joined */
DAMAR_INTERNAL void   sort_check(const void *sw); /* behind a radix sort on G_st: its error word queued for sort_verify */

#endif
