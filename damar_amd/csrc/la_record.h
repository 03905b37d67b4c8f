/* la_record.h -- the record a report kernel writes per local alignment and the host tail reads (host/tail.cpp): plain C,
 * for the kernels' header (kernels/kernels.h) and for host-only sources alike. */
#ifndef DAMAR_LA_RECORD_H
#define DAMAR_LA_RECORD_H

typedef struct
{ int abpos, bbpos, aepos, bepos, diffs;
  int atlen, btlen;
  int aread, bread;       /* block-local ids */
  unsigned int item, seq; /* work item and order of discovery inside it */
  unsigned int toff;      /* offset of the A trace in the trace pool; B trace follows */
} LaRecord;

#define DAMAR_MAX_JOBS 32
#define DAMAR_ITEM_WIDE   0x80000000u   /* in LaRecord.item: written by the wide kernel */
#define DAMAR_SEQ_BITS 24               /* above them in LaRecord.seq: the job of the launch the record belongs to */

#endif
