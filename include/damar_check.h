/* damar_check.h -- the record checker of .las files (host/lascheck.c).
 *
 * One routine for the three places that look at records in file order: the LAcheck tool (host/lacheck_main.c), the
 * writer of las.c under `daligner -C`, and tests.  The first group of properties is what the reference's utils/LAcheck.c
 * looks at (check_process, compare_sort, compare_duplicate, check_post), with its semantics and its wording; the strict
 * group holds what only files written by daligner / datander themselves promise.
 */
#ifndef DAMAR_CHECK_H
#define DAMAR_CHECK_H

#include "damar_align.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DAMAR_CHECK_PTP      0x01    /* -p: bbpos + the B values of the trace = bepos */
#define DAMAR_CHECK_SORT     0x02    /* -s: every record against the one before it */
#define DAMAR_CHECK_DUPES    0x04    /* -d: a record equal to the one before it (damar_lascheck_begin adds SORT) */
#define DAMAR_CHECK_IGNORE   0x08    /* -i: records flagged as discarded are counted, not looked at */
#define DAMAR_CHECK_STRICT   0x10    /* the properties of a file fresh from daligner / datander (messages start "strict:") */
#define DAMAR_CHECK_PAD      0x20    /* with STRICT: the 4 bytes behind ovl->bread are the record's padding on disk */
#define DAMAR_CHECK_ALL      0x40    /* go on behind an A read with a violation (LAcheck stops there and then leaves the
                                        record count alone); the count is compared in any case */

#define DAMAR_OVL_DISCARD    0x2     /* the flag bit the downstream tools set on a record they drop (lib/oflags.h) */

/* A report and its two kinds: a message (LAcheck: stderr), or the "aread bread" line LAcheck prints to stdout with it.
 * The callback gets (arg, kind, text); text is valid during the call only. */
enum { DAMAR_CHECK_MESSAGE = 0, DAMAR_CHECK_PAIR = 1 };  typedef void (*damar_check_report)(void *, int, const char *);

typedef struct
{ int      tspace, options;
  damar_check_report report;
  void    *arg;
  int64    seen;            /* records fed */
  int64    looked;          /* of them, looked at (all but -i's discarded ones) */
  int64    violations;
  int      stopped;         /* LAcheck semantics: nothing is looked at behind the A read of the first violation */
  int      have_prev, split;
  int      prev_a;          /* A read of the group before this one (0 at the start, as in the reference) */
  Overlap  prev;
} damar_lascheck;

/* Start a file of trace spacing `tspace`.  `report` may be NULL (violations are only counted). */
void  damar_lascheck_begin(damar_lascheck *ck, int tspace, int options, damar_check_report report, void *arg);
/* The next record of the file.  `trace`: its tlen values of `tbytes` bytes each (1 or 2), NULL: not at hand (the checks
 * that need them are left out).  A file of one-byte traces (tspace <= TRACE_XOVR) may be fed 16-bit values; STRICT then
 * reports values that do not fit a byte.  From bytes alone a clipped value shows as a wrong sum, which STRICT and PTP
 * report.  alen / blen: the reads' lengths, < 0: unknown.  Returns 0 once the checker has stopped, else 1. */
int   damar_lascheck_feed(damar_lascheck *ck, const Overlap *ovl, const void *trace, int tbytes, int alen, int blen);
/* The next record starts a group of its own even if its A read is that of the last one (the reference's reader does
 * this with what it holds when the file ends before the announced count is reached). */
void  damar_lascheck_break(damar_lascheck *ck);
/* The file is over; expected_novl is the count its header announces (< 0: none).  Returns the violations. */
int64 damar_lascheck_end(damar_lascheck *ck, int64 expected_novl);

/* A whole file against a whole database, as the LAcheck tool does it: messages to `err`, pair lines to `out` (either
 * may be NULL).  Returns 0 (clean), 1 (violations) or 2 (the file or the database cannot be read, said on `err`). */
int   damar_lascheck_file(const char *db, const char *las, int options, FILE *out, FILE *err);

#ifdef __cplusplus
}
#endif
#endif
