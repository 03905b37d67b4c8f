/* damar_host.h -- internal host-side declarations shared by the C-ABI shim, the
 * daligner driver and the per-pair tail (redundancy.c, bridge.c). */
#ifndef DAMAR_HOST_H
#define DAMAR_HOST_H

#include <stdio.h>

#include "damar_db.h"
#include "damar_align.h"
#include "damar_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A local alignment of one read pair while it is still being post-processed: the
 * reference keeps Path records whose trace field is an offset into a growing
 * uint16 pool (filter.c:1369-1374 Trace_Buffer, :2353-2357). */
typedef struct
{ int   tlen, diffs;
  int   abpos, bbpos;
  int   aepos, bepos;
  int64 toff;
} damar_path;

typedef struct
{ uint16 *val;
  int64   top, max;
} damar_tpool;

int64 damar_tpool_push(damar_tpool *tp, const uint16 *src, int n);

/* how often the rare branches of the host tail ran (tests assert the fixtures reach them) */
extern int64 damar_stat_redundancy_calls, damar_stat_fusions, damar_stat_bridges;

/* What Bridge needs beyond the paths: the two sequences (filter.c:1998, 2025). */
typedef struct
{ const char *aseq, *bseq;
  int         alen, blen;
} damar_bridge_ctx;

/* bridge.c: filter.c:1456-1571 Compute_Bridge_Path + :1747-1802 Bridge +
 * :1444-1454 Check_Bridge for one candidate (path1,path2).  Returns non-zero if the
 * candidate was skipped. */
int damar_bridge_pair(const damar_bridge_ctx *ctx, damar_path *jp, damar_path *kp,
                      damar_path *p1, damar_path *p2, damar_path *b1, damar_path *b2,
                      int aovl, int bovl, int comp, int ts, damar_tpool *tp,
                      damar_path *bm, int j);

void damar_bridge_release(void);       /* frees the calling thread's work buffers */

int  damar_handle_redundancies(damar_path *am, int n, damar_path *bm, int comp, int ts,
                               damar_tpool *tp, const damar_bridge_ctx *bridge);

void damar_emit_pair(damar_path *am, int na, damar_path *bm, int nb, damar_tpool *tp,
                     int comp, int ts, int aread, int bread,
                     const damar_bridge_ctx *bridge, Overlap_IO_Buffer *obuf, int64 *nrec);

int damar_append_overlap_buffer(Overlap_IO_Buffer *dst, const Overlap_IO_Buffer *src);

/* Detached overlap buffers for a writer thread (las.c) */
typedef struct { int trace_space, nthreads, symmetric, only_identity;
                 void *lens;            /* with checking on (damar_set_check): the read lengths noted at the spec, las.c's to free */
               } damar_write_params;
Overlap_IO_Buffer *damar_detach_overlap_buffers(Align_Spec *spec, damar_write_params *p);
void damar_write_detached(const damar_write_params *p, Overlap_IO_Buffer *bufs,
                          const char *dir1, const char *dir2, const char *ablock, const char *bblock, int lastRead);

int  damar_check_on(void);             /* las.c: damar_set_check(1) is in force */

/* piles.c: what the mask tools need beside the C-ABI of include/damar_hip.h */
typedef struct
{ int   nreads, maxlen;
  int  *read_len, *read_flags;
  int   nblocks;               /* 0: the database is not split */
  int  *block_first;           /* [nblocks + 1] */
  char *path;                  /* <dir>/.<root>, what track file names start with */
} damar_dbinfo;

int  damar_dbinfo_open(const char *name, damar_dbinfo *db);     /* stub + .idx, no bases */
void damar_dbinfo_close(damar_dbinfo *db);

/* What the host passes share in small: the flag bits of a record, the colours of the reference's PASS lines, and the
   routines every pass had a copy of. */
#define OVL_COMP       0x1                /* lib/oflags.h */
#define OVL_DISCARD    0x2
#define OVL_REPEAT     0x8
#define OVL_LOCAL      0x10
#define OVL_DIFF       0x20
#define OVL_STITCH     0x80
#define OVL_SYMDISCARD 0x100
#define OVL_OLEN       0x200
#define OVL_RLEN       0x400
#define OVL_TEMP       0x800
#define OVL_CONT       0x8000
#define OVL_GAP        0x10000
#define OVL_TRIM       0x20000
#define OVL_MODULE     0x40000

#define GREEN "\x1b[32m"                  /* lib/colors.h */
#define RESET "\x1b[0m"

/* value k of a trace of tbytes bytes a value, and of record rec of a batch */
static inline int damar_trace_at(const void *trace, int tbytes, int64 k)
{ const unsigned char *q = (const unsigned char *) trace + tbytes * k;
  return tbytes == 1 ? q[0] : (q[0] | (q[1] << 8));
}

static inline int damar_trace_value(const damar_trace_batch *t, int64 rec, int k)
{ return damar_trace_at(t->trace + t->trace_off[rec], t->tbytes, k);
}

/* LAgap.c:255: 1 when [ab, ae) lies within [bb, be), 2 when it is the other way round, else 0.  LAfilter.c:252 asks for
   the first alone: == 1 */
static inline int damar_contained(int ab, int ae, int bb, int be)
{ if (ab >= bb && ae <= be)
    return 1;
  if (bb >= ab && be <= ae)
    return 2;
  return 0;
}

static inline int damar_intersect(int ab, int ae, int bb, int be)      /* lib/utils.c:250 */
{ const int b = ab > bb ? ab : bb, e = ae < be ? ae : be;
  return b < e ? e - b : 0;
}

/* anno[0 .. nreads]: a track's byte counts per read into its offsets */
static inline void damar_counts_to_offsets(uint64 *anno, int nreads)
{ uint64 off = 0, c;
  int    j;
  for (j = 0; j <= nreads; j++)
    { c = anno[j];
      anno[j] = off;
      off += c;
    }
}

/* B read r's bases [from, to) as an alignment sees them: the read itself, or its complement; 4 beyond its ends */
static inline void damar_gather_b(const HITS_DB *blk, int r, int comp, int from, int to, char *dst)
{ const char *s = (const char *) blk->bases + blk->reads[r].boff;
  const int   len = blk->reads[r].rlen;
  int i;
  for (i = from; i < to; i++)
    if (i < 0 || i >= len)
      *dst++ = 4;
    else
      *dst++ = comp ? (char) (3 - s[len - 1 - i]) : s[i];
}

/* laspass.c: what a pass over a .las file needs.  Plain C, nothing of the GPU runtime. */
void *damar_grow(void *p, size_t n, const char *who);         /* realloc or, after a message, exit(1) */
/* 1 and *cap raised to need + need / 4 + slack when need is above *cap (the caller grows its arrays to *cap), else 0 */
static inline int damar_room(int64 *cap, int64 need, int64 slack)
{ if (need <= *cap)
    return 0;
  *cap = need + need / 4 + slack;
  return 1;
}
/* p with room for `need` elements of `size` bytes by that rule */
void *damar_reserve(void *p, int64 *cap, int64 need, size_t size, int64 slack, const char *who);

/* A batch takes the database's read table; which of its reads are looked up in it: none, the A read of every pile, or the
   B read of every record as well.  0, or 1 after "damar: <las> holds reads the database does not have". */
enum { DAMAR_BIND_ONLY = 0, DAMAR_BIND_A, DAMAR_BIND_AB };
int  damar_batch_bind(damar_pile_batch *b, const damar_dbinfo *db, const char *las, int reads);
int  damar_reads_missing(const char *las);                     /* that line alone, for a pass that looks per pile; 1 */

/* The records of a pass written to a .las file in file order.  open: the fopen alone (NULL: it failed, nothing is said);
   begin: the header; put: the ten words of rec (rec[0]: the number of trace values) and the trace -- vals, narrowed to
   tbytes bytes a value, or when vals is NULL the tbytes-wide values at bytes.  OVL_TEMP is taken off the flags word, a
   record flagged OVL_DISCARD is counted and, with purge, not written.  0; 1 (no message) when the write fails; 2 after
   "<tool>: Compression of trace to bytes fails, value too big".  close: with ok (the pass came to its end) the count goes
   into the header and *written receives it; "damar: cannot write <path>" once when a write, or with ok the close, failed.
   0, or 1 after that line. */
typedef struct damar_las_out damar_las_out;
int   damar_cannot_write(const char *path);                    /* that line alone, for the files a pass writes beside; 1 */
damar_las_out *damar_las_out_open(const char *path, int purge);
int   damar_las_out_begin(damar_las_out *o, int tspace);
int   damar_las_out_put(damar_las_out *o, const int *rec, const unsigned char *bytes, const uint16 *vals, int tbytes, const char *tool);
int64 damar_las_out_written(const damar_las_out *o);
int   damar_las_out_close(damar_las_out *o, int ok, int64 *written, int64 *discarded);

typedef struct damar_pile_reader damar_pile_reader;
damar_pile_reader *damar_piles_open(const char *las, int64 bound);     /* bound <= 0: 8 M records; DAMAR_PILE_BATCH lowers it */
int   damar_piles_next(damar_pile_reader *r, damar_pile_batch *b);
void  damar_piles_rewind(damar_pile_reader *r);
int   damar_piles_tspace(const damar_pile_reader *r);
int64 damar_piles_novl(const damar_pile_reader *r);
/* the reader with the traces on (LAq): tbound <= 0: 1 GiB of trace bytes per batch; DAMAR_PILE_TRACE_BYTES lowers it */
damar_pile_reader *damar_piles_open_traces(const char *las, int64 bound, int64 tbound);
int   damar_piles_next_traces(damar_pile_reader *r, damar_trace_batch *t);
void  damar_piles_close(damar_pile_reader *r);

int  damar_piles_on_host(void);                                  /* DAMAR_PILES=host */
int  damar_host_pile_coverage(const damar_pile_batch *b, const damar_repeat_params *p, int64 *histo, int64 *bases, int64 *inactive);
int  damar_host_pile_repeats(const damar_pile_batch *b, const damar_repeat_params *p, damar_pile_track *out);
int  damar_host_pile_tandem(const damar_pile_batch *b, int min_len, damar_pile_track *out);

int  damar_track_write_a2(const char *dbpath, const char *track, int block, int nreads, const uint64 *anno, const int *data, int64 ndata);
int  damar_track_write_anno(const char *dbpath, const char *track, int block, int len, const int64 *offs, const int *data);

/* quality.c: LAq (scrub/LAq.c) as calls */
int  damar_trace_batch_valid(const damar_trace_batch *b, int64 *ntiles);     /* what both paths index with; 0 after a message */
int  damar_host_pile_quality(const damar_trace_batch *b, const damar_q_params *p, int *q_out);
/* trim_q_offsets: dataq[ndata] is the q data of ALL reads ([ob, oe) this read's; the walk looks at its neighbours' too, a value
   past the end counts as 0), *tb / *te the interval to start from (0: the read's end) and the result.  0: no q data. */
int  damar_trim_from_q(const int *dataq, int64 ndata, int64 ob, int64 oe, int rlen, int tspace, int trim_q, int min_len, int ccs,
                       int *tb, int *te);
typedef struct
{ uint64 *q_anno, *trim_anno;  /* [nreads + 1] byte offsets, malloc'ed */
  int    *q_data, *trim_data;
  int64   nq, ntrim;
} damar_q_result;
/* the annotate pass over a file: q and trim of every read with a pile.  0, or 1 after a message. */
int  damar_q_track(const damar_dbinfo *db, const char *las, const damar_q_params *p, int trim_q, int min_len, damar_q_result *res);
/* -u: the trim track again from record headers, the q track and the trim track at hand (res->q_* stay NULL) */
int  damar_trim_update(const damar_dbinfo *db, const char *las, const uint64 *q_anno, const int *q_data, int64 nq,
                       const uint64 *trim_anno, const int *trim_data, int trim_q, int min_len, int ccs, damar_q_result *res);
void damar_q_result_free(damar_q_result *res);
/* a track of the whole database as damar_track_write_a2 writes it: anno[nreads + 1] and data, malloc'ed.  0, or 1 (no message) */
int  damar_track_read_a2(const char *dbpath, const char *track, int nreads, uint64 **anno, int **data, int64 *ndata);

/* bridge.c: the exact alignment of one box with its edit script (what damar_align_boxes returns per box): A[0..M) against
   B[0..N), M, N >= 1; script holds max(M, N) values at most, *slen receives their number; returns the differences */
int  damar_exact_box(const char *A, int M, const char *B, int N, int *script, int *slen);
int  damar_trim_on_host(void);                                   /* DAMAR_TRIM=host */
void damar_piles_rest(const damar_pile_reader *r, const int **diffs, const int **last_word);
const int *damar_piles_tlen(const damar_pile_reader *r);

/* trim.c: LAtrim (scrub/LAtrim.c, lib/trim.c) as a call: every record of `las` cut back to what the trim track keeps of
   both reads, written to `out` in file order (purge: without the records that end up discarded).  0, or 1 after a message. */
typedef struct
{ int64 novl, ntrimmed;        /* records seen, records cut */
  int64 novl_bases, ntrim_bases;
  int64 written, discarded;    /* records written, records flagged for removal */
  int64 boxes, box_a, box_b;   /* trace segments realigned, and the bases of A and of B in them */
} damar_trim_stats;
int  damar_trim_las(const char *db, const char *las, const char *out, const char *track, int purge, damar_trim_stats *st);
/* The same per batch of whole piles in memory (what damar_trim_las and gap.c run): open loads the trim track and the bases
   (NULL; *no_track set and no message when the track is not there), batch runs plan / align / settle on the batches of one
   file in file order and leaves every record's new coordinates, flags, differences and trace values (record i's are the
   tlen[i] values at trace + toff[i]) in arrays of the trimmer's, good until the next call; st is added to. */
typedef struct damar_trimmer damar_trimmer;
typedef struct
{ const int    *abpos, *aepos, *bbpos, *bepos, *flags, *diffs, *tlen;     /* [nrec] */
  const int64  *toff;
  const uint16 *trace;
} damar_trimmed;
damar_trimmer *damar_trimmer_open(const char *dbname, const damar_dbinfo *db, const char *track, int *no_track);
int  damar_trimmer_batch(damar_trimmer *tm, const damar_trace_batch *t, const int *rdiffs, const char *las, int64 first,
                         damar_trim_stats *st, damar_trimmed *res);
int  damar_trimmer_aread(const damar_trimmer *tm, int64 rec);
void damar_trimmer_close(damar_trimmer *tm);
/* quality.c: a track of the whole database in either form, the compressed one first (then .anno / .data, db/DB.c
   Load_Track): as damar_track_read_a2.  0, or 1 (no message) */
int  damar_track_read_any(const damar_dbinfo *db, const char *track, uint64 **anno, int **data, int64 *ndata);

/* gap.c: LAgap (scrub/LAgap.c) -- the plain routine behind damar_pile_gaps (DAMAR_PILES=host, and the piles the kernel
   leaves), the checks both paths share, and the pass over a file. */
typedef struct { int *ev; int64 n, cap; } damar_gap_list;       /* DAMAR_GAP_EVENT_INTS ints per event, n events */
int  damar_gap_inputs_valid(const damar_pile_batch *b, const damar_gap_params *p);          /* 0 after a message */
/* one pile: flags_out[the pile's records] from the batch's flags, its events appended to L, cnt[3] (contained, breaks,
   records dropped) added to */
void damar_host_gap_pile(const damar_pile_batch *b, int64 pile, const damar_gap_params *p, int *flags_out, damar_gap_list *L, int64 *cnt);
typedef struct
{ int64 novl, written, discarded;
  int64 contained, breaks, dropped;        /* the reference's closing counters */
  int64 piles, host_piles, events;         /* summed over the batches: damar_gap_last's counts */
  damar_trim_stats trim;                   /* -t */
} damar_gap_stats;
/* the pass over a file: per batch of whole piles the trim (p->trim_track), damar_pile_gaps, the reference's lines on stdout,
   and the records written to `out` in file order (p->purge: without the discarded ones).  0, or 1 after a message. */
void damar_gap_no_track(const char *track);      /* the reference's two lines for a track that cannot be loaded */
int  damar_gap_las(const char *db, const char *las, const char *out, const damar_gap_params *p, damar_gap_stats *st);

/* separate.c: LAseparate (scrub/LAseparate.c) -- the plain routine behind damar_pile_chains (DAMAR_PILES=host, and the
   groups the kernel leaves), the check both paths share, and the pass over a file. */
int  damar_separate_inputs_valid(const damar_pile_batch *b, const damar_separate_params *p, const damar_chain_out *out);     /* 0 after a message */
/* one group: the n records from `first` on of pile `pile`; one pile: its groups */
void damar_host_chain_group(const damar_pile_batch *b, int64 pile, int64 first, int n, const damar_separate_params *p, damar_chain_out *out);
void damar_host_chain_pile(const damar_pile_batch *b, int64 pile, const damar_separate_params *p, damar_chain_out *out);
typedef struct
{ int64 novl, written, written_discard;
  int64 kept, discarded;                   /* the reference's counters of its first pass */
  int64 groups, host_groups, multi;        /* summed over the batches: damar_separate_last's counts */
} damar_separate_stats;
/* the pass over a file, read once: per batch of whole piles damar_pile_chains, the records the verdict keeps written to
   `out` and the others to `out_discard`, the reference's lines of both its passes on stdout.  0, or 1 after a message. */
int  damar_separate_las(const char *db, const char *las, const char *out, const char *out_discard, const char *track, int kind,
                        damar_separate_stats *st);

/* fix.c: LAfix (scrub/LAfix.c without -X and -f) -- the plain routine behind damar_pile_patches (DAMAR_PILES=host, and the
   piles the kernel leaves), the checks both paths share, and the pass over a file. */
typedef struct { damar_fix_gap *g; int64 n, cap; } damar_fix_list;
int  damar_fix_inputs_valid(const damar_trace_batch *t, const damar_fix_params *p, const int *trim);       /* 0 after a message */
/* one pile kept from trim_ab to trim_ae: its repairs appended to L in the order they are spliced in */
void damar_host_fix_pile(const damar_trace_batch *t, int64 pile, const damar_fix_params *p, int trim_ab, int trim_ae, damar_fix_list *L);
typedef struct
{ int   min_len, lowq, maxgap, low_coverage;     /* -x -Q -g -l */
  const char *q_track, *trim_track, *rep_track;  /* -q, -t and -r (NULL: none) */
  const char **convert;                          /* -c, in the order given */
  int   nconvert;
  const char *trim_out;                          /* -T, NULL: none */
} damar_fix_opts;
typedef struct
{ int64 gaps, flips, chimers;              /* the reference's closing counters */
  int64 bases_before, bases_after;
  int64 reads_trimmed, reads_fixed;        /* headers written */
  int64 piles, host_piles, repairs;        /* summed over the batches: damar_fix_last's counts */
} damar_fix_stats;
/* the pass over a file: per batch of whole piles the flip step, damar_pile_patches, the splice, and the reads written to
   `fasta`; the reference's lines on stdout.  0, or 1 after a message. */
int  damar_fix_las(const char *db, const char *las, const char *fasta, const damar_fix_opts *o, damar_fix_stats *st);

/* filter.c: LAfilter (scrub/LAfilter.c without its experimental branches) -- the plain routine behind damar_pile_filter
   (DAMAR_PILES=host, and the piles the kernel leaves), the checks both paths share, and the pass over a file. */
int  damar_filter_inputs_valid(const damar_trace_batch *t, const int *diffs, const damar_filter_params *p, const damar_filter_out *out);     /* 0 after a message */
/* one pile: every array of out at the pile's records, and its DAMAR_FC_COUNT counters */
void damar_host_filter_pile(const damar_trace_batch *t, const int *diffs, int64 pile, const damar_filter_params *p, damar_filter_out *out);
typedef struct
{ damar_filter_params p;                   /* the numeric options; its pointers and `steps` are damar_filter_las's to fill */
  int   verbose, purge, do_trim;           /* -v -p -T */
  const char *trim_track, *rep_track;      /* -t -r */
  const char *exclude, *include;           /* -x -I (NULL: none) */
  const char *discarded_out, *discarded_in;        /* -a -A (NULL: none) */
} damar_filter_opts;
typedef struct
{ int64 novl, written, discarded;
  int64 cnt[DAMAR_FC_COUNT];               /* the reference's closing counters */
  int64 piles, host_piles;                 /* summed over the batches: damar_filter_last's counts */
  damar_trim_stats trim;                   /* -T */
} damar_filter_stats;
void damar_filter_no_track(const char *track);   /* the reference's two lines for a track that cannot be loaded */
/* the reference's main from its first fopen on: the tracks and lists loaded, then per batch of whole piles -f and -b, the
   trim (-T), damar_pile_filter, the reference's lines on stdout, the records written.  0, or 1 after a message. */
int  damar_filter_las(const char *db, const char *las, const char *out, const damar_filter_opts *o, damar_filter_stats *st);

/* correct.c: LAcorrect (corrector/LAcorrect.c) -- the plain routine behind damar_tile_consensus (DAMAR_PILES=host, and the
   tiles the kernel leaves), the check both paths share, and the pass over a file. */
int  damar_tile_batch_valid(const damar_tile_batch *b);                                      /* 0 after a message */
/* one tile: *out (room for *cap values, grown here) receives the called bases; their number, or -1 after a message */
int  damar_host_tile(const damar_tile_batch *b, int64 tile, unsigned char **out, int64 *cap);
void damar_host_tile_release(void);
typedef struct
{ int   verbose, nthreads, block;          /* -v -j -b (block <= 0: all reads) */
  const char *q_track, *read_ids;          /* -q, -r (NULL: all reads) */
} damar_correct_opts;
typedef struct
{ int64  reads, copies;                    /* headers written */
  int64  tiles, host_tiles, bases;         /* summed over the batches: damar_correct_last's counts */
  double ms_consensus, ms_kernel;          /* the damar_tile_consensus calls (wall), their kernels (HIP events) */
  double ms_postrace, ms_postrace_wait;    /* the whole-read alignments summed over the worker threads; what the pass waited for them */
  double ms_total;
  int64  postrace_boxes, postrace_host;    /* summed over the damar_align_reads calls: boxes, boxes the host routine did beside the kernel */
  double ms_postrace_kernel, ms_postrace_call;     /* their kernels (HIP events), the calls (wall) */
} damar_correct_stats;
/* the pass over a file: the reads written to <out>.NN.fasta, one file per part of -j; the reference's lines on stdout.
   The postrace alignments of a batch go through one damar_align_reads call; with DAMAR_POSTRACE=host or DAMAR_PILES=host
   they run in DAMAR_CORRECT_THREADS (8) worker threads.  0, or 1 after a message. */
int  damar_correct_las(const char *db, const char *las, const char *out, const damar_correct_opts *o, damar_correct_stats *st);

/* bridge.c: the exact alignment of one box into trace pairs (what damar_trace_boxes returns per box): A[0..M) against
   B[0..N), M, N >= 1, A's position 0 lying abpos >= 0 bases into the grid of ts; trace holds
   2 * ((abpos + M + ts - 1) / ts - abpos / ts) values, *tlen receives their number; returns the differences.  Works in the
   calling thread's buffers (damar_bridge_release frees them). */
int  damar_trace_box(const char *A, int M, const char *B, int N, int abpos, int ts, uint16 *trace, int *tlen);
int  damar_stitch_on_host(void);                                 /* DAMAR_STITCH=host */

/* stitch.c: LAstitch (scrub/LAstitch.c stitch_handler2) as a call: the records of one (A read, B read) run that the
   overlapper split are rejoined, the joint realigned exactly, the superfluous record flagged; written to `out` in file
   order (purge: without the discarded records).  0, or 1 after a message. */
typedef struct
{ int    fuzz, purge;          /* -f -p */
  int    anchor, merge, min_len, min_merge;      /* -a -m -l -M */
  double gap_diff;             /* -d */
  const char *lc_track, *rep_track;              /* -t -r, NULL: none */
} damar_stitch_params;
#define DAMAR_STITCH_ROUNDS 16
typedef struct
{ int64 novl, written, discarded;
  int64 stitched, stitched_lc; /* joins by the fuzz test, joins by a low-complexity break */
  int64 candidates;            /* pairs that passed the candidate tests: boxes + no_box */
  int64 no_box;                /* candidates Compute_Bridge_Path gave up on (a widening ran off a record, or bout < bin) */
  int64 widened;               /* boxes whose joint took at least one widening step */
  int64 boxes, box_a, box_b;   /* boxes realigned, and the bases of A and of B in them */
  int64 refused;               /* boxes Check_Bridge turned down */
  int64 rounds;                /* the most rounds a batch of piles took */
  int64 round_boxes[DAMAR_STITCH_ROUNDS];        /* boxes per round, summed over the batches; the last entry takes the rest */
} damar_stitch_stats;
int  damar_stitch_las(const char *db, const char *las, const char *out, const damar_stitch_params *p, damar_stitch_stats *st);

/* homogenize.c: TKhomogenize (scrub/TKhomogenize.c).  The plain routine behind the session calls of include/damar_hip.h
   (DAMAR_PILES=host), the checks both paths share, and the pass over a file. */
typedef struct damar_host_homog damar_host_homog;
void damar_bits_set_range(unsigned char *bits, int64 nbits, int64 beg, int64 end);          /* ba_assign_range(.., 1), held to nbits */
int  damar_trim_pairs(const uint64 *anno, const int *data, int nreads, int *pairs);         /* get_trim of every read; 1: not a trim track */
int  damar_homog_seed_valid(const int *read_len, int nreads, const uint64 *anno, const int *data, int64 ndata);     /* 0 after a message */
int  damar_homog_inputs_valid(const damar_trace_batch *t, int nreads, const int *read_len, const uint64 *anno, const int *data,
                              int64 ndata, int ends, const int *trim);
damar_host_homog *damar_host_homog_open(const int *read_len, int nreads, int res);
int  damar_host_homog_seed(damar_host_homog *h, const uint64 *anno, const int *data);
int  damar_host_homog_add(damar_host_homog *h, const damar_trace_batch *t, const uint64 *anno, const int *data, int ends, const int *trim);
int  damar_host_homog_finish(damar_host_homog *h, uint64 *anno, int **data, int64 *ndata, int64 *tagged);
void damar_host_homog_counts(const damar_host_homog *h, int64 *cnt /* [3] */);
void damar_host_homog_close(damar_host_homog *h);
typedef struct
{ int merge, ends, res;        /* -m, -e (-1: none), -r */
  const uint64 *iv_anno;       /* -i: the interval track of the whole database, byte offsets */
  const int    *iv_data;
  int64         iv_ndata;
  const uint64 *trim_anno;     /* -t, looked at when ends != -1 */
  const int    *trim_data;
} damar_homog_params;
typedef struct
{ uint64 *anno;                /* [nreads + 1] byte offsets, malloc'ed */
  int    *data;
  int64   ndata, tagged;
} damar_homog_result;
/* the pass over a file: open, seed (-m), add per batch of whole piles, finish.  0, or 1 after a message. */
int  damar_homogenize_track(const damar_dbinfo *db, const char *las, const damar_homog_params *p, damar_homog_result *res);
void damar_homog_result_free(damar_homog_result *res);

/* dust.c: DBdust (db/DBdust.c) -- the plain routine behind damar_dust_reads (DAMAR_DUST=host, and the reads the kernel
   leaves) and the command's work. */
typedef struct { int *iv; int64 n, cap; } damar_dust_list;       /* n retired candidates: start, last triplet */
int   damar_dust_on_host(void);                                   /* DAMAR_DUST=host */
int   damar_dust_params_valid(const damar_dust_params *p);        /* 0 after a message */
/* the machine over the triplets [start, stop) of seq[0 .. len) from an empty state; the retired candidates that start in
   [own_beg, own_end) appended to out; steps (or NULL): [0] += steps taken, [1] += steps that entered the walk.  Returns the
   longest the candidate list became. */
int   damar_host_dust_piece(const unsigned char *seq, int len, const damar_dust_params *p, int start, int own_beg, int own_end,
                            int stop, damar_dust_list *out, int64 *steps);
/* n candidates in order of their starts -> the [beg, end) pairs of the mask in out (room for n of them); their number */
int64 damar_host_dust_join(const int *cand, int64 n, int minlen, int *out);
/* one read: whole (piece <= 0) or cut into pieces of `piece` starts with `halo` triplets in front; out needs room for
   len pairs, work is the caller's scratch list; the number of pairs */
int64 damar_host_dust_read(const unsigned char *seq, int len, const damar_dust_params *p, int piece, int halo, int *out,
                           damar_dust_list *work, int64 *steps);
/* the track of a block, or of a database (appended to where it exists): stats (or NULL) [0 .. 6) += reads, host reads,
   intervals, bases, steps, walk steps.  0, or 1 after a message */
int   damar_dust_track(const char *name, const damar_dust_params *p, int64 *stats);

/* masks.c: both tools as calls (the commands and the Python interface are argument handling around them) */
typedef struct
{ int64 *histo;                /* [max_cov], malloc'ed, NULL when no estimate ran */
  int    cov_max;              /* MAX: the estimate */
  int64  cov_bases, cov_inactive;
  int    avg_rlen;
  int    cov;                  /* what the repeat pass used */
  uint64 *anno;                /* [nreads + 1] byte offsets, malloc'ed */
  int   *data;
  int64  ndata, merged, bases_total, bases_repeat;
} damar_repeat_result;

/* LArepeat.c main: estimate pass unless p->cov > 0 (or cov_only), then the repeat pass.  max_areads < 0: all piles.
   0, or 1 after the reference's message where the reference exits with 1. */
int  damar_repeat_track(const damar_dbinfo *db, const char *las, const damar_repeat_params *p, int max_areads, int cov_only,
                        damar_repeat_result *res);
void damar_repeat_result_free(damar_repeat_result *res);
/* TANmask.c make_a_pass for the reads [first, last): offs[last - first + 1] byte offsets and the data, both malloc'ed.
   0, or 1 when the file's reads lie outside the range. */
int  damar_tan_track(const damar_dbinfo *db, const char *las, int first, int last, int min_len, int64 **offs, int **data,
                     int64 *nmasks, int64 *masked);

#ifdef __cplusplus
}
#endif
#endif
