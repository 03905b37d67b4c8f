/* damar_hip.h -- device-resident entry points of libdamar_hip.so (C ABI, plain pointers
 * and sizes only).
 *
 * The reference has no FFI boundary: dalign/daligner.c calls Sort_Kmers / Match_Filter
 * (dalign/filter.h:64-70, declared for this library in damar_filter.h) directly.  Those
 * two calls hand over HOST buffers, so each of them pays a PCIe copy of the block's
 * bases.  The functions below split them at the PCIe boundary so that a caller that
 * keeps blocks resident in HBM (the multi-GPU block-pair scheduler, bench.py) can time
 * and reuse the device-side work alone:
 *
 *   Sort_Kmers(block,&len)            == damar_block_upload + damar_index_build
 *   Match_Filter(..., atab, btab, ..) == damar_match (+ damar_index_free(btab) when
 *                                        atab != btab, filter.c:2722-2731, 2880-2881)
 *
 * All functions are blocking, single-caller and non-reentrant like the reference's
 * filter.c (file-scope state); fatal errors print to stderr and
 * exit(1) like the reference (db/DB.h:84-86).
 */
#ifndef DAMAR_HIP_H
#define DAMAR_HIP_H

#include "damar_db.h"
#include "damar_align.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Select the GPU (0-based HIP ordinal) and create the stream; returns the number of
 * visible devices.  Called implicitly with device 0 (or $DAMAR_DEVICE) on first use.
 * Exits with a message if no HIP device is present: there is no CPU fallback. */
int   damar_hip_init(int device);
/* NUMA node of the host memory next to GPU `device`, or -1 if the host does not say (callable before damar_hip_init:
 * the node scheduler binds a worker's threads and memory policy to it first, host/daligner.c: node_worker) */
int   damar_hip_numa_node(int device);
const char *damar_hip_device_name(void);
void  damar_hip_sync(void);          /* hipDeviceSynchronize on the selected GPU */
/* Grow (and release again) the process's HBM footprint by `gigabytes`: a cold process pays ~25 ms per GB the first
 * time; called on a thread of its own next to reading the input, the real allocations find the memory ready. */
void  damar_prewarm(int gigabytes);

/* A read block resident in HBM: bases (1 B/base with the reference's 4-terminators,
 * db/DB.c:1562-1605), read offsets, coarse position->read table. */
typedef struct damar_dev_block damar_dev_block;
damar_dev_block *damar_block_upload(const HITS_DB *block);
/* The same on a stream of its own, remembered by the address of block->bases until Sort_Kmers(block) takes
 * it: lets a second host thread upload the next block while the GPU works (one caller thread at a time). */
void damar_block_preload(const HITS_DB *block);
/* damar_block_upload on that second stream, returning the block: for a host thread that prepares blocks ahead. */
damar_dev_block *damar_block_upload_bg(const HITS_DB *block);
/* A block the host keeps PACKED (damar_read_block_packed, include/damar_db.h): its .bps stretch goes up once per strand
 * and the device unpacks it, comp = 1 into the reverse complement (daligner.c:511-570) -- no host unpacking, no host
 * complement, a quarter of the PCIe bytes.  `block` carries reads / freq / tracks of the strand wanted (for comp 1: what
 * damar_complement_copy made of the packed block); it stays registered for the host tail until damar_packed_forget. */
damar_dev_block *damar_block_upload_packed(const HITS_DB *block, const damar_packed *pk, int comp);
void             damar_packed_forget(const HITS_DB *block);
void             damar_block_free(damar_dev_block *blk);

/* The opaque index that Sort_Kmers returns (filter.c:753-994): sorted k-mer codes,
 * base offsets and the code prefix table, all in HBM.  `own_block` != 0 makes
 * damar_index_free release the block too. */
typedef struct damar_dev_index damar_dev_index;
damar_dev_index *damar_index_build(damar_dev_block *blk, int own_block, int *len);
void             damar_index_free(damar_dev_index *idx);
uint64_t         damar_index_bytes(const damar_dev_index *idx);   /* HBM the index holds, for residency caps */
uint64_t         damar_block_bytes(const damar_dev_block *blk);   /* HBM a resident block holds (bases, packed bases, tables) */
void             damar_hbm_info(uint64_t *free_bytes, uint64_t *total_bytes);   /* of the selected GPU (hipMemGetInfo) */
void             damar_pool_trim(void);                            /* release the library's parked index buffers */
/* Test hook: copy the index back as reference-layout KmerPos records
 * {uint64 code; int rpos; int read} (filter.c:121-126), out must hold *len records. */
void             damar_index_download(const damar_dev_index *idx, void *out);
/* Test hook: 1 if the last damar_index_build made its unsorted keys inside the sort (packed, unmasked, unbiased, position
 * words in use, DAMAR_INDEX_GEN not 0), 0 if kmer_tuples wrote them to HBM first. */
int              damar_index_last_made(void);

/* Device part + host tail of Match_Filter (filter.c:2519-2929); records are appended
 * to OVL_IO_Buffer(spec)[0].  counts[0..2] = seed pairs, seed hits (Local_Alignment
 * calls), confirmed records -- the three numbers daligner -v prints. */
void damar_match(const HITS_DB *ablock, const HITS_DB *bblock,
                 damar_dev_index *aidx, damar_dev_index *bidx,
                 int self, int comp, Align_Spec *spec, int64 *counts);

/* Several comparisons behind ONE launch of the report kernel each time (4 per launch unless DAMAR_BATCH says otherwise, at most 16; fewer when their seed
 * pairs would pass a quarter of HBM): the seed stages run one after the other, then every wavefront works through the
 * work lists of all of them, so the wait for the longest alignment at the end of a launch is paid once per launch instead
 * of once per comparison.  Records are appended as if damar_match had been called for jobs[0], jobs[1], ... in order
 * (a daligner plan line, filter.c:2519 called per (B block, orientation) by daligner.c:993-1021, is one such batch);
 * counts as for damar_match. */
typedef struct
{ const HITS_DB *ablock, *bblock;
  damar_dev_index *aidx, *bidx;
  int self, comp;
  Align_Spec *spec;
  int64 counts[3];
} damar_match_job;
void damar_match_batch(damar_match_job *jobs, int njobs);

/* Restrict the following damar_match / Match_Filter calls to the read pairs whose B read (block-local
 * index) lies in [lo, hi); hi < 0 lifts the restriction.  The records of a range are exactly those the
 * unrestricted call writes for these B reads (the merge and the sort still cover the whole pair -- or, of a
 * comparison run in slabs, the slabs that meet the range), so a
 * scheduler can split one block pair over several GPUs and merge the parts' files ("split big
 * pairs ... legal because report work is independent per (bread,aread) run"). */
void damar_set_bread_range(int lo, int hi);

/* Asynchronous host tail: with damar_set_async(1) the per-read-pair tail of damar_match /
 * Match_Filter (redundancy handling, trace compression, buffer append) and the sort + write of
 * damar_write_overlaps run on one worker thread in submission order while the GPU proceeds
 * with the next block pair.  Call damar_async_drain() before releasing the blocks or the
 * Align_Spec, and before reading record counts (counts[2] of damar_match is 0 in this mode;
 * damar_async_totals returns the sum). */
void damar_set_async(int on);
void damar_async_drain(void);
void damar_async_totals(int64 *ncheck, double *tail_ms, double *write_ms);
/* In asynchronous mode the report launch of a damar_match_batch call is also left in flight when the call returns
 * (its own stream; the seed stages of the NEXT call run beside it -- DAMAR_OVERLAP=0 turns that off): counts[1] of the
 * comparisons of that last launch is then 0 at return.  Totals since the last call (drains first): seed hits, and the
 * report kernel's milliseconds and launches. */
void damar_async_counts(int64 *seed_hits, double *report_ms, int64 *launches);
double damar_async_d2h_ms(void);        /* time of the asynchronous record downloads since the last call */
/* What the Local_Alignment waves (align.c:409-1898) of the report launches stepped through since the last call (drains
 * first): band cells = sum over all wave steps of the diagonals computed (the reference's WAVE_STATS unit, align.c:81,
 * 353-368), wave steps counted per alignment pass, and iterations of the kernel's wave loop (each steps one or two passes:
 * half_steps / iterations of 2 means no idle half-wavefront). */
void damar_wave_totals(int64 *cells, int64 *half_steps, int64 *iterations);
/* Write_Overlap_Buffer + Reset_Overlap_Buffer (daligner.c:1020-1021), queued in async mode */
void damar_write_overlaps(Align_Spec *spec, const char *dirName1, const char *dirName2,
                          const char *ablock, const char *bblock, int lastRead);

/* datander (scrub/tandem.h:58-60): the 4-argument parameter call under a library-unique
 * name, and Match_Self with the block already resident in HBM.  counts = k-mers, seed hits,
 * confirmed records. */
int  damar_tandem_set_params(int kmer, int binshift, int hitmin, int nthreads);
void damar_match_self(const HITS_DB *ablock, damar_dev_block *blk, Align_Spec *spec, int64 *counts);
/* scrub/tandem.h:60, scrub/tandem.c:1182 */
void Match_Self(char *aname, HITS_DB *ablock, Align_Spec *settings);

/* Test hook: seed pairs of the last damar_match call as reference-layout SeedPair
 * records {int diag, apos, aread, bread} (filter.c:128-134) in sorted order.
 * Returns the number of seed pairs; copies at most `cap` records. */
int64 damar_last_seeds(void *out, int64 cap);

/* Test hook: the ordering step of the seed sort over the read pair only, on its own.  keys[0 .. nhits) are packed seeds
 * (read pair | A position of ppos bits | dbits low bits), work[0 .. nwork) the ascending indices of run heads: every
 * listed run (the seeds from its head on with the head's read pair) of up to 2048 seeds is put in order of its A positions
 * in place, equal positions in the order they had; everything else is left as it is.  Returns 0. */
int damar_order_runs_test(uint64 *keys, int64 nhits, int ppos, int dbits, const uint32 *work, int nwork);

/* Test hook: the work list of a comparison on its own -- the heads of the (bread, aread) runs report_thread enters that
 * survive the screen of the bucket sums.  keys[0 .. nhits) are seeds packed as ((bread << abits | aread) << ppos | apos) <<
 * dbits | bpos, the stretch [off, off + nhits) of a sorted list of gtotal seeds whose thread slices (1 << nshift of them;
 * nshift < 0: none) are those of the whole list; with dbits == 0 the diagonals are in vals, which is NULL otherwise.
 * minhit = (hitmin - 1) / kmer + 1; only B reads in [b_lo, b_hi) are kept.  mode 0: one pass over sorted seeds; mode 1: one
 * pass over seeds sorted by read pair only (refused with dbits == 0), *flag_out = 1 when a kept run has more than 2048 seeds;
 * mode 2: heads, then screen, scan and compaction.  Writes at most cap ascending seed indices to work_out and returns the
 * number of work items, or -1 for arguments it refuses. */
int64 damar_pair_work_test(const uint64 *keys, const uint32 *vals, int64 nhits, int64 off, int64 gtotal, int ppos, int dbits,
                           int abits, int minhit, int nshift, int binshift, int kmer, int hitmin, uint32 b_lo, uint32 b_hi,
                           int mode, uint32 *work_out, int64 cap, int64 *flag_out);

/* A comparison with more seed pairs than one seed stage holds -- the 32-bit seed index, or what the seed arrays can be
 * grown to in the device memory that is free -- is run in SLABS, consecutive ranges of B reads cut greedily: a slab takes
 * B reads while its seed pairs stay within that figure, and at least one.  Records, counts and damar_last_seeds are those
 * of the comparison in one piece.  damar_last_slabs: the slab table of the last damar_match, b_lo[0 .. n] (b_lo[n] = end
 * of the last slab) and hits[0 .. n-1], at most `cap` slabs copied; returns n, 1 for a comparison that was not split.
 * damar_slab_totals: out[0] = seed stages run (slabs, summed over the comparisons), out[1] = comparisons that were split,
 * in the last damar_match / damar_match_batch.  damar_slab_cut is the cut itself (host arithmetic, no device): returns
 * the number of slabs, -(r + 1) when B read r alone exceeds cap, 0 when max_slabs is too small.
 * With damar_set_bread_range the slabs outside the range are not run; their seed pairs still count in counts[0] and in
 * counter 0, which stay the whole comparison's as they are without slabs.  A comparison cut by the memory figure runs
 * its slabs one at a time (each slab's report launch is completed before the next slab's seed stage).
 * Test hooks, not options: DAMAR_TEST_SEED_CAP=<n> in the environment replaces the figure by n;
 * DAMAR_TEST_FREE_BYTES=<n> stands for the free device memory the figure is derived from. */
int  damar_last_slabs(int *b_lo /* [cap + 1] */, int64 *hits /* [cap] */, int cap);
void damar_slab_totals(int64 *out /* [2] */);
int  damar_slab_cut(const uint64_t *hits, int nreads, uint64_t cap, int *b_lo /* [max_slabs + 1] */, int64 *sums /* [max_slabs] */,
                    int max_slabs);

/* The cap on mutual k-mer matches per code that the last damar_match applied (filter.c:2634-2702:
 * 10000 unless the host memory limit forces it lower; INT32_MAX when MEM_LIMIT is 0). */
int damar_last_limit(void);

/* For the tests: the tiles of the A index that the merge's last COUNT sweep left to its general kernel (all of them
 * under DAMAR_MERGE_GENERAL; otherwise those whose B piece exceeds the stage or in which a cap might apply).  Looked at
 * only while damar_last_seeds keeps the seed list; -1 otherwise. */
int damar_last_merge_flagged(void);

/* -b: the reference derives its log base weights from the first block a PROCESS sorts and keeps
 * them (filter.c:774-789).  A caller that runs several jobs in one process calls this between
 * them to get what separate daligner processes would compute. */
void damar_bias_reset(void);

/* Test hook: batch Local_Alignment (align.c:1904 with low == hgh == diag, no borders)
 * on the GPU.  tasks[4*i..] = aread, bread, diag, anti (block-local read ids).
 * paths[12*i..] = A-view abpos,bbpos,aepos,bepos,diffs,tlen then the same for the
 * B-view; traces of task i start at trace_off[2*i] (A) and trace_off[2*i+1] (B) in
 * `traces` (capacity trace_cap values).  Returns 0, or -1 if trace_cap is too small. */
int damar_local_alignment_batch(damar_dev_block *ablk, damar_dev_block *bblk, int comp,
                                Align_Spec *spec, const int *tasks, int ntasks,
                                int *paths, int64 *trace_off, uint16 *traces, int64 trace_cap);
/* The same with the launch's switches: t8 != 0 and a trace spacing <= 125 make the device write its trace values as bytes
 * (what the pipeline's launches do by default); they arrive widened to 16 bits in `traces`.  A value that does not fit a
 * byte repeats the launch with 16-bit values and sets *t8_fell_back.  *wide_tasks = the tasks answered by the wide kernel
 * (reads of more than 16 000 trace spacings, alignments that overflowed the packed pebble pool): DAMAR_CNT_WIDE of the LAST
 * attempt's launch, set only where the wide kernel ran behind it, 0 otherwise.  Both may be NULL. */
int damar_local_alignment_batch_opts(damar_dev_block *ablk, damar_dev_block *bblk, int comp,
                                     Align_Spec *spec, const int *tasks, int ntasks,
                                     int *paths, int64 *trace_off, uint16 *traces, int64 trace_cap,
                                     int t8, int *t8_fell_back, int *wide_tasks);

/* SURVEY 8(f)4, the next consumer of the records: Compute_Trace_PTS (align.c:5577-5692 + iter_np
 * :4892-5261) for every record of an Overlap array, the way utils/LAshow.c:245-262 calls it per record.
 * ablk / bblk hold the A and B reads (B forward: the complement of COMP records is read in place);
 * ovls[i].aread / bread are DB read ids, afirst / bfirst the ids of the blocks' first reads;
 * ovls[i].path.trace = the trace points as stored in the .las, tbytes (1 or 2) bytes per value.
 * same != 0 applies the one-buffer rule of align.c:4933-4951 (LAshow never does).
 * On success returns 0: *script = malloc'ed array of all edit scripts, record i at
 * [soff[i], soff[i+1]) (soff has novl + 1 entries), diffs[i] = its summed segment distances.
 * Returns 1 after the reference's message where the reference exits (trace point out of bounds,
 * bad alignment between trace points). */
int  damar_trace_pts(damar_dev_block *ablk, int afirst, damar_dev_block *bblk, int bfirst,
                     const Overlap *ovls, int64 novl, int tbytes, int tspace, int mode, int same,
                     int64 *soff, int *diffs, int **script);
/* The same for Compute_Trace_MID (align.c:5694-5830 + middle_np :5263-5573, corrector/LAcorrect.c:545) */
int  damar_trace_mid(damar_dev_block *ablk, int afirst, damar_dev_block *bblk, int bfirst,
                     const Overlap *ovls, int64 novl, int tbytes, int tspace, int mode, int same,
                     int64 *soff, int *diffs, int **script);
/* ms[4]: trace_waves kernel, all kernels of the call (HIP events), whole call, inside the batches (wall);
 * cnt[4]: records, segments, segments deferred to the large-stripe launch, script values */
void damar_trace_last(double *ms, int64 *cnt);
void damar_trace_release(void);          /* frees the cached device buffers of damar_trace_pts */

/* Mask tracks from piles of overlaps (scrub/LArepeat.c, scrub/TANmask.c).  A batch is a run of whole piles -- all records
 * of one A read, in file order -- as structure of arrays: pile i is the records [pile_off[i], pile_off[i+1]) and belongs to
 * read pile_aread[i]; read_len / read_flags are the database's (all nreads reads, indexed by the records' read numbers).
 * The three calls take host arrays, own the transfers and run kernels/pile_sweep.hip; with DAMAR_PILES=host in the
 * environment they run the plain sweep of host/piles.c instead (no GPU is touched).  0 on success. */
typedef struct
{ int64        npiles, nrec;
  const int64 *pile_off;                   /* [npiles + 1] */
  const int   *pile_aread;                 /* [npiles] */
  const int   *abpos, *aepos, *bbpos, *bepos, *bread, *flags;     /* [nrec] */
  const int   *read_len, *read_flags;      /* [nreads] */
  int          nreads, maxlen;             /* maxlen: the longest read (sizes the position bits of the event key) */
} damar_pile_batch;

typedef struct
{ double xcov_enter, xcov_leave;           /* -h -l */
  int    cov;                              /* -c, or the estimate */
  int    merge_dist;                       /* -m (-1: none) */
  int    min_aln_len;                      /* -o */
  int    inc_identity;                     /* -I */
  int    inccov;                           /* -C */
  int    max_cov;                          /* -M: length of the coverage histogram */
} damar_repeat_params;

typedef struct
{ int   *count;                            /* [npiles], the caller's: ints of data that pile i produced */
  int   *data;                             /* malloc'ed by the call, the caller's to free: the piles' ints back to back */
  int64  ndata;
  int64  merged, repeat_bases;             /* LArepeat's MERGED and BASES_REPEAT of the batch */
} damar_pile_track;

/* LArepeat.c:168-233: histo[max_cov], *bases and *inactive are ADDED to */
int  damar_pile_coverage(const damar_pile_batch *b, const damar_repeat_params *p, int64 *histo, int64 *bases, int64 *inactive);
/* LArepeat.c:282-494: per pile {begin, end[, coverage]}...; a region still open at the pile's last event is its begin alone */
int  damar_pile_repeats(const damar_pile_batch *b, const damar_repeat_params *p, damar_pile_track *out);
/* TANmask.c:115-207 with an honest threshold: records with abpos - bepos <= 20 and aepos - bbpos > min_len */
int  damar_pile_tandem(const damar_pile_batch *b, int min_len, damar_pile_track *out);
void damar_pile_release(void);             /* frees the cached device buffers of the three calls */
/* of the last call: ms[4] = upload, sort, sweep, download; cnt[2] = events sorted, regions (tandem: intervals) written */
void damar_pile_last(double *ms, int64 *cnt);

/* Per-segment quality from the traces of piles (scrub/LAq.c handler_annotate).  A trace batch is a pile batch whose records
 * also carry their trace as it lies in the .las file: record i's tlen[i] values (diffs of a segment at even, its B length
 * at odd positions; tbytes bytes each, 1 for tspace <= 125, else 2) begin at trace + trace_off[i].  The tiles (segments of
 * tspace bases) of the batch's piles are numbered back to back, ceil(alen / tspace) per pile; q_out receives one value per
 * tile and *ntiles_out their number (q_out == NULL: only the number).  Runs kernels/pile_quality.hip; with DAMAR_PILES=host
 * the plain histogram of host/quality.c instead (no GPU is touched).  Segments and tiles of a batch stay below 2^31 each.
 * 0 on success. */
typedef struct
{ damar_pile_batch     p;
  const unsigned char *trace;              /* [trace_bytes] */
  const int64         *trace_off;          /* [nrec] */
  const int           *tlen;               /* [nrec] */
  int64                trace_bytes;
  int                  tbytes, tspace;
} damar_trace_batch;

typedef struct
{ int segmin, segmax;                      /* -s -S: a tile's value is the mean of its segmax lowest, 0 below segmin of them */
  int ccs;                                 /* -c: 25 instead of 0 below segmin */
} damar_q_params;

int  damar_pile_quality(const damar_trace_batch *b, const damar_q_params *p, int *q_out, int64 *ntiles_out);
void damar_q_release(void);                /* frees the cached device buffers of damar_pile_quality */
/* of the last device call: ms[4] = upload, count + scan, scatter + select, download; cnt[2] = segments counted, tiles */
void damar_q_last(double *ms, int64 *cnt);

/* Exact alignment of a batch of boxes (Compute_Alignment(DIFF_ALIGN), align.c:4734 through dandc_nd and split_nd): box i is
 * A = bases + aoff[i], m[i] >= 1 bases, against B = bases + boff[i], n[i] >= 1 bases, one base per byte, B already
 * complemented where that is wanted.  diffs[i] receives the box's differences; its edit script -- the indels of the
 * reference's optimal path in path order, -(a + 1) for a base of B alone in front of A position a, b + 1 for a base of A
 * alone in front of B position b, positions counted from the box's own corner -- is the values [soff[i], soff[i + 1]) of
 * *script (soff holds nbox + 1 entries; *script is malloc'ed, the caller's to free).  Runs kernels/box_align.hip, one
 * wavefront per box; a box with max(m, n) above what the kernel keeps in LDS goes to the host routine of host/bridge.c
 * (DAMAR_TEST_BOX_LIMIT lowers that bound, for tests).  With DAMAR_TRIM=host the host routine does all boxes and no GPU is
 * touched.  0 on success. */
typedef struct
{ int64        nbox;
  const int   *m, *n;                      /* [nbox] */
  const int64 *aoff, *boff;                /* [nbox] */
  const char  *bases;                      /* [nbases] */
  int64        nbases;
} damar_box_batch;

int  damar_align_boxes(const damar_box_batch *b, int *diffs, int64 *soff, int **script);
void damar_box_release(void);              /* frees the cached device buffers of damar_align_boxes */
/* of the last call: ms[4] = upload, kernel, download (HIP events; 0 on the host path), whole call (wall);
 * cnt[3] = boxes, boxes the host routine did beside the kernel, script values */
void damar_box_last(double *ms, int64 *cnt);
unsigned int damar_box_grid(void);         /* workgroups of the kernel's largest launch: a batch of more boxes gives a workgroup several */

/* The same alignment for boxes of read length -- a read against its correction, what LAcorrect writes behind " postrace=":
 * the batch, diffs, soff and *script are those of damar_align_boxes.  Runs kernels/read_align.hip, one workgroup of eight
 * wavefronts per box, the boxes dealt longest first; what bounds a box there is its differences, not its length: a box of
 * more than DAMAR_READ_MAXDIFF (8000) differences, or with max(m, n) above DAMAR_READ_MAXLEN (2^20), goes to the host
 * routine of host/bridge.c (DAMAR_TEST_READ_DIFFS lowers the first bound and DAMAR_TEST_READ_GRID the workgroups of a
 * launch, for tests).  With DAMAR_POSTRACE=host the host routine does all boxes and no GPU is touched.  0 on success. */
int  damar_align_reads(const damar_box_batch *b, int *diffs, int64 *soff, int **script);
void damar_read_release(void);             /* frees the cached device buffers of damar_align_reads */
/* of the last call: ms[4] = upload, kernel, download (HIP events; 0 on the host path), whole call (wall);
 * cnt[3] = boxes, boxes the host routine did beside the kernel, script values */
void damar_read_last(double *ms, int64 *cnt);
unsigned int damar_read_grid(void);        /* workgroups of the kernel's largest launch: a batch of more boxes gives a workgroup several */
int  damar_postrace_on_host(void);         /* DAMAR_POSTRACE=host */

/* Exact alignment of a batch of boxes into trace pairs (Compute_Alignment(DIFF_TRACE), align.c:4734 through trace_nd and
 * split_nd): box i is A = bases + aoff[i], m[i] >= 1 bases, against B = bases + boff[i], n[i] >= 1 bases, one base per
 * byte, B already complemented where that is wanted.  abpos[i] >= 0 is where the box begins in A (or that position modulo
 * tspace): the pairs are cut on A's own grid of tspace.  diffs[i] receives the box's differences; its pairs -- the
 * differences and the B length of every interval of the grid that the box touches, what the reference leaves in
 * path->trace, the cell beyond the last boundary folded into the one before it -- are the values [toff[i], toff[i + 1])
 * of *trace, 2 * ((abpos + m + tspace - 1) / tspace - abpos / tspace) of them (toff holds nbox + 1 entries; *trace is
 * malloc'ed, the caller's to free).  Runs kernels/box_trace.hip, one wavefront per box; a box with max(m, n) above 4096,
 * or with more than 255 intervals, goes to the host routine of host/bridge.c (DAMAR_TEST_BOX_LIMIT lowers the first bound,
 * for tests).  With DAMAR_STITCH=host the host routine does all boxes and no GPU is touched.  0 on success. */
typedef struct
{ int64        nbox;
  const int   *m, *n, *abpos;              /* [nbox] */
  const int64 *aoff, *boff;                /* [nbox] */
  const char  *bases;                      /* [nbases] */
  int64        nbases;
  int          tspace;
} damar_tbox_batch;

int  damar_trace_boxes(const damar_tbox_batch *b, int *diffs, int64 *toff, uint16 **trace);
void damar_tbox_release(void);             /* frees the cached device buffers of damar_trace_boxes */
/* of the last call: ms[4] = upload, kernel, download (HIP events; 0 on the host path), whole call (wall);
 * cnt[3] = boxes, boxes the host routine did beside the kernel, trace values */
void damar_tbox_last(double *ms, int64 *cnt);
unsigned int damar_tbox_grid(void);        /* workgroups of the kernel's largest launch: a batch of more boxes gives a workgroup several */

/* Repeat intervals carried across overlaps (scrub/TKhomogenize.c): for every record of a trace batch that is not an identity
 * overlap, the A read's intervals of at least 500 bases that the record covers are projected through its trace points onto
 * the B read and set in a bit mask of the whole database, one bit per `res` bases and one spare bit per read.  The mask is
 * indexed by the B read, so it outlives the batch: a session.
 *   open    the mask of all nreads reads, all zero, resident in HBM (totlen / 8 bytes at res 1); NULL after a message when
 *           it cannot be had -- there is no fallback;
 *   seed    -m: every interval of the track of at least 500 bases set in its own read;
 *   add     one trace batch (its read_len / nreads are the session's) against the interval track: anno[nreads + 1] byte
 *           offsets into data[ndata], a read's intervals as {begin, end} pairs in the order the reference walks them.
 *           ends = -1, or -e's n with trim[2 * nreads] = {begin, end} per read (0, 0 for a read the trim track leaves out);
 *   finish  the mask read out as a track: anno[nreads + 1] (the caller's) receives byte offsets, *data (malloc'ed, the
 *           caller's to free) the {begin, end} pairs, *tagged the sum of end - begin.  The mask stays as it is.
 * Runs kernels/homogenize.hip; with DAMAR_PILES=host the bit array of host/homogenize.c instead (no GPU is touched).
 * 0 on success, 1 after a message. */
typedef struct damar_homog damar_homog;
damar_homog *damar_homog_open(const int *read_len, int nreads, int res);
int  damar_homog_seed(damar_homog *h, const uint64 *anno, const int *data, int64 ndata);
int  damar_homog_add(damar_homog *h, const damar_trace_batch *b, const uint64 *anno, const int *data, int64 ndata, int ends,
                     const int *trim);
int  damar_homog_finish(damar_homog *h, uint64 *anno, int **data, int64 *ndata, int64 *tagged);
void damar_homog_close(damar_homog *h);
/* of the last session, summed over its calls so far: ms[4] = upload, mark (seed and add), read-out, download (HIP events; 0
 * on the host path); cnt[3] = records seen by add, ranges set in the mask (seed and add), intervals read out */
void damar_homog_last(double *ms, int64 *cnt);

/* Containments, gaps and breaks of piles (scrub/LAgap.c drop_containments and handle_gaps_and_breaks): per pile, inside every
 * run of one B read the contained record of a pair is discarded (OVL_DISCARD | OVL_CONT) and the shorter of two records that
 * intersect on A marked OVL_TEMP; the remaining records are counted over bins of 100 bases, and every run of bins covered at
 * most once is a break: left alone when an interval of the exclude track strictly contains it or (stitch > 0) a pair of
 * records of one B read bridges it within `stitch` bases, else the records on the far side of the pile's longest record are
 * discarded (OVL_DISCARD | OVL_GAP).  A run still open at the pile's last bin is always dropped.  flags_out[nrec] receives
 * every record's flags word, OVL_TEMP included.  ev->count[npiles] (the caller's) receives the events per pile, ev->ev
 * (malloc'ed, the caller's to free) DAMAR_GAP_EVENT_INTS ints per event, the piles' back to back in the order the reference
 * meets them: {first bin, bin after the run, kind, v0, v1, records dropped}; kind is one of DAMAR_GAP_MASKED (v0, v1: the
 * interval), _STITCHABLE (v0: pairs), _DROP_L, _DROP_R, _DROP_NONE (no record left to decide the side), with
 * DAMAR_GAP_TRAILING or'ed in for the open run.  Runs kernels/pile_gaps.hip, one wavefront per pile; a pile on a read of more
 * than DAMAR_GAP_MAXBINS bins (DAMAR_TEST_GAP_BINS lowers that, for tests), one with more than DAMAR_GAP_MAXEVENTS events,
 * and one whose B reads do not ascend is done by the routine of host/gap.c.  DAMAR_TEST_GAP_GRID lowers the number of
 * workgroups, for tests: each then takes several piles, as in a batch of more piles than the largest launch has workgroups.
 * With DAMAR_PILES=host that routine does all piles and no GPU is touched.  0 on success, 1 after a message. */
#define DAMAR_GAP_MAXBINS    4096          /* bins of 100 bases the kernel keeps in LDS: reads up to 409 500 bases */
#define DAMAR_GAP_MAXEVENTS  16            /* events of a pile the kernel has room for */
#define DAMAR_GAP_EVENT_INTS 6
enum { DAMAR_GAP_MASKED = 0, DAMAR_GAP_STITCHABLE, DAMAR_GAP_DROP_L, DAMAR_GAP_DROP_R, DAMAR_GAP_DROP_NONE, DAMAR_GAP_TRAILING = 0x100 };
typedef struct
{ int           stitch;                    /* -s */
  const uint64 *ex_anno;                   /* -e: [nreads + 1] byte offsets into ex_data, {begin, end} pairs; NULL: none */
  const int    *ex_data;
  int64         ex_ndata;
  int           purge;                     /* -p, -t: looked at by damar_gap_las (host/gap.c) alone; NULL: no trimming */
  const char   *trim_track;
} damar_gap_params;
typedef struct
{ int   *count;                            /* [npiles], the caller's */
  int   *ev;                               /* malloc'ed by the call */
  int64  nev;
  int64  contained, breaks, dropped;       /* the reference's three counters, of the batch */
} damar_gap_events;
int  damar_pile_gaps(const damar_pile_batch *b, const damar_gap_params *p, int *flags_out, damar_gap_events *ev);
void damar_gap_release(void);              /* frees the cached device buffers of damar_pile_gaps */
void damar_gap_limits(int *bins, int *events);     /* DAMAR_GAP_MAXBINS, DAMAR_GAP_MAXEVENTS as the library was built */
/* of the last call: ms[4] = upload, kernel, download (HIP events; 0 on the host path), whole call (wall);
 * cnt[3] = piles, piles the host routine did beside the kernel, break events */
void damar_gap_last(double *ms, int64 *cnt);

/* The overlaps of every (A read, B read) chained and judged (scrub/LAseparate.c chain() and separate_handler).  A group is
 * the run of one B read inside a pile.  Per group of two or more records: the records contained in an earlier one on both
 * reads marked OVL_CONT, then chains grown greedily from the record with the most non-repeat bases until no record is left,
 * the chains ordered by length; the best chain decides by `kind` (-T) whether the group is proper.  kind 0: a proper group
 * is discarded whole, another kept whole (OVL_DISCARD taken off).  kind 1: a group of exactly one, proper chain keeps what
 * the chaining left, every other group is discarded whole.  A group of one record is judged by that record.  out->flags
 * receives every record's flags word as the first pass of the reference leaves it, OVL_TEMP included; at the first record
 * of a group out->nchains, out->proper and out->nbest receive the number of chains, the verdict and the length of the best
 * chain (-1 at the group's other records), and out->best from there on the best chain's members in chain order as indices
 * into the group (a chain longer than its group -- a gap filler of under 100 bases taken twice -- is cut to the group's
 * length there), -1 behind them.  Runs kernels/pile_chains.hip: a lane per record for the repeat counts and the groups of
 * one, then one wavefront per pile with a lane per group.  A group of more than DAMAR_SEPARATE_MAXGROUP records or with
 * more than DAMAR_SEPARATE_MAXCHAINS chains is done by the routine of host/separate.c (DAMAR_TEST_SEPARATE_GROUP and
 * DAMAR_TEST_SEPARATE_CHAINS lower the two, for tests), with DAMAR_PILES=host all are.  A group of two or more records
 * that all come with OVL_CONT or OVL_DISCARD is refused with a message (the reference aborts on it).  0 on success. */
#define DAMAR_SEPARATE_MAXGROUP  64        /* records of a group: its working flags are three 64-bit masks */
#define DAMAR_SEPARATE_MAXCHAINS 16        /* chains of a group the kernel keeps the ends of */
typedef struct
{ const uint64 *rep_anno;                  /* -r: [nreads + 1] byte offsets into rep_data, {begin, end} pairs; NULL: none */
  const int    *rep_data;
  int64         rep_ndata;
  int           kind;                      /* -T: 0 for the repeat-aware overlapper, 1 for the forced alignment */
  int           twidth;                    /* the file's trace spacing */
  int           rep_checked;               /* the caller has had this track through a call already: its shape is not looked at again */
} damar_separate_params;
typedef struct
{ int *flags, *nchains, *proper, *nbest, *best;      /* [nrec] each, the caller's */
} damar_chain_out;
int  damar_pile_chains(const damar_pile_batch *b, const damar_separate_params *p, damar_chain_out *out);
void damar_separate_release(void);         /* frees the cached device buffers of damar_pile_chains */
void damar_separate_limits(int *group, int *chains);     /* DAMAR_SEPARATE_MAXGROUP, DAMAR_SEPARATE_MAXCHAINS as the library was built */
/* of the last call: ms[4] = upload, kernels, download (HIP events; 0 on the host path), whole call (wall);
 * cnt[3] = groups, groups the host routine did beside the kernel, groups of more than one record */
void damar_separate_last(double *ms, int64 *cnt);

/* Repairs of piles (scrub/LAfix.c fix_process without its chimer code): per pile of a trace batch, whose A read is kept
 * from trim[2 * pile] to trim[2 * pile + 1] (the trim track's interval after the flip step of host/fix.c; begin >= end: the
 * pile has no repairs),
 *   breaks   two consecutive records of one B read in one orientation that leave a gap on A are a candidate: the A interval
 *            on segment borders, the B stretch between the last and the first trace interval.  Candidates with a zero in B's
 *            q, with more than `maxspanners` records across both borders, with more than one scored segment strictly inside
 *            or with a B stretch over ten times the A interval are dropped; the rest sorted (stably) by A interval and
 *            quality, cut at `maxgap`, merged where they agree or intersect, and kept from `minsupport` on when A has a
 *            bad segment (q = 0 or q >= lowq) inside;
 *   weak     every bad segment inside the trim that no kept break contains is replaced by the B stretch, found through the
 *            trace, of the record across it (a spacing to spare on either side) with the lowest mean q, the first such
 *            record among equals; support counts the records that begin or end inside the segment.
 * out->count[npiles] (the caller's) receives the repairs per pile, out->gaps (malloc'ed, the caller's to free) the piles'
 * repairs back to back in the order they are spliced in (by A interval, then quality).  B's q is indexed flat into the q
 * track's data, as the reference does it; an index outside the data counts as q = 0.  Runs kernels/pile_patch.hip, one
 * wavefront per pile; a pile on a read of more than DAMAR_FIX_MAXSEGS segments (DAMAR_TEST_FIX_SEGS lowers that, for
 * tests), one with more than DAMAR_FIX_MAXCAND candidates or DAMAR_FIX_MAXREP repairs, and one whose B reads do not ascend is
 * done by the routine of host/fix.c.  With DAMAR_PILES=host that routine does all piles and no GPU is touched.
 * 0 on success, 1 after a message. */
#define DAMAR_FIX_MAXSEGS 4096             /* segments of the A read the kernel keeps in LDS */
#define DAMAR_FIX_MAXCAND 256              /* break candidates of a pile the kernel sorts and merges */
#define DAMAR_FIX_MAXREP  1024             /* repairs (kept breaks plus weak segments) of a pile the kernel has room for */
typedef struct
{ const uint64 *q_anno;                    /* -q: [nreads + 1] byte offsets into q_data, one value per segment */
  const int    *q_data;
  int64         q_ndata;
  const uint64 *rep_anno;                  /* -r: {begin, end} pairs; NULL: none */
  const int    *rep_data;
  int64         rep_ndata;
  int           lowq, maxgap;              /* -Q -g (-1: no cut) */
  int           maxspanners, minsupport;   /* 7 and 4, or -l's 3 and 2 */
  int           twidth;                    /* the trace spacing of the batch */
} damar_fix_params;
typedef struct { int ab, ae, bb, be, diff, b, support, comp; } damar_fix_gap;     /* comp: the record's OVL_COMP bit */
typedef struct
{ int           *count;                    /* [npiles], the caller's */
  damar_fix_gap *gaps;                     /* malloc'ed by the call */
  int64          ngaps;
} damar_fix_gaps;
int  damar_pile_patches(const damar_trace_batch *b, const damar_fix_params *p, const int *trim, damar_fix_gaps *out);
void damar_fix_release(void);              /* frees the cached device buffers of damar_pile_patches */
void damar_fix_limits(int *segs, int *cands);      /* DAMAR_FIX_MAXSEGS, DAMAR_FIX_MAXCAND as the library was built */
/* of the last call: ms[4] = upload, kernel, download (HIP events; 0 on the host path), whole call (wall);
 * cnt[3] = piles, piles the host routine did beside the kernel, repairs */
void damar_fix_last(double *ms, int64 *cnt);

/* Overlaps filtered per pile (scrub/LAfilter.c filter_handler without its experimental branches).  Per pile of a trace
 * batch, in the reference's order; `steps` says which half of it runs, since LAfilter's -T cuts the records between the two:
 *   DAMAR_FILTER_PRE    -f (reads above downsample * nreads / 100.0 discarded) and -b (OVL_DISCARD | OVL_DIFF on the first
 *                       trace segment but the last whose diffs * 100.0 / blen exceeds seg_rate), on the trace as it is;
 *   DAMAR_FILTER_MAIN   -s / -S per run of consecutive records of one B read (the head chained to the longest later record
 *                       of its orientation within the fuzz; its end and diffs updated, its trace dropped, OVL_DISCARD and
 *                       OVL_LOCAL taken off it, the joined record OVL_DISCARD | OVL_STITCH); filter() per record (-A -l -o
 *                       -u -d -n with -Y, and under -R 2 the trace points summed against bepos); -w per run; -z per pile;
 *                       -R 0 .. 6; the -x / -I read states.
 * `diffs` is the records' differences word.  Every array of `out` is the caller's and holds one value per record (cnt: per
 * pile); the records' abpos and bbpos do not change.  reason has one bit per site that prints a line in the reference
 * (DAMAR_FR_*), set whether or not the flag it stands for was set before; cont_by is the index within the pile of the record
 * that -R 6 found a record contained in, or -1.  Runs kernels/pile_filter.hip, one wavefront per pile; a pile with a run of
 * more than DAMAR_FILTER_MAXGROUP records of one B read, and under -z with -u a pile on a read of more than
 * DAMAR_FILTER_MAXLEN bases, is done by the routine of host/filter.c (DAMAR_TEST_FILTER_GROUP and DAMAR_TEST_FILTER_LEN lower
 * the two, for tests).  DAMAR_TEST_FILTER_GRID lowers the number of workgroups, for tests: each then takes several piles, as
 * in a batch of more piles than the largest launch has workgroups.  With DAMAR_PILES=host that routine does all piles and no
 * GPU is touched.  0, or 1 after a message. */
#define DAMAR_FILTER_MAXGROUP 64           /* records of one B read in a row that one lane takes */
#define DAMAR_FILTER_MAXLEN   400000       /* bases of the A read whose coverage bits the kernel keeps in LDS */
enum { DAMAR_FILTER_PRE = 1, DAMAR_FILTER_MAIN = 2 };
enum { DAMAR_FR_SYM = 0x1, DAMAR_FR_OLEN = 0x2, DAMAR_FR_LOCAL = 0x4, DAMAR_FR_DIFF = 0x8, DAMAR_FR_REPA_TIPS = 0x10,
       DAMAR_FR_REPA_LEN = 0x20, DAMAR_FR_REPA = 0x40, DAMAR_FR_REPB_LEN = 0x80, DAMAR_FR_REPB = 0x100, DAMAR_FR_TP = 0x200,
       DAMAR_FR_MULTI = 0x400, DAMAR_FR_SELF = 0x800, DAMAR_FR_CONT = 0x1000,
       DAMAR_FR_HEAD = 0x2000 };             /* no line: the record is the head of a stitch, its trace is gone */
enum { DAMAR_FC_DIFFS = 0, DAMAR_FC_UNALIGNED, DAMAR_FC_CONTAINED, DAMAR_FC_LENGTH, DAMAR_FC_REPEAT, DAMAR_FC_READLEN,
       DAMAR_FC_LOWCOV, DAMAR_FC_SYM, DAMAR_FC_MULTI, DAMAR_FC_MULTI_BASES, DAMAR_FC_STITCHED, DAMAR_FC_COUNT };
typedef struct
{ int           steps;                     /* DAMAR_FILTER_PRE | DAMAR_FILTER_MAIN */
  int           downsample, seg_rate;      /* -f (0: none) -b (outside 0 .. 100: none) */
  int           stitch, stitch_aggr;       /* -s / -S (-1: none), -S */
  int           min_rlen, min_olen, max_unaligned, min_nonrep;      /* -l -o -u -n (-1: none) */
  float         max_diffs;                 /* -d / 100 (<= 0: none) */
  int           merge_tips, multi, lowcov; /* -Y -w -z */
  int           remove;                    /* -R: bit k for -R k */
  int           include;                   /* -I given */
  const int    *trim;                      /* -t: get_trim of every read, [2 * nreads]; NULL: no trim track */
  const uint64 *rep_anno;                  /* -r: [nreads + 1] byte offsets into rep_data, {begin, end} pairs; needed with -n */
  const int    *rep_data;
  int64         rep_ndata;
  const int    *sym_off, *sym_len;         /* -A: read r's list is sym_data[sym_off[r] .. + sym_len[r]) ([nreads + 1] each); NULL: none */
  const int    *sym_data;
  int64         sym_ndata;
  const unsigned char *read_state;         /* -x / -I: 1 discard, 2 keep, per read; NULL: none */
} damar_filter_params;
typedef struct
{ int   *flags, *aepos, *bepos, *diffs, *tlen, *reason, *cont_by;      /* [nrec] */
  int   *cnt;                              /* [npiles * DAMAR_FC_COUNT] */
} damar_filter_out;
int  damar_pile_filter(const damar_trace_batch *b, const int *diffs, const damar_filter_params *p, damar_filter_out *out);
void damar_filter_release(void);           /* frees the cached device buffers of damar_pile_filter */
void damar_filter_limits(int *group, int *len);    /* DAMAR_FILTER_MAXGROUP, DAMAR_FILTER_MAXLEN as the library was built */
/* of the last call: ms[4] = upload, kernel, download (HIP events; 0 on the host path), whole call (wall);
 * cnt[3] = piles, piles the host routine did beside the kernel, records that leave the call discarded */
void damar_filter_last(double *ms, int64 *cnt);

/* Consensus of tiles (corrector/consensus.c as corrector/LAcorrect.c drives it): tile t of a batch is the sequences
 * [ent_off[t], ent_off[t + 1]) -- MAX_COVERAGE = 20 at the most, none: an empty tile -- sequence e the seq_len[e] >= 1 bases
 * from bases + seq_off[e], one base per byte (0 .. 3), a complemented read's already turned.  The first sequence founds a
 * profile of five counts per column; every later one is aligned to it by v3_align_onp (the O(NP) waves, all kept; the
 * path reversed with the reference's fix-ups) and folded in from right to left; the tile's call is
 * consensus_sequence(c, 0).  cons_off[ntiles + 1] (the caller's) receives where each tile's called bases (0 .. 3) lie in
 * *cons (malloc'ed, the caller's to free), added[ntiles] the sequences each tile took.  weight[ntiles], if given, orders
 * the tiles so that the lanes of a wavefront have about the same work (LAcorrect: the sum of the segments' differences).
 * Runs kernels/tile_consensus.hip, one lane per tile; a tile with a sequence over DAMAR_CORRECT_MAXSEG bases, one whose
 * profile outgrows DAMAR_CORRECT_MAXCOLS columns (DAMAR_TEST_CORRECT_COLS lowers that, for tests) and one whose waves
 * outgrow DAMAR_CORRECT_CELLS cells is done by the routine of host/correct.c and counted.  With DAMAR_PILES=host that
 * routine does all tiles and no GPU is touched.  0 on success, 1 after a message. */
#define DAMAR_CORRECT_MAXCOV  20           /* sequences of a tile: MAX_COVERAGE, LAcorrect.c:35 */
#define DAMAR_CORRECT_MAXSEG  320          /* bases of one sequence the kernel takes */
#define DAMAR_CORRECT_MAXCOLS 384          /* profile columns a lane has room for */
#define DAMAR_CORRECT_CELLS   8192         /* wave cells (an int16 and an int8 each) a lane has room for */
typedef struct
{ int64        ntiles;
  const int64 *ent_off;                    /* [ntiles + 1] */
  const int64 *seq_off;                    /* [ent_off[ntiles]] */
  const int   *seq_len;
  const unsigned char *bases;              /* [nbases] */
  int64        nbases;
  const int   *weight;                     /* [ntiles], or NULL: sequences times bases */
} damar_tile_batch;
int  damar_tile_consensus(const damar_tile_batch *b, int64 *cons_off, unsigned char **cons, int *added);
void damar_correct_release(void);          /* frees the cached device buffers of damar_tile_consensus */
void damar_correct_limits(int *seg, int *cols, int *cells);      /* the three limits as the library was built */
/* of the last call: ms[4] = upload, kernel, download (HIP events; 0 on the host path), whole call (wall);
 * cnt[3] = tiles, tiles the host routine did beside the kernel, bases called */
void damar_correct_last(double *ms, int64 *cnt);

/* The low-complexity mask of reads (db/DBdust.c, Myers' incremental SDUST): read i is the bases (one per byte, 0 .. 3)
 * from bases + read_off[i] to bases + read_off[i + 1].  out_off[nreads + 1] (the caller's) receives where each read's
 * [beg, end) pairs lie in *out, counted in ints; *out is malloc'ed and the caller's to free.  window, thresh and minlen are
 * the command's -w, -t and -m (minlen >= 2, as there); biased its -b, with the database's four base frequencies.
 * Runs kernels/dust.hip: a read is cut into pieces of DAMAR_DUST_PIECE triplet starts, one wavefront a piece, each with
 * DAMAR_DUST_HALO triplets in front of it and `window` behind, which makes the pieces' results those of the whole read
 * (DESIGN.md section 9l); a second kernel joins a read's intervals and applies minlen.  The routine of host/dust.c does
 * -- and damar_dust_last counts -- every read with biased set or a window outside 3 .. DAMAR_DUST_MAXWINDOW, and a read
 * one of whose pieces retires more than DAMAR_DUST_STRIPE candidates.  A start retires at most once, so with a stripe of
 * DAMAR_DUST_PIECE pairs no read does; DAMAR_TEST_DUST_STRIPE lowers the stripe, for tests of that way out.
 * With DAMAR_DUST=host that routine does all reads and no GPU is touched.  0 on success, 1 after a message. */
#define DAMAR_DUST_MAXWINDOW 64
#define DAMAR_DUST_PIECE     1024
#define DAMAR_DUST_HALO      (2 * DAMAR_DUST_MAXWINDOW)
#define DAMAR_DUST_STRIPE    DAMAR_DUST_PIECE
typedef struct
{ int    window;                           /* -w (64) */
  double thresh;                           /* -t (2.) */
  int    minlen;                           /* -m (10) */
  int    biased;                           /* -b */
  float  freq[4];                          /* with biased: HITS_DB.freq */
} damar_dust_params;
int  damar_dust_reads(const unsigned char *bases, const int64 *read_off, int64 nreads, const damar_dust_params *p,
                      int64 *out_off, int **out);
void damar_dust_release(void);             /* frees the cached device buffers of damar_dust_reads */
void damar_dust_limits(int *piece, int *halo, int *stripe, int *window);       /* the four limits as the library was built */
/* of the last call: ms[4] = upload, kernels, download (HIP events; 0 on the host path), whole call (wall);
 * cnt[3] = reads, reads the host routine did beside the kernel, intervals written */
void damar_dust_last(double *ms, int64 *cnt);
/* of the last call, kernel and host routine together: steps[0] = triplets stepped over (halos included), steps[1] = those
 * that entered the walk over the window's starts */
void damar_dust_steps(int64 *steps);

/* Phase timings (milliseconds, HIP events on the library's stream) of the last
 * damar_index_build / damar_match: see DAMAR_T_* below. */
enum { DAMAR_T_TUPLES = 0, DAMAR_T_KSORT, DAMAR_T_TABLE, DAMAR_T_MERGE, DAMAR_T_SSORT,
       DAMAR_T_WORK, DAMAR_T_REPORT, DAMAR_T_D2H, DAMAR_T_TAIL, DAMAR_T_COUNT };
void damar_last_timings(double *ms /* [DAMAR_T_COUNT] */);
/* bytes, files, records and aligned base pairs (sum of aepos - abpos) the .las writers have produced since the process started (host/las.c; with DAMAR_LAS_KEEP=<list>
   only the files whose path ends in a line of <list> reach the file system, the rest /dev/null: measurement of long plans) */
void damar_las_totals(int64 *out /* [4] */);
/* Checking of every .las file as it is written (daligner -C): with damar_set_check(1) the thread that writes a file runs
   its records and trace bytes, as they go to the file, through the routine of include/damar_check.h -- LAcheck's -p -s -d
   and the strict set, read lengths from the blocks that were compared -- files that DAMAR_LAS_KEEP discards included.  A
   violation is one line "damar: CHECK <file>: <message>" on stderr (16 per file at most) and is counted; nothing else
   changes, the file is written all the same.  Totals since the process started: files checked, records checked,
   violations, files checked of those that were discarded. */
void damar_set_check(int on);
void damar_check_totals(int64 *out /* [4] */);
/* The bounds (aepos <= alen, bepos <= blen) need the reads' lengths, which a write request does not carry: whoever runs
   the comparisons notes their two blocks (bblock may be NULL) at the Align_Spec the records go to, before the files are
   asked for.  The lengths are copied.  Without it the bounds are left out; does nothing while checking is off. */
void damar_check_note_blocks(Align_Spec *spec, const HITS_DB *ablock, const HITS_DB *bblock);

/* Counters of the last damar_match / damar_match_batch (summed over its comparisons): [0] seed pairs, [1] work items
 * (read pairs entered), [2] Local_Alignment calls, [3] records from the device, [4] trace values, [5] launches of the
 * report kernel (re-launches after a buffer overflow included). */
void damar_last_counters(int64 *c /* [8] */);

/* Sort kernels alone, for the roofline measurement: sorts n (u32 key, u32 payload)
 * pairs resident in HBM on `nbits` key bits `reps` times and returns the average
 * milliseconds per sort (HIP events). */
double damar_bench_sort_u32(uint32_t n, int nbits, int reps, uint32_t seed);

#ifdef __cplusplus
}
#endif
#endif
