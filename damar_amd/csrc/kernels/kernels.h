/* kernels.h -- host-callable launchers of the gfx950 kernels (internal to the shim). */
#ifndef DAMAR_KERNELS_H
#define DAMAR_KERNELS_H

#include "dev_common.h"
#include "../la_record.h"

/* sort_scan.hip */
size_t damar_scan_workspace_bytes(u64 n);
void   damar_exclusive_scan_u32(const u32 *in, u32 *out, u64 n, void *work, u64 *total_dev, hipStream_t st);
#define DAMAR_SCAN_TILE 4096      /* items per scan tile (sort_scan.hip) */
void   damar_tile_offsets_u32(const u32 *in, u64 n, void *work, u64 *total_dev, hipStream_t st);
void   damar_scan_tile_counts(u32 *tcount, u32 ntiles, u64 *total_dev, hipStream_t st);
/* radix_sort.hip: stable LSD radix sorts; each returns the side (0: k0/v0, 1: k1/v1) the result is on */
size_t damar_sort_workspace_bytes(u64 n);
void   damar_sort_set_threads(int threads);               /* tile shape: 256 or 512 threads per workgroup */
const u32 *damar_sort_error_word(const void *work);       /* device word, non-zero after a sort whose look-back timed out */
int    damar_radix_sort_keys_u64(u64 *k0, u64 *k1, u64 n, int lobit, int hibit, void *work, hipStream_t st);
void   damar_radix_sort_split_u64(u64 *k0, u64 *k1, u64 n, int lobit, int hibit, u32 *ohi, u32 *olo, void *work,
                                  hipStream_t st);
int    damar_radix_sort_u32(u32 *k0, u32 *v0, u32 *k1, u32 *v1, u64 n, int nbits, void *work, hipStream_t st);
int    damar_radix_sort_keys_u32(u32 *k0, u32 *k1, u64 n, int nbits, void *work, hipStream_t st);    /* keys only */
int    damar_radix_sort_u64(u64 *k0, u32 *v0, u64 *k1, u32 *v1, u64 n, int nbits, void *work, hipStream_t st);

/* pile_sweep.hip: mask tracks from piles of overlaps (scrub/LArepeat.c, scrub/TANmask.c) */
enum { DAMAR_PILE_COVER = 0, DAMAR_PILE_REPEAT = 1, DAMAR_PILE_TANDEM = 2 };
#define DAMAR_PILE_ERR_RANGE 1u      /* a coordinate does not fit the key's position bits */
typedef struct
{ /* the batch (include/damar_hip.h damar_pile_batch) */
  const long long *pile_off;
  const int *pile_aread, *abpos, *aepos, *bbpos, *bepos, *bread, *flags, *read_len, *read_flags;
  u32   npiles;
  int   mode, pbits;             /* event key = pile << (pbits + 1) | coordinate << 1 | tie bit */
  int   min_len, inc_identity, inccov, enter, leave, merge_dist;
  u64  *keys;                    /* [2 * records]: pile_events writes, pile_sweep reads them sorted */
  u32  *kept;                    /* [npiles] records of the pile that pass the filters */
  const u32 *koff;               /* [npiles] exclusive sums of kept */
  u64  *bases;                   /* [npiles] COVER: summed lengths of the kept records */
  int  *active;                  /* [npiles] COVER: length of their union */
  int  *rb, *re, *rc;            /* [kept records] REPEAT: raw regions of pile p from koff[p] */
  int  *out;                     /* [3 * kept records] ints of pile p from 3 * koff[p] */
  u32  *count;                   /* [npiles] how many */
  u64  *stats;                   /* [0] merges, [1] repeat bases */
  u32  *err;
} PileArgs;
void damar_launch_pile_events(const PileArgs *a, hipStream_t st);
void damar_launch_pile_sweep(const PileArgs *a, hipStream_t st);
void damar_launch_pile_gather(const int *out, const u32 *koff, const u32 *count, const u32 *doff, u32 npiles, int *dst, hipStream_t st);

/* A read block resident in HBM. */
typedef struct
{ const u8  *bases;     /* byte per base 0..3, 4 = terminator; bases[-1] == 4 (reference layout) */
  const u32 *pk;        /* the same positions at 2 bits per base (terminators read as 0): word w
                           holds bases 16w .. 16w+15, base 16w in bits 0-1; PK_PAD words either side */
  u32        rbias;     /* the bases in REVERSE order follow in the same array: base total-1-j sits at biased position
                           rbias + j (position of base p in the forward part: p + 16 * PK_PAD), see pack_bases */
  const u32 *boff;      /* [nreads+1] offset of read i in bases                                   */
  const u32 *coarse;    /* [(total >> COARSE_SHIFT) + 2] read containing position q<<COARSE_SHIFT */
  u32        nreads;
  u32        total;     /* boff[nreads]                                                           */
  int        maxlen;
  int        rpbits;    /* > 0: the index of this block keeps a k-mer's position as read << rpbits | offset in the
                           read (both fit 32 bits); 0: as offset in the block (decoded through coarse / boff)      */
  const u32 *moff;      /* mask track (-m): intervals of read i are mdat[2j], mdat[2j+1] for       */
  const int *mdat;      /* j in [moff[i]/2, moff[i+1]/2); NULL when the block carries no mask      */
} DevBlock;

/* the packed index keys of a block (k <= 16) as a source of the radix sort, see KmerCursor below */
typedef struct { DevBlock blk;  int kmer; } KmerKeys;
/* as damar_radix_sort_split_u64 on the bits [32, 32 + 2 * kmer) of the n keys kmer_tuples would have left in k0 -- which
   are never written: the histogram and the first pass make them from the block's 2-bit bases (k0 is still the other
   side of the ping-pong) */
void damar_radix_sort_split_kmers(const KmerKeys *src, u64 *k0, u64 *k1, u64 n, u32 *ohi, u32 *olo, void *work,
                                  hipStream_t st);

/* Seed-side kernels run beside a resident report launch that is bound by vector instruction issue: four report
   wavefronts and one seed wavefront share a SIMD, and at equal priority the seed wavefront -- which mostly waits for memory --
   gets a fifth of the issue slots whenever it is ready.  Raised priority lets it issue at once and go back to waiting.
   Which kernels do so is a run-time choice per source file (damar_*_set_prio; shim.hip: DAMAR_SEED_PRIO). */
#define SEED_PRIO_VAR(name, dflt) static __device__ int name = dflt;  static int name##_host = dflt;
#define SEED_PRIO(name)     do { if (name) __builtin_amdgcn_s_setprio(3); } while (0)
/* (a copy to a device symbol loads the file's code object and waits for the copy: only when the value differs from what
   the code object already holds -- the defaults are the compiled-in values, so that a cold command sets nothing) */
#define SEED_PRIO_SETTER(fn, name) \
  void fn(int on) { if (on != name##_host) { HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(name), &on, sizeof(int)));  name##_host = on; } }

#define COARSE_SHIFT 9
#define PK_PAD 4

#ifdef __HIPCC__
/* read containing base offset p (p is inside a read, never on a terminator) */
__device__ __forceinline__ u32 read_of_pos(const DevBlock &b, u32 p)
{ u32 r = b.coarse[p >> COARSE_SHIFT];
  while (b.boff[r + 1] <= p)
    r += 1;
  return r;
}
/* the position word of an index entry -> read and offset of the k-mer's last base in it: free when the block's index
   is packed (rpbits), two dependent look-ups otherwise */
__device__ __forceinline__ void pos_decode(const DevBlock &b, u32 v, u32 *r, u32 *x)
{ if (b.rpbits)
    { *r = v >> b.rpbits;
      *x = v & ((1u << b.rpbits) - 1u);
    }
  else
    { const u32 rr = read_of_pos(b, v);
      *r = rr;
      *x = v - b.boff[rr];
    }
}
__device__ __forceinline__ u32 pos_encode(const DevBlock &b, u32 r, u32 x, u32 p)
{ return b.rpbits ? ((r << b.rpbits) | x) : p; }

/* The k-mer slots of a block (k-mers in position order, kmer_index.hip): read r owns the slots
   [kmer_slot0(boff[r], r, k), kmer_slot0(boff[r + 1], r + 1, k)) -- a read of len bases has len + 1 - k of them -- and
   the k-mer of slot i of read r begins at block offset i + r * k. */
__device__ __forceinline__ u32 kmer_slot0(u32 b0, u32 r, int kmer) { return b0 - r * (u32) kmer; }

/* k <= 16: the code of the k-mer that begins at block offset f, out of the 2-bit copy of the block (two adjacent words,
   base 16w in the low bits of word w) instead of k byte loads; the code wants the FIRST base in its high bits, so the
   window is reversed pair-wise.  16 bases from f on always lie in two words, and the low 32 bits of their funnel shift
   hold them all. */
__device__ __forceinline__ u32 kmer_code16(const u32 *__restrict__ pk, u32 f, int kmer)
{ const u32 wq = f >> 4, o = (f & 15) << 1;
  const u32 win = __builtin_amdgcn_alignbit(pk[wq + 1], pk[wq], o);
  u32 r = __brev(win);                                                 /* base j now sits at bits 30-2j, its two bits swapped */
  r = ((r >> 1) & 0x55555555u) | ((r & 0x55555555u) << 1);
  return r >> (32 - 2 * kmer);
}

/* The packed index keys of a block as a SOURCE of the radix sort (radix_sort.hip): the key of slot i is what
   kmer_tuples<u64, true> stores at k0[i], code << 32 | position word, made from the 2-bit bases where the sort wants it.
   A wavefront asks for runs of 64 consecutive slots in ascending order: it finds the read of its first slot with all
   its lanes (a 64-ary search over the reads' first slots, three round trips for 2^18 reads), after that a lane only
   steps to the next read when its slot has left the current one. */

struct KmerCursor
{ u32 r, ks, ke;                       /* the read, its first slot, the first slot of the next read */

  /* slot: the wavefront's first slot (the same in every lane, < the number of slots; all 64 lanes are here) */
  __device__ __forceinline__ void open(const KmerKeys &g, u32 slot)
  { const u32 l = (u32) lane_id();
    u32 lo = 0, hi = g.blk.nreads;                 /* the read is in [lo, hi): slot0(lo) <= slot, slot0(hi) > slot or hi past the end */
    while (hi - lo > 1)
      { const u32  step = (hi - lo + 63) >> 6;
        const u32  c  = lo + l * step;
        const bool ok = c < hi && kmer_slot0(g.blk.boff[c < hi ? c : lo], c, g.kmer) <= slot;   /* (true in lane 0; slot0 never falls) */
        const u32  in = (u32) __popcll(wballot(ok));
        lo += (in - 1) * step;
        hi  = (lo + step < hi) ? lo + step : hi;
      }
    r  = lo;
    ks = kmer_slot0(g.blk.boff[r], r, g.kmer);
    ke = kmer_slot0(g.blk.boff[r + 1], r + 1, g.kmer);
  }
  /* the key of slot i (>= the slot of the call before, < the number of slots) */
  __device__ __forceinline__ u64 key(const KmerKeys &g, u32 i)
  { while (i >= ke)                                /* (reads without a k-mer are stepped over) */
      { r += 1;
        ks = ke;
        ke = kmer_slot0(g.blk.boff[r + 1], r + 1, g.kmer);
      }
    const u32 f = i + r * (u32) g.kmer, x = i - ks + (u32) (g.kmer - 1);
    return ((u64) kmer_code16(g.blk.pk, f, g.kmer) << 32) | (u64) pos_encode(g.blk, r, x, f + (u32) (g.kmer - 1));
  }
};
#endif

/* pk[w] for w in [-PK_PAD, total/16 + PK_PAD] from bases (which carry 64 padding bytes either side), then as many words
   of the reversed copy: pk points PK_PAD words into an array of 2 * damar_pack_words(total) words */
long long damar_pack_words(u32 total);
void damar_launch_pack_bases(const u8 *bases, u32 total, u32 *pk, hipStream_t st);
/* the block out of its .bps stretch (kmer_index.hip unpack_bps); blk needs boff, coarse, total; bases preset to 4 */
void damar_launch_unpack_bps(const u8 *raw, const u32 *foff, const DevBlock *blk, int comp, u8 *bases, hipStream_t st);

/* kmer_index.hip */
/* codes: u32 (k <= 16) or, with wide != 0, u64 (k <= 32) */
void damar_preload_index(void);  void damar_preload_scan(void);  void damar_preload_sort(void);
void damar_preload_merge(void);  void damar_preload_report(void);
void damar_sort_set_prio(int on);
void damar_merge_set_prio(int on);
void damar_index_set_prio(int on);
void damar_launch_kmer_tuples(const DevBlock *blk, int kmer, u32 nkmers, void *codes, int wide, u32 *pos, hipStream_t st);
/* keep[i] = 1 iff k-mer i lies inside one unmasked stretch of its read (filter.c:474-526) */
void damar_launch_mask_flags(const DevBlock *blk, int kmer, const u32 *pos, u32 n, u32 *keep, hipStream_t st);
/* -b: keep[] (cleared by the caller, blk->total entries) marks the block offsets where a k-mer ends */
void damar_launch_biased_tuples(const DevBlock *blk, int kmer, const int *logbase, void *codes, int wide, u32 *pos,
                                u32 *keep, hipStream_t st);
void damar_launch_suppress_flags(const void *codes, int wide, u32 n, int suppress, u32 *keep, hipStream_t st);
void damar_launch_compact_pairs(const void *k, int wide, const u32 *v, const u32 *keep, const u32 *off, u32 n,
                                void *ko, u32 *vo, hipStream_t st);

/* datander: distance to the previous equal k-mer of the same read, scattered back to position
 * order (dist[k-mer index]); scrub/tandem.c:556-589 + the (read,rpos) re-sort of :1298 */
void damar_launch_tandem_links(const DevBlock *blk, int kmer, const void *codes, int wide, const u32 *pos, u32 n,
                               int *dist, hipStream_t st);

/* seed_merge.hip */
typedef struct
{ const void *acode;  const u32 *apos;  u32 alen;                         /* codes: u32, or u64 when wide */
  const void *bcode;  const u32 *bpos;  u32 blen;
  int  wide;
  int  kbits;
  int  self, comp, identity;
  u32  limit;
  DevBlock ablk, bblk;
  int  pbits, abits;          /* key = bread << (abits+pbits) | aread << pbits | apos, all of it << dbits */
  int  dbits;                 /* > 0: bpos rides in the key's low dbits (packed seeds, no vals array); 0: diag in vals */
  u32  b_lo, b_hi;            /* a comparison run in slabs: the B reads of this slab (merge_range; the sweeps do not look) */
} MergeArgs;

typedef struct { u32 b0, b1, ja, ia;                   /* per tile of A entries: its piece of B, the ends of its border runs, */
                 u32 sh, pad[3]; } MergeTile;           /* and the shift that maps (code - first code of the tile) onto < 2048 buckets */

/* The merge is two sweeps over tiles of the A index (seed_merge.hip): COUNT leaves the hits per tile in the workspace
   (damar_merge_tile_counts; with gram != NULL also hitgram[ct] for ct < ngram, filter.c:1039-1165), the caller scans
   them in place (damar_scan_tile_counts) and EMIT writes the seed pairs. */
size_t damar_merge_workspace_bytes(u32 alen);
u32   *damar_merge_tile_counts(void *work, u32 alen);
u32    damar_merge_tiles(u32 alen);
void   damar_launch_merge_count(const MergeArgs *m, void *work, unsigned long long *gram, u32 ngram, hipStream_t st);
/* pid (optional): the read pair of every seed, bread << abits | aread, for the early cut */
void damar_launch_merge_emit(const MergeArgs *m, void *work, u64 nhits, u64 *keys, u32 *vals, u32 *pid, hipStream_t st);
/* A comparison run in slabs of B reads.  Both work on what a COUNT sweep (with every cap over the whole code run) has left
   in the workspace: hist[r] += the seed pairs with bread r (hist zeroed by the caller, m->bblk.nreads entries); and, before
   the scan of the tile counts, the counts narrowed to the B reads [m->b_lo, m->b_hi), after which the scan and EMIT yield
   that range's seed pairs only. */
void damar_launch_merge_bread_hist(const MergeArgs *m, void *work, unsigned long long *hist, hipStream_t st);
void damar_launch_merge_range(const MergeArgs *m, void *work, hipStream_t st);
/* the early cut (seed_merge.hip): heads of the runs report_thread enters, on the SORTED pair ids; their pairs into a
   bitmap over the pair ids; the seeds of those pairs out of the unsorted seeds */
/* (off, gtotal, here and below: the seeds are the stretch [off, off + nhits) of a sorted list of gtotal -- a slab of B reads;
   the reference's thread slices are those of the whole list.  0 and nhits for a comparison in one piece) */
void damar_launch_pair_heads_ids(const u32 *pids, u64 nhits, u64 off, u64 gtotal, int abits, int minhit, int nshift,
                                 u64 *send, u64 *bits, void *scan_work, u64 *total_dev, u32 *heads, hipStream_t st);
void damar_launch_pair_bitmap(const u32 *pids, const u32 *heads, u32 nheads, int abits, u32 b_lo, u32 b_hi, u32 *bitmap,
                              hipStream_t st);
void damar_launch_seed_cut_count(const u64 *keys, u64 nhits, int pbits, const u32 *bitmap, u32 *tcount, u64 *total_dev,
                                 hipStream_t st);
void damar_launch_seed_cut_scatter(const u64 *keys, const u32 *vals, u64 nhits, int pbits, const u32 *bitmap,
                                   const u32 *toff, u64 *okeys, u32 *ovals, hipStream_t st);
void damar_launch_pair_heads(const u64 *keys, u64 nhits, u64 off, u64 gtotal, int pbits, int abits, int minhit, int nshift,
                             u64 *send /* 64 entries of scratch */, u64 *bits, void *scan_work, u64 *total_dev,
                             u32 *heads, hipStream_t st);
/* run heads + screen in one pass (pair_work_mark): the first half leaves the number of work items in *total_dev */
/* (unsorted: the seed sort went over the read pair only -- the screen takes a run's seeds in any order, the caller puts the
   kept heads' runs in order of their A positions (damar_launch_order_runs) unless total_dev[1] != 0: a run too long for that,
   sort over all the bits) */
void damar_launch_pair_work(u64 *keys, const u32 *vals, u64 nhits, u64 off, u64 gtotal, int ppos, int dbits, int abits, int minhit, int nshift,
                            u64 *send /* 64 entries of scratch */, u64 *bits, void *scan_work, u64 *total_dev /* [2] */,
                            int binshift, int kmer, int hitmin, u32 b_lo, u32 b_hi, int unsorted, hipStream_t st);
/* (unsorted only) the runs of the work list's heads (ascending) into the order of their A positions, in place; runs of more
   than 2048 seeds are left as they are.  scratch: damar_order_runs_scratch_bytes(nhits) */
size_t damar_order_runs_scratch_bytes(u64 nhits);
void damar_launch_order_runs(u64 *keys, u64 nhits, int ppos, int dbits, const u32 *work, u32 nwork, void *scratch, hipStream_t st);
void damar_launch_pair_work_expand(const u64 *bits, const void *scan_work, u64 nhits, u32 *work, hipStream_t st);
#define WORK_COST_BITS 16
#define WORK_COST_MAX  ((1u << WORK_COST_BITS) - 1)
void damar_launch_work_cost(const u64 *keys, const u32 *vals, u64 nhits, int pbits, int abits, int dbits, const u32 *aboff,
                            const u32 *bboff, const u32 *work, u32 nwork, u32 coarse, u32 *key, u32 *val, hipStream_t st);
void damar_launch_pair_screen(const u64 *keys, const u32 *vals, u64 nhits, int pbits, int dbits, const u32 *heads, u32 nheads,
                              int minhit, int binshift, int kmer, int hitmin, int abits, u32 b_lo, u32 b_hi, u32 *keep, hipStream_t st);
void damar_launch_compact_u32(const u32 *src, const u32 *keep, const u32 *off, u32 n, u32 *out, hipStream_t st);
void damar_launch_compact_index(const u32 *flags, const u32 *off, u64 n, u32 *out, hipStream_t st);

#ifdef __HIPCC__
/* diagonal (apos - bpos) of seed i: from the packed key, or from the vals array of the unpacked layout */
__device__ __forceinline__ int seed_diag(u64 k, const u32 *__restrict__ vals, u64 i, u64 pmask, int dbits)
{ if (dbits)
    return (int) ((k >> dbits) & pmask) - (int) (k & ((1ull << dbits) - 1));
  return (int) vals[i];
}
#endif

/* report.hip */
/* LaRecord, DAMAR_MAX_JOBS, DAMAR_ITEM_WIDE, DAMAR_SEQ_BITS: la_record.h */

typedef struct
{ /* inputs */
  const u64 *keys;  const u32 *vals;  u64 nhits;
  const u32 *work;  u32 nwork;
  DevBlock ablk, bblk;
  int  pbits, abits, dbits;        /* seed key layout, see MergeArgs */
  int  kmer, hitmin, binshift, minhit;
  int  comp, self, symmetric, minover, hgap_min;
  int  tspace, ave_path, reach;
  const short *score, *table;      /* SCORE[32768], TABLE[32768] */
  int  mscore, dscore;             /* the two column scores the tables are built from (align.c:282-284) */
  /* per-slot scratch */
  void *state;   u64 state_stride;   int span;        /* ping-pong diagonal state: rings of `span` (2^n) diagonals */
  int  *marks;   u64 marks_stride;                    /* NA/NB                     */
  void *cells;   u32 cell_cap;                        /* pebbles                   */
  int  *buckets; u64 bucket_stride;  int bwidth;      /* score|lastp|lasta          */
  int  bucket_bits;                                   /* bits needed for bucket - mindiag */
  u16  *ttmp;    u32 ttmp_stride;                     /* 2 centred trace buffers   */
  /* outputs */
  LaRecord *recs;  u32 rec_cap;
  u16  *tpool;     u32 tpool_cap;
  u32  *widemap;                   /* one bit per work item: the two-pair kernel gave the pair up (pebbles beyond the packed format);
                                      NULL: no wide path behind this launch (the limits are fatal as until round 4) */
  void *wcells;    u32 wcell_cap;  /* the wide kernel's 16-byte pebbles: wcell_cap per slot */
  u32  cell_max;                   /* the largest pool a slot can get (DAMAR_MAX_CELLS; a test hook lowers it): a pair that overflows it is the wide kernel's */
  int  t8, t8max;                  /* t8: trace values leave as BYTES (tspace <= 125: align.c:3375-3396 Compress_TraceTo8 on the device, the
                                      pool then holds tpool_cap bytes' worth of values in its first half); a value above t8max (255) raises
                                      DAMAR_ERR_T8 and the host repeats the launch with 16-bit values, so that the reference's own check
                                      decides (it looks only at the records that are written) */
  const u32 *order; /* processing order of the work items (largest first), or NULL          */
  u32  *counters;  /* [1] records, [2] trace words, [3] error flags, [6] [7] where a wave gave up; shared by the jobs of a launch */
  u32  *cursor;    /* next work item of THIS job (counters + DAMAR_CNT_CURSOR + job) */
  u32  *nfilt;     /* seed hits of THIS job      (counters + DAMAR_CNT_NFILT + job)  */
  int   job;       /* index of this job in the launch: rides in the top byte of LaRecord.seq */
} ReportArgs;

/* One launch of a report kernel works through up to DAMAR_MAX_JOBS comparisons (ReportArgs each, in constant memory:
   wave-uniform reads of a job's fields are scalar loads).  Every wavefront starts with job (block index mod njobs) and
   moves on to the next when a job's queue is empty, so the long alignments of ALL jobs start at once and the tail of
   the launch (waiting for the longest alignment) is paid once per launch, not once per comparison. */
#define DAMAR_MAX_TSPACE 8192     /* consecutive pebbles of a chain then differ by < 2^15 diagonals and < 2^16 waves */
#define DAMAR_CNT_RECS      1     /* counters[1]: records written (asked for, when DAMAR_ERR_RECS is up) */
#define DAMAR_CNT_TPOOL     2     /* counters[2]: trace values written (asked for, when DAMAR_ERR_TPOOL is up) */
#define DAMAR_CNT_FLAGS     3     /* counters[3]: the DAMAR_ERR_* flags below */
#define DAMAR_CNT_WHERE     6     /* counters[6]: which loop gave up when DAMAR_ERR_BAND is up (report.hip GUARD) */
#define DAMAR_CNT_CELLS     8     /* counters[8..9]   (64 bits): band cells of the launch's wave steps (packed kernel) */
#define DAMAR_CNT_HALFSTEPS 10    /* counters[10..11] (64 bits): wave steps, counted per half-wavefront (= per alignment pass)   */
#define DAMAR_CNT_ITERS     12    /* counters[12..13] (64 bits): iterations of the wave loop (each steps one or two halves)      */
#define DAMAR_CNT_WIDE    14      /* counters[14]: read pairs left to the wide kernel (report_wide_kernel) */
#define DAMAR_CNT_CURSOR  16      /* counters[16 + job]: next work item of a job  */
#define DAMAR_CNT_NFILT   (DAMAR_CNT_CURSOR + DAMAR_MAX_JOBS)      /* counters[.. + job]: its seed hits */
#define DAMAR_COUNTER_WORDS (DAMAR_CNT_NFILT + DAMAR_MAX_JOBS)

#define DAMAR_ERR_CELLS   1u
#define DAMAR_ERR_RECS    2u
#define DAMAR_ERR_TPOOL   4u
#define DAMAR_ERR_BAND    8u
#define DAMAR_ERR_T8     32u    /* a trace value does not fit a byte (see ReportArgs.t8) */
#define DAMAR_ERR_WIDE   16u    /* a band outgrew the ring of diagonals of the slot buffers: relaunch with a larger ring */

int  damar_report_waves_per_simd(void);
int  damar_report2_waves_per_simd(void);
int  damar_report2_slots_per_wave(void);     /* scratch slots (read pairs in flight) per wavefront of the packed kernel */
void damar_launch_report(const ReportArgs *jobs, int njobs, int nslots, hipStream_t st);
void damar_launch_report_wide(const ReportArgs *jobs, int njobs, int nslots, hipStream_t st);
/* datander report: one work item per read of a.ablk, dist as produced by damar_launch_tandem_links */
void damar_launch_tandem_report(const ReportArgs *a, const int *dist, int nslots, hipStream_t st);

/* batch Local_Alignment for tests: task i = (aread, bread, diag, anti) */
typedef struct { int aread, bread, diag, anti; } LaTask;
void damar_launch_la_batch(const ReportArgs *a, const LaTask *tasks, u32 ntasks, int nslots, hipStream_t st);
/* several read pairs (or batch tasks, tasks != NULL) per wavefront: report_packed.h; nslots a multiple of damar_report2_slots_per_wave() */
void damar_launch_report2(const ReportArgs *jobs, int njobs, const LaTask *tasks, u32 ntasks, int nslots, hipStream_t st);
void damar_launch_tandem_report2(const ReportArgs *a, const int *dist, int nslots, hipStream_t st);     /* datander through the same kernel */
/* the reads / tasks the two-pair kernel left to the 16-byte pebbles (a->widemap, reads beyond DAMAR_MAX_MARKS spacings) */
void damar_launch_tandem_report_wide(const ReportArgs *a, const int *dist, int nslots, hipStream_t st);
void damar_launch_la_batch_wide(const ReportArgs *a, const LaTask *tasks, u32 ntasks, int nslots, hipStream_t st);
#define DAMAR_MAX_MARKS 16000         /* trace-grid indexes ride in the top 14 bits of a chain head (report.hip PK_HBITS) */
#define DAMAR_MAX_CELLS (1u << 18)    /* pebbles per slot: 18 bits of a chain head */

u64 damar_report_state_stride(int span);

/* pile_quality.hip: LAq's per-tile quality from the traces of a batch of piles (scrub/LAq.c:312-409).  Tiles are numbered
   through the batch: pile p owns [pile_tile0[p], pile_tile0[p + 1]). */
typedef struct
{ u32 npiles, nrec, ntiles;
  int tspace, tbytes;
  u32 segmin, segmax;
  int ccs;
  const long long *pile_off;          /* [npiles + 1] */
  const int *pile_aread, *pile_alen;  /* [npiles] */
  const u32 *pile_tile0;              /* [npiles + 1] */
  const int *abpos, *aepos, *bread, *tlen;       /* [nrec] */
  const long long *trace_off;         /* [nrec] bytes into trace */
  const u8  *trace;
  u32 *depth;                         /* [ntiles + 1] zeroed: segments per tile (q_count), used up again by q_scatter */
  const u32 *off;                     /* [ntiles + 1] exclusive scan of depth */
  u16 *vals;                          /* a run of difference counts per tile, in no order */
  int *q;                             /* [ntiles] */
} QArgs;

void damar_launch_q_count(const QArgs *a, hipStream_t st);
void damar_launch_q_scatter(const QArgs *a, hipStream_t st);
void damar_launch_q_select(const QArgs *a, hipStream_t st);

/* homogenize.hip: repeat intervals carried across overlaps into a bit mask of the whole database (scrub/TKhomogenize.c).
   Read r owns the words [woff[r], woff[r + 1]) of `words`: bit j of the read is bit j % 32 of word j / 32, one bit per `res`
   bases, alen = (res > 1 ? ceil(rlen / res) : rlen) of them are read back and one spare bit follows. */
typedef struct
{ u32 npiles, nrec, nreads;
  int tspace, tbytes;
  int res, ends;                      /* ends: -1, or -e's n (trim is set then) */
  const long long *pile_off;          /* [npiles + 1] */
  const int *pile_aread;              /* [npiles] */
  const int *abpos, *aepos, *bbpos, *bepos, *bread, *flags, *tlen;       /* [nrec] */
  const long long *trace_off;         /* [nrec] bytes into trace */
  const u8  *trace;
  const u64 *iv_anno;                 /* [nreads + 1] byte offsets into iv_data */
  const int *iv_data;                 /* {begin, end} pairs */
  const int *trim;                    /* [2 * nreads] or NULL */
  const int *read_len;                /* [nreads] */
  const u64 *woff;                    /* [nreads + 1] */
  u32 *words;
  u64 *nranges;                       /* added to: ranges set */
  u32 *count;                         /* [nreads] intervals of a read (hom_count) */
  const u32 *off;                     /* [nreads] exclusive scan of count */
  int *out;                           /* {begin, end} pairs, read r's from 2 * off[r] */
} HomArgs;

void damar_launch_hom_mark(const HomArgs *a, hipStream_t st);
void damar_launch_hom_seed(const HomArgs *a, hipStream_t st);
void damar_launch_hom_count(const HomArgs *a, hipStream_t st);
void damar_launch_hom_emit(const HomArgs *a, hipStream_t st);

/* pile_gaps.hip: LAgap's containments, gaps and breaks, one wavefront per pile (include/damar_hip.h damar_pile_gaps; the
   DAMAR_GAP_* bounds and kinds are defined there).  A pile with status 1 afterwards is the host's: a read of more than
   maxbins bins, skip[pile] set, or more than maxev events. */
typedef struct
{ u32 npiles;
  int maxbins, maxev, stitch;
  const long long *pile_off;          /* [npiles + 1] */
  const int *pile_aread;              /* [npiles] */
  const int *abpos, *aepos, *bbpos, *bepos, *bread, *flags;       /* [nrec] */
  const int *read_len;                /* [nreads] */
  const u64 *ex_anno;                 /* [nreads + 1] byte offsets into ex_data, NULL: no exclude track */
  const int *ex_data;
  const u8  *skip;                    /* [npiles] */
  int *flags_out;                     /* [nrec] */
  int *status, *nev;                  /* [npiles] */
  int *ev;                            /* [npiles * DAMAR_GAP_MAXEVENTS * DAMAR_GAP_EVENT_INTS] */
  int *cnt;                           /* [npiles * 3]: contained, breaks, records dropped */
} GapArgs;

void damar_launch_pile_gaps(const GapArgs *a, u32 grid, hipStream_t st);      /* min(npiles, grid) workgroups */
u32  damar_pile_gaps_grid(void);      /* workgroups of the largest launch: beyond that many piles a workgroup does several */

/* pile_chains.hip: LAseparate's chains and verdicts (include/damar_hip.h damar_pile_chains; the DAMAR_SEPARATE_* bounds are
   defined there).  Two launches over the piles: the first gives every record its repeat counts and the marks of its
   place in its group and settles the groups of one record, the second chains the groups of two or more.  A group whose
   first record has status 1 afterwards is the host's: more than maxgroup records, more than maxchains chains. */
typedef struct
{ u32 npiles;
  int kind, twidth, maxgroup, maxchains;
  const long long *pile_off;          /* [npiles + 1] */
  const int *pile_aread;              /* [npiles] */
  const int *abpos, *aepos, *bbpos, *bepos, *bread, *flags;       /* [nrec] */
  const int *read_len;                /* [nreads] */
  const u64 *rep_anno;                /* [nreads + 1] byte offsets into rep_data, NULL: no repeat track */
  const int *rep_data;
  int *arep, *brep;                   /* [nrec]: the first launch's, for the second */
  int *o_flags, *o_nchains, *o_proper, *o_nbest, *o_best, *status;     /* [nrec] */
} ChainArgs;

void damar_launch_pile_chains(const ChainArgs *a, u32 grid, hipStream_t st);    /* both launches, min(npiles, grid) workgroups each */
u32  damar_pile_chains_grid(void);

/* dust.hip: DBdust's mask, one wavefront per piece of a read (include/damar_hip.h damar_dust_reads; the DAMAR_DUST_* bounds
   are defined there).  Piece q is the starts from piece_first[q] on of read piece_read[q]; the pieces of read i are
   [read_piece[i], read_piece[i + 1]).  damar_launch_dust_pieces leaves nint[i] pairs per read at the head of its first
   stripe (-1: a stripe was too small, the read is the host's); with out_off made from them, damar_launch_dust_gather moves
   the pairs to out. */
typedef struct
{ u32 npieces, nreads;
  int window, thresh2i, minlen, stripe;
  double thresh;
  const u8  *bases;
  const long long *read_off;          /* [nreads + 1] */
  const u32 *piece_read;              /* [npieces] */
  const int *piece_first;             /* [npieces] */
  const u32 *read_piece;              /* [nreads + 1] */
  int *cand;                          /* [npieces * stripe * 2] */
  int *ncand;                         /* [npieces]: candidates retired, beyond `stripe` not written */
  int *nint;                          /* [nreads] */
  u64 *steps;                         /* [2]: steps taken, steps that entered the walk; added to */
  const long long *out_off;           /* [nreads] ints into out */
  int *out;
} DustArgs;

void damar_launch_dust_pieces(const DustArgs *a, hipStream_t st);       /* the pieces, then the join per read */
void damar_launch_dust_gather(const DustArgs *a, hipStream_t st);

/* pile_filter.hip: LAfilter's screens, one wavefront per pile (include/damar_hip.h damar_pile_filter; the DAMAR_FILTER_*
   bounds, the DAMAR_FR_* reason bits and the DAMAR_FC_* counters are defined there).  A pile with status 1 afterwards is the
   host's: a run of more than maxgroup records of one B read, or under -z with -u a read of more than maxlen bases. */
typedef struct
{ u32 npiles;
  int steps, maxgroup, maxlen, mask_words;    /* mask_words: u32 words of dynamic LDS, 0 without -z -u */
  int downsample, max_rid, seg_rate, stitch, stitch_aggr, min_rlen, min_olen, max_unaligned, min_nonrep;
  float max_diffs;
  int merge_tips, multi, lowcov, remove, include, tbytes;
  const long long *pile_off;          /* [npiles + 1] */
  const int *pile_aread;              /* [npiles] */
  const int *abpos, *aepos, *bbpos, *bepos, *bread, *flags, *diffs, *tlen;
  const long long *trace_off;         /* [nrec], bytes */
  const u8  *trace;
  const int *read_len;
  const int *trim;                    /* [2 * nreads] or NULL */
  const u64 *rep_anno;                /* byte offsets; NULL without -n */
  const int *rep_data;
  const int *sym_off, *sym_len, *sym_data;      /* NULL without -A */
  const u8  *read_state;              /* NULL without -x / -I */
  int *o_flags, *o_ae, *o_be, *o_df, *o_tl, *o_why, *o_by;      /* [nrec] */
  int *status;                        /* [npiles] */
  int *cnt;                           /* [npiles * DAMAR_FC_COUNT] */
} FilterArgs;

void damar_launch_pile_filter(const FilterArgs *a, u32 grid, hipStream_t st);      /* min(npiles, grid) workgroups */
u32  damar_pile_filter_grid(void);    /* workgroups of the largest launch: beyond that many piles a workgroup does several */

/* pile_patch.hip: LAfix's breaks and weak segments, one wavefront per pile (include/damar_hip.h damar_pile_patches; the
   DAMAR_FIX_* bounds and damar_fix_gap are defined there).  Pile q writes its repairs to gaps + slot_off[q], where it has
   room for slot_off[q + 1] - slot_off[q] of them (the host's bound: candidate pairs plus bad segments, DAMAR_FIX_MAXREP at
   the most).  A pile with status 1 afterwards is the host's: a read of more than maxsegs segments, skip[pile] set, more
   than DAMAR_FIX_MAXCAND candidates, or more than DAMAR_FIX_MAXREP repairs. */
typedef struct
{ u32 npiles;
  int maxsegs, tspace, tbytes;
  int lowq, maxgap, maxspanners, minsupport;
  const long long *pile_off;          /* [npiles + 1] */
  const int *pile_aread;              /* [npiles] */
  const int *trim;                    /* [2 * npiles] */
  const int *abpos, *aepos, *bbpos, *bepos, *bread, *flags, *tlen;       /* [nrec] */
  const long long *trace_off;         /* [nrec] bytes into trace */
  const u8  *trace;
  const int *read_len;                /* [nreads] */
  const u64 *q_anno;                  /* [nreads + 1] byte offsets into q_data */
  const int *q_data;
  long long  q_ndata;
  const u64 *rep_anno;                /* NULL: no repeat track */
  const int *rep_data;
  const u8  *skip;                    /* [npiles] */
  const long long *slot_off;          /* [npiles + 1] */
  int *gaps;                          /* the eight ints of a damar_fix_gap per repair */
  int *status, *ngaps;               /* [npiles] */
} FixArgs;

void damar_launch_pile_patch(const FixArgs *a, hipStream_t st);

/* graph_edges.hip: the edges of OGbuild's overlap graph (touring/OGbuild.c).  A candidate edge as the pile kernel appends it */
#define GE_INTS 16                  /* e[9] (a b ab ae bb be flags ovh diffs), owner, right | slot << 1 | live << 3, ra, rb, pad, seq lo, seq hi */
enum { GC_NCAND, GC_NPROBE, GC_NEG, GC_EDGES, GC_REDGES, GC_SYM, GC_PARALLEL, GC_LEFT, GC_COUNT };
typedef struct
{ u32 npiles, nrec, nreads;
  const long long *pile_off;  const int *pile_aread;
  const int *abpos, *aepos, *bbpos, *bepos, *bread, *flags, *diffs;
  u64  first_rec;                     /* of the batch, in the file */
  const int *read_len, *trim;         /* [nreads], [2 * nreads] */
  /* resident across the batches of a file */
  u32 *status;                        /* [nreads] DAMAR_OG_CONTAINED, later DAMAR_OG_PROPER or-ed in */
  int *minfirst, *hasfirst;           /* [nreads] the symmetric discards: smallest B among a pile's, B read seen */
  int *cand;   u64 cand_cap;          /* GE_INTS per candidate */
  u64 *probe;  u64 probe_cap;         /* A << 32 | B of the records the building pass asks the discards for */
  u64 *ctr;                           /* [GC_COUNT] */
  /* the finishing kernels */
  u64  ncand, nprobe;
  u64 *key;  u32 *val;                /* the sort's keys and values */
  const u32 *val_in;
  int  rbits;                         /* bits of a read number */
  u32 *beg, *end;                     /* [2 * nreads] a list's stretch of the sorted candidates: left lists, then right lists */
  u32 *keep;                          /* [ncand] */
  const u32 *pos;                     /* exclusive scan of keep */
  u32 *kcount;                        /* [2 * nreads] edges a list keeps */
  u32 *hostread;                      /* [nreads] 1: a side over maxdeg, all its edges kept for the host routine */
  int  maxdeg;
  int *out;                           /* 9 ints per kept edge */
} GraphArgs;
void damar_launch_graph_count(const GraphArgs *a, hipStream_t st);      /* what a batch will append: ctr[GC_NCAND], ctr[GC_NPROBE] += */
void damar_launch_graph_emit(const GraphArgs *a, hipStream_t st);       /* the same pass, appending (the counters reset to the fill before) */
void damar_launch_graph_settle(const GraphArgs *a, hipStream_t st);     /* discards applied, statuses, key = file order */
void damar_launch_graph_keys(const GraphArgs *a, hipStream_t st);       /* key = list, b, zeros first, in the order of val_in */
void damar_launch_graph_bounds(const GraphArgs *a, hipStream_t st);
void damar_launch_graph_reads(const GraphArgs *a, hipStream_t st);
void damar_launch_graph_gather(const GraphArgs *a, hipStream_t st);

/* tile_consensus.hip: the consensus of tiles, one lane per tile.  Task i is tile order[i] of the batch (the host sorts by
   weight and leaves out the empty tiles and those with a sequence over its limit); its sequences are [ent_off[t],
   ent_off[t + 1]).  Lane l of the grid works in work + l * stripe: 5 * maxcols count bytes, maxcols match codes,
   maxscript int16 script values, cells int16 furthest points, cells int8 codes (maxcols even, so that all are aligned).
   status[i] = 0: len[i] called bases at out + i * maxcols; else the task is the host's (TC_ROOM: a limit was met). */
typedef struct
{ u32 ntasks, blocks;
  int maxcols, maxscript, cells;
  size_t stripe;
  const u32 *order;                   /* [ntasks] */
  const long long *ent_off;           /* [ntiles + 1] */
  const long long *seq_off;           /* [nent] */
  const int *seq_len;
  const u8  *bases;
  u8  *work;
  u8  *out;
  int *status, *len;                  /* [ntasks] */
} TileArgs;

void damar_launch_tile_consensus(const TileArgs *a, hipStream_t st);

/* box_align.hip: exact alignment of a batch of boxes with their edit scripts (align.c:4734 DIFF_ALIGN).  A box with
   max(m, n) <= maxlen <= DAMAR_BOX_MAXLEN is done and leaves its differences, the length of its script (-1: it hit a bound of
   the kernel and is the host's after all) and the script at script + coff[box], max(m, n) values of room; the others are
   not touched.  read_align.hip takes the same record: maxdiff and order are its own, and box_align reads neither. */
#define DAMAR_BOX_MAXLEN 1000
typedef struct
{ u32 nbox;
  union
  { int maxlen;                       /* the kernel's bound: box_align's on max(m, n), */
    int maxdiff;                      /* read_align's on the differences of a box */
  };
  const u32 *order;                   /* read_align's: [nbox], the order its workgroups take the boxes in */
  const int *m, *n;                   /* [nbox] */
  const long long *aoff, *boff;       /* [nbox] bytes into bases */
  const long long *coff;              /* [nbox] values into script */
  const u8  *bases;
  int *diffs, *slen;                  /* [nbox] */
  int *script;
} BoxArgs;

void damar_launch_box_align(const BoxArgs *a, hipStream_t st);
u32  damar_box_align_grid(void);      /* workgroups of the largest launch: beyond that many boxes a workgroup does several */

/* read_align.hip: the same alignment for boxes of read length, one workgroup of several wavefronts per box, the bases left
   in global memory and the frontiers sized by the differences.  Box order[i] is the i-th longest.  A box with max(m, n) <=
   DAMAR_READ_MAXLEN and at most maxdiff <= DAMAR_READ_MAXDIFF differences is done and leaves what box_align leaves; a box
   beyond either bound, or one that hits a loop bound, has length -1 and is the host's. */
#define DAMAR_READ_MAXDIFF 8000
#define DAMAR_READ_MAXLEN  (1 << 20)

void damar_launch_read_align(const BoxArgs *a, u32 grid, hipStream_t st);
u32  damar_read_align_grid(void);     /* workgroups of the largest launch: beyond that many boxes a workgroup does several */

/* box_trace.hip: exact alignment of a batch of boxes into trace pairs (align.c:4734 DIFF_TRACE).  Box i is m[i] bases of A
   against n[i] of B, its A side beginning abpos[i] bases into A's grid of tspace.  A box with max(m, n) <= maxlen <=
   DAMAR_TBOX_MAXLEN and no more intervals than the kernel's ledger holds is done and leaves its differences, the number
   of its values (-1: it hit a bound of the kernel and is the host's after all) and the values at trace + toff[box],
   2 * ((abpos % tspace + m + tspace - 1) / tspace) of them; the others are not touched. */
#define DAMAR_TBOX_MAXLEN 4096
typedef struct
{ u32 nbox, nlarge;                   /* nlarge: boxes above what the first launch takes (0: the second is not made) */
  const u32 *large;                   /* [nlarge] which they are */
  int maxlen, tspace;
  const int *m, *n, *abpos;           /* [nbox] */
  const long long *aoff, *boff;       /* [nbox] bytes into bases */
  const long long *toff;              /* [nbox] values into trace */
  const u8  *bases;
  int *diffs, *tlen;                  /* [nbox] */
  u16 *trace;
} TBoxArgs;

void damar_launch_box_trace(const TBoxArgs *a, hipStream_t st);
u32  damar_box_trace_grid(void);      /* workgroups of the largest launch: beyond that many boxes a workgroup does several */
u32  damar_box_trace_small(void);     /* the largest box of the first of the two launches */

/* trace_pts.hip: Compute_Trace_PTS for batches of records (align.c:5577-5692, 4892-5261) */
typedef struct
{ u32 aread, bread;       /* block-local read ids */
  u32 flags;              /* bit 0 = B complemented (COMP_FLAG), bit 1 = A and B are one buffer */
  int abpos, bbpos, aepos, bepos;
  u32 poff;               /* first trace-point value of the record in the point array */
  int tlen;               /* trace-point values (pairs diffs, B length) */
  u32 seg0;               /* index of the record's first segment */
  u32 stage0;             /* first staging slot of the record (segment s gets dmax + |M_s - N_s| slots) */
  int dmax;               /* largest trace-point difference count of the record (align.c:5614-5621) */
  u32 slots;              /* staging slots set aside for the record */
} TraceRecIn;

typedef struct
{ u32 apos, bpos;         /* first base of the segment in the blocks' base arrays (B: last, if complemented) */
  int a0, b0;             /* the same as offsets into the two reads (script values)  */
  u32 mn;                 /* M | N << 16                                             */
  u32 flags;              /* TraceRecIn.flags & 3, bit 2 = void (record failed the bounds check), dmax << 8 */
  u32 stage;              /* slot of the segment in the staging area                 */
  u32 rec;
} TraceSeg;

typedef struct
{ const TraceSeg *segs;
  const u32 *list;  u32 nwork;          /* segment ids to do (NULL = 0 .. nwork-1)     */
  const u8 *abases, *bbases;
  const u32 *apk, *bpk;               /* the same bases at 2 bits (DevBlock.pk)      */
  short *vf;  signed char *hf;  u32 cap; /* per-thread stripes of cap cells             */
  int *stage;  u32 *count;  int *dist;
  int *mid;                             /* kind 1: A and B offset of each segment's mid point */
  u32 *over;  u32 over_cap;  u32 *nover;  u32 *need;  u32 *err;
  u32 *next;                            /* slot kernel: next batch of 64 segments to hand out */
} TraceArgs;

#define DAMAR_TRACE_ERR_POINTS 1u       /* trace point out of bounds (align.c:5575)   */
#define DAMAR_TRACE_ERR_ALIGN  2u       /* bad alignment between trace points (:4890) */
#define DAMAR_TRACE_ERR_INTERNAL 4u      /* staging bound of the mid-point pieces violated */

/* pts: the records' trace points as stored in the .las (tbytes 1 or 2) */
/* key / val: per segment its own difference count (<= 255) and its index, for the work order */
void damar_launch_trace_layout(const TraceRecIn *recs, u32 nrecs, const void *pts, int tbytes, int tspace,
                               const DevBlock *ablk, const DevBlock *bblk, TraceSeg *segs, u32 *key, u32 *val, u32 *err,
                               hipStream_t st);
void damar_launch_trace_waves(const TraceArgs *t, int mode, int kind, u32 nblocks, hipStream_t st);
size_t damar_trace_slot_area_cells(void);
size_t damar_trace_slot_vf_bytes(int mode, int kind);
void damar_launch_trace_waves_slots(const TraceArgs *t, int mode, int kind, u32 nblocks, hipStream_t st);
void damar_launch_trace_gather(const TraceRecIn *recs, u32 nrecs, int mid, const u32 *count, const int *dist, u32 *segoff,
                               u32 *tlen, int *diffs, hipStream_t st);
void damar_launch_trace_mid_layout(const TraceRecIn *recs, u32 nrecs, const TraceSeg *segs, const int *mid,
                                   const DevBlock *ablk, const DevBlock *bblk, TraceSeg *out, u32 *key, u32 *val, u32 *err,
                                   hipStream_t st);
void damar_launch_trace_pack(const TraceSeg *segs, u32 nsegs, const u32 *count, const u32 *segoff, const u32 *recoff,
                             const int *stage, int *script, hipStream_t st);
#endif
