/* damar_graph.h -- the overlap graph of a filtered .las file (touring/OGbuild.c): the session that makes its edges from
 * batches of piles, on the GPU (kernels/graph_edges.hip) or with DAMAR_PILES=host by the plain routine of host/graph.c,
 * and the command around it.  DESIGN.md section 9m.
 */
#ifndef DAMAR_GRAPH_H
#define DAMAR_GRAPH_H

#include "damar_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DAMAR_GRAPH_MAXDEG   1024      /* edges on one side of a read that the per-read kernel holds; more: the host routine */
#define DAMAR_GRAPH_EDGE_INTS   9      /* a b ab ae bb be flags ovh diffs */

#define DAMAR_OG_CONTAINED (1 << 0)    /* a read's status, the reference's bits */
#define DAMAR_OG_WIDOW     (1 << 1)
#define DAMAR_OG_PROPER    (1 << 2)
#define DAMAR_OG_USED      (1 << 3)
#define DAMAR_OG_OPTIONAL  (1 << 4)

/* What the two passes of the reference leave behind before post_build's -c: the lists sorted, without their parallel
   edges, compacted.  Read r's left edges are left[EDGE_INTS * loff[r] .. EDGE_INTS * loff[r + 1]).  All malloc'ed. */
typedef struct
{ int     nreads;
  int64  *loff, *roff;                 /* [nreads + 1] */
  int    *left, *right;
  unsigned char *status;               /* [nreads] */
  int64   cnt_left, cnt_right;         /* the slots the reference's counting pass allots (its "left edges" lines) */
  int64   edges, redges, symdiscard;   /* its three counters */
  int64   parallel, removed;           /* what remove_parallel_edges counts, what the compaction took out */
  int64   neg_rec;                     /* -1, or the first record in file order with a negative overhang */
  int64   nneg;                        /* the host routine alone (so nneg > 0 from damar_og_edges says the device path handed the file
                                          over to it): every such event in the counting pass's order, */
  int64  *neg;                         /*   5 values each: record, overhang, A read, B read, 1 where the building pass gets there */
} damar_graph_result;

typedef struct damar_graph damar_graph;
/* trim: get_trim of every read, {begin, end} pairs */
damar_graph *damar_graph_open(const int *read_len, int nreads, const int *trim);
/* the records of a batch are the records first_rec .. of the file; diffs: their differences */
int  damar_graph_batch(damar_graph *g, const damar_pile_batch *b, const int *diffs, int64 first_rec);
int  damar_graph_finish(damar_graph *g, damar_graph_result *res);
void damar_graph_close(damar_graph *g);
void damar_graph_result_free(damar_graph_result *res);
/* of the last session: ms[4] = upload, pile kernel, finishing kernels, download; cnt[4] = records, candidate edges,
   reads the host routine finished (a side over the limit), edges kept */
void damar_graph_last(double *ms, int64 *cnt);
int  damar_graph_maxdeg(void);         /* DAMAR_GRAPH_MAXDEG, or what the environment lowers it to for a test */

/* the host routine (host/graph.c), the same session without the GPU */
typedef struct damar_host_graph damar_host_graph;
damar_host_graph *damar_host_graph_open(const int *read_len, int nreads, const int *trim);
int  damar_host_graph_batch(damar_host_graph *g, const damar_pile_batch *b, const int *diffs, int64 first_rec);
int  damar_host_graph_finish(damar_host_graph *g, damar_graph_result *res);
void damar_host_graph_close(damar_host_graph *g);
int  damar_graph_inputs_valid(const damar_pile_batch *b, const int *diffs, int nreads);       /* 0 after a message */
/* remove_dupes on both lists of one read and remove_lr_dupes across them, a = b = -1 in the edges that go: what they count */
int64 damar_host_graph_dedupe(int *left, int64 nl, int *right, int64 nr);
/* compress_graph_side: the dropped edges of one kind of list taken out, off[nreads + 1] moved up: how many went */
int64 damar_host_graph_compress(int *edges, int64 *off, int nreads);

/* the command as a call.  0, or the exit status of the reference after its message */
typedef struct
{ int   split, contained;              /* -s -c */
  const char *track, *format, *prio;   /* -t -f -p (NULL: trim, graphml, ovl) */
} damar_og_opts;
int  damar_og_build(const char *db, const char *las, const char *out, const damar_og_opts *o);
/* the edges alone, before -c: the trim track by name */
int  damar_og_edges(const char *db, const char *las, const char *track, damar_graph_result *res);

#ifdef __cplusplus
}
#endif
#endif
