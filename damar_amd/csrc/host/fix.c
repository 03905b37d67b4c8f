/* fix.c -- LAfix (scrub/LAfix.c without its -X chimer code and its -f quality streams) as calls: per pile the missed
 * adapters cut off (the flip step), the breaks and the weak segments of the A read located with the B stretch that
 * replaces each, and the patched read spliced from pieces of A and B and written as FASTA.
 *   - damar_fix_inputs_valid: what both paths index with,
 *   - damar_host_fix_pile: the plain routine for the breaks and the weak segments, the reference's loops as written
 *     (DAMAR_PILES=host, the piles kernels/pile_patch.hip leaves, and the second opinion for that kernel),
 *   - damar_fix_las: the pass over a file -- per batch of whole piles the trim interval, the flip step, damar_pile_patches,
 *     the splice, the -c intervals carried through it, the reads written.
 * Nothing here touches the GPU runtime. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "damar_hip.h"
#include "damar_host.h"

#define FASTA_WIDTH     60                /* LAfix.c:38-43 */
#define MIN_INT_LEN     5
#define MIN_SPAN        400
#define MIN_SPAN_REPEAT 800

static int track_shaped(const uint64 *anno, int64 ndata, int nreads)
{ int r;
  if (anno[0] % 4 || anno[nreads] > 4 * (uint64) ndata)
    return 0;
  for (r = 0; r < nreads; r++)
    if (anno[r] > anno[r + 1] || anno[r + 1] % 4)
      return 0;
  return 1;
}

int damar_fix_inputs_valid(const damar_trace_batch *t, const damar_fix_params *p, const int *trim)
{ const damar_pile_batch *b;
  const char *why = "malformed batch";
  int64 ntiles, i, pi;
  if (t == NULL || p == NULL || !damar_trace_batch_valid(t, &ntiles))
    return 0;
  b = &t->p;
  if (b->npiles > 0 && trim == NULL)
    goto bad;
  if (p->twidth != t->tspace)
    { why = "the trace spacing of the parameters is not the batch's";
      goto bad;
    }
  if (p->q_anno == NULL || p->q_ndata < 0 || (p->q_ndata > 0 && p->q_data == NULL) || !track_shaped(p->q_anno, p->q_ndata, b->nreads))
    { why = "the q track is not ints for the database's reads";
      goto bad;
    }
  for (i = 0; i < p->q_ndata; i++)          /* both paths order the mean q of a stretch as a positive number */
    if (p->q_data[i] < 0)
      { why = "the q track holds a negative value";
        goto bad;
      }
  if (p->rep_anno != NULL)
    { int r;
      why = "the repeat track is not pairs of ints for the database's reads";
      if (p->rep_ndata < 0 || (p->rep_ndata > 0 && p->rep_data == NULL) || !track_shaped(p->rep_anno, p->rep_ndata, b->nreads))
        goto bad;
      for (r = 0; r <= b->nreads; r++)
        if (p->rep_anno[r] % 8)
          goto bad;
    }
  for (pi = 0; pi < b->npiles; pi++)
    { const int aread = b->pile_aread[pi], alen = b->read_len[aread];
      for (i = b->pile_off[pi]; i < b->pile_off[pi + 1]; i++)
        { if (b->bread[i] < 0 || b->bread[i] >= b->nreads)
            { why = "a record's B read is not in the database";
              goto bad;
            }
          if (b->aepos[i] < b->abpos[i] || b->aepos[i] > alen)
            { why = "a record's A coordinates lie outside its read";
              goto bad;
            }
          if (t->tlen[i] < 2 || t->tlen[i] % 2)
            { why = "a record without a whole trace";
              goto bad;
            }
        }
      if (trim[2 * pi] >= trim[2 * pi + 1])
        continue;
      if (trim[2 * pi] < 0 || trim[2 * pi + 1] > alen)
        { why = "a trim interval lies outside its read";
          goto bad;
        }
      if ((int64) ((p->q_anno[aread + 1] - p->q_anno[aread]) / 4) != (alen + t->tspace - 1) / t->tspace)
        { why = "the q track does not hold one value per segment of an A read";
          goto bad;
        }
    }
  return 1;
bad:
  fprintf(stderr, "damar: fix: %s\n", why);
  return 0;
}

/***** the plain routine ************************************************************************/

/* the reference indexes the q track's data flat, base + k with base where a read's values begin: a value outside the data
   (B's segment at be / tw when be is the end of a read of a whole number of segments, as the last read) counts as 0 */
static int q_at(const damar_fix_params *p, int64 base, int64 k)
{ const int64 at = base + k;
  return (at < 0 || at >= p->q_ndata) ? 0 : p->q_data[at];
}

/* getRepeatCount, LAfix.c:285 */
static int repeat_bases(const damar_fix_params *p, int aread, int beg, int end)
{ uint64 rb, re;
  int n = 0;
  if (p->rep_anno == NULL)
    return 0;
  for (rb = p->rep_anno[aread] / 4, re = p->rep_anno[aread + 1] / 4; rb < re; rb += 2)
    { const int lo = beg > p->rep_data[rb] ? beg : p->rep_data[rb], hi = end < p->rep_data[rb + 1] ? end : p->rep_data[rb + 1];
      if (lo < hi)
        n += hi - lo;
    }
  return n;
}

typedef struct
{ const damar_trace_batch *t;
  const damar_pile_batch  *b;
  int64 lo;
  int   n, aread;
} Pile;

#define AB(i) (pl->b->abpos[pl->lo + (i)])
#define AE(i) (pl->b->aepos[pl->lo + (i)])
#define BB(i) (pl->b->bbpos[pl->lo + (i)])
#define BE(i) (pl->b->bepos[pl->lo + (i)])
#define BR(i) (pl->b->bread[pl->lo + (i)])
#define FL(i) (pl->b->flags[pl->lo + (i)])
#define TL(i) (pl->t->tlen[pl->lo + (i)])
#define TR(i, k) damar_trace_value(pl->t, pl->lo + (i), (k))

/* spanners_point, LAfix.c:1413: the reference stops counting beyond max, which changes nothing of the answer */
static int point_spanned(const Pile *pl, const damar_fix_params *p, int pt)
{ const int min_span = repeat_bases(p, pl->aread, pt, pt + 1) ? MIN_SPAN_REPEAT : MIN_SPAN;
  int span = 0, i;
  for (i = 0; i < pl->n; i++)
    if (AB(i) < pt - min_span && AE(i) > pt + min_span)
      span += 1;
  return span > p->maxspanners;
}

static int gap_before(const damar_fix_gap *x, const damar_fix_gap *y)      /* cmp_gaps, LAfix.c:252 */
{ if (x->ab != y->ab) return x->ab < y->ab;
  if (x->ae != y->ae) return x->ae < y->ae;
  return x->diff < y->diff;
}

/* a stable sort, as the merge sort behind the reference's qsort is: equal candidates stay in the order they were found */
static void sort_gaps(damar_fix_gap *g, int64 n)
{ int64 i, j;
  for (i = 1; i < n; i++)
    { const damar_fix_gap x = g[i];
      for (j = i; j > 0 && gap_before(&x, &g[j - 1]); j--)
        g[j] = g[j - 1];
      g[j] = x;
    }
}

static damar_fix_gap *next_gap(damar_fix_list *L)
{ if (L->n >= L->cap)
    { L->cap = L->cap + L->cap / 4 + 256;
      L->g = (damar_fix_gap *) damar_grow(L->g, sizeof(damar_fix_gap) * (size_t) L->cap, "fix");
    }
  return L->g + L->n++;
}

/* fix_process from "locate breaks in A" to the second sort, LAfix.c:1896-2402 */
void damar_host_fix_pile(const damar_trace_batch *t, int64 pile, const damar_fix_params *p, int trim_ab, int trim_ae, damar_fix_list *L)
{ Pile  P, *pl = &P;
  const int tw = t->tspace;
  const int64 first = L->n;
  damar_fix_gap *d;
  int64 qa, dcur, i, j;
  int   nsegs, seg_first, seg_last, s;

  P.t = t;
  P.b = &t->p;
  P.lo = t->p.pile_off[pile];
  P.n = (int) (t->p.pile_off[pile + 1] - P.lo);
  P.aread = t->p.pile_aread[pile];
  if (trim_ab >= trim_ae)
    return;
  qa = (int64) (p->q_anno[P.aread] / 4);
  nsegs = (t->p.read_len[P.aread] + tw - 1) / tw;

  /* the breaks: LAfix.c:1898-2031 */
  for (s = 1; s < P.n; s++)
    { int ab, ae, bb, be, beg, end, q = 0, weak = 0, scored = 0, k;
      int64 qb;
      if (BR(s - 1) != BR(s) || AE(s - 1) >= AB(s) || ((FL(s - 1) ^ FL(s)) & OVL_COMP))
        continue;
      ab = (AE(s - 1) - 1) / tw;
      ae = AB(s) / tw + 1;
      bb = BE(s - 1) - TR(s - 1, TL(s - 1) - 1);
      be = BB(s) + TR(s, 1);
      if (bb >= be)
        continue;
      if (FL(s) & OVL_COMP)
        { const int blen = t->p.read_len[BR(s)], was = bb;
          bb = blen - be;
          be = blen - was;
        }
      qb = (int64) (p->q_anno[BR(s)] / 4);
      beg = bb / tw;
      end = be / tw + 1;
      for (k = beg; k < end; k++)
        { const int v = q_at(p, qb, k);
          if (v == 0)
            weak = 1;
          q += v;
        }
      if (weak)
        continue;
      if (point_spanned(pl, p, ab * tw) && point_spanned(pl, p, ae * tw))
        continue;
      for (k = ab + 1; k < ae - 1; k++)
        if (q_at(p, qa, k) != 0)
          scored += 1;
      if (scored > 1)
        continue;
      if ((ae - ab) * tw * 10 < be - bb)
        continue;
      d = next_gap(L);
      d->ab = ab * tw;  d->ae = ae * tw;  d->bb = bb;  d->be = be;
      d->b = BR(s);  d->support = 1;  d->comp = FL(s) & OVL_COMP;
      d->diff = (int) (tw * 1.0 * q / (be - bb));
    }
  d = L->g + first;
  dcur = L->n - first;
  sort_gaps(d, dcur);

  /* breaks at one place in A merged, LAfix.c:2039-2065 */
  for (i = 0; i < dcur; i++)
    { if (d[i].support == -1)
        continue;
      if (p->maxgap != -1 && (d[i].ae - d[i].ab >= p->maxgap || abs(d[i].be - d[i].bb) >= p->maxgap))
        { d[i].support = -1;
          continue;
        }
      for (j = i + 1; j < dcur && d[i].ab == d[j].ab && d[i].ae == d[j].ae; j++)
        { if (d[j].support == -1)
            continue;
          if (abs((d[j].be - d[j].bb) - (d[i].be - d[i].bb)) < 50)
            { d[i].support += 1;
              d[j].support = -1;
            }
        }
    }
  /* breaks that intersect merged, LAfix.c:2069-2096 */
  for (i = 0; i < dcur; i++)
    { if (d[i].support == -1)
        continue;
      for (j = i + 1; j < dcur && d[i].ae > d[j].ab && d[i].ab < d[j].ae; j++)
        { if (d[j].support == -1)
            continue;
          if (d[i].support > d[j].support)
            { d[i].support += d[j].support;
              d[j].support = -1;
            }
          else
            { d[j].support += d[i].support;
              d[i].support = -1;
              break;
            }
        }
    }
  /* breaks with too little support or without a bad segment in A dropped, LAfix.c:2110-2138 */
  for (i = 0, j = 0; i < dcur; i++)
    { int bad = 0, k;
      if (d[i].support < p->minsupport)
        continue;
      for (k = d[i].ab / tw; k < d[i].ae / tw; k++)
        { const int v = q_at(p, qa, k);
          if (v == 0 || v >= p->lowq)
            { bad = 1;
              break;
            }
        }
      if (bad)
        d[j++] = d[i];
    }
  dcur = j;
  L->n = first + dcur;

  /* the weak segments, LAfix.c:2142-2314; the two loops are held to the read's segments (the reference runs on) */
  seg_first = trim_ab / tw;
  seg_last = trim_ae / tw;
  while (seg_first < nsegs && q_at(p, qa, seg_first) == 0)
    seg_first += 1;
  while (seg_last > 0 && q_at(p, qa, seg_last - 1) == 0)
    seg_last -= 1;
  for (s = seg_first; s < seg_last; s++)
    { const int v = q_at(p, qa, s), ab = s * tw, ae = (s + 1) * tw;
      int   inside = 0, border = 0, best = -1, best_bb = 0, best_be = 0, r;
      float q_min = 0;
      if (v != 0 && v < p->lowq)
        continue;
      d = L->g + first;
      for (j = 0; j < dcur; j++)
        if (d[j].support != -1 && d[j].ab <= ab && d[j].ae >= ae)
          { inside = 1;
            break;
          }
      if (inside)
        continue;
      for (r = 0; r < P.n; r++)
        { if (AB(r) + tw <= ab && AE(r) - tw >= ae)
            { int bb = -1, be = BB(r), apos = AB(r), k = 0, beg, end, q = 0;
              int64 qb;
              float q_new;
              while (apos <= ab && k + 1 < TL(r))
                { apos = (apos / tw + 1) * tw;
                  bb = be;
                  be += TR(r, k + 1);
                  k += 2;
                }
              if (FL(r) & OVL_COMP)
                { const int blen = t->p.read_len[BR(r)], was = bb;
                  bb = blen - be;
                  be = blen - was;
                }
              qb = (int64) (p->q_anno[BR(r)] / 4);
              beg = bb / tw;
              end = be / tw;
              for (k = beg; k < end; k++)
                { const int w = q_at(p, qb, k);
                  if (w == 0)
                    { q = 0;
                      break;
                    }
                  q += w;
                }
              if (q == 0)
                continue;
              q_new = (float) (1.0 * q / (end - beg));
              if (best == -1 || q_new < q_min)
                { best_bb = bb;  best_be = be;  q_min = q_new;  best = r; }
            }
          if ((AB(r) >= ab && AB(r) <= ae) || (AE(r) >= ab && AE(r) <= ae))
            border += 1;
        }
      if (best == -1)
        continue;
      d = next_gap(L);
      d->ab = ab;  d->ae = ae;  d->bb = best_bb;  d->be = best_be;
      d->b = BR(best);  d->support = border;  d->comp = FL(best) & OVL_COMP;
      d->diff = (int) q_min;
      dcur += 1;
    }
  sort_gaps(L->g + first, dcur);
}

/***** the flip step ****************************************************************************/

typedef struct
{ const uint64 *anno;          /* NULL: no track */
  const int    *data;
} Track;

/* get_trim, lib/utils.c:258; 1: the read's entry is not an interval.  (trim.c's trim_of is another rule: there such an
   entry keeps nothing, and the track is never missing.) */
static int trim_of(const Track *tt, int alen, int rid, int *b, int *e)
{ if (tt->anno == NULL)
    { *b = 0;
      *e = alen;
      return 0;
    }
  { const uint64 ob = tt->anno[rid] / 4, oe = tt->anno[rid + 1] / 4;
    *b = *e = 0;
    if (ob == oe)
      return 0;
    if (oe - ob != 2)
      return 1;
    if (tt->data[ob] < tt->data[ob + 1])
      { *b = tt->data[ob];
        *e = tt->data[ob + 1];
      }
  }
  return 0;
}

/* spanners_interval, LAfix.c:1378: tb, te are the track's interval, not what the flips have made of it so far */
static int interval_spanners(const Pile *pl, const damar_fix_params *p, int tb, int te, int b, int e)
{ const int min_span = (e - b - repeat_bases(p, pl->aread, b, e) < 100) ? MIN_SPAN_REPEAT : MIN_SPAN;
  const int lo = tb > b - min_span ? tb : b - min_span, hi = te < e + min_span ? te : e + min_span;
  int span = 0, i;
  for (i = 0; i < pl->n; i++)
    if (AB(i) <= lo && AE(i) >= hi)
      span += 1;
  return span;
}

/* filter_flips, LAfix.c:1633: a complement overlap of the read with itself that crosses the anti-diagonal, or two of them
   with a gap between, show an adapter that was missed; the read is cut there, the longer side kept */
static int cut_flips(const Pile *pl, const damar_fix_params *p, int tb, int te, int *trim_b, int *trim_e)
{ const int tw = pl->t->tspace, alen = pl->b->read_len[pl->aread];
  int self_c = 0, b = -1, e = -1, cut = 0, i, j;
  for (i = 0; i < pl->n; i++)
    { if (pl->aread < BR(i))
        { if (b != -1)
            e = i;
          break;
        }
      if (pl->aread == BR(i))
        { if (b == -1)
            b = i;
          if (FL(i) & OVL_COMP)
            self_c += 1;
        }
    }
  if (self_c == 0)
    return 0;
  for (i = b; i < e; i++)
    { int sab, sae, sbb, sbe;
      if (!(FL(i) & OVL_COMP) || !damar_intersect(AB(i), AE(i), alen - BE(i), alen - BB(i)))
        continue;
      sab = AB(i);
      sae = (sab / tw + 1) * tw;
      sbb = BB(i);
      sbe = sbb + TR(i, 1);
      for (j = 2; j < TL(i) - 2; j += 2)
        { if (damar_intersect(sab, sae + 1, alen - sbe, alen - sbb - 1) && interval_spanners(pl, p, tb, te, sab, sae) <= 1)
            { printf("%8d CROSS @ %5d..%5d x %5d..%5d\n", pl->aread, sab, sae, alen - sbe, alen - sbb);
              cut = 1;
              if (*trim_b < sab && sae < *trim_e)
                { if (sab - *trim_b < *trim_e - sae)
                    *trim_b = sae;
                  else
                    *trim_e = sab;
                }
            }
          sab = sae;
          sae += tw;
          sbb = sbe;
          sbe += TR(i, j + 1);
        }
    }
  for (i = b; i < e - 1; i++)
    { int ab, ae, ab_c, ae_c;
      if (!(FL(i) & OVL_COMP) || !(FL(i + 1) & OVL_COMP))
        continue;
      ab = AE(i);
      ae = AB(i + 1);
      ab_c = alen - BB(i + 1);
      ae_c = alen - BE(i);
      if (damar_intersect(ab, ae, ab_c, ae_c) && interval_spanners(pl, p, tb, te, ab, ae) <= 1)
        { const int mid = (ab + ae) / 2;
          printf("%8d GAP   @ %5d..%5d x %5d..%5d\n", pl->aread, ab, ae, ab_c, ae_c);
          cut = 1;
          if (*trim_b < mid && mid < *trim_e)
            { if (mid - *trim_b < *trim_e - mid)
                *trim_b = mid;
              else
                *trim_e = mid;
            }
        }
    }
  return cut;
}

/***** the pass over a file *********************************************************************/

/* wrap_write, lib/utils.c:170.  A replaced stretch can hold a zero byte (see b_piece), and a line ends at one. */
static void write_wrapped(FILE *f, const char *seq, int len)
{ int j;
  for (j = 0; j + FASTA_WIDTH < len; j += FASTA_WIDTH)
    fprintf(f, "%.*s\n", FASTA_WIDTH, seq + j);
  if (j < len)
    fprintf(f, "%.*s\n", len - j, seq + j);
}

static void a_piece(const HITS_DB *blk, int r, int from, int to, char *dst)
{ const char *s = (const char *) blk->bases + blk->reads[r].boff;
  int i;
  for (i = from; i < to; i++)
    *dst++ = "acgt"[(int) s[i] & 3];
}

/* B's bases [bb, be) as the reference splices them in.  Its complement routine turns the be - bb + 1 bases from bb around,
   one more than the stretch, and the first be - bb of the result are copied: the complement of B[be] down to B[bb + 1].
   B[blen] is the zero byte that ends a loaded read, and stays one. */
static void b_piece(const HITS_DB *blk, int r, int comp, int bb, int be, char *dst)
{ const char *s = (const char *) blk->bases + blk->reads[r].boff;
  const int   blen = blk->reads[r].rlen;
  int i;
  if (!comp)
    for (i = bb; i < be; i++)
      *dst++ = (i < 0 || i >= blen) ? 0 : "acgt"[(int) s[i] & 3];
  else
    for (i = be; i > bb; i--)
      *dst++ = (i < 0 || i >= blen) ? 0 : "tgca"[(int) s[i] & 3];
}

typedef struct
{ const char *name;
  uint64 *anno;
  int    *data;
  int64   ndata;
} Named;

/* the -c intervals of a read that had no repair, cut to the trim: LAfix.c:2326-2377 */
static void tracks_trimmed(FILE *fo, const Named *cv, int ncv, int aread, int trim_ab, int trim_ae)
{ int i;
  for (i = 0; i < ncv; i++)
    { uint64 ob = cv[i].anno[aread] / 4;
      const uint64 oe = cv[i].anno[aread + 1] / 4;
      int first = 1;
      for (; ob < oe; ob += 2)
        { int beg = cv[i].data[ob] - trim_ab, end = cv[i].data[ob + 1] - trim_ab;
          if (end < 0)
            continue;
          if (beg < 0)
            beg = 0;
          if (beg > trim_ae - trim_ab)
            break;
          if (end > trim_ae - trim_ab)
            end = trim_ae - trim_ab;
          fprintf(fo, first ? " %s=" : ",", cv[i].name);
          fprintf(fo, "%d,%d", beg, end);
          first = 0;
        }
    }
}

/* the -c intervals carried through the pieces of A that were kept, ap = {begin, end, where in the new read} per piece:
   LAfix.c:2581-2680.  1 after the reference's message. */
static int tracks_patched(FILE *fo, const Named *cv, int ncv, int aread, const int *ap, int nap, int rlen)
{ int i, j;
  for (i = 0; i < ncv; i++)
    { uint64 ob = cv[i].anno[aread] / 4;
      const uint64 oe = cv[i].anno[aread + 1] / 4;
      int first = 1;
      for (; ob < oe; ob += 2)
        { const int ib = cv[i].data[ob], ie = cv[i].data[ob + 1];
          int ib_adj = -1, ie_adj = -1;
          if (nap == 0 || ie < ap[0] || ib > ap[nap - 2])
            continue;
          for (j = 0; j < nap; j += 3)
            { if (ib_adj == -1 && ib < ap[j + 1])
                ib_adj = ap[j + 2] + ((ib > ap[j] ? ib : ap[j]) - ap[j]);
              if (ie_adj == -1 && ie <= ap[j + 1])
                { if (ie < ap[j] && j > 0)
                    { ie_adj = ap[j - 1] + (ap[j - 2] - ap[j - 3]);
                      break;
                    }
                  else if (ie > ap[j])
                    { ie_adj = ap[j + 2] + (ie - ap[j]);
                      break;
                    }
                }
            }
          if (ie_adj - ib_adj <= MIN_INT_LEN)
            continue;
          fprintf(fo, first ? " %s=" : ",", cv[i].name);
          if (ib_adj < 0 || ib_adj > rlen || ib_adj > ie_adj || ie_adj > rlen)
            { fprintf(stderr, "adjust interval %d..%d outside read length %d\n", ib_adj, ie_adj, rlen);
              return 1;
            }
          fprintf(fo, "%d,%d", ib_adj, ie_adj);
          first = 0;
        }
    }
  return 0;
}

static int load_named(const damar_dbinfo *db, const char *name, Named *t)
{ t->name = name;
  return damar_track_read_any(db, name, &t->anno, &t->data, &t->ndata);
}

int damar_fix_las(const char *dbname, const char *las, const char *fasta, const damar_fix_opts *o, damar_fix_stats *st)
{ damar_dbinfo db;
  damar_pile_reader *r = NULL;
  damar_trace_batch  t;
  damar_fix_params   p;
  damar_fix_gaps     out;
  HITS_DB blk;
  Named   q, tr, rep, *cv = NULL;
  Track   tt;
  FILE   *fo = NULL, *ft = NULL;
  char   *seq = NULL;
  int    *trim = NULL, *count = NULL, *ap = NULL;
  int64   tcap = 0, scap = 0, apcap = 0, pi;
  int     got, rc = 1, have_db = 0, have_blk = 0, i, ncv = 0;

  memset(st, 0, sizeof(*st));
  memset(&q, 0, sizeof(q));  memset(&tr, 0, sizeof(tr));  memset(&rep, 0, sizeof(rep));  memset(&out, 0, sizeof(out));
  memset(&p, 0, sizeof(p));
  if ((fo = fopen(fasta, "w")) == NULL)
    { fprintf(stderr, "could not open '%s'\n", fasta);
      return 1;
    }
  if (o->trim_out != NULL && (ft = fopen(o->trim_out, "w")) == NULL)
    { fprintf(stderr, "error: could not open '%s'\n", o->trim_out);
      goto done;
    }
  if (damar_dbinfo_open(dbname, &db))
    { fprintf(stderr, "could not open database '%s'\n", dbname);
      goto done;
    }
  have_db = 1;
  cv = (Named *) calloc((size_t) o->nconvert + 1, sizeof(Named));
  if (cv == NULL)
    goto done;
  for (i = 0; i < o->nconvert; i++, ncv++)
    if (load_named(&db, o->convert[i], &cv[i]))
      { fprintf(stderr, "(null): Track '%s' does not exist\n", o->convert[i]);
        fprintf(stderr, "could not open track '%s'\n", o->convert[i]);
        goto done;
      }
  if ((r = damar_piles_open_traces(las, 0, 0)) == NULL)
    goto done;
  printf(GREEN "PASS fix" RESET "\n");
  { const char *names[3] = { o->q_track, o->trim_track, o->rep_track };
    Named *into[3] = { &q, &tr, &rep };
    for (i = 0; i < 3; i++)
      if (names[i] != NULL && load_named(&db, names[i], into[i]))
        { fprintf(stderr, "(null): Track '%s' does not exist\n", names[i]);
          fprintf(stderr, "failed to open track %s\n", names[i]);
          goto done;
        }
  }
  if (damar_read_block(dbname, &blk))
    goto done;
  have_blk = 1;
  p.q_anno = q.anno;  p.q_data = q.data;  p.q_ndata = q.ndata;
  p.rep_anno = rep.anno;  p.rep_data = rep.data;  p.rep_ndata = rep.ndata;
  p.lowq = o->lowq;  p.maxgap = o->maxgap;
  p.maxspanners = o->low_coverage ? 3 : 7;
  p.minsupport = o->low_coverage ? 2 : 4;
  p.twidth = damar_piles_tspace(r);
  tt.anno = tr.anno;  tt.data = tr.data;

  while ((got = damar_piles_next_traces(r, &t)) > 0)
    { damar_pile_batch *b = &t.p;
      const damar_fix_gap *g;
      double ms[4];
      int64  c3[3], npiles;
      int    stop = 0;         /* 1: a read failed the reference's checks; the piles before it are still written */
      char   msg[256];

      msg[0] = 0;
      if (damar_batch_bind(b, &db, las, DAMAR_BIND_A))
        goto done;
      if (damar_room(&tcap, b->npiles, 1024))
        { trim = (int *) damar_grow(trim, sizeof(int) * 2 * (size_t) tcap, "fix");
          count = (int *) damar_grow(count, sizeof(int) * (size_t) tcap, "fix");
        }
      /* per pile the trim interval, the flip step, the -T line and the reference's two checks: LAfix.c:1817-1894.  A pile
         that is skipped has an empty interval from here on. */
      for (pi = 0; pi < b->npiles && !stop; pi++)
        { Pile P;
          const int aread = b->pile_aread[pi], alen = db.read_len[aread];
          int tb, te, fb, fe, nq;
          P.t = &t;  P.b = b;  P.lo = b->pile_off[pi];  P.n = (int) (b->pile_off[pi + 1] - P.lo);  P.aread = aread;
          trim[2 * pi] = trim[2 * pi + 1] = -1;
          if (trim_of(&tt, alen, aread, &tb, &te))
            { fprintf(stderr, "damar: fix: track %s holds more than an interval for read %d\n", o->trim_track, aread);
              goto done;
            }
          if (tb >= te)
            continue;
          fb = tb;
          fe = te;
          for (i = 0; i < P.n; i++)
            if (b->bread[P.lo + i] < 0 || b->bread[P.lo + i] >= db.nreads || t.tlen[P.lo + i] < 2)
              { fprintf(stderr, "damar: %s holds a record this database or this tool cannot take\n", las);
                goto done;
              }
          if (cut_flips(&P, &p, tb, te, &fb, &fe))
            st->flips += 1;
          tb = fb > tb ? fb : tb;
          te = fe < te ? fe : te;
          if (te - tb < o->min_len)
            { printf("skip read %d len %d < min Len %d due to missed adapter\n", aread, te - tb, o->min_len);
              continue;
            }
          if (ft != NULL)
            fprintf(ft, "%d %d %d\n", aread, tb, te);
          nq = (int) ((q.anno[aread + 1] / 4) - (q.anno[aread] / 4));
          if (nq != (alen + p.twidth - 1) / p.twidth)
            { snprintf(msg, sizeof(msg), "read %d expected %d Q track entries, found %d\n", aread, (alen + p.twidth - 1) / p.twidth, nq);
              stop = 1;
            }
          else if (tb < 0 || tb > alen || tb > te || te > alen)
            { snprintf(msg, sizeof(msg), "trim interval %d..%d outside read length %d\n", tb, te, alen);
              stop = 1;
            }
          else
            { trim[2 * pi] = tb;
              trim[2 * pi + 1] = te;
            }
        }
      npiles = b->npiles;
      if (stop)
        { b->npiles = pi - 1;
          b->nrec = b->pile_off[b->npiles];
        }
      out.count = count;
      out.gaps = NULL;
      if (damar_pile_patches(&t, &p, trim, &out))
        goto done;
      damar_fix_last(ms, c3);
      st->piles += c3[0];  st->host_piles += c3[1];  st->repairs += c3[2];

      for (pi = 0, g = out.gaps; pi < b->npiles; g += count[pi], pi++)
        { const int aread = b->pile_aread[pi], tb = trim[2 * pi], te = trim[2 * pi + 1], n = count[pi];
          /* the pieces of A are taken in ascending order and may begin left of the trim (a break there moves the start to its
             end), so they hold the read's length at the most; the reference sizes its buffer the same way */
          int rlen = 0, nap = 0, ab = tb, ae, need = db.read_len[aread] + 8, k;
          if (tb >= te)
            continue;
          if (n == 0)
            { if (te - tb < o->min_len)
                continue;
              fprintf(fo, ">trimmed_%d source=%d", aread, aread);
              tracks_trimmed(fo, cv, ncv, aread, tb, te);
              fprintf(fo, "\n");
              seq = (char *) damar_reserve(seq, &scap, need, 1, 0, "fix");
              a_piece(&blk, aread, tb, te, seq);
              write_wrapped(fo, seq, te - tb);
              st->reads_trimmed += 1;
              continue;
            }
          for (k = 0; k < n; k++)
            need += abs(g[k].be - g[k].bb) + 1;
          seq = (char *) damar_reserve(seq, &scap, need, 1, 0, "fix");
          if (3 * ((int64) n + 1) > apcap)
            { apcap = 3 * ((int64) n + 1) + 64;
              ap = (int *) damar_grow(ap, sizeof(int) * (size_t) apcap, "fix");
            }
          /* the new read from pieces of A and B: LAfix.c:2440-2560 */
          for (k = 0; k < n; k++)
            { if (tb > g[k].ab)
                { ab = g[k].ae;
                  continue;
                }
              if (te < g[k].ae)
                break;
              ae = g[k].ab;
              if (tb < ae && tb > ab)
                ab = tb;
              if (ab > ae || g[k].bb > g[k].be)
                { fprintf(stderr, "damar: fix: the repairs of read %d run into each other\n", aread);
                  goto done;
                }
              if (ab < ae)
                { ap[nap] = ab;  ap[nap + 1] = ae;  ap[nap + 2] = rlen;
                  nap += 3;
                  a_piece(&blk, aread, ab, ae, seq + rlen);
                  rlen += ae - ab;
                }
              ab = g[k].ae;
              st->gaps += 1;
              st->bases_before += g[k].ae - g[k].ab;
              st->bases_after += g[k].be - g[k].bb;
              b_piece(&blk, g[k].b, g[k].comp, g[k].bb, g[k].be, seq + rlen);
              rlen += g[k].be - g[k].bb;
            }
          ae = te;
          if (ab < ae)
            { ap[nap] = ab;  ap[nap + 1] = ae;  ap[nap + 2] = rlen;
              nap += 3;
              a_piece(&blk, aread, ab, ae, seq + rlen);
              rlen += ae - ab;
            }
          if (rlen < o->min_len)
            continue;
          fprintf(fo, ">fixed_%d source=%d", aread, aread);
          if (tracks_patched(fo, cv, ncv, aread, ap, nap, rlen))
            { free(out.gaps);
              out.gaps = NULL;
              goto done;
            }
          fprintf(fo, "\n");
          write_wrapped(fo, seq, rlen);
          st->reads_fixed += 1;
        }
      free(out.gaps);
      out.gaps = NULL;
      b->npiles = npiles;
      if (stop)
        { fputs(msg, stderr);
          goto done;
        }
    }
  if (got < 0)
    goto done;
  /* fix_post, LAfix.c:216; the %' flag of its last line groups nothing in the C locale */
  printf("gaps:    %5d\n", (int) st->gaps);
  printf("flips:   %5d\n", (int) st->flips);
  printf("chimers: %5d\n", (int) st->chimers);
  printf("replaced %llu with %llu bases\n", (unsigned long long) st->bases_before, (unsigned long long) st->bases_after);
  rc = 0;
done:
  if (fo != NULL && fclose(fo) != 0 && rc == 0)
    rc = damar_cannot_write(fasta);
  if (ft != NULL) fclose(ft);
  fflush(stdout);
  damar_piles_close(r);
  if (have_blk) damar_close_block(&blk);
  if (have_db) damar_dbinfo_close(&db);
  for (i = 0; i < ncv; i++)
    { free(cv[i].anno);  free(cv[i].data); }
  free(cv);
  free(q.anno);  free(q.data);  free(tr.anno);  free(tr.data);  free(rep.anno);  free(rep.data);
  free(trim);  free(count);  free(ap);  free(seq);
  return rc;
}
