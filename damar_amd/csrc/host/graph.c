/* graph.c -- OGbuild (touring/OGbuild.c) as calls: the overlap graph of a filtered .las file.
 *   - damar_host_graph_*: the plain routine (DAMAR_PILES=host; the second opinion for kernels/graph_edges.hip, and what
 *     finishes a read with more edges on a side than the kernel holds).  One pass: the candidate edges are kept in file
 *     order and settled when the symmetric discards of the whole file are known,
 *   - -c, -s and the three writers, on the compacted graph either path returns,
 *   - damar_og_build: the command; damar_og_edges: the edges alone.
 * Nothing here touches the GPU runtime. */
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "damar_graph.h"
#include "damar_host.h"

#define EI DAMAR_GRAPH_EDGE_INTS
#define OVL_OPTIONAL (1 << 19)            /* lib/oflags.h */
enum { E_A, E_B, E_AB, E_AE, E_BB, E_BE, E_FLAGS, E_OVH, E_DIFFS };

int damar_graph_inputs_valid(const damar_pile_batch *b, const int *diffs, int nreads)
{ int64 i;
  if (b == NULL || b->npiles < 0 || b->nrec < 0 || b->nrec > 0x7fffffff || (b->nrec > 0 && diffs == NULL))
    goto bad;
  if (b->npiles == 0 ? b->nrec != 0 : (b->pile_off[0] != 0 || b->pile_off[b->npiles] != b->nrec))
    goto bad;
  for (i = 0; i < b->npiles; i++)
    if (b->pile_off[i] > b->pile_off[i + 1] || b->pile_aread[i] < 0 || b->pile_aread[i] >= nreads)
      goto bad;
  for (i = 0; i < b->nrec; i++)
    if (b->bread[i] < 0 || b->bread[i] >= nreads)
      goto bad;
  return 1;
bad:
  fprintf(stderr, "damar: graph: malformed batch, or a read that is not in the database\n");
  return 0;
}

/***** the plain routine ************************************************************************/

typedef struct
{ int   e[EI];
  int   owner, right, slot, live;      /* whose list, which one; 0/2: A's own edge, 1/3: the mirrored one */
  int   ra, rb;                        /* the record's reads: what the symmetric discards are asked for */
} Cand;

struct damar_host_graph
{ int    nreads;
  const int *rlen, *trim;
  unsigned char *contained, *hasfirst;
  int   *minfirst;                     /* the smallest B read among a pile's OVL_SYMDISCARD records */
  Cand  *cand;   int64 ncand, ccap;
  int   *probe;  int64 nprobe, pcap;   /* (A, B) of every record the building pass asks the discards for */
  int64 *neg;    int64 nneg, ncap;
  int   *flags;  int64 fcap;
  int64  nrec;
};

damar_host_graph *damar_host_graph_open(const int *read_len, int nreads, const int *trim)
{ damar_host_graph *g = (damar_host_graph *) calloc(1, sizeof(*g));
  int r;
  if (g == NULL)
    return NULL;
  g->nreads = nreads;  g->rlen = read_len;  g->trim = trim;
  g->contained = (unsigned char *) calloc((size_t) nreads + 1, 1);
  g->hasfirst  = (unsigned char *) calloc((size_t) nreads + 1, 1);
  if (g->contained == NULL || g->hasfirst == NULL)
    { damar_host_graph_close(g);
      return NULL;
    }
  g->minfirst  = (int *) damar_grow(NULL, sizeof(int) * ((size_t) nreads + 1), "graph");
  for (r = 0; r < nreads; r++)
    g->minfirst[r] = INT_MAX;
  return g;
}

void damar_host_graph_close(damar_host_graph *g)
{ if (g == NULL)
    return;
  free(g->contained);  free(g->hasfirst);  free(g->minfirst);  free(g->cand);  free(g->probe);  free(g->neg);  free(g->flags);
  free(g);
}

/* drop_parallel_edges (OGbuild.c:1262-1301): every live record of a run of one B read that holds more than one; a run whose
   first record is discarded already is entered one record later */
static void drop_parallel(const int *bread, int *flags, int64 n)
{ int64 i = 0;
  while (i < n - 1)
    { int64 j = i + 1;
      int   more = 0;
      if (flags[i] & OVL_DISCARD)
        { i += 1;
          continue;
        }
      for ( ; j < n && bread[j] == bread[i]; j++)
        if (!(flags[j] & OVL_DISCARD))
          { flags[j] |= OVL_DISCARD;
            more = 1;
          }
      if (more)
        flags[i] |= OVL_DISCARD;
      i = j;
    }
}

static Cand *new_cand(damar_host_graph *g)
{ g->cand = (Cand *) damar_reserve(g->cand, &g->ccap, g->ncand + 1, sizeof(Cand), 1024, "graph");
  return g->cand + g->ncand++;
}

static void neg_event(damar_host_graph *g, int64 rec, int ovh, int a, int b, int live)
{ g->neg = (int64 *) damar_reserve(g->neg, &g->ncap, 5 * (g->nneg + 1), sizeof(int64), 64, "graph");
  g->neg[5 * g->nneg] = rec;  g->neg[5 * g->nneg + 1] = ovh;  g->neg[5 * g->nneg + 2] = a;  g->neg[5 * g->nneg + 3] = b;
  g->neg[5 * g->nneg + 4] = live;
  g->nneg += 1;
}

/* A's own edge (assign_edge) and the mirrored one (assign_edge_reversed) of record i */
static void edge_of(Cand *c, const damar_pile_batch *b, const int *diffs, int64 i, int a, int flags, int mirrored, int alen, int blen, int ovh)
{ int *e = c->e;
  e[E_FLAGS] = flags;  e[E_DIFFS] = diffs[i] & 0xffff;  e[E_OVH] = ovh;
  if (!mirrored)
    { e[E_A] = a;  e[E_B] = b->bread[i];
      e[E_AB] = b->abpos[i];  e[E_AE] = b->aepos[i];  e[E_BB] = b->bbpos[i];  e[E_BE] = b->bepos[i];
    }
  else
    { e[E_A] = b->bread[i];  e[E_B] = a;
      if (flags & OVL_COMP)
        { e[E_AB] = blen - b->bepos[i];  e[E_AE] = blen - b->bbpos[i];
          e[E_BB] = alen - b->aepos[i];  e[E_BE] = alen - b->abpos[i];
        }
      else
        { e[E_AB] = b->bbpos[i];  e[E_AE] = b->bepos[i];  e[E_BB] = b->abpos[i];  e[E_BE] = b->aepos[i]; }
    }
}

/* handler_count and handler_build (OGbuild.c:1345-1719) on one pile, without the symmetric discards of the file */
static void host_pile(damar_host_graph *g, const damar_pile_batch *b, const int *diffs, int64 pile, int64 first_rec)
{ const int64 lo = b->pile_off[pile], hi = b->pile_off[pile + 1];
  const int a = b->pile_aread[pile], alen = g->rlen[a], tab = g->trim[2 * a], tae = g->trim[2 * a + 1];
  int64 i;
  g->flags = (int *) damar_reserve(g->flags, &g->fcap, hi - lo + 1, sizeof(int), 256, "graph");
  memcpy(g->flags, b->flags + lo, sizeof(int) * (size_t) (hi - lo));
  drop_parallel(b->bread + lo, g->flags, hi - lo);
  for (i = lo; i < hi; i++)
    { const int br = b->bread[i], flags = g->flags[i - lo], blen = g->rlen[br];
      const int ab = b->abpos[i], ae = b->aepos[i], bb = b->bbpos[i], be = b->bepos[i];
      int tbb = g->trim[2 * br], tbe = g->trim[2 * br + 1], live, k;
      Cand *c;
      if (a == br)
        continue;
      if (flags & OVL_SYMDISCARD)
        { if (br < g->minfirst[a]) g->minfirst[a] = br;
          g->hasfirst[br] = 1;
        }
      if (ab == tab && ae == tae)
        { g->contained[a] = 1;
          continue;
        }
      if (flags & OVL_COMP)
        { const int t = tbb;
          tbb = blen - tbe;
          tbe = blen - t;
        }
      if (bb == tbb && be == tbe)
        { g->contained[br] = 1;
          continue;
        }
      if (flags & OVL_DISCARD)
        continue;
      live = !(flags & OVL_SYMDISCARD);
      if (live)
        { g->probe = (int *) damar_reserve(g->probe, &g->pcap, 2 * (g->nprobe + 1), sizeof(int), 2048, "graph");
          g->probe[2 * g->nprobe] = a;  g->probe[2 * g->nprobe + 1] = br;
          g->nprobe += 1;
        }
      for (k = 0; k < 2; k++)              /* the left end, then the right end */
        { const int at = k == 0 ? ab == tab : ae == tae;
          const int ovh = k == 0 ? bb - tbb : tbe - be;
          const int inside = k == 0 ? ae < tae : ab > tab;
          if (!at || ovh == 0)
            continue;
          if (ovh < 0)
            { neg_event(g, first_rec + i, ovh, a, br, live);
              continue;
            }
          c = new_cand(g);
          edge_of(c, b, diffs, i, a, flags, 0, alen, blen, ovh);
          c->owner = a;  c->right = k;  c->slot = 2 * k;  c->live = live;  c->ra = a;  c->rb = br;
          if (inside)
            { c = new_cand(g);
              edge_of(c, b, diffs, i, a, flags, 1, alen, blen, k == 0 ? tae - ae : ab - tab);
              c->owner = br;  c->right = (flags & OVL_COMP) ? k : !k;  c->slot = 2 * k + 1;  c->live = live;  c->ra = a;  c->rb = br;
            }
        }
    }
}

int damar_host_graph_batch(damar_host_graph *g, const damar_pile_batch *b, const int *diffs, int64 first_rec)
{ int64 p;
  if (g == NULL || !damar_graph_inputs_valid(b, diffs, g->nreads))
    return 1;
  for (p = 0; p < b->npiles; p++)
    host_pile(g, b, diffs, p, first_rec);
  g->nrec += b->nrec;
  return 0;
}

/* the loop over the sorted pairs (OGbuild.c:1416-1445) in closed form: the pairs are (B, A) of the OVL_SYMDISCARD records;
   it runs where A read `a` is the first member of a pair, and finds `b` among the second members of the pairs whose first
   member is `a` at most: the smallest first member with that second member is one of them, or none is */
static int sym_hit(const damar_host_graph *g, int a, int b)
{ return g->hasfirst[a] && g->minfirst[b] <= a; }

typedef struct { int a, b; int64 i; } SortKey;
static int cmp_key(const void *x, const void *y)
{ const SortKey *p = (const SortKey *) x, *q = (const SortKey *) y;
  if (p->a != q->a) return p->a < q->a ? -1 : 1;
  if (p->b != q->b) return p->b < q->b ? -1 : 1;
  return (p->i > q->i) - (p->i < q->i);
}

/* n edges put into the order of (ka, kb), ties as they lie: the reference's qsort is glibc's merge sort on arrays this small */
static void stable_sort(int *e, int64 n, int mode)
{ SortKey *k;
  int     *tmp;
  int64    i;
  if (n < 2)
    return;
  k = (SortKey *) damar_grow(NULL, sizeof(SortKey) * (size_t) n, "graph");
  tmp = (int *) damar_grow(NULL, sizeof(int) * EI * (size_t) n, "graph");
  for (i = 0; i < n; i++)
    { const int *x = e + EI * i;
      k[i].i = i;
      if (mode == 0)      { k[i].a = x[E_A];  k[i].b = x[E_B]; }                           /* cmp_ogedge */
      else if (mode == 1) { k[i].a = -(x[E_AE] - x[E_AB]);  k[i].b = 0; }                  /* cmp_ogedge_ovl_rev */
      else                { k[i].a = -x[E_OVH];  k[i].b = 0; }                             /* cmp_ogedge_ovh_rev */
    }
  qsort(k, (size_t) n, sizeof(SortKey), cmp_key);
  for (i = 0; i < n; i++)
    memcpy(tmp + EI * i, e + EI * k[i].i, sizeof(int) * EI);
  memcpy(e, tmp, sizeof(int) * EI * (size_t) n);
  free(k);  free(tmp);
}

/* remove_dupes (OGbuild.c:732-754): the earlier of two neighbours with one b */
static int64 drop_dupes(int *e, int64 n)
{ int64 i, dropped = 0;
  for (i = 0; i + 1 < n; i++)              /* the b of an edge is compared before the edge is dropped: the test sees the lists as they came */
    if (e[EI * (i + 1) + E_B] == e[EI * i + E_B])
      { e[EI * i + E_A] = -2;
        dropped += 1;
      }
  for (i = 0; i < n; i++)
    if (e[EI * i + E_A] == -2)
      e[EI * i + E_A] = e[EI * i + E_B] = -1;
  return dropped;
}

int64 damar_host_graph_dedupe(int *left, int64 nl, int *right, int64 nr)
{ int64 dropped = 0, i, j;
  if (nl > 0) dropped += drop_dupes(left, nl);
  if (nr > 0) dropped += drop_dupes(right, nr);
  /* remove_lr_dupes (OGbuild.c:756-781): a dropped left edge (b == -1) meets every right edge dropped so far, again */
  for (i = 0; i < nl; i++)
    for (j = 0; j < nr; j++)
      if (left[EI * i + E_B] == right[EI * j + E_B])
        { right[EI * j + E_A] = right[EI * j + E_B] = -1;
          dropped += 1;
        }
  return dropped;
}

/* compress_graph_side (OGbuild.c:818-850) */
int64 damar_host_graph_compress(int *e, int64 *off, int nreads)
{ int64 adj = 0, i;
  int r;
  for (r = 0; r < nreads; r++)
    { const int64 b = off[r], t = off[r + 1];
      off[r] -= adj;
      for (i = b; i < t; i++)
        if (e[EI * i + E_A] == -1 || e[EI * i + E_B] == -1)
          adj += 1;
        else if (adj > 0)
          memmove(e + EI * (i - adj), e + EI * i, sizeof(int) * EI);
    }
  off[nreads] -= adj;
  return adj;
}

void damar_graph_result_free(damar_graph_result *res)
{ free(res->loff);  free(res->roff);  free(res->left);  free(res->right);  free(res->status);  free(res->neg);
  memset(res, 0, sizeof(*res));
}

int damar_host_graph_finish(damar_host_graph *g, damar_graph_result *res)
{ const int nr = g->nreads;
  int64 *cur[2], *off[2], k;
  int   *list[2], r, s;
  memset(res, 0, sizeof(*res));
  res->nreads = nr;
  res->neg_rec = -1;
  list[0] = list[1] = NULL;
  for (s = 0; s < 2; s++)
    { off[s] = (int64 *) calloc((size_t) nr + 2, sizeof(int64));
      cur[s] = (int64 *) calloc((size_t) nr + 2, sizeof(int64));
    }
  if (off[0] == NULL || cur[0] == NULL || off[1] == NULL || cur[1] == NULL)
    goto nomem;
  res->status = (unsigned char *) damar_grow(NULL, (size_t) nr + 1, "graph");
  for (r = 0; r < nr; r++)
    res->status[r] = DAMAR_OG_WIDOW;
  for (k = 0; k < g->nprobe; k++)
    res->symdiscard += sym_hit(g, g->probe[2 * k], g->probe[2 * k + 1]);
  for (k = 0; k < g->ncand; k++)
    off[g->cand[k].right][g->cand[k].owner] += 1;
  for (s = 0; s < 2; s++)
    { int64 sum = 0;
      for (r = 0; r <= nr; r++)
        { const int64 c = off[s][r];
          off[s][r] = sum;
          sum += c;
        }
      list[s] = (int *) calloc((size_t) sum * EI + 1, sizeof(int));      /* a slot never filled stays an edge of zeros, as the reference's does */
      if (list[s] == NULL)
        goto nomem;
    }
  res->cnt_left = off[0][nr];  res->cnt_right = off[1][nr];
  for (k = 0; k < g->ncand; k++)
    { const Cand *c = g->cand + k;
      if (!c->live || sym_hit(g, c->ra, c->rb))
        continue;
      /* the reference fills from the front of a list and leaves the slots of the records it passed over at its end; the
         sort that follows puts the zeros first either way */
      memcpy(list[c->right] + EI * (off[c->right][c->owner] + cur[c->right][c->owner]++), c->e, sizeof(int) * EI);
      res->status[c->owner] = DAMAR_OG_PROPER;
      if (c->slot & 1) res->redges += 1;
      else             res->edges += 1;
    }
  for (r = 0; r < nr; r++)
    { if (g->contained[r])
        res->status[r] = DAMAR_OG_CONTAINED;
      for (s = 0; s < 2; s++)
        stable_sort(list[s] + EI * off[s][r], off[s][r + 1] - off[s][r], 0);
      res->parallel += damar_host_graph_dedupe(list[0] + EI * off[0][r], off[0][r + 1] - off[0][r], list[1] + EI * off[1][r], off[1][r + 1] - off[1][r]);
    }
  res->removed = damar_host_graph_compress(list[0], off[0], nr) + damar_host_graph_compress(list[1], off[1], nr);
  res->loff = off[0];  res->roff = off[1];  res->left = list[0];  res->right = list[1];
  free(cur[0]);  free(cur[1]);
  if (g->nneg > 0)
    { res->neg = (int64 *) damar_grow(NULL, sizeof(int64) * 5 * (size_t) g->nneg, "graph");
      memcpy(res->neg, g->neg, sizeof(int64) * 5 * (size_t) g->nneg);
      res->nneg = g->nneg;
      res->neg_rec = g->neg[0];
      for (k = 0; k < g->nneg; k++)
        res->neg[5 * k + 4] = g->neg[5 * k + 4] && !sym_hit(g, (int) g->neg[5 * k + 2], (int) g->neg[5 * k + 3]);
    }
  return 0;
nomem:
  fprintf(stderr, "damar: out of memory (graph)\n");
  for (s = 0; s < 2; s++)
    { free(off[s]);  free(cur[s]);  free(list[s]); }
  free(res->status);
  memset(res, 0, sizeof(*res));
  return 1;
}

/***** -c, -s and the writers, on the compacted graph *******************************************/

typedef struct
{ damar_graph_result *g;
  int *comp, ncomp;
} Graph;

/* proper_edges (OGbuild.c:890-915) */
static int proper_edges(const Graph *G, const int *e, int64 n)
{ int64 i;
  int   cnt = 0;
  for (i = 0; i < n; i++)
    if (!(e[EI * i + E_FLAGS] & OVL_OPTIONAL) && (G->g->status[e[EI * i + E_B]] & DAMAR_OG_PROPER))
      cnt += 1;
  return cnt;
}

/* add_contained_edges (OGbuild.c:917-1095): the statuses change while a round runs, so this stays a loop on the host */
static void add_contained(Graph *G, int contained, int by_ovh)
{ damar_graph_result *g = G->g;
  unsigned char *status = g->status;
  const int nr = g->nreads;
  int64 cap = nr + 1, n = 0, nn;
  int  *ins = (int *) damar_grow(NULL, sizeof(int) * (size_t) cap, "graph"), *next = (int *) damar_grow(NULL, sizeof(int) * (size_t) cap, "graph");
  int   r, s;
  printf("adding contained edges (c = %d)\n", contained);
  if (contained == -1)
    contained = INT_MAX;
  for (r = 0; r < nr; r++)
    if (status[r] == DAMAR_OG_PROPER)
      ins[n++] = r;
  printf("  inspecting %d proper reads\n", (int) n);
  while (n > 0)
    { int64 i;
      nn = 0;
      for (i = 0; i < n; i++)
        { const int a = ins[i];
          if (status[a] != DAMAR_OG_PROPER)
            continue;
          for (s = 0; s < 2; s++)
            { int  *e = (s == 0 ? g->left : g->right) + EI * (s == 0 ? g->loff : g->roff)[a];
              const int64 m = (s == 0 ? g->loff : g->roff)[a + 1] - (s == 0 ? g->loff : g->roff)[a];
              int64 j;
              int   took = 0;
              if (proper_edges(G, e, m) != 0)
                continue;
              stable_sort(e, m, by_ovh ? 2 : 1);
              for (j = 0; j < m && took < contained; j++)
                { if (e[EI * j + E_FLAGS] & OVL_OPTIONAL)
                    continue;
                  status[e[EI * j + E_B]] = DAMAR_OG_PROPER | DAMAR_OG_OPTIONAL;
                  if (nn + 1 >= cap)
                    { cap = cap + cap / 4 + 1024;
                      ins = (int *) damar_grow(ins, sizeof(int) * (size_t) cap, "graph");
                      next = (int *) damar_grow(next, sizeof(int) * (size_t) cap, "graph");
                    }
                  next[nn++] = e[EI * j + E_B];
                  took += 1;
                }
            }
        }
      { SortKey *k = (SortKey *) damar_grow(NULL, sizeof(SortKey) * (size_t) (nn + 1), "graph");
        for (i = 0; i < nn; i++) { k[i].a = next[i];  k[i].b = 0;  k[i].i = i; }
        qsort(k, (size_t) nn, sizeof(SortKey), cmp_key);
        for (i = 0; i < nn; i++) ins[i] = k[i].a;
        free(k);
      }
      n = nn;
      if (n > 0)
        printf("  set %d reads to proper\n", (int) n);
    }
  free(ins);  free(next);
}

/* assign_component (OGbuild.c:524-673): what is reached from the first read without a component, over edges to proper
   reads; a read that reaches nothing new keeps -1 */
static void components(Graph *G)
{ const damar_graph_result *g = G->g;
  const int nr = g->nreads;
  int *stack = (int *) damar_grow(NULL, sizeof(int) * ((size_t) nr + 1), "graph");
  int  r, cur = 0, s;
  for (r = 0; r < nr; r++)
    G->comp[r] = -1;
  for (r = 0; r < nr; r++)
    { int64 top = 0, reached = 0;
      if (G->comp[r] != -1 || !(g->status[r] & DAMAR_OG_PROPER))
        continue;
      G->comp[r] = cur;
      stack[top++] = r;
      while (top > 0)
        { const int x = stack[--top];
          for (s = 0; s < 2; s++)
            { const int *e = s == 0 ? g->left : g->right;
              const int64 *off = s == 0 ? g->loff : g->roff;
              int64 j;
              for (j = off[x]; j < off[x + 1]; j++)
                { const int y = e[EI * j + E_B];
                  if (G->comp[y] == -1 && (g->status[y] & DAMAR_OG_PROPER))
                    { G->comp[y] = cur;
                      stack[top++] = y;
                      reached += 1;
                    }
                }
            }
        }
      if (reached == 0) G->comp[r] = -1;
      else              cur += 1;
    }
  printf("  %d components\n", cur);
  G->ncomp = cur;
  free(stack);
}

/* the reference converts a double that is not a number where both intervals are empty (an edge of zeros): what the
   conversion instruction of x86-64 leaves then is INT_MIN, and that is written here */
static int divergence(const int *e)
{ const int den = (e[E_AE] - e[E_AB]) + (e[E_BE] - e[E_BB]);
  if (den == 0)
    return INT_MIN;
  return (int) (100.0 * 2 * e[E_DIFFS] / den);
}

enum { F_GML, F_GRAPHML, F_TGF };

static void write_edge(FILE *f, int fmt, const int *e, char side)
{ const int div = divergence(e);
  if (fmt == F_GRAPHML)
    { fprintf(f, "    <edge source=\"%d\" target=\"%d\">\n", e[E_A], e[E_B]);
      fprintf(f, "      <data key=\"length\">%d</data>\n", e[E_OVH]);
      fprintf(f, "      <data key=\"flags\">%d</data>\n", e[E_FLAGS]);
      fprintf(f, "      <data key=\"divergence\">%d</data>\n", div);
      fprintf(f, "      <data key=\"end\">%c</data>\n", side);
      fprintf(f, "    </edge>\n");
    }
  else if (fmt == F_GML)
    { fprintf(f, "  edge [\n    source %d\n    target %d\n    length %d\n    flags %d\n    divergence %d\n    end \"%c\"\n  ]\n",
              e[E_A], e[E_B], e[E_OVH], e[E_FLAGS], div, side);
    }
  else
    fprintf(f, "%d %d %d %d %d %c\n", e[E_A], e[E_B], e[E_OVH], e[E_FLAGS], div, side);
}

/* the edges of one component (-1: all) to proper reads: visit() per edge, the reads they touch marked USED; TGF counts
   them first (in, out) and writes them after its nodes */
static void walk_edges(const Graph *G, FILE *f, int fmt, int component, int write, int mark, int *nin, int *nout)
{ const damar_graph_result *g = G->g;
  unsigned char *status = g->status;
  int r, s;
  for (r = 0; r < g->nreads; r++)
    { int used = 0;
      if (!(status[r] & DAMAR_OG_PROPER) || (component != -1 && G->comp[r] != component))
        continue;
      for (s = 0; s < 2; s++)
        { const int *e = s == 0 ? g->left : g->right;
          const int64 *off = s == 0 ? g->loff : g->roff;
          int64 j;
          for (j = off[r]; j < off[r + 1]; j++)
            { const int y = e[EI * j + E_B];
              if (!(status[y] & DAMAR_OG_PROPER))
                continue;
              if (mark)
                { status[y] |= DAMAR_OG_USED;
                  used = 1;
                }
              if (nin != NULL)
                { nout[r] += 1;
                  nin[y] += 1;
                }
              if (write)
                write_edge(f, fmt, e + EI * j, s == 0 ? 'l' : 'r');
            }
        }
      if (used)
        status[r] |= DAMAR_OG_USED;
    }
}

static void write_one(const Graph *G, FILE *f, int fmt, int component)
{ const damar_graph_result *g = G->g;
  unsigned char *status = g->status;
  int r;
  if (fmt == F_TGF)
    { int *nin = (int *) calloc((size_t) g->nreads + 1, sizeof(int)), *nout = (int *) calloc((size_t) g->nreads + 1, sizeof(int));
      walk_edges(G, f, fmt, component, 0, 1, nin, nout);
      for (r = 0; r < g->nreads; r++)
        if (status[r] & DAMAR_OG_USED)
          { fprintf(f, "%d %d %d %d\n", r, (status[r] & DAMAR_OG_OPTIONAL) ? 1 : 0, nin[r], nout[r]);
            status[r] ^= DAMAR_OG_USED;
          }
      fprintf(f, "#\n");
      walk_edges(G, f, fmt, component, 1, 0, NULL, NULL);
      free(nin);  free(nout);
      return;
    }
  if (fmt == F_GML)
    fprintf(f, "graph [\n  label \"og\"\n  directed 1\n");
  else
    { fprintf(f, "<?xml version=\"1.0\" encoding=\"UTF-8\" ?>\n");
      fprintf(f, "<graphml xmlns=\"http://graphml.graphdrawing.org/xmlns\"\n");
      fprintf(f, "         xmlns:xsi=\"http://www.w3.org/2001/XMLSchema-instance\"\n");
      fprintf(f, "         xsi:schemaLocation=\"http://graphml.graphdrawing.org/xmlns/1.0/graphml.xsd\">\n");
      fprintf(f, "  <key attr.name=\"length\"     attr.type=\"int\"    for=\"edge\" id=\"length\" />\n");
      fprintf(f, "  <key attr.name=\"flags\"      attr.type=\"int\"    for=\"edge\" id=\"flags\" />\n");
      fprintf(f, "  <key attr.name=\"end\"        attr.type=\"string\" for=\"edge\" id=\"end\" />\n");
      fprintf(f, "  <key attr.name=\"divergence\" attr.type=\"int\"    for=\"edge\" id=\"divergence\" />\n");
      fprintf(f, "  <key attr.name=\"read\"       attr.type=\"int\"    for=\"node\" id=\"read\" />\n");
      fprintf(f, "  <key attr.name=\"optional\"   attr.type=\"int\"    for=\"node\" id=\"optional\" />\n");
      fprintf(f, "  <graph id=\"og\" edgedefault=\"directed\">\n");
    }
  walk_edges(G, f, fmt, component, 1, 1, NULL, NULL);
  for (r = 0; r < g->nreads; r++)
    { const int optional = (status[r] & DAMAR_OG_OPTIONAL) ? 1 : 0;
      if (!(status[r] & DAMAR_OG_USED))
        continue;
      if (fmt == F_GML)
        fprintf(f, "  node [\n    id %d\n    read %d\n    optional %d\n  ]\n", r, r, optional);
      else
        { fprintf(f, "    <node id=\"%d\">\n", r);
          fprintf(f, "      <data key=\"read\">%d</data>\n", r);
          fprintf(f, "      <data key=\"optional\">%d</data>\n", optional);
          fprintf(f, "    </node>\n");
        }
      status[r] ^= DAMAR_OG_USED;
    }
  if (fmt == F_GML)
    fprintf(f, "]\n");
  else
    fprintf(f, "  </graph>\n</graphml>\n");
}

/* write_graph (OGbuild.c:1141-1219) */
static void write_graph(const Graph *G, const char *path, int fmt, int split)
{ static const char *ext[] = { "gml", "graphml", "tgf" };
  char *name = (char *) damar_grow(NULL, strlen(path) + 40, "graph");
  int   i;
  for (i = split ? 0 : -1; i < (split ? G->ncomp : 0); i++)
    { FILE *f;
      if (split) sprintf(name, "%s_%05d.%s", path, i, ext[fmt]);
      else       strcpy(name, path);
      if ((f = fopen(name, "w")) == NULL)
        { fprintf(stderr, "failed to create %s\n", name);
          continue;
        }
      write_one(G, f, fmt, i);
      fclose(f);
    }
  free(name);
}

/***** the pass over a file *********************************************************************/

typedef struct
{ int64 *at;     int64 n, cap;        /* a progress line of lib/pass.c: before which pile (counted over the file) */
  double *pct;
} Ticks;

/* through the session -- the GPU unless DAMAR_PILES=host, or `host` -- batch by batch.  ticks (or NULL): the lines a pass of
   the reference prints, one where the file position behind a pile's first record header has crossed another tenth.
   pile_first (or NULL): malloc'ed, the record each pile begins with. */
static int run_session(const damar_dbinfo *db, const char *las, const int *pairs, int host, damar_graph_result *res, Ticks *ticks,
                       int64 **pile_first, int64 *npiles_out)
{ damar_pile_reader *r = damar_piles_open(las, 0);
  damar_graph      *g = NULL;
  damar_host_graph *h = NULL;
  damar_pile_batch  b;
  int64 first = 0, pos = 12, size = 0, tick = 0, next_tick = 0, npiles = 0, pcap = 0, *pf = NULL;
  int   got, rc = 1;
  if (r == NULL)
    return 1;
  if (ticks != NULL)
    { FILE *f = fopen(las, "r");
      if (f != NULL)
        { fseeko(f, 0, SEEK_END);
          size = (int64) ftello(f);
          fclose(f);
        }
      tick = next_tick = size / 10;
    }
  if (host) h = damar_host_graph_open(db->read_len, db->nreads, pairs);
  else      g = damar_graph_open(db->read_len, db->nreads, pairs);
  if (g == NULL && h == NULL)
    goto done;
  while ((got = damar_piles_next(r, &b)) > 0)
    { const int *diffs, *last, *tlen = damar_piles_tlen(r);
      const int  tbytes = damar_piles_tspace(r) <= 125 ? 1 : 2;
      int64 p, i;
      damar_piles_rest(r, &diffs, &last);
      if (damar_batch_bind(&b, db, las, DAMAR_BIND_AB))
        goto done;
      for (p = 0; p < b.npiles; p++)
        { if (ticks != NULL && pos + 40 >= next_tick)
            { ticks->at = (int64 *) damar_reserve(ticks->at, &ticks->cap, ticks->n + 1, sizeof(int64), 16, "graph");
              ticks->pct = (double *) damar_grow(ticks->pct, sizeof(double) * (size_t) ticks->cap, "graph");
              ticks->at[ticks->n] = npiles;
              ticks->pct[ticks->n++] = 100.0 * (double) (pos + 40) / (double) size;
              next_tick += tick;
            }
          if (pile_first != NULL)
            { pf = (int64 *) damar_reserve(pf, &pcap, npiles + 1, sizeof(int64), 1024, "graph");
              pf[npiles] = first + b.pile_off[p];
            }
          npiles += 1;
          for (i = b.pile_off[p]; i < b.pile_off[p + 1]; i++)
            pos += 40 + (int64) tbytes * tlen[i];
        }
      if (host ? damar_host_graph_batch(h, &b, diffs, first) : damar_graph_batch(g, &b, diffs, first))
        goto done;
      first += b.nrec;
    }
  if (got < 0)
    goto done;
  if (host ? damar_host_graph_finish(h, res) : damar_graph_finish(g, res))
    goto done;
  rc = 0;
done:
  damar_graph_close(g);
  damar_host_graph_close(h);
  damar_piles_close(r);
  if (pile_first != NULL && rc == 0)
    { *pile_first = pf;
      *npiles_out = npiles;
    }
  else
    free(pf);
  return rc;
}

/* the device path leaves a file with a negative overhang to the host routine: what the reference prints then depends on
   every such record, and the run ends in an error */
static int edges_of(const damar_dbinfo *db, const char *las, const int *pairs, damar_graph_result *res, Ticks *ticks, int64 **pile_first,
                    int64 *npiles)
{ const int host = damar_piles_on_host();
  if (run_session(db, las, pairs, host, res, ticks, pile_first, npiles))
    return 1;
  if (!host && res->neg_rec >= 0)
    { damar_graph_result_free(res);
      if (pile_first != NULL)
        { free(*pile_first);
          *pile_first = NULL;
        }
      return run_session(db, las, pairs, 1, res, NULL, pile_first, npiles);
    }
  return 0;
}

static int *load_trim(const damar_dbinfo *db, const char *track, int *missing)
{ uint64 *anno = NULL;
  int    *data = NULL, *pairs;
  int64   nd = 0;
  *missing = 0;
  if (damar_track_read_any(db, track, &anno, &data, &nd))
    { *missing = 1;
      return NULL;
    }
  pairs = (int *) damar_grow(NULL, sizeof(int) * 2 * ((size_t) db->nreads + 1), "graph");
  if (damar_trim_pairs(anno, data, db->nreads, pairs))
    { fprintf(stderr, "OGbuild: the trim track '%s' does not hold one interval per read at most\n", track);
      free(pairs);
      pairs = NULL;
    }
  free(anno);  free(data);
  return pairs;
}

int damar_og_edges(const char *dbname, const char *las, const char *track, damar_graph_result *res)
{ damar_dbinfo db;
  int *pairs, missing, rc;
  memset(res, 0, sizeof(*res));
  if (damar_dbinfo_open(dbname, &db))
    { fprintf(stderr, "could not open '%s'\n", dbname);
      return 1;
    }
  if ((pairs = load_trim(&db, track != NULL ? track : "trim", &missing)) == NULL)
    { if (missing)
        fprintf(stderr, "ERROR: failed to open %s\n", track != NULL ? track : "trim");
      damar_dbinfo_close(&db);
      return 1;
    }
  rc = edges_of(&db, las, pairs, res, NULL, NULL, NULL);
  free(pairs);
  damar_dbinfo_close(&db);
  return rc;
}

static void og_usage(void)
{ printf("usage: [-s] [-c <int>] [-t <track>] [-f gml|graphml|tgf] [-p ovl|ovh] database input.las output.format\n\n");
  printf("Builds the overlap graph based on the alignments in the input las file.\n\n");
  printf("options: -c n      try to add otherwise containted reads to dead ends in the graph\n");
  printf("                   0 disabled, >0 maximum number of edges, -1 all edges (default %d)\n", 0);
  printf("         -p mode   which edges should be added when running in -c mode (default %s)\n", "ovl");
  printf("                   ovl longest overlap, ovh longer overhang\n");
  printf("         -f frmt   output graph format. gml, graphml or tgf (default %s)\n", "graphml");
  printf("         -s        write on file for each component of the overlap graph.\n");
  printf("                   files are named output.<component.number>.format\n");
  printf("         -t track  which trim track to use (%s)\n", "trim");
}

void damar_og_usage(void) { og_usage(); }

static void print_ticks(const Ticks *t, int64 upto)
{ int64 k;
  for (k = 0; k < t->n && t->at[k] <= upto; k++)
    printf("%3.0f%% done\n", t->pct[k]);
}

int damar_og_build(const char *dbname, const char *las, const char *out, const damar_og_opts *o)
{ const char *format = o->format != NULL ? o->format : "graphml", *prio = o->prio != NULL ? o->prio : "ovl";
  const char *track = o->track != NULL ? o->track : "trim";
  damar_graph_result res;
  damar_dbinfo db;
  Graph  G;
  Ticks  ticks;
  FILE  *f;
  int64 *pile_first = NULL, npiles = 0, k;
  int   *pairs, fmt, by_ovh, missing, rc = 1;

  memset(&ticks, 0, sizeof(ticks));
  memset(&res, 0, sizeof(res));
  if (strcmp(format, "gml") == 0) fmt = F_GML;
  else if (strcmp(format, "graphml") == 0) fmt = F_GRAPHML;
  else if (strcmp(format, "tgf") == 0) fmt = F_TGF;
  else
    { fprintf(stderr, "error: unknown graph format %s\n", format);
      og_usage();
      return 1;
    }
  if (strcmp(prio, "ovh") == 0) by_ovh = 1;
  else if (strcmp(prio, "ovl") == 0) by_ovh = 0;
  else
    { fprintf(stderr, "error: unknown edge priority %s\n", prio);
      og_usage();
      return 1;
    }
  if ((f = fopen(las, "r")) == NULL)
    { fprintf(stderr, "could not open '%s'\n", las);
      return 1;
    }
  fclose(f);
  if (damar_dbinfo_open(dbname, &db))
    { fprintf(stderr, "could not open '%s'\n", dbname);
      return 1;
    }
  if (o->contained < -1)
    { fprintf(stderr, "unvalid value %d for -c\n", o->contained);
      damar_dbinfo_close(&db);
      return 1;
    }
  if ((pairs = load_trim(&db, track, &missing)) == NULL)
    { if (missing)
        { fprintf(stderr, "(null): Track '%s' does not exist\n", track);       /* track_load's own line, then pre_build's */
          fprintf(stderr, "ERROR: failed to open %s\n", track);
        }
      damar_dbinfo_close(&db);
      return 1;
    }
  if (edges_of(&db, las, pairs, &res, &ticks, &pile_first, &npiles))
    goto done;

  printf(GREEN "PASS - calculating memory requirements" RESET "\n");
  print_ticks(&ticks, npiles);
  for (k = 0; k < res.nneg; k++)           /* the counting pass says so and goes on */
    fprintf(stderr, "error: ovh %5d <= 0 %7d -> %7d. Trim track most likely incompatible with overlaps.\n", (int) res.neg[5 * k + 1],
            (int) res.neg[5 * k + 2], (int) res.neg[5 * k + 3]);
  printf("%d left edges\n", (int) res.cnt_left);
  printf("%d right edges\n", (int) res.cnt_right);
  printf(GREEN "PASS - building graph" RESET "\n");
  for (k = 0; k < res.nneg; k++)
    if (res.neg[5 * k + 4])                /* the building pass ends at the first one it gets to */
      { int64 p = 0;
        while (p + 1 < npiles && pile_first[p + 1] <= res.neg[5 * k])
          p += 1;
        print_ticks(&ticks, p);
        fprintf(stderr, "error: ovh %5d <= 0 %7d -> %7d. Trim track most likely incompatible with overlaps.\n", (int) res.neg[5 * k + 1],
                (int) res.neg[5 * k + 2], (int) res.neg[5 * k + 3]);
        goto done;
      }
  print_ticks(&ticks, npiles);
  printf(GREEN "processing graph" RESET "\n");
  printf("  %llu edges\n", (unsigned long long) res.edges);
  printf("  %llu redges\n", (unsigned long long) res.redges);
  printf("  %llu symmetric discards\n", (unsigned long long) res.symdiscard);
  printf("sorting edges\n");
  printf("parallel edges\n");
  printf("  %lld parallel edges\n", (long long) res.parallel);
  if (res.removed > 0)
    printf("removed %d edges\n", (int) res.removed);
  G.g = &res;
  G.ncomp = 0;
  G.comp = (int *) damar_grow(NULL, sizeof(int) * ((size_t) db.nreads + 1), "graph");
  if (o->contained != 0)
    add_contained(&G, o->contained, by_ovh);
  if (o->split)
    { printf("components\n");
      components(&G);
    }
  write_graph(&G, out, fmt, o->split);
  free(G.comp);
  rc = 0;
done:
  fflush(stdout);
  damar_graph_result_free(&res);
  free(pile_first);  free(ticks.at);  free(ticks.pct);  free(pairs);
  damar_dbinfo_close(&db);
  return rc;
}
