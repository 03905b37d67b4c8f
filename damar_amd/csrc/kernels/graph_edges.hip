/* graph_edges.hip -- the edges of OGbuild's overlap graph for gfx950 (touring/OGbuild.c:1262-1719 and 732-869; the plain
 * version is host/graph.c).
 *
 *   graph_pile<EMIT>  a wavefront per pile, its lanes over the records in chunks of 64.  drop_parallel_edges marks every live
 *              record of a stretch of one B read that holds two live records or more: stretch heads are a ballot of
 *              "B differs from the record before", a lane's stretch is the bits between the head at or below it and the next
 *              head above it, and the live count of that stretch is a popcount.  A stretch may cross a chunk border: the live
 *              count of the open stretch is carried into the next chunk, and where the chunk's last stretch goes on behind
 *              it the wave looks ahead for one more live record of that B read.  Then each lane does its record: the
 *              symmetric-discard tables, the two containment tests (atomic OR into the resident status array), and up to
 *              four candidate edges -- A's left edge and its mirror, A's right edge and its mirror -- appended to the
 *              resident candidate buffer behind one atomic add per chunk.  The pass runs twice per batch: once counting, so
 *              that the buffer can be grown, once appending.  Candidates are made for every record the reference's counting
 *              pass allots a slot for; which of them are filled is known only when the whole file has been seen.
 *   graph_settle  a lane per candidate: one that its record's symmetric discard takes away becomes an edge of zeros (the
 *              reference leaves its slot as calloc made it), one that stays makes its owner PROPER.  The rule is
 *              "hasfirst[A] and minfirst[B] <= A" (host/graph.c sym_hit).  Key: the record's place in the file and the slot.
 *   graph_keys    after a stable sort by that key: key = list (left lists of all reads, then right lists), b, zeros first.
 *   graph_bounds  after a stable sort by that key: where each list begins and ends.
 *   graph_reads   a wavefront per read: remove_dupes on both lists, remove_lr_dupes with the count it makes (below), the
 *              keep flag of every edge.  A read with more than maxdeg edges on a side keeps all of them for the host routine.
 *   graph_gather  after a scan of the keep flags: the kept edges, nine ints each, in list order.
 *
 * Wave size 64, plain C++ and vector atomics only.  Every index into a per-read array is a read number the stage has checked
 * against nreads; every index into the candidate buffer is below the count the counting pass made room for.
 */
#include "dev_common.h"
#include "kernels.h"
#include "damar_graph.h"

#define GR_THREADS 256
#define GR_WAVES   (GR_THREADS / WAVE)
#define GR_MAX_BLOCKS 65536u
#define GR_COMP     0x1
#define GR_DISCARD  0x2
#define GR_SYM      0x100

static u32 blocks_for(u64 n, u32 per)
{ const u64 b = (n + per - 1) / per;
  return (u32) (b < 1 ? 1 : (b > GR_MAX_BLOCKS ? GR_MAX_BLOCKS : b));
}

__device__ __forceinline__ void put_edge(int *c, int a, int b, int ab, int ae, int bb, int be, int flags, int ovh, int diffs, int owner,
                                         int right, int slot, int live, int ra, int rb, u64 seq)
{ c[0] = a;  c[1] = b;  c[2] = ab;  c[3] = ae;  c[4] = bb;  c[5] = be;  c[6] = flags;  c[7] = ovh;  c[8] = diffs & 0xffff;
  c[9] = owner;  c[10] = right | (slot << 1) | (live << 3);  c[11] = ra;  c[12] = rb;  c[13] = 0;
  c[14] = (int) (u32) seq;  c[15] = (int) (u32) (seq >> 32);
}

template <bool EMIT>
__global__ __launch_bounds__(GR_THREADS)
void graph_pile(GraphArgs g)
{ const int l = lane_id();
  const u32 nwaves = gridDim.x * GR_WAVES;
  for (u32 p = blockIdx.x * GR_WAVES + (threadIdx.x >> 6); p < g.npiles; p += nwaves)
    { const long long lo = g.pile_off[p], hi = g.pile_off[p + 1];
      const int a = g.pile_aread[p], alen = g.read_len[a], tab = g.trim[2 * a], tae = g.trim[2 * a + 1];
      int carry = 0;                              /* live records of the stretch that is open at the chunk's begin, 2 at most */
      int symmin = 0x7fffffff;
      for (long long c0 = lo; c0 < hi; c0 += WAVE)
        { const long long i = c0 + l;
          const bool valid = i < hi;
          const int  nv = (int) ((hi - c0 < WAVE) ? hi - c0 : WAVE);
          const int  br = valid ? g.bread[i] : -1;
          int        fl = valid ? g.flags[i] : GR_DISCARD;
          const int  prevb = (valid && i > lo) ? g.bread[i - 1] : -2;
          const bool live0 = valid && !(fl & GR_DISCARD);
          const u64  H = wballot(valid && l > 0 && br != prevb), L = wballot(live0);
          const bool joins = first_i(prevb) == first_i(br) && c0 > lo;       /* the chunk's first stretch began before it */
          const u64  upto = lanes_below(l) | (1ull << l);
          const u64  Hle = H & upto, Hgt = H & ~upto;
          const int  s = Hle ? 63 - __builtin_clzll(Hle) : 0;
          const int  e = Hgt ? __builtin_ctzll(Hgt) : nv;
          const u64  smask = (e >= 64 ? ~0ull : ((1ull << e) - 1)) & ~lanes_below(s);
          int  cnt = __builtin_popcountll(L & smask);
          /* the chunk's last stretch: does it go on behind the chunk with a live record? */
          const int  lastb = bcast_i(br, nv - 1);
          int  ahead = 0;
          for (long long k0 = c0 + WAVE; k0 < hi; k0 += WAVE)
            { const long long k = k0 + l;
              const bool in = k < hi;
              const bool same = in && g.bread[k] == lastb;
              const u64  brk = wballot(!same);
              const u64  liv = wballot(same && !(g.flags[in ? k : lo] & GR_DISCARD));
              const u64  run = brk ? ((1ull << __builtin_ctzll(brk)) - 1) : ~0ull;
              if (liv & run) ahead = 1;
              if (ahead || brk) break;
            }
          if (Hle == 0 && joins) cnt += carry;
          if (Hgt == 0) cnt += ahead;
          if (live0 && cnt >= 2) fl |= GR_DISCARD;
          { /* what the next chunk inherits: the live records of this chunk's last stretch */
            const int s63 = H ? 63 - __builtin_clzll(H) : 0;
            int c = __builtin_popcountll(L & ~lanes_below(s63));
            if (H == 0 && joins) c += carry;
            carry = c > 2 ? 2 : c;
          }

          /* the record */
          int  n = 0, probe = 0;
          int  ab = 0, ae = 0, bb = 0, be = 0, blen = 0, tbb = 0, tbe = 0, ovl = 0, ovr = 0;
          bool live = false, left = false, right = false, lmir = false, rmir = false, neg = false;
          if (valid && br != a)
            { ab = g.abpos[i];  ae = g.aepos[i];  bb = g.bbpos[i];  be = g.bepos[i];
              blen = g.read_len[br];  tbb = g.trim[2 * br];  tbe = g.trim[2 * br + 1];
              if (fl & GR_SYM)
                { symmin = br < symmin ? br : symmin;
                  if (!EMIT) g.hasfirst[br] = 1;
                }
              if (fl & GR_COMP)
                { const int t = tbb;
                  tbb = blen - tbe;
                  tbe = blen - t;
                }
              if (ab == tab && ae == tae)
                { if (!EMIT) atomicOr(&g.status[a], (u32) DAMAR_OG_CONTAINED); }
              else if (bb == tbb && be == tbe)
                { if (!EMIT) atomicOr(&g.status[br], (u32) DAMAR_OG_CONTAINED); }
              else if (!(fl & GR_DISCARD))
                { live = !(fl & GR_SYM);
                  probe = live;
                  ovl = bb - tbb;  ovr = tbe - be;
                  if (ab == tab && ovl != 0) { if (ovl < 0) neg = true; else { left = true;  lmir = ae < tae; } }
                  if (ae == tae && ovr != 0) { if (ovr < 0) neg = true; else { right = true;  rmir = ab > tab; } }
                  n = left + lmir + right + rmir;
                }
            }
          if (!EMIT && neg)
            atomicMin(&g.ctr[GC_NEG], g.first_rec + (u64) i);
          const int incl = wave_incl_scan_i(n), pincl = wave_incl_scan_i(probe);
          const int tot = bcast_i(incl, 63), ptot = bcast_i(pincl, 63);
          u64 base = 0, pbase = 0;
          if (l == 0)
            { if (tot > 0)  base = atomicAdd(&g.ctr[GC_NCAND], (u64) tot);
              if (ptot > 0) pbase = atomicAdd(&g.ctr[GC_NPROBE], (u64) ptot);
            }
          base = bcast_u64(base, 0);  pbase = bcast_u64(pbase, 0);
          if (EMIT)
            { u64 at = base + (u64) (incl - n);
              const u64 seq = (g.first_rec + (u64) i) << 2;
              const int d = n > 0 ? g.diffs[i] : 0, liv = live ? 1 : 0, comp = fl & GR_COMP;
              if (probe && pbase + (u64) (pincl - 1) < g.probe_cap)
                g.probe[pbase + (u64) (pincl - 1)] = ((u64) (u32) a << 32) | (u32) br;
              if (at + (u64) n <= g.cand_cap)
                { if (left)
                    put_edge(g.cand + GE_INTS * at++, a, br, ab, ae, bb, be, fl, ovl, d, a, 0, 0, liv, a, br, seq);
                  if (lmir)
                    { if (comp) put_edge(g.cand + GE_INTS * at++, br, a, blen - be, blen - bb, alen - ae, alen - ab, fl, tae - ae, d, br, 0, 1, liv, a, br, seq | 1);
                      else      put_edge(g.cand + GE_INTS * at++, br, a, bb, be, ab, ae, fl, tae - ae, d, br, 1, 1, liv, a, br, seq | 1);
                    }
                  if (right)
                    put_edge(g.cand + GE_INTS * at++, a, br, ab, ae, bb, be, fl, ovr, d, a, 1, 2, liv, a, br, seq | 2);
                  if (rmir)
                    { if (comp) put_edge(g.cand + GE_INTS * at++, br, a, blen - be, blen - bb, alen - ae, alen - ab, fl, ab - tab, d, br, 1, 3, liv, a, br, seq | 3);
                      else      put_edge(g.cand + GE_INTS * at++, br, a, bb, be, ab, ae, fl, ab - tab, d, br, 0, 3, liv, a, br, seq | 3);
                    }
                }
            }
        }
      if (!EMIT)
        { symmin = wave_min_i(symmin);
          if (l == 0 && symmin != 0x7fffffff)
            atomicMin(&g.minfirst[a], symmin);
        }
    }
}

void damar_launch_graph_count(const GraphArgs *a, hipStream_t st)
{ if (a->npiles > 0)
    hipLaunchKernelGGL(graph_pile<false>, dim3(blocks_for(a->npiles, GR_WAVES)), dim3(GR_THREADS), 0, st, *a);
}

void damar_launch_graph_emit(const GraphArgs *a, hipStream_t st)
{ if (a->npiles > 0)
    hipLaunchKernelGGL(graph_pile<true>, dim3(blocks_for(a->npiles, GR_WAVES)), dim3(GR_THREADS), 0, st, *a);
}

/***** after the last batch ***********************************************************************/

__device__ __forceinline__ bool sym_hit(const GraphArgs &g, int a, int b)
{ return g.hasfirst[a] != 0 && g.minfirst[b] <= a; }

__global__ __launch_bounds__(GR_THREADS)
void graph_settle(GraphArgs g)
{ const u64 stride = (u64) gridDim.x * GR_THREADS;
  const u64 n = g.ncand > g.nprobe ? g.ncand : g.nprobe;
  const u64 rounds = (n + stride - 1) / stride;
  u32 ne = 0, nre = 0, nsym = 0, nleft = 0;      /* per lane */
  for (u64 k = 0; k < rounds; k++)
    { const u64 i = k * stride + (u64) blockIdx.x * GR_THREADS + threadIdx.x;
      if (i < g.ncand)
        { int *c = g.cand + GE_INTS * i;
          const int w = c[10];
          if (!(w & 1)) nleft += 1;
          if (!(w & 8) || sym_hit(g, c[11], c[12]))
            { for (int j = 0; j < 9; j++) c[j] = 0;
              c[13] = 0;                          /* an edge of zeros */
            }
          else
            { c[13] = 1;
              atomicOr(&g.status[c[9]], (u32) DAMAR_OG_PROPER);
              if (w & 2) nre += 1; else ne += 1;
            }
          g.key[i] = ((u64) (u32) c[15] << 32) | (u32) c[14];
          g.val[i] = (u32) i;
        }
      if (i < g.nprobe)
        nsym += sym_hit(g, (int) (g.probe[i] >> 32), (int) (u32) g.probe[i]) ? 1 : 0;
    }
  const int se = wave_sum_i((int) ne), sr = wave_sum_i((int) nre), ss = wave_sum_i((int) nsym), sl = wave_sum_i((int) nleft);
  if (lane_id() == 0)
    { if (se) atomicAdd(&g.ctr[GC_EDGES], (u64) se);
      if (sr) atomicAdd(&g.ctr[GC_REDGES], (u64) sr);
      if (ss) atomicAdd(&g.ctr[GC_SYM], (u64) ss);
      if (sl) atomicAdd(&g.ctr[GC_LEFT], (u64) sl);
    }
}

__global__ __launch_bounds__(GR_THREADS)
void graph_keys(GraphArgs g)
{ const u64 stride = (u64) gridDim.x * GR_THREADS;
  for (u64 i = (u64) blockIdx.x * GR_THREADS + threadIdx.x; i < g.ncand; i += stride)
    { const u32 v = g.val_in[i];
      const int *c = g.cand + GE_INTS * (u64) v;
      const u64 list = (u64) (c[10] & 1) * g.nreads + (u32) c[9];
      g.key[i] = (list << (g.rbits + 1)) | ((u64) (u32) c[1] << 1) | (u32) c[13];
      g.val[i] = v;
    }
}

__global__ __launch_bounds__(GR_THREADS)
void graph_bounds(GraphArgs g)
{ const u64 stride = (u64) gridDim.x * GR_THREADS;
  for (u64 i = (u64) blockIdx.x * GR_THREADS + threadIdx.x; i < g.ncand; i += stride)
    { const u64 list = g.key[i] >> (g.rbits + 1);
      if (i == 0 || (g.key[i - 1] >> (g.rbits + 1)) != list) g.beg[list] = (u32) i;
      if (i + 1 == g.ncand || (g.key[i + 1] >> (g.rbits + 1)) != list) g.end[list] = (u32) (i + 1);
    }
}

/* remove_dupes drops the earlier of two neighbours with one b; the comparison reads a b before that edge is dropped, so the
   flags of a list do not depend on one another.  remove_lr_dupes then walks the left list in order and, per left edge,
   every right edge: equal b drops the right edge and counts.  The b of the edges both lists keep are distinct within a
   list (the lists are sorted), so a kept left edge meets one right edge at most; a DROPPED left edge (b == -1) meets every
   right edge that is dropped by then -- those remove_dupes dropped and those the left edges before it took -- and counts
   each again.  With m[i] = 1 where kept left edge i has a partner: count = sum m[i] + sum over dropped left edges i of
   (dropped right edges + sum of m before i). */
__global__ __launch_bounds__(GR_THREADS)
void graph_reads(GraphArgs g)
{ __shared__ int  Lb[GR_WAVES][DAMAR_GRAPH_MAXDEG], Rb[GR_WAVES][DAMAR_GRAPH_MAXDEG];
  __shared__ u8   hit[GR_WAVES][DAMAR_GRAPH_MAXDEG], mL[GR_WAVES][DAMAR_GRAPH_MAXDEG];
  const int l = lane_id(), w = threadIdx.x >> 6;
  const u32 nwaves = gridDim.x * GR_WAVES;
  u64 counted = 0;                                /* per wave, in lane 0 */
  for (u32 r = blockIdx.x * GR_WAVES + w; r < g.nreads; r += nwaves)
    { const u32 lb = g.beg[r], rb = g.beg[g.nreads + r];
      const int nl = (int) (g.end[r] - lb), nr = (int) (g.end[g.nreads + r] - rb);
      if (nl == 0 && nr == 0)
        continue;
      if (nl > g.maxdeg || nr > g.maxdeg)
        { for (int i = l; i < nl; i += WAVE) g.keep[lb + i] = 1;
          for (int j = l; j < nr; j += WAVE) g.keep[rb + j] = 1;
          if (l == 0)
            { g.hostread[r] = 1;  g.kcount[r] = (u32) nl;  g.kcount[g.nreads + r] = (u32) nr; }
          continue;
        }
      for (int i = l; i < nl; i += WAVE) Lb[w][i] = g.cand[GE_INTS * (u64) g.val[lb + i] + 1];
      for (int j = l; j < nr; j += WAVE) { Rb[w][j] = g.cand[GE_INTS * (u64) g.val[rb + j] + 1];  hit[w][j] = 0; }
      wave_mem_sync();
      int dl = 0, dr = 0;
      for (int i = l; i < nl; i += WAVE) dl += (i + 1 < nl && Lb[w][i + 1] == Lb[w][i]);
      for (int j = l; j < nr; j += WAVE) dr += (j + 1 < nr && Rb[w][j + 1] == Rb[w][j]);
      dl = wave_sum_i(dl);  dr = wave_sum_i(dr);
      for (int i = l; i < nl; i += WAVE)
        { const bool gone = i + 1 < nl && Lb[w][i + 1] == Lb[w][i];
          const int  v = Lb[w][i];
          int m = 0;
          if (!gone)
            for (int j = 0; j < nr; j++)
              if (Rb[w][j] == v && !(j + 1 < nr && Rb[w][j + 1] == v))
                { hit[w][j] = 1;
                  m = 1;
                }
          mL[w][i] = (u8) (gone ? 2 : m);
        }
      wave_mem_sync();
      int sum = 0, before = 0;
      for (int c0 = 0; c0 < nl; c0 += WAVE)
        { const int i = c0 + l;
          const int t = i < nl ? mL[w][i] : 0;
          const u64 bal = wballot(t == 1);
          if (t == 1) sum += 1;
          if (t == 2) sum += dr + before + __builtin_popcountll(bal & lanes_below(l));
          before += __builtin_popcountll(bal);
        }
      sum = wave_sum_i(sum);
      int kl = 0, kr = 0;
      for (int i = l; i < nl; i += WAVE)
        { const u32 k = mL[w][i] != 2;
          g.keep[lb + i] = k;
          kl += (int) k;
        }
      for (int j = l; j < nr; j += WAVE)
        { const u32 k = !(j + 1 < nr && Rb[w][j + 1] == Rb[w][j]) && !hit[w][j];
          g.keep[rb + j] = k;
          kr += (int) k;
        }
      kl = wave_sum_i(kl);  kr = wave_sum_i(kr);
      if (l == 0)
        { g.kcount[r] = (u32) kl;  g.kcount[g.nreads + r] = (u32) kr;
          counted += (u64) (dl + dr + sum);
        }
      wave_mem_sync();
    }
  if (l == 0 && counted)
    atomicAdd(&g.ctr[GC_PARALLEL], counted);
}

__global__ __launch_bounds__(GR_THREADS)
void graph_gather(GraphArgs g)
{ const u64 stride = (u64) gridDim.x * GR_THREADS;
  for (u64 i = (u64) blockIdx.x * GR_THREADS + threadIdx.x; i < g.ncand; i += stride)
    if (g.keep[i])
      { const int *c = g.cand + GE_INTS * (u64) g.val[i];
        int *o = g.out + 9 * (u64) g.pos[i];
        for (int j = 0; j < 9; j++) o[j] = c[j];
      }
}

void damar_launch_graph_settle(const GraphArgs *a, hipStream_t st)
{ const u64 n = a->ncand > a->nprobe ? a->ncand : a->nprobe;
  if (n > 0)
    hipLaunchKernelGGL(graph_settle, dim3(blocks_for(n, GR_THREADS)), dim3(GR_THREADS), 0, st, *a);
}
void damar_launch_graph_keys(const GraphArgs *a, hipStream_t st)
{ if (a->ncand > 0)
    hipLaunchKernelGGL(graph_keys, dim3(blocks_for(a->ncand, GR_THREADS)), dim3(GR_THREADS), 0, st, *a);
}
void damar_launch_graph_bounds(const GraphArgs *a, hipStream_t st)
{ if (a->ncand > 0)
    hipLaunchKernelGGL(graph_bounds, dim3(blocks_for(a->ncand, GR_THREADS)), dim3(GR_THREADS), 0, st, *a);
}
void damar_launch_graph_reads(const GraphArgs *a, hipStream_t st)
{ if (a->ncand > 0)
    hipLaunchKernelGGL(graph_reads, dim3(blocks_for(a->nreads, GR_WAVES)), dim3(GR_THREADS), 0, st, *a);
}
void damar_launch_graph_gather(const GraphArgs *a, hipStream_t st)
{ if (a->ncand > 0)
    hipLaunchKernelGGL(graph_gather, dim3(blocks_for(a->ncand, GR_THREADS)), dim3(GR_THREADS), 0, st, *a);
}
