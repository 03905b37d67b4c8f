/* box_trace.hip -- exact alignment of a batch of boxes into trace pairs, for gfx950: what Compute_Alignment(DIFF_TRACE)
 * leaves in path->diffs, path->tlen and path->trace (align.c:4734-4869, through trace_nd :4497 and split_nd :4327); the
 * plain version is host/bridge.c settle / realign_box, and the rules marked "tie rule" there are the ones kept here, value
 * for value.  This is the realignment of LAstitch's joints (host/stitch.c): a box spans four trace intervals and the
 * joint at least, a few thousand bases at most, and a complement joint is aligned against coordinates that leave the two
 * sides close to unrelated, so a box may carry as many differences as it has columns.
 *
 * A box is A[0..M) against B[0..N); A's position 0 lies `abpos` bases into A's own grid of `tspace`, and the result is one
 * (differences, B length) pair per interval of that grid the box touches.  The search is box_search.h's, the one
 * box_align.hip runs: two frontiers of furthest rows per diagonal, advanced one difference at a time until they meet.  The
 * meeting point cuts the box in two; a half that lies inside one interval is booked whole (its differences and its B
 * length are all the ledger wants), a half that crosses a boundary is cut again, a box of at most one difference is
 * booked column by column.
 *
 * One wavefront (a workgroup of 64 lanes) per box, boxes dealt to workgroups in a grid-stride loop.  Everything of a box
 * lives in LDS until its pairs are written: the bases, both frontiers (two buffers each), the stack of boxes still to do
 * and the ledger cells.  The lanes share the diagonals of a frontier step; lane 0 does the ledger arithmetic, a handful of
 * additions per cut.  The kernel is built for two sizes, and a batch is two launches that each take their own boxes (the
 * second one from a list of the large boxes, with no more workgroups than the list is long):
 *
 *                      max(M, N)      frontiers   bases   cells + stack   LDS per workgroup   workgroups per CU (160 KiB)
 *   box_trace<1032>    1 .. 1024        8,256 B   2,064 B     1,344 B           11,664 B        14
 *   box_trace<4104>    1025 .. 4096    32,832 B   8,208 B     1,344 B           42,384 B         3
 *
 * A frontier buffer holds SPAN shorts: a search reaches ceil(D / 2) differences and a box holds D <= max(M, N) of them
 * whatever its bases are, so 2,052 diagonals either side of the corner's are room for every box of 4,096 -- unrelated
 * sides included.  The stitch boxes of a file at spacing 100 (400 to 700 bases) are all the first launch's, at fourteen
 * wavefronts per CU; keeping them out of the large build is what the second size is for: at 42 KB a box they would
 * run three to a CU.
 * Integer work only, no atomics, plain vector stores.  Every loop is bounded whatever the bases hold: the search by the
 * frontier's room, the recursion by a step count, the stack by its depth, the ledger by its cells; a box that hits a bound
 * is reported with length -1 and done by the host routine, as is one larger than the kernel keeps.
 */
#include "dev_common.h"
#include "kernels.h"
#include "box_search.h"

#define TB_CELLS 512                      /* ledger cells of a box: 255 intervals and the spare one */
#define TB_STACK 40
#define TB_GRID  4096u
#define TB_SMALL 1024                     /* the largest box of the first launch */

template <int SPAN, int MAXLEN, bool LISTED>
__global__ __launch_bounds__(WAVE)
void box_trace(TBoxArgs a, int above, int upto)
{ static_assert((MAXLEN + 1) / 2 <= SPAN / 2 - 3, "a frontier of a box of the largest size fits its buffer");
  __shared__ short s_f[2][SPAN], s_g[2][SPAN];
  __shared__ u8    s_base[2 * MAXLEN + 16];
  __shared__ u16   s_cell[TB_CELLS];
  __shared__ short s_todo[TB_STACK][4];   /* boxes still to do: a0, m, b0, n inside the top box */
  const int l = lane_id();
  const int ts = a.tspace;

  /* the first launch passes over all boxes, the second over the list of the large ones */
  const u32 nwork = LISTED ? a.nlarge : a.nbox;
  for (u32 w = blockIdx.x; w < nwork; w += gridDim.x)
    { const u32 box = LISTED ? a.large[w] : w;
      if (box >= a.nbox)
        continue;
      const int M = a.m[box], N = a.n[box];
      const int cap = (M > N) ? M : N;
      if (M < 1 || N < 1 || cap <= above || cap > upto || cap > MAXLEN)        /* the other launch's, or the host routine's */
        continue;
      const int org = a.abpos[box] % ts;                       /* where the box begins in its first interval */
      const int ncell = 2 * ((org + M + ts - 1) / ts + 1);     /* one interval beyond the last */
      if (org < 0 || ncell > TB_CELLS)
        continue;
      const u8 *ga = a.bases + a.aoff[box], *gb = a.bases + a.boff[box];
      int total = -1, sp = 1, steps = 0, bad = 0;

      __syncthreads();
      for (int i = l; i < M; i += WAVE) s_base[i] = ga[i];
      for (int i = l; i < N; i += WAVE) s_base[M + i] = gb[i];
      for (int i = l; i < ncell; i += WAVE) s_cell[i] = 0;
      if (l == 0)
        { s_todo[0][0] = 0;  s_todo[0][1] = (short) M;  s_todo[0][2] = 0;  s_todo[0][3] = (short) N; }
      __syncthreads();

      /* the ledger (bridge.c): lane 0's.  at: bases from the grid line in front of the box */
#define CELL_ADD(i, dd, bl) do { if (2 * (i) + 1 < ncell) { s_cell[2 * (i)] += (u16) (dd);  s_cell[2 * (i) + 1] += (u16) (bl); } else bad = 1; } while (0)
#define ROOM(at) ((((at) / ts) + 1) * ts - (at))

      while (sp > 0)
        { bad = __shfl(bad, 0);                                /* lane 0 keeps the ledger and is the one to find it full */
          if (bad)
            break;
          sp -= 1;
          const int a0 = s_todo[sp][0], m = s_todo[sp][1], b0 = s_todo[sp][2], n = s_todo[sp][3];
          if (++steps > 4 * cap + 16)
            { bad = 1;
              break;
            }
          if (m <= 0)                                          /* only B left: n insertions at this point of A */
            { if (l == 0)
                CELL_ADD((org + a0) / ts, n, n);
              continue;
            }
          if (n <= 0)                                          /* bases of A with nothing opposite, dealt to their intervals */
            { if (l == 0)
                { int at = org + a0, len = m, take = ROOM(at);
                  for (int i = at / ts; len > 0; len -= take, take = ts, i++)
                    { if (take > len) take = len;
                      CELL_ADD(i, take, 0);
                    }
                }
              continue;
            }
          int col = 0, row = 0;
          const int D = bx_middle(s_base + a0, m, s_base + M + b0, n, s_f, s_g, l, &col, &row);
          if (D < 0 || col < 0 || col > m || row < 0 || row > n)
            { bad = 1;
              break;
            }
          if (total < 0)
            total = D;
          if (D >= 2)
            { /* tie rule: a half is booked whole when it does not cross a trace boundary, else it is cut again */
              const bool front_whole = ROOM(org + a0) >= col;
              const bool back_whole  = ROOM(org + a0 + col) >= m - col;
              const int  push = (front_whole ? 0 : 1) + (back_whole ? 0 : 1);
              if (sp + push > TB_STACK)
                { bad = 1;
                  break;
                }
              __syncthreads();
              if (l == 0)
                { int top = sp;
                  if (front_whole)
                    CELL_ADD((org + a0) / ts, (D + 1) / 2, row);
                  if (back_whole)
                    CELL_ADD((org + a0 + col) / ts, D / 2, n - row);
                  else
                    { s_todo[top][0] = (short) (a0 + col);  s_todo[top][1] = (short) (m - col);
                      s_todo[top][2] = (short) (b0 + row);  s_todo[top][3] = (short) (n - row);
                      top += 1;
                    }
                  if (!front_whole)
                    { s_todo[top][0] = (short) a0;  s_todo[top][1] = (short) col;
                      s_todo[top][2] = (short) b0;  s_todo[top][3] = (short) row;
                    }
                }
              sp += push;
              __syncthreads();
            }
          else if (l == 0)
            { /* zero or one difference: matches up to it, the difference, matches behind it.  tie rule: the meeting point
                 sits behind the difference when A is not the shorter side, on it otherwise */
              const int lone_a = (D == 1 && m >= n);
              const int head = lone_a ? col - 1 : col;
              if (head < 0)
                bad = 1;
              for (int part = 0; part < 2 && !bad; part++)
                { int at = org + a0 + (part ? col : 0), len = part ? m - col : head, take = ROOM(at);
                  if (part == 1 && D == 0)
                    break;
                  for (int i = at / ts; len > 0; len -= take, take = ts, i++)
                    { if (take > len) take = len;
                      CELL_ADD(i, 0, take);
                    }
                  if (part == 0 && D == 1)
                    CELL_ADD((org + a0 + head) / ts, 1, (m <= n) ? 1 : 0);
                }
            }
        }
#undef CELL_ADD
#undef ROOM
      bad = __shfl(bad, 0);
      __syncthreads();
      if (l == 0 && s_cell[ncell - 1] != 0)                    /* insertions booked exactly on the last boundary belong to
                                                                  the interval before it */
        { s_cell[ncell - 3] += s_cell[ncell - 1];
          s_cell[ncell - 4] += s_cell[ncell - 2];
        }
      __syncthreads();
      if (!bad)
        { u16 *out = a.trace + a.toff[box];
          for (int i = l; i < ncell - 2; i += WAVE)
            out[i] = s_cell[i];
        }
      if (l == 0)
        { a.diffs[box] = total;
          a.tlen[box] = bad ? -1 : ncell - 2;
        }
    }
}

void damar_launch_box_trace(const TBoxArgs *a, hipStream_t st)
{ if (a->nbox == 0)
    return;
  const dim3 grid(a->nbox < TB_GRID ? a->nbox : TB_GRID);
  hipLaunchKernelGGL((box_trace<1032, TB_SMALL, false>), grid, dim3(WAVE), 0, st, *a, 0, a->maxlen < TB_SMALL ? a->maxlen : TB_SMALL);
  if (a->nlarge > 0 && a->maxlen > TB_SMALL)                   /* 42 KB of LDS a workgroup: only as many as there are large boxes */
    hipLaunchKernelGGL((box_trace<4104, DAMAR_TBOX_MAXLEN, true>), dim3(a->nlarge < TB_GRID ? a->nlarge : TB_GRID), dim3(WAVE), 0, st, *a,
                       TB_SMALL, a->maxlen);
}

u32 damar_box_trace_grid(void) { return TB_GRID; }
u32 damar_box_trace_small(void) { return TB_SMALL; }
