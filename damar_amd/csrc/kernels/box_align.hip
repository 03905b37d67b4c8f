/* box_align.hip -- exact alignment of a batch of small boxes with their edit scripts, for gfx950: what
 * Compute_Alignment(DIFF_ALIGN) gives (align.c:4734, through dandc_nd :4653 and split_nd :4327); the plain version is
 * host/bridge.c damar_exact_box, and the rules marked "tie rule" there are the ones kept here, value for value.
 *
 * A box is A[0..M) against B[0..N), a trace segment of an overlap: M at most one trace spacing, N a little more.  The
 * algorithm is Myers' O(ND) search in its linear-space form: a forward and a backward frontier of furthest rows per
 * diagonal advance one difference at a time until they meet, the meeting point cuts the box in two, and both halves are
 * done the same way until a box holds at most one difference.
 *
 * One wavefront (a workgroup of 64 lanes) per box, boxes dealt to workgroups in a grid-stride loop:
 *   - the box's bases, both frontiers (two buffers each: a new frontier is computed out of the complete old one, which is
 *     what lets the diagonals be dealt to the lanes) and the stack of boxes still to do live in LDS, about 10.5 KB;
 *   - a frontier step gives lane i the i-th diagonal from the top; the reference sweeps the diagonals downwards and stops
 *     at the first that runs into the other frontier, so the lowest lane of the ballot is the meeting point;
 *   - the extension along a diagonal is a byte loop per lane over LDS; the lanes of a step finish at different times,
 *     which is the price of keeping one box inside one wavefront and all state out of HBM;
 *   - the script goes straight to the box's slot in global memory (max(M, N) values at most, its indels in path order).
 * Integer work only, no atomics.  Every loop is bounded whatever the bases hold: the search by the frontier's room, the
 * recursion by a step count; a box that hits a bound is reported with length -1 and done by the host routine.
 */
#include "dev_common.h"
#include "kernels.h"
#include "box_search.h"                   /* bx_middle: the search, shared with box_trace.hip */

#define BX_SPAN  1024                     /* rows per frontier buffer */
#define BX_HALF  (BX_SPAN / 2)
#define BX_STACK 32
#define BX_GRID  4096u

static_assert((DAMAR_BOX_MAXLEN + 1) / 2 <= BX_HALF - 3, "a frontier of a box of the largest size fits its buffer");

__global__ __launch_bounds__(WAVE)
void box_align(BoxArgs a)
{ __shared__ short s_f[2][BX_SPAN], s_g[2][BX_SPAN];
  __shared__ u8    s_base[2 * DAMAR_BOX_MAXLEN + 16];
  __shared__ short s_todo[BX_STACK][4];   /* boxes still to do: a0, m, b0, n inside the top box */
  const int l = lane_id();

  for (u32 box = blockIdx.x; box < a.nbox; box += gridDim.x)
    { const int M = a.m[box], N = a.n[box];
      const int cap = (M > N) ? M : N;
      if (M < 1 || N < 1 || cap > a.maxlen)                    /* the host routine's */
        continue;
      const u8 *ga = a.bases + a.aoff[box], *gb = a.bases + a.boff[box];
      int *out = a.script + a.coff[box];
      int  pos = 0, total = -1, sp = 1, steps = 0, bad = 0;

      __syncthreads();
      for (int i = l; i < M; i += WAVE) s_base[i] = ga[i];
      for (int i = l; i < N; i += WAVE) s_base[M + i] = gb[i];
      if (l == 0)
        { s_todo[0][0] = 0;  s_todo[0][1] = (short) M;  s_todo[0][2] = 0;  s_todo[0][3] = (short) N; }
      __syncthreads();

      while (sp > 0 && !bad)
        { sp -= 1;
          const int a0 = s_todo[sp][0], m = s_todo[sp][1], b0 = s_todo[sp][2], n = s_todo[sp][3];
          if (++steps > 4 * cap + 16)
            { bad = 1;
              break;
            }
          if (m <= 0)                                          /* only B left: n bases of B alone at this point of A */
            { for (int i = l; i < n; i += WAVE)
                if (pos + i < cap) out[pos + i] = -a0 - 1;
              pos += n;
              continue;
            }
          if (n <= 0)
            { for (int i = l; i < m; i += WAVE)
                if (pos + i < cap) out[pos + i] = b0 + 1;
              pos += m;
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
            { if (sp + 2 > BX_STACK)
                { bad = 1;
                  break;
                }
              __syncthreads();
              if (l == 0)                                      /* tie rule: the half in front of the meeting point first */
                { s_todo[sp][0] = (short) (a0 + col);  s_todo[sp][1] = (short) (m - col);
                  s_todo[sp][2] = (short) (b0 + row);  s_todo[sp][3] = (short) (n - row);
                  s_todo[sp + 1][0] = (short) a0;  s_todo[sp + 1][1] = (short) col;
                  s_todo[sp + 1][2] = (short) b0;  s_todo[sp + 1][3] = (short) row;
                }
              sp += 2;
              __syncthreads();
            }
          else if (D == 1 && m != n)                           /* tie rule: a square box holds a substitution, no entry */
            { if (l == 0 && pos < cap)
                out[pos] = (m > n) ? b0 + row + 1 : -(a0 + col) - 1;
              pos += 1;
            }
        }
      if (l == 0)
        { a.diffs[box] = total;
          a.slen[box] = (bad || pos > cap) ? -1 : pos;
        }
    }
}

void damar_launch_box_align(const BoxArgs *a, hipStream_t st)
{ if (a->nbox > 0)
    hipLaunchKernelGGL(box_align, dim3(a->nbox < BX_GRID ? a->nbox : BX_GRID), dim3(WAVE), 0, st, *a);
}

u32 damar_box_align_grid(void) { return BX_GRID; }
