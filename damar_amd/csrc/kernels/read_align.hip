/* read_align.hip -- exact alignment of a batch of boxes of read length with their edit scripts, for gfx950: what
 * Compute_Alignment(DIFF_ALIGN) gives for a read against its correction (LAcorrect's " postrace="); the plain version is
 * host/bridge.c damar_exact_box, the small-box version kernels/box_align.hip, and the tie rules are theirs, value for value.
 *
 * What a box of 5 to 100 kb with differences in the low thousands needs is room for its differences, not for its length:
 *   - one workgroup of RA_THREADS lanes (eight wavefronts) per box does the whole divide and conquer of script_box; the
 *     boxes are dealt longest first, a workgroup taking box order[w], order[w + grid], ...;
 *   - the four frontier buffers are int rows in LDS, 4 x RA_SPAN x 4 bytes = 128 KB of the CU's 160 KB, so one workgroup is
 *     resident per CU and the eight wavefronts are what hides the latency of the base loads.  A search that reaches d
 *     differences per side uses 2d + 3 rows, so RA_SPAN = 8192 holds every box of DAMAR_READ_MAXDIFF = 8000 differences at
 *     any length;
 *   - the bases stay in global memory: a pair of reads does not fit beside the frontiers.  The slide along a diagonal
 *     compares eight bases per load (read_search.h);
 *   - a frontier step deals its diagonals from the top down over all lanes, and the meeting point is the hit of smallest
 *     index, by a reduction across the wavefronts: one barrier per step;
 *   - the stack of boxes still to do is explicit: differences halve per level, so 64 entries are room to spare;
 *   - the script goes to the box's slot in global memory in path order.
 * Integer work only, plain vector stores, no atomics.  Every loop is bounded whatever the bases hold: a search by the
 * difference bound, the recursion by a step count; a box that hits a bound is reported with length -1 and is the host
 * routine's.
 */
#include "dev_common.h"
#include "kernels.h"
#include "read_search.h"

#define RA_THREADS 512
#define RA_SPAN    8192                   /* rows per frontier buffer */
#define RA_HALF    (RA_SPAN / 2)
#define RA_STACK   64
#define RA_GRID    4096u

static_assert((DAMAR_READ_MAXDIFF + 1) / 2 <= RA_HALF - 3, "the frontiers of a box of the most differences fit their buffers");

__global__ __launch_bounds__(RA_THREADS)
void read_align(BoxArgs a)
{ __shared__ int s_f[2][RA_SPAN], s_g[2][RA_SPAN];
  __shared__ int s_todo[RA_STACK][4];     /* boxes still to do: a0, m, b0, n inside the top box */
  __shared__ int s_red[2][RA_THREADS / WAVE];
  __shared__ int s_meet[2];
  const int t = (int) threadIdx.x;
  const int dmax = (a.maxdiff + 1) / 2;   /* what either search of a box of maxdiff differences reaches */

  for (u32 at = blockIdx.x; at < a.nbox; at += gridDim.x)
    { const u32 box = a.order[at];
      if (box >= a.nbox)
        continue;
      const int M = a.m[box], N = a.n[box];
      const int cap = (M > N) ? M : N;
      if (M < 1 || N < 1 || cap > DAMAR_READ_MAXLEN)           /* the host routine's */
        continue;
      const u8 *ga = a.bases + a.aoff[box], *gb = a.bases + a.boff[box];
      int *out = a.script + a.coff[box];
      int  pos = 0, total = -1, sp = 1, steps = 0;
      int  bad = (M - N > a.maxdiff || N - M > a.maxdiff);     /* as many differences at the least */

      __syncthreads();
      if (t == 0)
        { s_todo[0][0] = 0;  s_todo[0][1] = M;  s_todo[0][2] = 0;  s_todo[0][3] = N; }
      __syncthreads();

      while (sp > 0 && !bad)
        { sp -= 1;
          const int a0 = s_todo[sp][0], m = s_todo[sp][1], b0 = s_todo[sp][2], n = s_todo[sp][3];
          if (++steps > 4 * cap + 16)
            { bad = 1;
              break;
            }
          if (m <= 0)                                          /* only B left: n bases of B alone at this point of A */
            { for (int i = t; i < n; i += RA_THREADS)
                if (pos + i < cap) out[pos + i] = -a0 - 1;
              pos += n;
              continue;
            }
          if (n <= 0)
            { for (int i = t; i < m; i += RA_THREADS)
                if (pos + i < cap) out[pos + i] = b0 + 1;
              pos += m;
              continue;
            }
          int col = 0, row = 0;
          const int D = rd_middle<RA_SPAN, RA_THREADS>(ga + a0, m, gb + b0, n, s_f, s_g, s_red, s_meet, dmax, t, &col, &row);
          if (D < 0 || col < 0 || col > m || row < 0 || row > n)
            { bad = 1;
              break;
            }
          if (total < 0)
            { total = D;
              if (D > a.maxdiff)
                { bad = 1;
                  break;
                }
            }
          if (D >= 2)
            { if (sp + 2 > RA_STACK)
                { bad = 1;
                  break;
                }
              __syncthreads();
              if (t == 0)                                      /* tie rule: the half in front of the meeting point first */
                { s_todo[sp][0] = a0 + col;  s_todo[sp][1] = m - col;
                  s_todo[sp][2] = b0 + row;  s_todo[sp][3] = n - row;
                  s_todo[sp + 1][0] = a0;  s_todo[sp + 1][1] = col;
                  s_todo[sp + 1][2] = b0;  s_todo[sp + 1][3] = row;
                }
              sp += 2;
              __syncthreads();
            }
          else if (D == 1 && m != n)                           /* tie rule: a square box holds a substitution, no entry */
            { if (t == 0 && pos < cap)
                out[pos] = (m > n) ? b0 + row + 1 : -(a0 + col) - 1;
              pos += 1;
            }
        }
      if (t == 0)
        { a.diffs[box] = total;
          a.slen[box] = (bad || pos > cap) ? -1 : pos;
        }
    }
}

void damar_launch_read_align(const BoxArgs *a, u32 grid, hipStream_t st)
{ if (grid < 1 || grid > RA_GRID)
    grid = RA_GRID;
  if (a->nbox > 0)
    hipLaunchKernelGGL(read_align, dim3(a->nbox < grid ? a->nbox : grid), dim3(RA_THREADS), 0, st, *a);
}

u32 damar_read_align_grid(void) { return RA_GRID; }
