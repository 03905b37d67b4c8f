/* read_search.h -- the two-frontier search of kernels/read_align.hip: the middle of an optimal path of a box of read length,
 * by one workgroup of THREADS lanes (host/bridge.c middle, align.c:4327-4495 split_nd).  It is the search of box_search.h
 * with three things changed: the bases stay in global memory and a slide compares eight of them per load; the frontier
 * rows are int; and a frontier step is dealt over all wavefronts of the workgroup, the meeting point taken by a reduction
 * across them.  SPAN, the rows of one frontier buffer, bounds the differences and not the length: a search that reaches d
 * differences on either side touches the diagonals -d .. d around its corner, 2d + 3 rows with the rim, whatever M and N
 * are.  The rules marked "tie rule" are bridge.c's, value for value. */
#ifndef DAMAR_READ_SEARCH_H
#define DAMAR_READ_SEARCH_H

#include <limits.h>
#include "dev_common.h"

__device__ __forceinline__ u64 rd_load8(const u8 *p)      /* eight bases from any address, the first in the low byte */
{ u64 v;
  __builtin_memcpy(&v, p, 8);
  return v;
}

/* bx_slide_fwd: along diagonal k from row r while the bases agree, and it stops at the base that one stops at */
__device__ __forceinline__ int rd_slide_fwd(const u8 *A, const u8 *B, int M, int N, int k, int r)
{ const int end = (N < M - k) ? N : M - k;
  if (r < 0 || k + r < 0)
    return r;
  while (r + 8 <= end)
    { const u64 x = rd_load8(B + r) ^ rd_load8(A + k + r);
      if (x != 0)
        return r + (__builtin_ctzll(x) >> 3);
      r += 8;
    }
  while (r < end && B[r] == A[k + r])
    r += 1;
  return r;
}

/* bx_slide_bwd: r only falls, so its two upper bounds are looked at once */
__device__ __forceinline__ int rd_slide_bwd(const u8 *A, const u8 *B, int M, int N, int k, int r)
{ const int top = (-k > 0) ? -k : 0;
  if (r >= N || k + r >= M)
    return r;
  while (r - 7 >= top)
    { const u64 x = rd_load8(B + r - 7) ^ rd_load8(A + k + r - 7);
      if (x != 0)
        return r - (__builtin_clzll(x) >> 3);
      r -= 8;
    }
  while (r >= top && B[r] == A[k + r])
    r -= 1;
  return r;
}

/* the smallest `best` of the workgroup (INT_MAX: nobody has one): the wavefronts' minima meet in red[0 .. THREADS / WAVE).
   The barrier inside also publishes the frontier the step wrote. */
template <int THREADS>
__device__ __forceinline__ int rd_first_hit(int best, int *red, int t)
{ const int w = wave_min_i(best);
  if ((t & (WAVE - 1)) == 0)
    red[t / WAVE] = w;
  __syncthreads();
  int win = red[0];
  for (int i = 1; i < THREADS / WAVE; i++)
    win = (red[i] < win) ? red[i] : win;
  return win;
}

/* Middle of an optimal path of the box (bridge.c middle): returns the box's differences, *col / *row the meeting point;
   -1 when either search would pass dmax differences.  All lanes call it and all get the same answer.  A step deals the
   diagonals from the top down, lane t taking the t-th, the (t + THREADS)-th and so on; the reference sweeps downwards and
   stops at the first diagonal that runs into the other frontier, so the hit with the smallest index of the whole step is
   the meeting point.  The new frontier goes to the other buffer, so what the lanes below the hit still write changes
   nothing that is returned.  red: two sets of reduction slots used in turn, so that a wavefront ahead by one step does not
   write what a slower one still reads; mt: two ints. */
template <int SPAN, int THREADS>
__device__ int rd_middle(const u8 *A, int M, const u8 *B, int N, int (*F)[SPAN], int (*G)[SPAN], int (*red)[THREADS / WAVE],
                         int *mt, int dmax, int t, int *col, int *row)
{ constexpr int HALF = SPAN / 2;
  const int del = M - N;
  int flo = 0, fhi = 0, fc = 0, glo = del, ghi = del, gc = 0, par = 0;
  const int r0 = rd_slide_fwd(A, B, M, N, 0, 0);
  if (r0 >= M && N == M)                  /* the box is a single run of matches */
    { *col = *row = M;
      return 0;
    }
  __syncthreads();
  if (t == 0)
    { F[0][HALF] = r0;
      G[0][HALF] = rd_slide_bwd(A, B, M, N, del, N - 1);
    }
  __syncthreads();

  for (int d = 1; d <= dmax && d <= HALF - 3; d++)
    { /* forward: diagonals fhi + 1 down to flo - 1 */
      int cnt = fhi - flo + 3, best = INT_MAX, brow = 0;
      for (int i = t; i < cnt; i += THREADS)
        { const int k = fhi + 1 - i;
          const int right = ((k + 1 <= fhi) ? F[fc][k + 1 + HALF] : (k + 1 > fhi + 1) ? -3 : -2) + 1;
          const int diag  = ((k >= flo && k <= fhi) ? F[fc][k + HALF] : (k > fhi + 1) ? -3 : -2) + 1;
          const int down  = (k - 1 >= flo) ? F[fc][k - 1 + HALF] : -2;
          int r = right > diag ? right : diag;
          if (down > r) r = down;
          if (k >= glo && k <= ghi)
            { const int wall = G[gc][k - del + HALF];
              if (r > wall)
                { best = i;               /* tie rule: the first of (right, diag) past the other search, else just below it */
                  brow = (right > wall) ? right : (diag > wall) ? diag : wall + 1;
                  break;
                }
            }
          F[fc ^ 1][k + HALF] = rd_slide_fwd(A, B, M, N, k, r);
        }
      int win = rd_first_hit<THREADS>(best, red[par], t);
      par ^= 1;
      if (win != INT_MAX)
        { if (best == win)
            { mt[0] = brow;
              mt[1] = fhi + 1 - win + brow;
            }
          __syncthreads();
          *row = mt[0];
          *col = mt[1];
          return 2 * d - 1;
        }
      fc ^= 1;  flo -= 1;  fhi += 1;

      /* backward, against the forward frontier of the same number of differences */
      cnt = ghi - glo + 3;
      best = INT_MAX;
      for (int i = t; i < cnt; i += THREADS)
        { const int k = ghi + 1 - i;
          const int left = ((k + 1 <= ghi) ? G[gc][k + 1 - del + HALF] : N + 1) + 1;
          const int diag = (k >= glo && k <= ghi) ? G[gc][k - del + HALF] : N + 1;
          const int up   = (k - 1 >= glo) ? G[gc][k - 1 - del + HALF] : N + 1;
          int r = left < diag ? left : diag;
          if (up < r) r = up;
          if (k >= flo && k <= fhi)
            { const int wall = F[fc][k + HALF];
              if (r <= wall)
                { best = i;               /* tie rule, mirrored */
                  brow = (left <= wall) ? left : (diag <= wall) ? diag : wall;
                  break;
                }
            }
          G[gc ^ 1][k - del + HALF] = rd_slide_bwd(A, B, M, N, k, r - 1);
        }
      win = rd_first_hit<THREADS>(best, red[par], t);
      par ^= 1;
      if (win != INT_MAX)
        { if (best == win)
            { mt[0] = brow;
              mt[1] = ghi + 1 - win + brow;
            }
          __syncthreads();
          *row = mt[0];
          *col = mt[1];
          return 2 * d;
        }
      gc ^= 1;  glo -= 1;  ghi += 1;
    }
  return -1;
}

#endif
