/* box_search.h -- the two-frontier search of the box kernels (box_align.hip, box_trace.hip): the middle of an optimal path
 * of a box, by one wavefront, with the frontiers in LDS (host/bridge.c middle, align.c:4327-4495 split_nd).  SPAN, the rows
 * of one frontier buffer, is the kernel's: a search reaches ceil(D / 2) differences on either side, and a box of A[0..M)
 * against B[0..N) holds D <= max(M, N) of them, so SPAN / 2 - 3 >= (max(M, N) + 1) / 2 holds every box of that size
 * whatever its bases are.  The rules marked "tie rule" are bridge.c's, value for value. */
#ifndef DAMAR_BOX_SEARCH_H
#define DAMAR_BOX_SEARCH_H

#include "dev_common.h"

__device__ __forceinline__ int bx_slide_fwd(const u8 *A, const u8 *B, int M, int N, int k, int r)
{ const int end = (N < M - k) ? N : M - k;
  while (r < end && k + r >= 0 && B[r] == A[k + r])
    r += 1;
  return r;
}

__device__ __forceinline__ int bx_slide_bwd(const u8 *A, const u8 *B, int M, int N, int k, int r)
{ const int top = (-k > 0) ? -k : 0;
  while (r >= top && r < N && k + r < M && B[r] == A[k + r])
    r -= 1;
  return r;
}

/* Middle of an optimal path of the box (bridge.c middle): returns the box's differences, *col / *row the meeting point;
   -1 when the frontiers outgrow their buffers.  All lanes call it and all get the same answer. */
template <int SPAN>
__device__ int bx_middle(const u8 *A, int M, const u8 *B, int N, short (*F)[SPAN], short (*G)[SPAN], int l, int *col, int *row)
{ constexpr int HALF = SPAN / 2;
  const int del = M - N;
  int flo = 0, fhi = 0, fc = 0, glo = del, ghi = del, gc = 0;
  const int r0 = bx_slide_fwd(A, B, M, N, 0, 0);
  if (r0 >= M && N == M)                  /* the box is a single run of matches */
    { *col = *row = M;
      return 0;
    }
  __syncthreads();
  if (l == 0)
    { F[0][HALF] = (short) r0;
      G[0][HALF] = (short) bx_slide_bwd(A, B, M, N, del, N - 1);
    }
  __syncthreads();

  for (int d = 1; d <= HALF - 3; d++)
    { /* forward: diagonals fhi + 1 down to flo - 1 */
      int cnt = fhi - flo + 3;
      for (int base = 0; base < cnt; base += WAVE)
        { const int  k = fhi + 1 - (base + l);
          const bool act = base + l < cnt;
          bool hit = false;
          int  r = 0, meet = 0;
          if (act)
            { const int right = ((k + 1 <= fhi) ? F[fc][k + 1 + HALF] : (k + 1 > fhi + 1) ? -3 : -2) + 1;
              const int diag  = ((k >= flo && k <= fhi) ? F[fc][k + HALF] : (k > fhi + 1) ? -3 : -2) + 1;
              const int down  = (k - 1 >= flo) ? F[fc][k - 1 + HALF] : -2;
              r = right > diag ? right : diag;
              if (down > r) r = down;
              if (k >= glo && k <= ghi)
                { const int wall = G[gc][k - del + HALF];
                  if (r > wall)
                    { hit = true;         /* tie rule: the first of (right, diag) past the other search, else just below it */
                      meet = (right > wall) ? right : (diag > wall) ? diag : wall + 1;
                    }
                }
            }
          const u64 met = wballot(hit);
          if (met != 0)
            { const int win = __ffsll((long long) met) - 1;
              *row = __shfl(meet, win);
              *col = __shfl(k, win) + *row;
              return 2 * d - 1;
            }
          if (act)
            F[fc ^ 1][k + HALF] = (short) bx_slide_fwd(A, B, M, N, k, r);
        }
      __syncthreads();
      fc ^= 1;  flo -= 1;  fhi += 1;

      /* backward, against the forward frontier of the same number of differences */
      cnt = ghi - glo + 3;
      for (int base = 0; base < cnt; base += WAVE)
        { const int  k = ghi + 1 - (base + l);
          const bool act = base + l < cnt;
          bool hit = false;
          int  r = 0, meet = 0;
          if (act)
            { const int left = ((k + 1 <= ghi) ? G[gc][k + 1 - del + HALF] : N + 1) + 1;
              const int diag = (k >= glo && k <= ghi) ? G[gc][k - del + HALF] : N + 1;
              const int up   = (k - 1 >= glo) ? G[gc][k - 1 - del + HALF] : N + 1;
              r = left < diag ? left : diag;
              if (up < r) r = up;
              if (k >= flo && k <= fhi)
                { const int wall = F[fc][k + HALF];
                  if (r <= wall)
                    { hit = true;         /* tie rule, mirrored */
                      meet = (left <= wall) ? left : (diag <= wall) ? diag : wall;
                    }
                }
            }
          const u64 met = wballot(hit);
          if (met != 0)
            { const int win = __ffsll((long long) met) - 1;
              *row = __shfl(meet, win);
              *col = __shfl(k, win) + *row;
              return 2 * d;
            }
          if (act)
            G[gc ^ 1][k - del + HALF] = (short) bx_slide_bwd(A, B, M, N, k, r - 1);
        }
      __syncthreads();
      gc ^= 1;  glo -= 1;  ghi += 1;
    }
  return -1;
}

#endif
