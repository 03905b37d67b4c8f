/* tile_core.h -- the consensus of one tile (corrector/consensus.c: consensus_add, v3_align_onp, consensus_sequence) as
 * integer code that the kernel (kernels/tile_consensus.hip) and the host routine (host/correct.c) both compile: the host
 * routine is the second opinion of the kernel in its storage and its limits, not in its text.  The includer sets
 *   TC_FN   the function qualifiers,
 *   TC_VT   the type of a wave's furthest points (int16 in the kernel, int on the host),
 *   TC_ST   the type of a script value.
 *
 * A tile is a list of sequences (one base per byte, 0..3).  The first founds a profile of five counts per column; every
 * later one is aligned to it by the O(NP) wave search with every wave kept, the path reversed with the reference's
 * fix-ups, the indels emitted in path order and folded into the profile from right to left.  match() depends on the
 * profile alone, so it is evaluated once per column and add (pc[]): the search then is dalign's iter_np against the
 * string pc, in which TC_NOBASE matches nothing.
 *
 * Row D >= 0 of the waves spans the diagonals low0 - D/2 - 1 .. hgh0 + D/2 + 1 (a sentinel either side), rows -2 and -1
 * the span of row 0; the rows lie back to back.  The search needs min(M, N) waves at the most: a substitution costs one
 * wave, an indel away from the corner two, the |M - N| indels towards it none.
 *
 * Returns 0, TC_ROOM when a limit of the storage is met (nothing of the tile is valid then), TC_BAD when a walk left the
 * storage it was given (does not happen on waves this code wrote; every loop is bounded all the same). */
#ifndef DAMAR_TILE_CORE_H
#define DAMAR_TILE_CORE_H

#define TC_NOBASE 5
#define TC_ROOM   1
#define TC_BAD    2

typedef struct
{ unsigned char *cnt;          /* [5 * maxcols]: column c's counts of A C G T - at cnt + 5 * c */
  unsigned char *pc;           /* [maxcols] */
  TC_VT         *vf;           /* [cap] furthest points */
  signed char   *hf;           /* [cap] predecessor, later successor, codes */
  TC_ST         *script;       /* [maxscript] */
  long long      cap;
  int            maxcols, maxscript;
} tc_work;

TC_FN long long tc_row(int w0, int low0, int D)          /* index of diagonal 0 in row D >= -2 */
{ const long long m = D > 0 ? D >> 1 : 0, q = D > 0 ? (D - 1) >> 1 : 0;
  return (long long) (D + 2) * w0 + 2 * m * q - (low0 - m - 1);
}

TC_FN long long tc_rows_end(int w0, int D)               /* cells of the rows -2 .. D */
{ const long long d = D + 1, m = d > 0 ? d >> 1 : 0, q = d > 0 ? (d - 1) >> 1 : 0;
  return (d + 2) * w0 + 2 * m * q;
}

/* consensus.c:32 match(), per column */
TC_FN void tc_match_codes(const unsigned char *cnt, unsigned char *pc, int M)
{ int c;
  for (c = 0; c < M; c++)
    { const unsigned char *e = cnt + 5 * c;
      int nmax = e[0], cmax = 0;
      if (e[1] > nmax) { nmax = e[1];  cmax = 1; }
      if (e[2] > nmax) { nmax = e[2];  cmax = 2; }
      if (e[3] > nmax) { nmax = e[3];  cmax = 3; }
      pc[c] = (unsigned char) (e[4] >= nmax ? TC_NOBASE : cmax);
    }
}

TC_FN int tc_slide(const unsigned char *pc, const unsigned char *B, int k, int j, int lim)
{ if (j < 0 || k + j < 0)
    return j;
  while (j < lim && B[j] == pc[k + j])
    j += 1;
  return j;
}

#define TC_CHOOSE(am, ac, ap, mdir, pdir)                         \
  { if ((ac) < (am))                                              \
      { if ((ap) < (am)) { code = (mdir);  j = (am); }            \
        else             { code = (pdir);  j = (ap); }            \
      }                                                           \
    else if ((ap) < (ac)) { code = 0;  j = (ac); }                \
    else                  { code = (pdir);  j = (ap); }           \
  }

/* consensus.c:57 v3_align_onp of pc[0..M) against B[0..N), M, N >= 1: the script's values are b + 1 for a column alone
   in front of B[b] and -(c + 1) for a base of B alone in front of column c; *nins receives the number of the latter */
TC_FN int tc_align(tc_work *w, int M, const unsigned char *B, int N, int *nscript, int *nins)
{ const int del = M - N, w0 = (del < 0 ? -del : del) + 3, low0 = del < 0 ? del : 0;
  const int dmax = M < N ? M : N;
  const unsigned char *pc = w->pc;
  TC_VT *vf = w->vf;
  signed char *hf = w->hf;
  int low = low0, hgh = del < 0 ? 0 : del;
  int D, k, j, code, steps;
  long long r0, r1, r2;

  if (tc_rows_end(w0, 0) > w->cap)
    return TC_ROOM;
  r2 = tc_row(w0, low0, -2);
  r1 = tc_row(w0, low0, -1);
  for (k = low - 1; k <= hgh + 1; k++)
    vf[r2 + k] = vf[r1 + k] = (TC_VT) -2;
  vf[r1] = (TC_VT) -1;
  low += 1;
  hgh -= 1;
  for (D = 0; ; D++)
    { int am, ac, ap;
      if (D > dmax)
        return TC_BAD;
      if (tc_rows_end(w0, D) > w->cap)
        return TC_ROOM;
      r0 = tc_row(w0, low0, D);
      r1 = tc_row(w0, low0, D - 1);
      r2 = tc_row(w0, low0, D - 2);
      if ((D & 1) == 0)
        { hgh += 1;
          low -= 1;
        }
      vf[r0 + hgh + 1] = vf[r0 + low - 1] = (TC_VT) -2;
      j = -2;
      for (k = hgh; k > del; k--)
        { ap = j + 1;
          am = vf[r2 + k - 1];
          ac = vf[r1 + k] + 1;
          TC_CHOOSE(am, ac, ap, -1, 4)
          j = tc_slide(pc, B, k, j, N < M - k ? N : M - k);
          vf[r0 + k] = (TC_VT) j;
          hf[r0 + k] = (signed char) code;
        }
      j = -2;
      for (k = low; k < del; k++)
        { ap = vf[r2 + k + 1] + 1;
          am = j;
          ac = vf[r1 + k] + 1;
          TC_CHOOSE(am, ac, ap, 2, 1)
          j = tc_slide(pc, B, k, j, N < M - k ? N : M - k);
          vf[r0 + k] = (TC_VT) j;
          hf[r0 + k] = (signed char) code;
        }
      ap = vf[r0 + del + 1] + 1;
      am = j;
      ac = vf[r1 + del] + 1;
      TC_CHOOSE(am, ac, ap, 2, 4)
      j = tc_slide(pc, B, del, j, N);
      vf[r0 + del] = (TC_VT) j;
      hf[r0 + del] = (signed char) code;
      if (j >= N)
        break;
    }

  /* predecessor links into successor links, from (D, del) back to (0, 0), with the fix-ups of consensus.c:192-294 */
  { int e, h, m, c = N;
    const int maxsteps = 2 * (M + N) + 8;
#define TC_AT(DD, kk) (tc_row(w0, low0, (DD)) + (kk))
    hf[TC_AT(0, 0)] = 3;
    k = del;
    e = hf[TC_AT(D, k)];
    hf[TC_AT(D, k)] = 3;
    for (steps = 0; e != 3; steps++)
      { if (steps > maxsteps)
          return TC_BAD;
        h = k + e;
        if (e > 1) h -= 3;
        else if (e == 0) D -= 1;
        else D -= 2;
        if (D < 0 || h < low0 - (D >> 1) || h > (del < 0 ? 0 : del) + (D >> 1))
          return TC_BAD;
        if (h < k)
          { const int x = vf[TC_AT(D, h)];
            m = k < 0 ? -k : 0;
            if (x <= c)
              c = x - 1;
            while (c >= m && c < N && k + c < M && B[c] == pc[k + c])
              c -= 1;
            if (e < 1)
              { if (c <= vf[TC_AT(D + 2, k + 1)])      { e = 4;  h = k + 1;  D = D + 2; }
                else if (c == vf[TC_AT(D + 1, k)])     { e = 0;  h = k;  D = D + 1; }
                else vf[TC_AT(D, h)] = (TC_VT) (c + 1);
              }
            else
              { m = (k == del) ? D : D - 2;
                if (c <= vf[TC_AT(m, k + 1)])          { e = (k == del) ? 4 : 1;  h = k + 1;  D = m; }
                else if (c == vf[TC_AT(D - 1, k)])     { e = 0;  h = k;  D = D - 1; }
                else vf[TC_AT(D, h)] = (TC_VT) (c + 1);
              }
          }
        m = hf[TC_AT(D, h)];
        hf[TC_AT(D, h)] = (signed char) e;
        e = m;
        k = h;
      }

    /* forward again: one value per indel, consensus.c:296-338 */
    { int n = 0, ins = 0;
      k = D = 0;
      e = hf[TC_AT(0, 0)];
      for (steps = 0; e != 3; steps++)
        { if (steps > maxsteps)
            return TC_BAD;
          h = k - e;
          c = vf[TC_AT(D, k)];
          if (e > 1) h += 3;
          else if (e == 0) D += 1;
          else D += 2;
          if (D > dmax || h < low0 - (D >> 1) || h > (del < 0 ? 0 : del) + (D >> 1))
            return TC_BAD;
          if (h != k)
            { if (n >= w->maxscript)
                return TC_ROOM;
              if (h > k)
                w->script[n++] = (TC_ST) (c + 1);
              else
                { w->script[n++] = (TC_ST) -(c + k + 1);
                  ins += 1;
                }
            }
          k = h;
          e = hf[TC_AT(D, h)];
        }
      *nscript = n;
      *nins = ins;
    }
#undef TC_AT
  }
  return 0;
}

/* consensus.c:701-790: the script folded into the profile from right to left, in place */
TC_FN int tc_fold(tc_work *w, int M, const unsigned char *B, int N, int nscript, int nins, int added)
{ unsigned char *cnt = w->cnt;
  int n = M - 1 + nins, p = M - 1, b = N - 1, i, x, c;
#define TC_COPY(dst, src) { if ((dst) != (src)) for (x = 0; x < 5; x++) cnt[5 * (dst) + x] = cnt[5 * (src) + x]; }
  for (i = nscript - 1; i >= 0; i--)
    { c = w->script[i];
      if (c > 0)
        { c -= 1;
          while (c <= b)
            { if (p < 0 || n < p)
                return TC_BAD;
              TC_COPY(n, p)
              cnt[5 * n + B[b]] += 1;
              n -= 1;  b -= 1;  p -= 1;
            }
          if (p < 0 || n < p)
            return TC_BAD;
          TC_COPY(n, p)
          cnt[5 * n + 4] += 1;
          n -= 1;  p -= 1;
        }
      else
        { c = -c - 1;
          while (c <= p)
            { if (b < 0 || n < p)
                return TC_BAD;
              TC_COPY(n, p)
              cnt[5 * n + B[b]] += 1;
              n -= 1;  b -= 1;  p -= 1;
            }
          if (b < 0 || n < 0)
            return TC_BAD;
          for (x = 0; x < 5; x++) cnt[5 * n + x] = 0;
          cnt[5 * n + B[b]] += 1;
          cnt[5 * n + 4] = (unsigned char) added;
          n -= 1;  b -= 1;
        }
    }
  if (n != p)
    return TC_BAD;
  while (b >= 0)
    { if (n < 0)
        return TC_BAD;
      cnt[5 * n + B[b]] += 1;
      n -= 1;  b -= 1;
    }
#undef TC_COPY
  return 0;
}

/* One tile: the nent >= 1 sequences bases + off[i], len[i] >= 1 bases each, added in order.  out (room for maxcols values)
   receives the called bases without the dashes, *nout their number: consensus_sequence(c, 0), consensus.c:801. */
TC_FN int tc_tile(tc_work *w, const unsigned char *bases, const long long *off, const int *len, int nent,
                  unsigned char *out, int *nout)
{ unsigned char *cnt = w->cnt;
  int M = len[0], e, c, x, n = 0;
  if (M > w->maxcols)
    return TC_ROOM;
  for (c = 0; c < M; c++)
    { const int b = bases[off[0] + c] & 3;
      for (x = 0; x < 5; x++) cnt[5 * c + x] = 0;
      cnt[5 * c + b] = 1;
    }
  for (e = 1; e < nent; e++)
    { const unsigned char *B = bases + off[e];
      int ns = 0, ni = 0, st;
      tc_match_codes(cnt, w->pc, M);
      if ((st = tc_align(w, M, B, len[e], &ns, &ni)) != 0)
        return st;
      if (M + ni > w->maxcols)
        return TC_ROOM;
      if ((st = tc_fold(w, M, B, len[e], ns, ni, e)) != 0)
        return st;
      M += ni;
    }
  for (c = 0; c < M; c++)
    { const unsigned char *q = cnt + 5 * c;
      int nmax = 0, cmax = 0;
      const int cov = q[0] + q[1] + q[2] + q[3];
      for (x = 0; x < 5; x++)
        if (q[x] > nmax) { nmax = q[x];  cmax = x; }
      if (nent <= 2 ? cov != nent : 2 * cov < nent)
        cmax = 4;
      if (cmax != 4)
        out[n++] = (unsigned char) cmax;
    }
  *nout = n;
  return 0;
}

#endif
