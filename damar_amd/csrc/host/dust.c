/* dust.c -- DBdust (db/DBdust.c: Myers' incremental SDUST) as calls.  Plain C, nothing of the GPU runtime.
 *
 *   - damar_host_dust_piece: the machine run over the triplets [start, stop) of one read from an empty state, the retired
 *     candidates whose start lies in [own_beg, own_end) appended to a list.  start = 0, the whole read owned: the read as the
 *     reference does it.  A later start with the halo of DESIGN.md section 9l in front: one piece of it, as the kernel
 *     (kernels/dust.hip) cuts it.  Integer counts, or with p->biased the reference's running sums of doubles (whole reads
 *     only: those sums carry the read's whole history in their last bits).
 *   - damar_host_dust_join: the retired candidates of a read in order of their starts into the mask -- the +1 joining rule,
 *     the -m cut, [beg, end) pairs.
 *   - damar_host_dust_read: both for one read, whole or in pieces.
 *   - damar_dust_track: the command's work -- a block or database loaded (db.c), its reads through damar_dust_reads in
 *     batches, .dust.anno / .dust.data written or, for a whole database that has them, extended.
 *
 * The operations on doubles are the reference's, in its forms: a product on the right of the tests (:333, :341, :345 and
 * :427, :435, :439), a quotient for the stored score (:346, :440).  Compiled without contraction. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "damar_hip.h"
#include "damar_host.h"

typedef struct { int beg, end; double score; } dust_cand;

static int list_push(damar_dust_list *L, int beg, int end)
{ if (L->n + 1 > L->cap)
    { L->cap = L->n + L->n / 4 + 64;
      L->iv = (int *) damar_grow(L->iv, sizeof(int) * 2 * (size_t) L->cap, "dust candidates");
    }
  L->iv[2 * L->n] = beg;
  L->iv[2 * L->n + 1] = end;
  L->n += 1;
  return 0;
}

int damar_dust_params_valid(const damar_dust_params *p)
{ if (p == NULL || p->window <= 0 || !(p->thresh > 0.) || p->minlen < 2)
    { fprintf(stderr, "damar: dust: window, threshold and minimum length must be positive (-m at least 2)\n");
      return 0;
    }
  if (p->biased)
    for (int i = 0; i < 4; i++)
      if (!(p->freq[i] > 0.f))
        { fprintf(stderr, "damar: dust: -b needs the four base frequencies\n");
          return 0;
        }
  return 1;
}

/* the triplet that starts at base k */
static inline int tri_at(const unsigned char *s, int k) { return (s[k] << 4) | (s[k + 1] << 2) | s[k + 2]; }

/* counts as ints and as doubles share one text: W is the weight of a count (1, or the skew of its triplet) */
#define DUST_MACHINE(NUM, W, T2)                                                                                    \
  { NUM wsqr = 0, lsqr = 0, trun;                                                                                   \
    for (j = start; j < stop; j++)                                                                                  \
      { const int c = tri_at(seq, j);                                                                               \
        if (j - start > w - 3)                            /* the window's oldest triplet leaves */                   \
          { d = tri_at(seq, ++wb);                                                                                  \
            wsqr -= (--wcount[d]) * W(d);                                                                           \
          }                                                                                                         \
        wsqr += (wcount[c]++) * W(c);                                                                               \
        if (lb < wb)                                      /* the suffix stays inside the window */                   \
          { d = tri_at(seq, ++lb);                                                                                  \
            lsqr -= (--lcount[d]) * W(d);                                                                           \
          }                                                                                                         \
        trun = (lcount[c]++) * W(c);                                                                                \
        lsqr += trun;                                                                                               \
        if (trun >= T2)                                   /* c too often: the suffix starts behind its first */       \
          while (lb < j)                                                                                            \
            { d = tri_at(seq, ++lb);                                                                                \
              lsqr -= (--lcount[d]) * W(d);                                                                         \
              if (d == c)                                                                                           \
                break;                                                                                              \
            }                                                                                                       \
        if (n > 0 && cand[n - 1].beg <= wb)               /* at most one start has left the window */                \
          { n -= 1;                                                                                                 \
            if (cand[n].beg >= own_beg && cand[n].beg < own_end)                                                    \
              list_push(out, cand[n].beg, cand[n].end);                                                             \
          }                                                                                                         \
        if (wsqr <= lsqr * t)                                                                                       \
          continue;                                                                                                 \
        walks += 1;                                                                                                 \
        { int    k = 0, s;                                /* cand[0 .. k) have been looked at */                     \
          double mscore = 0.;                                                                                       \
          for (s = lb; s > wb; s--)                       /* the suffix grown back towards the window's start */     \
            { d = tri_at(seq, s);                                                                                   \
              lsqr += (lcount[d]++) * W(d);                                                                         \
              if (lsqr >= t * (j - s))                                                                              \
                { while (k < n && cand[k].beg >= s)                                                                 \
                    { if (cand[k].score > mscore)                                                                   \
                        mscore = cand[k].score;                                                                     \
                      k += 1;                                                                                       \
                    }                                                                                               \
                  if (lsqr >= mscore * (j - s))                                                                     \
                    { mscore = (1. * lsqr) / (j - s);                                                               \
                      if (k > 0 && cand[k - 1].beg == s)                                                            \
                        { cand[k - 1].end = j;                                                                      \
                          cand[k - 1].score = mscore;                                                               \
                        }                                                                                           \
                      else                                                                                          \
                        { memmove(cand + k + 1, cand + k, sizeof(dust_cand) * (size_t) (n - k));                    \
                          cand[k].beg = s;  cand[k].end = j;  cand[k].score = mscore;                               \
                          k += 1;                                                                                   \
                          n += 1;                                                                                   \
                          if (n > longest) longest = n;                                                             \
                        }                                                                                           \
                    }                                                                                               \
                }                                                                                                   \
            }                                                                                                       \
          for (s++; s <= lb; s++)                         /* and cut back to where it was */                         \
            { d = tri_at(seq, s);                                                                                   \
              lsqr -= (--lcount[d]) * W(d);                                                                         \
            }                                                                                                       \
        }                                                                                                           \
      }                                                                                                             \
  }

#define W_ONE(e)  1
#define W_SKEW(e) skew[e]

int damar_host_dust_piece(const unsigned char *seq, int len, const damar_dust_params *p, int start, int own_beg, int own_end,
                          int stop, damar_dust_list *out, int64 *steps)
{ const int    w = p->window, ntri = len - 2;
  const double t = p->thresh, thresh2r = 2. * t;
  const int    thresh2i = (int) ceil(thresh2r);
  int          wcount[64], lcount[64];
  double       skew[64];
  dust_cand   *cand;
  int          n = 0, longest = 0, wb, lb, j, d;
  int64        walks = 0;

  if (stop > ntri)
    stop = ntri;
  if (start < 0)
    start = 0;
  if (stop <= start)
    return 0;
  cand = (dust_cand *) damar_grow(NULL, sizeof(dust_cand) * (size_t) (w + 2), "dust candidates");      /* cand[0]: the latest start */
  memset(wcount, 0, sizeof(wcount));
  memset(lcount, 0, sizeof(lcount));
  wb = lb = start - 1;
  if (p->biased)
    { int a, b, c, e = 0;
      for (a = 0; a < 4; a++)
        for (b = 0; b < 4; b++)
          for (c = 0; c < 4; c++)
            skew[e++] = .015625 / (p->freq[a] * p->freq[b] * p->freq[c]);        /* a product of floats, :251 */
      DUST_MACHINE(double, W_SKEW, thresh2r)
    }
  else
    DUST_MACHINE(int, W_ONE, thresh2i)
  if (stop == ntri)                                       /* the read's end: every candidate left, earliest start first */
    while (n > 0)
      { n -= 1;
        if (cand[n].beg >= own_beg && cand[n].beg < own_end)
          list_push(out, cand[n].beg, cand[n].end);
      }
  free(cand);
  if (steps != NULL)
    { steps[0] += stop - start;
      steps[1] += walks;
    }
  return longest;
}

int64 damar_host_dust_join(const int *cand, int64 n, int minlen, int *out)
{ int64 k, m = 0;
  int   have = 0, beg = 0, end = -2;                      /* end: the last base of the interval at hand */
  for (k = 0; k <= n; k++)
    { const int cb = k < n ? cand[2 * k] : 0, ce = k < n ? cand[2 * k + 1] + 2 : 0;
      if (k < n && have && end + 1 >= cb)
        { if (end < ce)
            end = ce;
          continue;
        }
      if (have && end - beg >= minlen - 1)
        { out[2 * m] = beg;
          out[2 * m + 1] = end + 1;
          m += 1;
        }
      beg = cb;  end = ce;  have = 1;
    }
  return m;
}

int64 damar_host_dust_read(const unsigned char *seq, int len, const damar_dust_params *p, int piece, int halo, int *out,
                           damar_dust_list *work, int64 *steps)
{ const int ntri = len - 2;
  work->n = 0;
  if (ntri <= 0)
    return 0;
  if (piece <= 0)
    damar_host_dust_piece(seq, len, p, 0, 0, ntri, ntri, work, steps);
  else
    for (int a = 0; a < ntri; a += piece)
      { const int b = a + piece < ntri ? a + piece : ntri;
        damar_host_dust_piece(seq, len, p, a - halo, a, b, b + p->window, work, steps);
      }
  return damar_host_dust_join(work->iv, work->n, p->minlen, out);
}

int damar_dust_on_host(void)
{ const char *e = getenv("DAMAR_DUST");
  return e != NULL && strcmp(e, "host") == 0;
}

/***** the command's work *************************************************************************************************/

#define DUST_BATCH_BASES (32ll << 20)       /* bases per damar_dust_reads call: 256 MiB of stripes on the device */

int damar_dust_track(const char *name, const damar_dust_params *p, int64 *stats)
{ HITS_DB blk;
  char    aname[4400], dname[4400];
  FILE   *afile, *dfile;
  int     first = 0, size = 8, i;
  int64   indx = 0;
  unsigned char *buf = NULL;
  int64  *roff = NULL, *ooff = NULL;

  if (damar_read_block(name, &blk))
    return 1;
  { damar_dust_params q = *p;                             /* -b takes the database's frequencies */
    if (q.biased)
      for (i = 0; i < 4; i++) q.freq[i] = blk.freq[i];
    if (!damar_dust_params_valid(&q))
      return 1;
  }
  if (blk.part > 0)
    { snprintf(aname, sizeof(aname), "%s.%d.dust.anno", blk.path, blk.part);
      snprintf(dname, sizeof(dname), "%s.%d.dust.data", blk.path, blk.part);
    }
  else
    { snprintf(aname, sizeof(aname), "%s.dust.anno", blk.path);
      snprintf(dname, sizeof(dname), "%s.dust.data", blk.path);
    }
  /* a whole database that has the track gets the reads beyond it appended; a block is always written anew (:183-213) */
  if ((afile = fopen(aname, "r+")) == NULL || blk.part > 0)
    { if (afile != NULL)
        fclose(afile);
      afile = fopen(aname, "w");
      dfile = fopen(dname, "w");
      if (afile == NULL || dfile == NULL)
        return damar_cannot_write(afile == NULL ? aname : dname);
      fwrite(&blk.nreads, sizeof(int), 1, afile);
      fwrite(&size, sizeof(int), 1, afile);
      fwrite(&indx, sizeof(int64), 1, afile);
    }
  else
    { if ((dfile = fopen(dname, "r+")) == NULL)
        return damar_cannot_write(dname);
      if (fread(&first, sizeof(int), 1, afile) != 1)
        { fprintf(stderr, "damar: DBdust: cannot read %s\n", aname);
          return 1;
        }
      if (first >= blk.nreads)
        { fclose(afile);
          fclose(dfile);
          damar_close_block(&blk);
          return 0;
        }
      fseeko(afile, 0, SEEK_SET);
      fwrite(&blk.nreads, sizeof(int), 1, afile);
      fwrite(&size, sizeof(int), 1, afile);
      fseeko(afile, 0, SEEK_END);
      fseeko(dfile, 0, SEEK_END);
      indx = ftello(dfile);
    }

  { damar_dust_params q = *p;
    if (q.biased)
      for (i = 0; i < 4; i++) q.freq[i] = blk.freq[i];
    roff = (int64 *) damar_grow(NULL, sizeof(int64) * (size_t) (blk.nreads + 2), "dust batch");
    ooff = (int64 *) damar_grow(NULL, sizeof(int64) * (size_t) (blk.nreads + 2), "dust batch");
    for (i = first; i < blk.nreads; )
      { int   e = i, r, *iv = NULL;
        int64 nb = 0, k;
        double ms[4];
        int64  cnt[4], st[2];
        while (e < blk.nreads && (e == i || nb + blk.reads[e].rlen <= DUST_BATCH_BASES))
          nb += blk.reads[e++].rlen;
        buf = (unsigned char *) damar_grow(buf, (size_t) nb + 16, "dust batch");
        roff[0] = 0;
        for (r = i; r < e; r++)                           /* the batch's reads back to back, without the block's separators */
          { memcpy(buf + roff[r - i], (const char *) blk.bases + blk.reads[r].boff, (size_t) blk.reads[r].rlen);
            roff[r - i + 1] = roff[r - i] + blk.reads[r].rlen;
          }
        if (damar_dust_reads(buf, roff, e - i, &q, ooff, &iv))
          return 1;
        for (r = 0; r < e - i; r++)
          { k = indx + (int64) sizeof(int) * ooff[r + 1];
            fwrite(&k, sizeof(int64), 1, afile);
          }
        if (ooff[e - i] > 0 && fwrite(iv, sizeof(int), (size_t) ooff[e - i], dfile) != (size_t) ooff[e - i])
          return damar_cannot_write(dname);
        indx += (int64) sizeof(int) * ooff[e - i];
        free(iv);
        if (stats != NULL)
          { damar_dust_last(ms, cnt);
            damar_dust_steps(st);
            stats[0] += cnt[0];  stats[1] += cnt[1];  stats[2] += cnt[2];  stats[3] += nb;
            stats[4] += st[0];  stats[5] += st[1];
          }
        i = e;
      }
  }
  free(buf);
  free(roff);
  free(ooff);
  if (fclose(afile) != 0)
    return damar_cannot_write(aname);
  if (fclose(dfile) != 0)
    return damar_cannot_write(dname);
  damar_close_block(&blk);
  return 0;
}
