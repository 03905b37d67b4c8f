/* ref_localalign.c -- TEST INFRASTRUCTURE ONLY.  A small driver of OUR OWN that is linked against the REAL
 * reference (dalign/align.c, db/DB.c compiled where they lie by oracle/Makefile.ref, output
 * oracle/_ref/ref_localalign) and calls the reference's Local_Alignment (align.c:1904) the way filter.c:2316 does:
 * low == hgh == the seed's diagonal, no borders, B already complemented where COMP_FLAG is set.
 *
 * Input: a family file written by tests/la_shapes.py write_family():
 *
 *     int32 ngroups, then per group
 *     int32 na, nb, ntasks, tspace, comp;  float64 e
 *     na + nb reads, each int32 length and that many bases 0..3
 *     ntasks tasks, each int32 aread, bread, diag, anti
 *
 * Output, per task in order: the 12 path integers (A path as left in align->path, then the B path returned: abpos,
 * bbpos, aepos, bepos, diffs, tlen), the A trace and the B trace as uint16.  tests/la_shapes.py dump() writes the same
 * from the oracle's answers; tests/test_la_host.py compares the two and the md5 committed under tests/golden/.
 *
 *     ref_localalign <family file> <out.bin>
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>

#include "db/DB.h"
#include "dalign/align.h"

static void need(int ok, const char *what)
{ if (!ok)
    { fprintf(stderr, "ref_localalign: %s\n", what);
      exit(1);
    }
}

/* reads in the block layout: a 4 in front of the first base and behind the last */
static char **load_reads(FILE *in, int n, int *len)
{ char **r = (char **) malloc(sizeof(char *) * (size_t) (n > 0 ? n : 1));
  int    i;
  for (i = 0; i < n; i++)
    { char *buf;
      need(fread(len + i, sizeof(int32_t), 1, in) == 1 && len[i] >= 0, "short family file (read length)");
      buf = (char *) malloc((size_t) len[i] + 2);
      buf[0] = buf[len[i] + 1] = 4;
      need(fread(buf + 1, 1, (size_t) len[i], in) == (size_t) len[i], "short family file (bases)");
      r[i] = buf + 1;
    }
  return r;
}

int main(int argc, char *argv[])
{ FILE *in, *out;
  int32_t ngroups, g;
  float   freq[4] = { .25f, .25f, .25f, .25f };
  Work_Data *work;

  need(argc == 3, "usage: ref_localalign <family file> <out.bin>");
  need((in = fopen(argv[1], "rb")) != NULL && (out = fopen(argv[2], "wb")) != NULL, "cannot open files");
  need(fread(&ngroups, sizeof(int32_t), 1, in) == 1, "short family file");
  work = New_Work_Data();
  for (g = 0; g < ngroups; g++)
    { int32_t h[5];
      double  e;
      int    *alen, *blen, t;
      char  **a, **b;
      Align_Spec *spec;

      need(fread(h, sizeof(int32_t), 5, in) == 5 && fread(&e, sizeof(double), 1, in) == 1, "short family file (group)");
      alen = (int *) malloc(sizeof(int) * (size_t) (h[0] + 1));
      blen = (int *) malloc(sizeof(int) * (size_t) (h[1] + 1));
      a = load_reads(in, h[0], alen);
      b = load_reads(in, h[1], blen);
      spec = New_Align_Spec(e, h[3], freq, 1, 1, 0, 0, 1);
      need(spec != NULL, "New_Align_Spec failed");
      for (t = 0; t < h[2]; t++)
        { int32_t   tk[4], rec[12];
          Alignment aln;
          Path      ap, *bp;

          need(fread(tk, sizeof(int32_t), 4, in) == 4, "short family file (task)");
          need(tk[0] >= 0 && tk[0] < h[0] && tk[1] >= 0 && tk[1] < h[1], "task names a read the group does not have");
          aln.path  = &ap;
          aln.flags = h[4] ? COMP_FLAG : 0;
          aln.aseq  = a[tk[0]];  aln.alen = alen[tk[0]];
          aln.bseq  = b[tk[1]];  aln.blen = blen[tk[1]];
          bp = Local_Alignment(&aln, work, spec, tk[2], tk[2], tk[3], -1, -1);
          need(bp != NULL, "Local_Alignment failed");
          rec[0] = ap.abpos;   rec[1] = ap.bbpos;   rec[2] = ap.aepos;   rec[3] = ap.bepos;   rec[4] = ap.diffs;    rec[5] = ap.tlen;
          rec[6] = bp->abpos;  rec[7] = bp->bbpos;  rec[8] = bp->aepos;  rec[9] = bp->bepos;  rec[10] = bp->diffs;  rec[11] = bp->tlen;
          fwrite(rec, sizeof(int32_t), 12, out);
          fwrite(ap.trace, sizeof(uint16), (size_t) ap.tlen, out);
          fwrite(bp->trace, sizeof(uint16), (size_t) bp->tlen, out);
        }
      Free_Align_Spec(spec);
      for (t = 0; t < h[0]; t++) free(a[t] - 1);
      for (t = 0; t < h[1]; t++) free(b[t] - 1);
      free(a);  free(b);  free(alen);  free(blen);
    }
  Free_Work_Data(work);
  need(fclose(out) == 0, "write failed");
  fclose(in);
  return 0;
}
