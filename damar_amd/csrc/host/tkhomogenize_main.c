/* TKhomogenize -- the repeat intervals of a track carried across the overlaps of a .las file onto the B reads: the command
 * of scrub/TKhomogenize.c (option letters, defaults, checks, messages and exit codes of its main, :548-692) around
 * damar_homogenize_track (homogenize.c).  The mask of the database lives on the GPU (kernels/homogenize.hip) unless
 * DAMAR_PILES=host is set.  The reference's DEBUG_HOMOGENIZE lines for A read 592526 are not reproduced. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "damar_hip.h"
#include "damar_host.h"

#define GREEN "\x1b[32m"                  /* lib/colors.h */
#define RESET "\x1b[0m"
#define MAX_BUF_SIZE (10L * 1024 * 1024 * 1024)       /* TKhomogenize.c:46 */

static void usage(void)
{ printf("usage:   [-m] [-ber <int>] [-iIt <track>] <db> <overlaps>\n");
  printf("options: -b ... track block\n");
  printf("         -m ... merge input intervals into the output track (%d)\n", 0);
  printf("         -i ... input interval track (%s)\n", "repeats");
  printf("         -I ... output interval track (%s)\n", "hrepeats");
  printf("         -e ... only annotate n bases at the ends of the reads (%d), requires -t \n", -1);
  printf("         -t ... trim track (%s)\n", "trim");
  printf("         -r ... base pair resolution (%d)\n", 1);
  printf("                scales memory usage by the same factor and improves runtime\n");
}

/* lib/utils.c:143-168 */
static void format_bytes(unsigned long bytes, char *buf)
{ static const char *suffix[] = { "b", "kb", "mb", "gb", "tb", "eb" };
  if (bytes < 1024)
    sprintf(buf, "%lub", bytes);
  else
    { double b = bytes;
      int    i = 0;
      while (b >= 1024)
        { b /= 1024.0;
          i++;
        }
      sprintf(buf, "%.1f%s", b, suffix[i]);
    }
}

int main(int argc, char *argv[])
{ damar_homog_params p;
  damar_homog_result res;
  damar_dbinfo db;
  const char *track_in = "repeats", *track_out = "hrepeats", *track_trim = "trim";
  uint64 *ia = NULL, *ta = NULL;
  int    *id = NULL, *td = NULL;
  int64   ni = 0, nt = 0;
  unsigned long total = 0, nbuf = 0;
  char  buf[128];
  int   block = 0, nbufs = 0, c, i;
  FILE *f;

  memset(&p, 0, sizeof(p));
  p.ends = -1;
  p.res = 1;
  opterr = 0;
  while ((c = getopt(argc, argv, "mr:e:b:i:I:t:")) != -1)
    switch (c)
      { case 'm': p.merge = 1; break;
        case 'r': p.res = atoi(optarg); break;
        case 'b': block = atoi(optarg); break;
        case 'i': track_in = optarg; break;
        case 'I': track_out = optarg; break;
        case 't': track_trim = optarg; break;
        case 'e': p.ends = atoi(optarg); break;
        default:
          usage();
          exit(1);
      }
  if (argc - optind != 2)
    { usage();
      exit(1);
    }
  if (p.ends < -1 || p.ends == 0)
    { fprintf(stderr, "invalid -e argument %d\n", p.ends);
      exit(1);
    }
  if ((f = fopen(argv[optind + 1], "r")) == NULL)
    { fprintf(stderr, "could not open '%s'\n", argv[optind + 1]);
      exit(1);
    }
  fclose(f);
  if (damar_dbinfo_open(argv[optind], &db))
    { fprintf(stderr, "failed top open database %s\n", argv[optind]);
      exit(1);
    }
  if (p.ends != -1 && damar_track_read_a2(db.path, track_trim, db.nreads, &ta, &td, &nt))
    { fprintf(stderr, "-e requires a trim track\n");
      exit(1);
    }
  if (p.res < 1)                                                 /* the reference divides by it */
    { fprintf(stderr, "invalid -r argument %d\n", p.res);
      exit(1);
    }

  printf(GREEN "PASS homogenising\n" RESET);
  if (damar_track_read_a2(db.path, track_in, db.nreads, &ia, &id, &ni))
    { fflush(stdout);
      fprintf(stderr, "could not load track %s\n", track_in);
      exit(1);
    }
  for (i = 0; i < db.nreads; i++)                                /* pre_homogenize's buffers (:119-181): what it reports */
    { const int len = p.res > 1 ? (db.read_len[i] + p.res - 1) / p.res : db.read_len[i];
      nbuf += ((unsigned long) len + 1 + 7) / 8;
      total += ((unsigned long) len + 1 + 7) / 8;
      if (nbuf > MAX_BUF_SIZE)
        { nbuf = 0;
          nbufs++;
        }
    }
  format_bytes(total, buf);
  printf("allocated %s in %d buffers\n", buf, nbufs + 1);
  if (p.merge)
    printf("copying existing annotation\n");
  fflush(stdout);

  p.iv_anno = ia;  p.iv_data = id;  p.iv_ndata = ni;
  p.trim_anno = ta;  p.trim_data = td;
  if (damar_homogenize_track(&db, argv[optind + 1], &p, &res))
    exit(1);
  printf("tagged %llu as repeat\n", (unsigned long long) res.tagged);
  fflush(stdout);
  if (damar_track_write_a2(db.path, track_out, block, db.nreads, res.anno, res.data, res.ndata))
    exit(1);
  if (res.ndata == 0)
    { /* track_write (lib/tracks.c:241-247) takes the fwrite of 0 bytes for a failure and returns before it writes the
         header a second time: the message, an empty .d2, and an .a2 whose header still says 0 compressed bytes */
      char path[4600];
      const uint64 zero = 0;
      if (block > 0) snprintf(path, sizeof(path), "%s.%d.%s.a2", db.path, block, track_out);
      else           snprintf(path, sizeof(path), "%s.%s.a2", db.path, track_out);
      if ((f = fopen(path, "r+")) != NULL)
        { if (fseek(f, 16, SEEK_SET) == 0)
            fwrite(&zero, 8, 1, f);
          fclose(f);
        }
      fprintf(stderr, "failed to write track data of 0 (0) bytes\n");
    }
  damar_homog_result_free(&res);
  free(ia);  free(id);  free(ta);  free(td);
  damar_dbinfo_close(&db);
  return 0;
}
