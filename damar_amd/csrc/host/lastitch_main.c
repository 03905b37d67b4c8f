/* LAstitch -- rejoins the records of a .las file that the overlapper split at a bad stretch of either read and realigns
 * the joint: the command of scrub/LAstitch.c (option letters, usage text, messages and exit codes of its main, :1567-1778)
 * around damar_stitch_las (stitch.c).  The joints are realigned on the GPU (kernels/box_trace.hip) unless DAMAR_STITCH=host
 * is set.  -L (the reference's two passes with cached reads) is accepted and changes nothing: all reads are in memory
 * here.  -v is accepted as in the reference, whose handler prints nothing more with it. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "damar_hip.h"
#include "damar_host.h"

#define GREEN "\x1b[32m"                  /* lib/colors.h */
#define RESET "\x1b[0m"

static void usage(void)
{ fprintf(stderr, "usage: [-pvL] [-amlf <int>] [-rt <track>] <db> <ovl.in> <ovl.out>\n");
  fprintf(stderr, "options: -v ... verbose\n");
  fprintf(stderr, "         -f ... fuzzing for stitch (%d)\n", 40);
  fprintf(stderr, "         -L ... two pass processing with read caching\n");
  fprintf(stderr, "         -p ... purge discarded overlaps\n");
  fprintf(stderr, "\nEXPERIMENTAL\n");
  fprintf(stderr, "                try to stitch overlaps, that break in low complexity regions. Only works if trace spacing is >= 126\n");
  fprintf(stderr, "         -t ... low complexity (LC) or tandem repeat (TR) interval track (e.g. dust, tan)\n");
  fprintf(stderr, "         -r ... repeat track - is used to evaluate unique anchor bases\n");
  fprintf(stderr, "         -a ... anchor bases left and right of LC/TR interval (default: %d)\n", 500);
  fprintf(stderr, "         -m ... merge LC/TR intervals that are closer then m bases (default: %d)\n", 10);
  fprintf(stderr, "         -l ... consider only LC/TR intervals of length greater than -l bases (default: %d)\n", 500);
  fprintf(stderr, "         -M ... merge only LC/TR intervals that are at least -M bases long (default: %d)\n", 200);
  fprintf(stderr,
          "         -d ... gap difference in percent (default: %.2f). Stitch only overlaps where gap size difference in A-read and B-read is lower then -m %%\n",
          0.3);
}

int main(int argc, char *argv[])
{ damar_stitch_params p;
  damar_stitch_stats  st;
  damar_dbinfo        db;
  FILE *f;
  int   c;

  memset(&p, 0, sizeof(p));
  p.fuzz = 40;  p.anchor = 500;  p.merge = 10;  p.min_len = 500;  p.min_merge = 200;  p.gap_diff = 0.3;
  opterr = 0;
  while ((c = getopt(argc, argv, "Lpvf:t:a:m:l:d:r:M:")) != -1)
    switch (c)
      { case 'p': p.purge = 1; break;
        case 'L': break;
        case 'v': break;
        case 'f': p.fuzz = atoi(optarg); break;
        case 'M': p.min_merge = atoi(optarg); break;
        case 'a': p.anchor = atoi(optarg); break;
        case 'm': p.merge = atoi(optarg); break;
        case 'l': p.min_len = atoi(optarg); break;
        case 'd': p.gap_diff = atof(optarg); break;
        case 't': p.lc_track = optarg; break;
        case 'r': p.rep_track = optarg; break;
        default:
          usage();
          exit(1);
      }
  if (argc - optind < 3)
    { usage();
      exit(1);
    }
  if ((f = fopen(argv[optind + 1], "r")) == NULL)
    { fprintf(stderr, "could not open '%s'\n", argv[optind + 1]);
      exit(1);
    }
  fclose(f);
  if ((f = fopen(argv[optind + 2], "w")) == NULL)
    { fprintf(stderr, "could not open '%s'\n", argv[optind + 2]);
      exit(1);
    }
  fclose(f);
  if (damar_dbinfo_open(argv[optind], &db))
    { fprintf(stderr, "could not open database '%s'\n", argv[optind]);
      exit(1);
    }
  damar_dbinfo_close(&db);
  if (p.fuzz < 0)
    { fprintf(stderr, "invalid fuzzing value of %d\n", p.fuzz);
      exit(1);
    }
  /* the reference prints this line before its pass; a track that cannot be loaded ends it before that */
  if (damar_stitch_las(argv[optind], argv[optind + 1], argv[optind + 2], &p, &st))
    exit(1);
  printf(GREEN "PASS stitching" RESET "\n");
  printf("stitched %lld out of %lld overlaps\n", (long long) st.stitched, (long long) st.novl);
  if (p.lc_track != NULL)
    printf("stitched low complexity %lld out of %lld overlaps\n", (long long) st.stitched_lc, (long long) st.novl);
  damar_tbox_release();
  return 0;
}
