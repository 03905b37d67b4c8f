/* LAtrim -- cuts the overlaps of a .las file back to what the trim track keeps of both reads and realigns the cut ends: the
 * command of scrub/LAtrim.c (option letters, usage text, messages and exit codes of its main, :153-294) around
 * damar_trim_las (trim.c).  The cut segments are aligned on the GPU (kernels/box_align.hip) unless DAMAR_TRIM=host is set.
 * -L (the reference's two passes with cached reads) is accepted and changes nothing: all reads are in memory here. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "damar_hip.h"
#include "damar_host.h"

#define GREEN "\x1b[32m"                  /* lib/colors.h */
#define RESET "\x1b[0m"

static void usage(void)
{ fprintf(stderr, "usage:  [-vpL] [-t <track>] <db> <overlaps.in> <overlaps.out>\n");
  fprintf(stderr, "options: -v ... verbose\n");
  fprintf(stderr, "         -p ... purge discarded overlaps\n");
  fprintf(stderr, "         -t ... trim track name (default: %s)\n", "trim");
  fprintf(stderr, "         -L ... two pass processing with read caching\n");
}

int main(int argc, char *argv[])
{ damar_trim_stats st;
  damar_dbinfo     db;
  const char *track = "trim";
  int   purge = 0, verbose = 0, c;
  FILE *f;

  opterr = 0;
  while ((c = getopt(argc, argv, "vpLt:")) != -1)
    switch (c)
      { case 'p': purge = 1; break;
        case 'v': verbose = 1; break;
        case 'L': break;
        case 't': track = optarg; break;
        default:
          usage();
          exit(1);
      }
  if (argc - optind != 3)
    { usage();
      exit(1);
    }
  if (damar_dbinfo_open(argv[optind], &db))
    { fprintf(stderr, "could not open database '%s'\n", argv[optind]);
      exit(1);
    }
  damar_dbinfo_close(&db);
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
  if (damar_trim_las(argv[optind], argv[optind + 1], argv[optind + 2], track, purge, &st))
    exit(1);
  printf(GREEN "PASS trim\n" RESET);
  if (verbose)
    { printf("nOvls    : %13lld nTrimOvls : %13lld\n", (long long) st.novl, (long long) st.ntrimmed);
      printf("nOvlBases: %13lld nTrimBases: %13lld\n", (long long) st.novl_bases, (long long) st.ntrim_bases);
    }
  damar_box_release();
  return 0;
}
