/* LAseparate -- splits the overlaps of a block pair by their chains into the file a later step takes and the file of the
 * rest: the command of scrub/LAseparate.c (option letters, usage text, messages and exit codes of its main, :1682-1863)
 * around damar_separate_las (separate.c).  The groups run on the GPU (kernels/pile_chains.hip) unless DAMAR_PILES=host is
 * set.  The input is read once and both files are written from the one verdict; the reference reads it once per file.
 * -L (the reference's extra pass with cached reads), -o, -l and -v are accepted and change nothing, as in the reference,
 * where none of them reaches the chaining. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "damar_hip.h"
#include "damar_host.h"

static void usage(void)
{ fprintf(stderr, "[-vLT] [-lo <int>] [-r <track>] <db> <overlaps_in> <overlaps_out> <overlaps_out_discard>\n");
  fprintf(stderr, "options: -v ... verbose\n");
  fprintf(stderr, "         -L ... two pass processing with read caching\n");
  fprintf(stderr, "         -o ... min overlap length (default: %d)\n", 0);
  fprintf(stderr, "         -l ... min read length (default: %d)\n", 0);
  fprintf(stderr, "         -r ... repeat track name (default %s)\n", "rep");
  fprintf(stderr, "         -T ... separate Type: 0 - for RepComp, 1 - for ForceAlign\n");
}

int main(int argc, char *argv[])
{ damar_separate_stats st;
  damar_dbinfo db;
  const char *track = "rep";
  uint64 *anno = NULL;
  int    *data = NULL;
  int64   ndata = 0;
  FILE *f;
  int   kind = 0, c, i, rc;

  opterr = 0;
  while ((c = getopt(argc, argv, "vLo:l:r:T:")) != -1)
    switch (c)
      { case 'L': case 'v': case 'o': case 'l':
          break;
        case 'T':
          kind = atoi(optarg);
          if (kind < 0 || kind > 1)
            { fprintf(stderr, "Unsupported type: %d\n", kind);
              exit(1);
            }
          break;
        case 'r': track = optarg; break;
        default:
          fprintf(stderr, "unknown option %c\n", c);
          usage();
          exit(1);
      }
  if (argc - optind != 4)
    { usage();
      exit(1);
    }
  for (i = 1; i < 4; i++)
    { if ((f = fopen(argv[optind + i], i == 1 ? "r" : "w")) == NULL)
        { fprintf(stderr, "could not open %s\n", argv[optind + i]);
          exit(1);
        }
      fclose(f);
    }
  if (damar_dbinfo_open(argv[optind], &db))
    { fprintf(stderr, "could not open %s\n", argv[optind]);
      exit(1);
    }
  if (damar_track_read_any(&db, track, &anno, &data, &ndata))
    { damar_filter_no_track(track);
      exit(1);
    }
  free(anno);
  free(data);
  damar_dbinfo_close(&db);
  rc = damar_separate_las(argv[optind], argv[optind + 1], argv[optind + 2], argv[optind + 3], track, kind, &st);
  damar_separate_release();
  return rc ? 1 : 0;
}
