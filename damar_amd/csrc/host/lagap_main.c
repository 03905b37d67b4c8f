/* LAgap -- drops the contained overlaps of every pile and the overlaps on the far side of its gaps and breaks: the command
 * of scrub/LAgap.c (option letters, usage text, messages and exit codes of its main, :1975-2182) around damar_gap_las
 * (gap.c).  The piles run on the GPU (kernels/pile_gaps.hip) unless DAMAR_PILES=host is set; -t trims the overlaps first
 * (trim.c, kernels/box_align.hip unless DAMAR_TRIM=host).
 * -L (the reference's two passes with cached reads) is accepted and changes nothing: all reads are in memory here.
 * -R loads its track and does nothing else with it, as in the reference, whose only consumer is commented out.
 * -C (the reference's experimental chimer detection) is not supported: a message and exit status 1. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "damar_hip.h"
#include "damar_host.h"

static void usage(void)
{ fprintf(stderr, "usage:   [-s <int>] [-pL] [-etR <track>] [-C file] <db> <ovl.in> <ovl.out>\n");
  fprintf(stderr, "options: -s ... stitch distance (%d)\n", 0);
  fprintf(stderr, "         -p ... purge discarded overlaps\n");
  fprintf(stderr, "         -e ... exclude gaps in track intervals\n");
  fprintf(stderr, "         -t ... trim overlaps before gap detection\n");
  fprintf(stderr, "         -L ... two pass processing with read caching\n");
  fprintf(stderr, "EXPERIMENTAL: \n");
  fprintf(stderr, "         -C ... discard chimeric reads and overlaps. Write chimer reads IDs into <file>.\n");
  fprintf(stderr, "         -R ... repeat track - used to detect chimers in large repeats\n");
}

int main(int argc, char *argv[])
{ damar_gap_params p;
  damar_gap_stats  st;
  damar_dbinfo     db;
  const char *exclude = NULL, *repeat = NULL, *chimer = NULL;
  uint64 *ex_anno = NULL, *r_anno = NULL;
  int    *ex_data = NULL, *r_data = NULL;
  int64   r_ndata = 0;
  FILE *f;
  int   c, rc;

  memset(&p, 0, sizeof(p));
  opterr = 0;
  while ((c = getopt(argc, argv, "Ls:pe:R:t:C:")) != -1)
    switch (c)
      { case 'R': repeat = optarg; break;
        case 'e': exclude = optarg; break;
        case 'C': chimer = optarg; break;
        case 't': p.trim_track = optarg; break;
        case 's': p.stitch = atoi(optarg); break;
        case 'p': p.purge = 1; break;
        case 'L': break;
        default:
          usage();
          exit(1);
      }
  if (argc - optind < 3)
    { usage();
      exit(1);
    }
  if (chimer != NULL)
    { fprintf(stderr, "LAgap: -C (chimer detection) is not supported\n");
      exit(1);
    }
  if ((f = fopen(argv[optind + 1], "r")) == NULL)
    { fprintf(stderr, "could not open input track '%s'\n", argv[optind + 1]);
      exit(1);
    }
  fclose(f);
  if ((f = fopen(argv[optind + 2], "w")) == NULL)
    { fprintf(stderr, "could not open output track '%s'\n", argv[optind + 2]);
      exit(1);
    }
  fclose(f);
  if (damar_dbinfo_open(argv[optind], &db))
    { fprintf(stderr, "could not open database '%s'\n", argv[optind]);
      exit(1);
    }
  if (exclude != NULL && damar_track_read_any(&db, exclude, &ex_anno, &ex_data, &p.ex_ndata))
    { damar_gap_no_track(exclude);
      exit(1);
    }
  p.ex_anno = ex_anno;
  p.ex_data = ex_data;
  if (repeat != NULL && damar_track_read_any(&db, repeat, &r_anno, &r_data, &r_ndata))
    { damar_gap_no_track(repeat);
      exit(1);
    }
  free(r_anno);
  free(r_data);
  damar_dbinfo_close(&db);
  rc = damar_gap_las(argv[optind], argv[optind + 1], argv[optind + 2], &p, &st);
  free(ex_anno);
  free(ex_data);
  damar_gap_release();
  damar_box_release();
  return rc ? 1 : 0;
}
