/* LArepeat -- a repeat annotation track from the coverage of a read's pile of overlaps: the command of scrub/LArepeat.c
 * (option letters, defaults, checks, messages and exit codes of its main, :496-631) around damar_repeat_track (masks.c).
 * The sweeps run on the GPU (kernels/pile_sweep.hip) unless DAMAR_PILES=host is set. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "damar_hip.h"
#include "damar_host.h"

#define MIN_OVERLAP_GROUPS 1000
#define DEFAULT_MAX_COVERAGE 100

static void usage(void)
{ printf("usage:   [-CEI] [-hl <float>] [-t <track>] [-bcmnoM <int>] <db> <overlaps>\n");
  printf("options: -h ... repeat enter coverage (%.1f)\n", 2.0);
  printf("         -l ... repeat leave coverage (%.1f)\n", 1.7);
  printf("         -t ... track name (repeats)\n");
  printf("         -o ... min overlap length\n");
  printf("         -C ... add the region's coverage to the track\n");
  printf("         -E ... only report coverage based on overlaps\n");
  printf("         -I ... include identity overlaps\n");
  printf("         -b ... track block\n");
  printf("         -c ... expected coverage (%d)\n", -1);
  printf("         -m ... merge distance in bp (%d)\n", -1);
  printf("         -n ... # of a reads used for coverage estimate (%d)\n", -1);
  printf("         -M ... maximum coverage (%d)\n", DEFAULT_MAX_COVERAGE);
}

int main(int argc, char *argv[])
{ damar_repeat_params p;
  damar_repeat_result res;
  damar_dbinfo db;
  const char *track = "repeats";
  int   block = 0, max_areads = -1, cov_only = 0, c, rc, j;
  FILE *f;

  memset(&p, 0, sizeof(p));
  p.xcov_enter = 2.0;  p.xcov_leave = 1.7;  p.merge_dist = -1;  p.cov = -1;  p.max_cov = DEFAULT_MAX_COVERAGE;
  opterr = 0;
  while ((c = getopt(argc, argv, "Ch:l:m:c:n:t:b:o:EIM:")) != -1)
    switch (c)
      { case 'E': cov_only = 1; break;
        case 'I': p.inc_identity = 1; break;
        case 'o': p.min_aln_len = atoi(optarg); break;
        case 'C': p.inccov = 1; break;
        case 'M': p.max_cov = atoi(optarg); break;
        case 'b': block = atoi(optarg); break;
        case 'h': p.xcov_enter = atof(optarg); break;
        case 'l': p.xcov_leave = atof(optarg); break;
        case 'm': p.merge_dist = atoi(optarg); break;
        case 'c': p.cov = atoi(optarg); break;
        case 'n': max_areads = atoi(optarg); break;
        case 't': track = optarg; break;
        default:
          usage();
          exit(1);
      }
  if (argc - optind != 2)
    { usage();
      exit(1);
    }
  if (p.xcov_enter < p.xcov_leave)
    { fprintf(stderr, "invalid arguments: low %.2f > high %.2f\n", p.xcov_leave, p.xcov_enter);
      exit(1);
    }
  if (max_areads != -1 && max_areads < MIN_OVERLAP_GROUPS)
    { fprintf(stderr, "invalid arguments: number of overlap groups tested should be larger than %d\n", MIN_OVERLAP_GROUPS);
      exit(1);
    }
  if ((f = fopen(argv[optind + 1], "r")) == NULL)
    { fprintf(stderr, "could not open '%s'\n", argv[optind + 1]);
      exit(1);
    }
  fclose(f);
  if (p.max_cov < DEFAULT_MAX_COVERAGE)
    { fprintf(stderr, "maximum coverage cannot be smallert than '%d'\n", DEFAULT_MAX_COVERAGE);
      exit(1);
    }
  if (damar_dbinfo_open(argv[optind], &db))
    exit(1);

  rc = damar_repeat_track(&db, argv[optind + 1], &p, max_areads, cov_only, &res);
  if (res.histo != NULL)
    { printf("PASS estimate coverage\n");
      for (j = 0; j < p.max_cov; j++)
        printf("COV %d READS %lld\n", j, (long long) res.histo[j]);
      printf("MAX %d\n", res.cov_max);
      printf("INACTIVE %lld (%d%%) OF %lld\n", (long long) res.cov_inactive,
             (int) (100.0 * res.cov_inactive / res.cov_bases), (long long) res.cov_bases);
      printf("AVG_RLEN %d\n", res.avg_rlen);
    }
  if (rc == 2)
    { fprintf(stderr, "ERROR: coverage estimation resulted in %d\n", res.cov);
      fprintf(stderr, "       bypass estimation using the -c <coverage> argument\n");
      exit(1);
    }
  if (rc)
    exit(1);
  if (!cov_only)
    { printf("PASS repeats\n");
      if (damar_track_write_a2(db.path, track, block, db.nreads, res.anno, res.data, res.ndata))
        exit(1);
      printf("COV_ENTER %.1f\n", p.xcov_enter);
      printf("COV_LEAVE %.1f\n", p.xcov_leave);
      printf("REGIONS %d\n", (int) (res.ndata / (2 + p.inccov)));
      printf("MERGED %d\n", (int) res.merged);
      printf("BASES_TOTAL %lld\n", (long long) res.bases_total);
      printf("BASES_REPEAT %lld\n", (long long) res.bases_repeat);
      printf("BASES_REPEAT_PERCENT %d%%\n", (int) (res.bases_repeat * 100.0 / res.bases_total));
    }
  damar_repeat_result_free(&res);
  damar_dbinfo_close(&db);
  damar_pile_release();
  return 0;
}
