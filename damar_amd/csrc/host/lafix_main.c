/* LAfix -- patches the weak segments and the breaks of every read from the reads that overlap it and writes the patched
 * reads as FASTA: the command of scrub/LAfix.c (option letters, usage text, messages and exit codes of its main,
 * :2703-2959) around damar_fix_las (fix.c).  The search per pile runs on the GPU (kernels/pile_patch.hip) unless
 * DAMAR_PILES=host is set.
 * -X (the reference's experimental chimer detection) is not supported: a message and exit status 1.  -d -b -C -F, which
 * only act under -X, are accepted and change nothing; so is -R, whose range is still checked.
 * -f (quality streams) is not supported: a message and exit status 1. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "damar_hip.h"
#include "damar_host.h"

static void usage(void)
{ printf("usage: [-ladX] [-bCxQgFR <int>] [-ctqr <track>] [-f <patched.quiva>] [-T <file>] <db> <in.las> <patched.fasta>\n");
  printf("       -c ... convert track intervals (multiple -c possible)\n");
  printf("       -f ... patch quality streams\n");
  printf("       -x ... min length for fixed sequences (%d)\n", 1000);
  printf("       -Q ... segment quality threshold (%d)\n", 28);
  printf("       -g ... max gap length for patching (%d)\n", 500);
  printf("       -t ... trim reads based on a track\n");
  printf("       -q ... quality track (default: %s)\n", "q");
  printf("       -l ... low coverage mode\n");
  printf("EXPERIMENTAL OPTIONS\n");
  printf("       -X ... fix chimeric reads in repeat regions\n");
  printf("       -r ... repeat track\n");
  printf("       -d ... discard all chimeric reads, (default: 0, i.e. keep longest part of chimeric reads)\n");
  printf("       -b ... minimum border coverage to start a chimer detection (default: %d)\n", 7);
  printf("       -C ... maximum chimer length (default: %d)\n", 8000);
  printf("       -T ... write trim interval after gap-, cross-, and chimer-detection into a file.\n");
  printf("       -F ... allow LAS chain to have a fuzzy begin and end overlap. LAS chains are used to find spanners over putative chimeric break intervals. (default: %d)\n", 0);
  printf("       -R ... Fix chimers only in regions that are at least -R <int repetitive. (default: %d)\n", 70);
}

int main(int argc, char *argv[])
{ damar_fix_opts  o;
  damar_fix_stats st;
  const char **convert = NULL;
  const char  *quiva = NULL;
  FILE *f;
  int   chimers = 0, repeat_perc = 70, c, rc;

  memset(&o, 0, sizeof(o));
  o.min_len = 1000;
  o.lowq = 28;
  o.maxgap = 500;
  o.q_track = "q";
  opterr = 0;
  while ((c = getopt(argc, argv, "dlXx:f:c:Q:g:t:q:r:b:C:T:F:R:")) != -1)
    switch (c)
      { case 'l': o.low_coverage = 1; break;
        case 'X': chimers = 1; break;
        case 'd': case 'F': case 'b': case 'C': break;
        case 'Q': o.lowq = atoi(optarg); break;
        case 'R': repeat_perc = atoi(optarg); break;
        case 'g': o.maxgap = atoi(optarg); break;
        case 'x': o.min_len = atoi(optarg); break;
        case 'f': quiva = optarg; break;
        case 'T': o.trim_out = optarg; break;
        case 'q': o.q_track = optarg; break;
        case 't': o.trim_track = optarg; break;
        case 'r': o.rep_track = optarg; break;
        case 'c':
          convert = (const char **) realloc(convert, sizeof(char *) * ((size_t) o.nconvert + 1));
          if (convert == NULL)
            exit(1);
          convert[o.nconvert++] = optarg;
          break;
        default:
          usage();
          exit(1);
      }
  if (argc - optind != 3)
    { usage();
      exit(1);
    }
  if (chimers)
    { fprintf(stderr, "LAfix: -X (chimer detection) is not supported\n");
      exit(1);
    }
  if (quiva != NULL)
    { fprintf(stderr, "LAfix: -f (quality streams) is not supported\n");
      exit(1);
    }
  if ((f = fopen(argv[optind + 1], "r")) == NULL)
    { fprintf(stderr, "could not open '%s'\n", argv[optind + 1]);
      exit(1);
    }
  fclose(f);
  if (repeat_perc < 0 || repeat_perc > 100)
    { /* the reference has opened its outputs and the database by now */
      if ((f = fopen(argv[optind + 2], "w")) != NULL) fclose(f);
      if (o.trim_out != NULL && (f = fopen(o.trim_out, "w")) != NULL) fclose(f);
      fprintf(stderr, "invalid chimer repeat percentage %d. Must be within [0, 100]\n", repeat_perc);
      exit(1);
    }
  o.convert = convert;
  rc = damar_fix_las(argv[optind], argv[optind + 1], argv[optind + 2], &o, &st);
  free(convert);
  damar_fix_release();
  return rc ? 1 : 0;
}
