/* LAcorrect -- every read rewritten as the consensus of the tiles its pile lays over it, written as FASTA: the command of
 * corrector/LAcorrect.c (option letters, usage text, messages and exit codes of its main, :1567-1794) around
 * damar_correct_las (correct.c).  The consensus per tile runs on the GPU (kernels/tile_consensus.hip) unless
 * DAMAR_PILES=host is set, and so does the whole-read alignment behind " postrace=" (kernels/read_align.hip) unless that or
 * DAMAR_POSTRACE=host is set.
 * -j <n> writes n files, as the reference's n threads do; here it says nothing about threads.  -x stands in the usage text
 * and is not an option, as in the reference. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "damar_hip.h"
#include "damar_host.h"

static void usage(void)
{ printf("[-v] [-r <file>] [-jx <int>] [-q <track>] <db> <in.las> <out.fasta>\n");
  printf("options: -v ... verbose\n");
  printf("         -j ... number of threads\n");
  printf("         -q ... q track (%s)\n", "q");
  printf("         -b ... block (%d)\n", -1);
  printf("         -r ... text file with ids of the reads to be corrected\n");
}

int main(int argc, char *argv[])
{ damar_correct_opts  o;
  damar_correct_stats st;
  FILE *f;
  long long novl;
  int   twidth, c, rc;

  memset(&o, 0, sizeof(o));
  o.nthreads = 1;
  o.block = -1;
  o.q_track = "q";
  opterr = 0;
  while ((c = getopt(argc, argv, "vr:b:j:q:")) != -1)
    switch (c)
      { case 'r': o.read_ids = optarg; break;
        case 'v': o.verbose += 1; break;
        case 'j': o.nthreads = atoi(optarg); break;
        case 'b': o.block = atoi(optarg); break;
        case 'q': o.q_track = optarg; break;
        default:
          usage();
          exit(1);
      }
  if (argc - optind != 3)
    { usage();
      exit(1);
    }
  if ((f = fopen(argv[optind + 1], "r")) == NULL)
    { fprintf(stderr, "could not open '%s'\n", argv[optind + 1]);
      exit(1);
    }
  if (fread(&novl, sizeof(novl), 1, f) != 1 || fread(&twidth, sizeof(twidth), 1, f) != 1)
    { fprintf(stderr, "failed to read %s header\n", argv[optind + 1]);
      exit(1);
    }
  fclose(f);
  rc = damar_correct_las(argv[optind], argv[optind + 1], argv[optind + 2], &o, &st);
  damar_correct_release();
  damar_read_release();
  return rc ? 1 : 0;
}
