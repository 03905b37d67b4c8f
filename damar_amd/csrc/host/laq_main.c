/* LAq -- the quality track (a value per trace-spacing segment of every read, from its overlaps' traces) and the trim track
 * derived from it: the command of scrub/LAq.c (option letters, defaults, checks, messages and exit codes of its main,
 * :570-746) around damar_q_track and damar_trim_update (quality.c).  The per-segment estimate runs on the GPU
 * (kernels/pile_quality.hip) unless DAMAR_PILES=host is set; -u reads record headers and tracks only and stays on the host. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "damar_hip.h"
#include "damar_host.h"

#define GREEN "\x1b[32m"                  /* lib/colors.h */
#define RESET "\x1b[0m"

static void usage(void)
{ fprintf(stderr, "[-uc] [-mbdsS <int>] [-L <file>] [-tT <track>] <db> <overlaps>\n");
  fprintf(stderr, "options: -b ... track block number\n");
  fprintf(stderr, "         -d ... trim with Q cutoff (diff: %d)\n", 25);
  fprintf(stderr, "         -s ... min number of segments for Q estimate (%d)\n", 1);
  fprintf(stderr, "         -S ... max number of segments for Q estimate (%d)\n", 20);
  fprintf(stderr, "         -o ... min overlap length after trim (%d)\n", 1000);
  fprintf(stderr, "         -u ... update trim %s using overlaps and existing %s track (%d)\n", "trim", "q", 0);
  fprintf(stderr, "         -L ... log Q cutoff to file\n");
  fprintf(stderr, "         -t ... input trim track (%s)\n", "trim");
  fprintf(stderr, "         -T ... output trim track (%s)\n", "trim");
  fprintf(stderr, "         -q ... input q track (%s)\n", "q");
  fprintf(stderr, "         -Q ... output q track (%s)\n", "q");
  fprintf(stderr, "\nEXPERIMENTAL\n");
  fprintf(stderr, "         -c ... CCS- or HiFI-reads: allow quality values of 0!\n");
}

int main(int argc, char *argv[])
{ damar_q_params p;
  damar_q_result res;
  damar_dbinfo   db;
  const char *trim_in = "trim", *trim_out = "trim", *q_in = "q", *q_out = "q", *qlog = NULL;
  int   block = 0, update = 0, trim_q = 25, min_len = 1000, c;
  unsigned int segmin = 1, segmax = 20;
  FILE *f;

  memset(&p, 0, sizeof(p));
  opterr = 0;
  while ((c = getopt(argc, argv, "s:S:o:ub:d:L:t:T:q:Q:c")) != -1)
    switch (c)
      { case 's': segmin = (unsigned int) atoi(optarg); break;
        case 'S': segmax = (unsigned int) atoi(optarg); break;
        case 'L': qlog = optarg; break;
        case 'd': trim_q = atoi(optarg); break;
        case 'o': min_len = atoi(optarg); break;
        case 'u': update = 1; break;
        case 'b': block = atoi(optarg); break;
        case 't': trim_in = optarg; break;
        case 'T': trim_out = optarg; break;
        case 'q': q_in = optarg; break;
        case 'Q': q_out = optarg; break;
        case 'c': p.ccs = 1; break;
        default:
          usage();
          exit(1);
      }
  if (argc - optind != 2)
    { usage();
      exit(1);
    }
  if (trim_q == 0)
    { fprintf(stderr, "error: -q not specified\n");
      exit(1);
    }
  if (segmin < 1)
    { fprintf(stderr, "error: invalid -s\n");
      exit(1);
    }
  if (segmin > segmax)
    { fprintf(stderr, "error: invalid -s -S combination\n");
      exit(1);
    }
  if (segmax > 0x7fffffffu)                                    /* the reference takes a negative -S for 2^32 minus it: no cap */
    segmax = 0x7fffffffu;
  if (segmin > 0x7fffffffu)
    segmin = 0x7fffffffu;
  p.segmin = (int) segmin;
  p.segmax = (int) segmax;
  if ((f = fopen(argv[optind + 1], "r")) == NULL)
    { fprintf(stderr, "could not open '%s'\n", argv[optind + 1]);
      exit(1);
    }
  fclose(f);
  if (damar_dbinfo_open(argv[optind], &db))
    { fprintf(stderr, "failed to open %s\n", argv[optind]);
      exit(1);
    }

  if (update)
    { uint64 *qa = NULL, *ta = NULL;
      int    *qd = NULL, *td = NULL;
      int64   nq = 0, nt = 0;
      printf(GREEN "PASS update quality estimate and trimming" RESET "\n");
      fflush(stdout);
      if (damar_track_read_a2(db.path, q_in, db.nreads, &qa, &qd, &nq))
        { fprintf(stderr, "could not open %s track\n", q_in);
          exit(1);
        }
      if (damar_track_read_a2(db.path, trim_in, db.nreads, &ta, &td, &nt))
        { fprintf(stderr, "could not open %s track\n", trim_in);
          exit(1);
        }
      if (damar_trim_update(&db, argv[optind + 1], qa, qd, nq, ta, td, trim_q, min_len, p.ccs, &res))
        exit(1);
      if (damar_track_write_a2(db.path, trim_out, block, db.nreads, res.trim_anno, res.trim_data, res.ntrim))
        exit(1);
      free(qa);  free(qd);  free(ta);  free(td);
    }
  else
    { printf(GREEN "PASS quality estimate and trimming" RESET "\n");
      fflush(stdout);
      if (damar_q_track(&db, argv[optind + 1], &p, trim_q, min_len, &res))
        exit(1);
      if (damar_track_write_a2(db.path, trim_out, block, db.nreads, res.trim_anno, res.trim_data, res.ntrim) ||
          damar_track_write_a2(db.path, q_out, block, db.nreads, res.q_anno, res.q_data, res.nq))
        exit(1);
    }
  if (qlog != NULL)
    { if ((f = fopen(qlog, "w")) != NULL)
        { fprintf(f, "%d\n", trim_q);
          fclose(f);
        }
      else
        fprintf(stderr, "error: failed to open %s\n", qlog);
    }
  damar_q_result_free(&res);
  damar_dbinfo_close(&db);
  damar_q_release();
  return 0;
}
