/* DBdust -- the low-complexity mask track of a block or a database: the command of db/DBdust.c (:92-217) around
 * damar_dust_track (dust.c).  Messages, usage text and exit statuses are the reference's, down to what its option loop
 * prints for an option it does not know (the argument after it).  A .dam is refused: this project reads .db only. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "damar_hip.h"
#include "damar_host.h"

static void usage(void)
{ fprintf(stderr, "usage: [-b] [-w <int(64)>] [-t<double(2.)>] [-m<int(10)>] <path:db|dam>\n");
  fprintf(stderr, "options: -b ... biased, i.e. take into account the frequency of a given base\n");
  fprintf(stderr, "         -w ... scan window size\n");
  fprintf(stderr, "         -t ... thershold for being a low complexity interval\n");
  fprintf(stderr, "         -m ... intervals greater than -m bases are reported\n");
}

int main(int argc, char *argv[])
{ damar_dust_params p;
  int   c, minlen = 9;
  int64 stats[6] = { 0, 0, 0, 0, 0, 0 };

  memset(&p, 0, sizeof(p));
  p.window = 64;
  p.thresh = 2.;
  opterr = 0;
  while ((c = getopt(argc, argv, "bw:t:m:")) != -1)
    switch (c)
      { case 'b':
          p.biased = 1;
          break;
        case 'w':
          p.window = atoi(optarg);
          if (p.window <= 0)
            { fprintf(stderr, "[ERROR] Window must be positive (%d)\n", p.window);
              exit(1);
            }
          break;
        case 't':
          p.thresh = atof(optarg);
          if (p.thresh <= 0.)
            { fprintf(stderr, "[ERROR] Threshold must be positive (%f)\n", p.thresh);
              exit(1);
            }
          break;
        case 'm':
          minlen = atof(optarg) - 1;                      /* the last base's distance from the first, :139 */
          if (minlen <= 0)
            { fprintf(stderr, "[ERROR] Minimum hit size must be positive (%d)\n", minlen);
              exit(1);
            }
          break;
        default:
          fprintf(stderr, "Unsupported option: %s\n", argv[optind]);
          usage();
          exit(1);
      }
  if (optind + 1 > argc)
    { fprintf(stderr, "[ERROR] DB is required!\n");
      usage();
      exit(1);
    }
  p.minlen = minlen + 1;
  { /* a .dam by its suffix, or by being the only file of that root */
    const char *name = argv[optind];
    const size_t n = strlen(name);
    char  path[4400];
    FILE *f;
    int   dam = n > 4 && strcmp(name + n - 4, ".dam") == 0;
    if (!dam && !(n > 3 && strcmp(name + n - 3, ".db") == 0))
      { char *root = damar_root(name, ".db"), *dot = strrchr(root, '.'), *end;
        const char *slash = strrchr(name, '/');
        if (dot != NULL && dot[1] != '\0' && strtol(dot + 1, &end, 10) > 0 && *end == '\0')
          *dot = '\0';                                    /* a block's number */
        snprintf(path, sizeof(path), "%.*s%s.db", slash == NULL ? 0 : (int) (slash - name + 1), name, root);
        if ((f = fopen(path, "r")) != NULL)
          fclose(f);
        else
          { snprintf(path, sizeof(path), "%.*s%s.dam", slash == NULL ? 0 : (int) (slash - name + 1), name, root);
            if ((f = fopen(path, "r")) != NULL)
              { fclose(f);
                dam = 1;
              }
          }
        free(root);
      }
    if (dam)
      { fprintf(stderr, "DBdust: %s is a .dam: only a .db is read here\n", name);
        exit(1);
      }
  }
  if (damar_dust_track(argv[optind], &p, stats))
    exit(1);
  if (getenv("DAMAR_DUST_STATS") != NULL)                 /* for measurement: what the calls counted, on stderr */
    fprintf(stderr, "DBdust: reads %lld host_reads %lld intervals %lld bases %lld steps %lld walk_steps %lld\n", (long long) stats[0],
            (long long) stats[1], (long long) stats[2], (long long) stats[3], (long long) stats[4], (long long) stats[5]);
  damar_dust_release();
  return 0;
}
