/* OGbuild -- the overlap graph of a filtered .las file: the command of touring/OGbuild.c (option letters, defaults, checks,
 * messages and exit codes of its main, :1789-1942) around damar_og_build (graph.c).  The edges are made on the GPU
 * (kernels/graph_edges.hip) unless DAMAR_PILES=host is set; -c, -s and the writers are host code. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "damar_graph.h"

void damar_og_usage(void);

int main(int argc, char *argv[])
{ damar_og_opts o;
  int c;

  memset(&o, 0, sizeof(o));
  opterr = 0;
  while ((c = getopt(argc, argv, "sc:f:p:t:")) != -1)
    switch (c)
      { case 'p': o.prio = optarg; break;
        case 'f': o.format = optarg; break;
        case 's': o.split = 1; break;
        case 't': o.track = optarg; break;
        case 'c': o.contained = atoi(optarg); break;
        default:
          damar_og_usage();
          exit(1);
      }
  if (argc - optind < 3)
    { damar_og_usage();
      exit(1);
    }
  return damar_og_build(argv[optind], argv[optind + 1], argv[optind + 2], &o);
}
