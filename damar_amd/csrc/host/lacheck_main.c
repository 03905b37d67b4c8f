/* lacheck_main.c -- LAcheck [-p] [-s] [-d] [-i] [-x] <db> <las>
 *
 * The reference suite's checker of .las files (utils/LAcheck.c) on the routine of lascheck.c: the same four options,
 * the same lines on stderr and stdout, the same exit status.  -x adds the strict set, the properties of a file as
 * daligner or datander wrote it (include/damar_check.h).  <db> is the whole database: records carry its read numbers.
 */
#include <stdio.h>
#include <stdlib.h>
#include <unistd.h>

#include "damar_check.h"

static void usage(void)
{ fprintf(stderr, "usage  : [-p] [-s] [-d] [-i] [-x] <db> <las>\n");
  fprintf(stderr, "options: -p ... check pass-through points (0)\n");
  fprintf(stderr, "         -s ... check sort order (0)\n");
  fprintf(stderr, "         -d ... report duplicates. implies -s (0)\n");
  fprintf(stderr, "         -i ... ignore overlaps that are discarded (default: 0)\n");
  fprintf(stderr, "         -x ... strict: what daligner and datander promise of their own files (0)\n");
}

int main(int argc, char *argv[])
{ int options = 0, c;
  opterr = 0;
  while ((c = getopt(argc, argv, "psdix")) != -1)
    switch (c)
    { case 'p': options |= DAMAR_CHECK_PTP;    break;
      case 's': options |= DAMAR_CHECK_SORT;   break;
      case 'd': options |= DAMAR_CHECK_DUPES;  break;
      case 'i': options |= DAMAR_CHECK_IGNORE; break;
      case 'x': options |= DAMAR_CHECK_STRICT; break;
      default:
        usage();
        return 1;
    }
  if (argc - optind != 2)
    { usage();
      return 1;
    }
  return damar_lascheck_file(argv[optind], argv[optind + 1], options, stdout, stderr) != 0;
}
