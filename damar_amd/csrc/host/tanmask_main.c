/* TANmask -- the tandem mask track of a block from datander's self-overlaps: the command of scrub/TANmask.c (:328-531)
 * around damar_tan_track (masks.c).  The reference's -l does not reach its sweep (a local MIN_LEN in its main shadows the
 * one TANDEM() reads, :88 against :334), so it masks with threshold 0 whatever -l says; this command accepts -l and does
 * the same.  The library call and the Python interface take the threshold they are given. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "damar_hip.h"
#include "damar_host.h"

static void usage(void)
{ fprintf(stderr, "usage:  \n\n");
  fprintf(stderr, "TANmask [-v] [-l<int>] [-m<track(tan)>] <source:db> <overlaps:las> ...\n\n");
  fprintf(stderr, "options: -v ... verbose\n");
  fprintf(stderr, "         -l ... minimum alignment length (default: 500)\n");
  fprintf(stderr, "         -m ... output track name (default: %s)\n", "tan");
}

int main(int argc, char *argv[])
{ damar_dbinfo db;
  const char *mask = "tan";
  int   verbose = 0, min_len = 500, c, i;
  int64 nreads = 0, totlen = 0, nmasks = 0, masked = 0;

  opterr = 0;
  while ((c = getopt(argc, argv, "vl:m:")) != -1)
    switch (c)
      { case 'v': verbose = 1; break;
        case 'l': min_len = atoi(optarg); break;
        case 'm': mask = optarg; break;
        default:
          fprintf(stderr, "Unsupported option: %s\n", argv[optind - 1]);
          usage();
          exit(1);
      }
  if (optind + 2 > argc)
    { fprintf(stderr, "[ERROR] - at least one subject block and one LAS file are required\n\n");
      usage();
      exit(1);
    }
  { /* :379-382: the database, never one of its blocks */
    char *root = damar_root(argv[optind], ".db"), *dot = strrchr(root, '.'), *end;
    if (dot != NULL && dot[1] != '\0' && strtol(dot + 1, &end, 10) > 0 && *end == '\0')
      { FILE *f;
        char  path[4400];
        snprintf(path, sizeof(path), "%s%s", argv[optind], strstr(argv[optind], ".db") ? "" : ".db");
        if ((f = fopen(path, "r")) == NULL)         /* no database of that very name: it names a block */
          { fprintf(stderr, "TANmask: Cannot be called on a block: %s\n", argv[optind]);
            exit(1);
          }
        fclose(f);
      }
    free(root);
  }
  if (damar_dbinfo_open(argv[optind], &db))
    exit(1);
  if (verbose)
    { printf("\nTANmask -l%d -m%s %s", min_len, mask, argv[optind]);
      for (i = optind + 1; i < argc; i++)
        printf(" %s", argv[i]);
      printf("\n");
    }
  for (c = optind + 1; c < argc; c++)
    { char  *las = damar_root(argv[c], ".las"), *dot = strrchr(las, '.'), *end;
      char   dir[4096], path[8300];
      const char *slash = strrchr(argv[c], '/');
      int    part = 0, first = 0, last = db.nreads, rc;
      int64 *offs = NULL;
      int   *data = NULL;
      int64  nm, mk;

      if (dot != NULL)
        { long v = strtol(dot + 1, &end, 10);
          if (*end == '\0' && end != dot + 1)
            { if (db.nblocks == 0 || v < 1 || v > db.nblocks)
                { fprintf(stderr, "TANmask: DB %s has no block %ld\n", argv[optind], v);
                  exit(1);
                }
              part = (int) v;
              first = db.block_first[part - 1];
              last = db.block_first[part];
              *dot = '\0';
            }
        }
      if (slash == NULL) strcpy(dir, ".");
      else               snprintf(dir, sizeof(dir), "%.*s", (int) (slash - argv[c]), argv[c]);
      if (part > 0) snprintf(path, sizeof(path), "%s/%s.%d.las", dir, las, part);
      else          snprintf(path, sizeof(path), "%s/%s.las", dir, las);
      (void) min_len;                                          /* see the head of this file */
      rc = damar_tan_track(&db, path, first, last, 0, &offs, &data, &nm, &mk);
      if (rc == 2)
        { fprintf(stderr, "TANmask: .las file overlaps don't correspond to reads in block %d of DB\n", part);
          exit(1);
        }
      if (rc)
        exit(1);
      if (damar_track_write_anno(db.path, mask, part, last - first, offs, data))
        exit(1);
      for (i = first; i < last; i++)
        totlen += db.read_len[i];
      nreads += last - first;
      nmasks += nm;
      masked += mk;
      free(offs);
      free(data);
      free(las);
    }
  if (verbose)
    { printf("\nInput:    %7lld (100.0%%) reads     %12lld (100.0%%) bases\n", (long long) nreads, (long long) totlen);
      printf("Masks:    %7lld (%5.1f%%) masks     %12lld (%5.1f%%) bases\n", (long long) nmasks, (100. * nmasks) / nreads,
             (long long) masked, (100. * masked) / totlen);
    }
  damar_dbinfo_close(&db);
  damar_pile_release();
  return 0;
}
