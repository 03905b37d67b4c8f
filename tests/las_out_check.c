/* las_out_check.c -- the record writer of host/laspass.c on its own: a program that writes a handful of small .las files
 * into the directory it is given and says on stdout what every call returned.  tests/test_las_out.py builds it from
 * laspass.c alone, runs it and reads the files back.
 *   <name> put <outcome> ...  close <rc> written <n> discarded <n>  */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "damar_host.h"

#define MAXT 8

typedef struct { int flags, tlen; int v[MAXT]; } Rec;

static const char *g_dir;

/* the records of r through one writer: as 16-bit values (wide) or as the bytes a file of tbytes would hold */
static void run(const char *name, int tspace, int tbytes, int purge, int as_vals, const char *tool, const Rec *r, int n)
{ char   path[4096];
  damar_las_out *o;
  int64  written = -1, discarded = -1;
  int    i, k, rc;
  snprintf(path, sizeof(path), "%s/%s.las", g_dir, name);
  if ((o = damar_las_out_open(path, purge)) == NULL)
    { printf("%s open failed\n", name);
      exit(1);
    }
  printf("%s begin %d put", name, damar_las_out_begin(o, tspace));
  for (i = 0; i < n; i++)
    { int    rec[10];
      uint16 vals[MAXT];
      unsigned char bytes[2 * MAXT];
      for (k = 0; k < r[i].tlen; k++)
        { vals[k] = (uint16) r[i].v[k];
          if (tbytes == 1)
            bytes[k] = (unsigned char) r[i].v[k];
          else
            memcpy(bytes + 2 * k, vals + k, 2);
        }
      rec[0] = r[i].tlen;  rec[1] = 10 + i;  rec[2] = 100 * i;  rec[3] = 7;  rec[4] = 100 * i + 150;  rec[5] = 160;
      rec[6] = r[i].flags;  rec[7] = 3;  rec[8] = 5 + i;  rec[9] = 0;
      printf(" %d", damar_las_out_put(o, rec, as_vals ? NULL : bytes, as_vals ? vals : NULL, tbytes, tool));
    }
  printf(" written-so-far %lld", (long long) damar_las_out_written(o));
  rc = damar_las_out_close(o, 1, &written, &discarded);
  printf(" close %d written %lld discarded %lld\n", rc, (long long) written, (long long) discarded);
}

int main(int argc, char **argv)
{ static const Rec mixed[] = { { 0x0, 4, { 3, 90, 2, 70 } }, { 0x2, 2, { 1, 50 } }, { 0x801, 2, { 0, 255 } }, { 0x0, 0, { 0 } },
                               { 0x802, 4, { 9, 99, 8, 88 } }, { 0x1, 2, { 255, 255 } } };
  static const Rec wide[] = { { 0x0, 4, { 3, 256, 2, 1000 } }, { 0x800, 2, { 65535, 0 } }, { 0x0, 0, { 0 } } };
  static const Rec big[] = { { 0x0, 2, { 1, 100 } }, { 0x0, 2, { 1, 256 } }, { 0x0, 4, { 2, 255, 3, 50 } } };
  if (argc != 2)
    return 2;
  g_dir = argv[1];
  run("keep", 100, 1, 0, 1, "(null)", mixed, 6);
  run("purge", 100, 1, 1, 1, "(null)", mixed, 6);
  run("bytes1", 100, 1, 0, 0, "(null)", mixed, 6);
  run("vals2", 200, 2, 0, 1, "(null)", wide, 3);
  run("bytes2", 200, 2, 0, 0, "(null)", wide, 3);
  run("refused_null", 100, 1, 0, 1, "(null)", big, 3);
  run("refused_latrim", 100, 1, 1, 1, "LAtrim", big, 3);
  run("empty", 100, 1, 0, 1, "(null)", mixed, 0);
  return 0;
}
