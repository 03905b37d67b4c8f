/* laspass.c -- what every pass over a .las file needs beside its own middle (trim.c, stitch.c, gap.c, filter.c and the
 * passes that write no .las): memory that grows or ends the run, a batch bound to the database's read table, and the
 * records written back in file order as lib/pass.c writes them.
 * Plain C: nothing of the GPU runtime, nothing of the other host files. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "damar_host.h"

void *damar_grow(void *p, size_t n, const char *who)
{ void *q = realloc(p, n ? n : 1);
  if (q == NULL)
    { fprintf(stderr, "damar: out of memory (%zu bytes, %s)\n", n, who);
      exit(1);
    }
  return q;
}

void *damar_reserve(void *p, int64 *cap, int64 need, size_t size, int64 slack, const char *who)
{ if (damar_room(cap, need, slack))
    p = damar_grow(p, size * (size_t) *cap, who);
  return p;
}

/***** a batch and the database ********************************************************************/

int damar_reads_missing(const char *las)
{ fprintf(stderr, "damar: %s holds reads the database does not have\n", las);
  return 1;
}

int damar_batch_bind(damar_pile_batch *b, const damar_dbinfo *db, const char *las, int reads)
{ int64 i;
  b->read_len = db->read_len;  b->read_flags = db->read_flags;
  b->nreads = db->nreads;  b->maxlen = db->maxlen;
  if (reads >= DAMAR_BIND_A)
    for (i = 0; i < b->npiles; i++)
      if (b->pile_aread[i] < 0 || b->pile_aread[i] >= db->nreads)
        return damar_reads_missing(las);
  if (reads >= DAMAR_BIND_AB)
    for (i = 0; i < b->nrec; i++)
      if (b->bread[i] < 0 || b->bread[i] >= db->nreads)
        return damar_reads_missing(las);
  return 0;
}

/***** the records written ***************************************************************************/

int damar_cannot_write(const char *path)
{ fprintf(stderr, "damar: cannot write %s\n", path);
  return 1;
}

struct damar_las_out
{ FILE  *f;
  char  *path;
  int    purge, failed;        /* failed: a write was refused; close says so */
  int64  written, discarded;
  unsigned char *buf;          /* a record with its trace narrowed */
  int64  cap;
};

damar_las_out *damar_las_out_open(const char *path, int purge)
{ FILE *f = fopen(path, "w");
  damar_las_out *o;
  if (f == NULL)
    return NULL;
  o = (damar_las_out *) memset(damar_grow(NULL, sizeof(*o), "las out"), 0, sizeof(*o));
  o->f = f;
  o->path = strcpy((char *) damar_grow(NULL, strlen(path) + 1, "las out"), path);
  o->purge = purge;
  return o;
}

int damar_las_out_begin(damar_las_out *o, int tspace)
{ const int64 zero = 0;
  if (fwrite(&zero, sizeof(int64), 1, o->f) != 1 || fwrite(&tspace, sizeof(int), 1, o->f) != 1)
    o->failed = 1;
  return o->failed;
}

/* lib/pass.c:230 takes OVL_TEMP off every record it writes; lib/pass.c's Write_Overlap narrows the trace */
int damar_las_out_put(damar_las_out *o, const int *rec, const unsigned char *bytes, const uint16 *vals, int tbytes, const char *tool)
{ const int   tlen = rec[0];
  const int64 need = 40 + (int64) tbytes * tlen;
  int w[10], k;
  if (rec[6] & OVL_DISCARD)
    { o->discarded += 1;
      if (o->purge)
        return 0;
    }
  o->buf = (unsigned char *) damar_reserve(o->buf, &o->cap, need, 1, 1024, "las out");
  memcpy(w, rec, 40);
  w[6] &= ~OVL_TEMP;
  memcpy(o->buf, w, 40);
  if (vals == NULL)
    { if (tlen > 0)
        memcpy(o->buf + 40, bytes, (size_t) (need - 40));
    }
  else if (tbytes == 1)
    for (k = 0; k < tlen; k++)
      { if (vals[k] > 255)
          { fprintf(stderr, "%s: Compression of trace to bytes fails, value too big\n", tool);
            return 2;
          }
        o->buf[40 + k] = (unsigned char) vals[k];
      }
  else
    memcpy(o->buf + 40, vals, sizeof(uint16) * (size_t) tlen);
  if (fwrite(o->buf, 1, (size_t) need, o->f) != (size_t) need)
    return o->failed = 1;
  o->written += 1;
  return 0;
}

int64 damar_las_out_written(const damar_las_out *o)
{ return o->written; }

int damar_las_out_close(damar_las_out *o, int ok, int64 *written, int64 *discarded)
{ int bad = o->failed;
  if (ok && !bad)
    { rewind(o->f);
      bad = fwrite(&o->written, sizeof(int64), 1, o->f) != 1;
    }
  if (fclose(o->f) != 0 && ok)
    bad = 1;
  if (bad)
    damar_cannot_write(o->path);
  if (ok)
    *written = o->written;
  *discarded = o->discarded;
  free(o->path);  free(o->buf);  free(o);
  return bad;
}
