/* lascheck.c -- the properties of the records of a .las file, checked in file order (include/damar_check.h).
 *
 * The first group is what the reference's utils/LAcheck.c looks at, stated anew: its reader (lib/pass.c) hands the
 * checker the records of one A read at a time, and the checker's answer after each such group is "go on" only while
 * nothing has been found.  Fed record by record that reads:
 *
 *   - a record whose A read differs from the last one's starts a group; with -s it is held against the A read of the
 *     group BEFORE (prev_a, 0 at the start of the file), and against nothing else;
 *   - every other record is held against the record before it -- a discarded one under -i included -- by
 *     (aread, bread, complement flag, abpos); "equal to previous" (-d) needs these equal and flags, aepos, bbpos,
 *     bepos and tlen as well;
 *   - the bounds, and with -p the B values of the trace, for every record looked at;
 *   - once a group has ended with something found, nothing more is counted or looked at, and the count announced by the
 *     header is compared only if nothing was found.
 *
 * The messages of this group are the reference's, so that the tool's output can be held against it line by line.
 * The strict group (DAMAR_CHECK_STRICT) is what tests/test_gpu_parity.py asserts of daligner's own files.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "damar_check.h"
#include "damar_host.h"                   /* damar_trace_at alone: the checker stays a program of its own */

static void say(damar_lascheck *ck, int kind, const char *fmt, ...) __attribute__((format(printf, 3, 4)));

#include <stdarg.h>
static void say(damar_lascheck *ck, int kind, const char *fmt, ...)
{ char    text[256];
  va_list ap;
  if (kind == DAMAR_CHECK_MESSAGE)
    ck->violations += 1;
  if (ck->report == NULL)
    return;
  va_start(ap, fmt);
  vsnprintf(text, sizeof(text), fmt, ap);
  va_end(ap);
  ck->report(ck->arg, kind, text);
}

void damar_lascheck_begin(damar_lascheck *ck, int tspace, int options, damar_check_report report, void *arg)
{ memset(ck, 0, sizeof(*ck));
  if (options & DAMAR_CHECK_DUPES)
    options |= DAMAR_CHECK_SORT;
  ck->tspace = tspace;  ck->options = options;
  ck->report = report;  ck->arg = arg;
}

void damar_lascheck_break(damar_lascheck *ck)
{ ck->split = 1;
}

static int three_way(int64 a, int64 b)
{ return (a > b) - (a < b);
}

/* the order -s asks for */
static int by_sort_keys(const Overlap *l, const Overlap *r)
{ int c;
  if ((c = three_way(l->aread, r->aread)) != 0) return c;
  if ((c = three_way(l->bread, r->bread)) != 0) return c;
  if ((c = three_way(COMP(l->flags), COMP(r->flags))) != 0) return c;
  return three_way(l->path.abpos, r->path.abpos);
}

/* what -d asks for beyond equal sort keys */
static int same_beyond_keys(const Overlap *l, const Overlap *r)
{ return l->flags == r->flags && l->path.aepos == r->path.aepos && l->path.bbpos == r->path.bbpos &&
         l->path.bepos == r->path.bepos && l->path.tlen == r->path.tlen;
}

static void strict_checks(damar_lascheck *ck, const Overlap *o, const void *trace, int tbytes)
{ const Path *p = &o->path;
  const long long n = (long long) ck->seen;
  const int ts = ck->tspace;

  if (p->tlen & 1)
    say(ck, DAMAR_CHECK_MESSAGE, "strict: overlap %lld: tlen %d is odd", n, p->tlen);
  if (p->aepos <= p->abpos)
    say(ck, DAMAR_CHECK_MESSAGE, "strict: overlap %lld: empty A interval [%d,%d)", n, p->abpos, p->aepos);
  if (p->bepos <= p->bbpos)
    say(ck, DAMAR_CHECK_MESSAGE, "strict: overlap %lld: empty B interval [%d,%d)", n, p->bbpos, p->bepos);
  if (trace != NULL && ts > 0 && p->abpos >= 0 && p->aepos > p->abpos && p->tlen >= 0)      /* (no traces at hand, or a run with -T: not held against the panels) */
    { const int panels = p->aepos / ts - p->abpos / ts + (p->aepos % ts != 0);
      if (p->tlen / 2 != panels)
        say(ck, DAMAR_CHECK_MESSAGE, "strict: overlap %lld (%d x %d): %d trace pairs for the %d panels of [%d,%d)",
            n, o->aread, o->bread, p->tlen / 2, panels, p->abpos, p->aepos);
    }
  if (trace != NULL && p->tlen > 0)
    { long long diffs = 0;
      int j, wide = 0;
      for (j = 0; j + 1 < p->tlen; j += 2)
        diffs += damar_trace_at(trace, tbytes, j);
      if (diffs != p->diffs)
        say(ck, DAMAR_CHECK_MESSAGE, "strict: overlap %lld (%d x %d): the trace holds %lld differences, the record %d",
            n, o->aread, o->bread, diffs, p->diffs);
      if (tbytes == 2 && ts <= TRACE_XOVR)
        { for (j = 0; j < p->tlen; j++)
            if (damar_trace_at(trace, 2, j) > 255)
              wide = damar_trace_at(trace, 2, j);
          if (wide)
            say(ck, DAMAR_CHECK_MESSAGE, "strict: overlap %lld (%d x %d): trace value %d does not fit the file's one-byte traces",
                n, o->aread, o->bread, wide);
        }
    }
  if (ck->options & DAMAR_CHECK_PAD)
    { uint32 pad;
      memcpy(&pad, (const char *) &o->bread + sizeof(o->bread), sizeof(pad));
      if (pad != 0)
        say(ck, DAMAR_CHECK_MESSAGE, "strict: overlap %lld: padding bytes are 0x%08x, not zero", n, pad);
    }
}

int damar_lascheck_feed(damar_lascheck *ck, const Overlap *o, const void *trace, int tbytes, int alen, int blen)
{ const int opt = ck->options;
  const int first = !ck->have_prev || ck->split || o->aread != ck->prev.aread;
  long long n;

  if (ck->stopped)
    return 0;
  if (first && ck->have_prev)
    { ck->prev_a = ck->prev.aread;                       /* the group that has just ended */
      if (ck->violations > 0 && !(opt & DAMAR_CHECK_ALL))
        { ck->stopped = 1;
          return 0;
        }
    }
  ck->split = 0;
  ck->seen += 1;
  n = (long long) ck->seen;

  if (!((opt & DAMAR_CHECK_IGNORE) && (o->flags & DAMAR_OVL_DISCARD)))
    { ck->looked += 1;
      if (first)
        { if ((opt & DAMAR_CHECK_SORT) && ck->prev_a > o->aread)
            say(ck, DAMAR_CHECK_MESSAGE, "overlap %lld: not sorted", n);
        }
      else
        { const int c = by_sort_keys(&ck->prev, o);
          if (c > 0 && (opt & DAMAR_CHECK_SORT))
            { say(ck, DAMAR_CHECK_PAIR, "%d %d", ck->prev.aread, ck->prev.bread);
              say(ck, DAMAR_CHECK_MESSAGE, "overlap %lld: not sorted", n);
            }
          else if (c == 0 && (opt & DAMAR_CHECK_DUPES) && same_beyond_keys(&ck->prev, o))
            { say(ck, DAMAR_CHECK_PAIR, "%d %d", o->aread, o->bread);
              say(ck, DAMAR_CHECK_MESSAGE, "overlap %lld: equal to previous overlap", n);
            }
        }
      if (o->path.abpos < 0)
        say(ck, DAMAR_CHECK_MESSAGE, "overlap %lld: abpos < 0", n);
      if (o->path.bbpos < 0)
        say(ck, DAMAR_CHECK_MESSAGE, "overlap %lld: bbpos < 0", n);
      if (alen >= 0 && o->path.aepos > alen)
        say(ck, DAMAR_CHECK_MESSAGE, "overlap %lld: aepos > lena", n);
      if (blen >= 0 && o->path.bepos > blen)
        say(ck, DAMAR_CHECK_MESSAGE, "overlap %lld: bepos > lenb", n);
      if (o->path.tlen < 0)
        say(ck, DAMAR_CHECK_MESSAGE, "overlap %lld: invalid tlen %d", n, o->path.tlen);
      if ((opt & DAMAR_CHECK_PTP) && (trace != NULL || o->path.tlen <= 0))
        { int be = o->path.bbpos, j;
          for (j = 0; j + 1 < o->path.tlen; j += 2)
            be += damar_trace_at(trace, tbytes, j + 1);
          if (be != o->path.bepos)
            say(ck, DAMAR_CHECK_MESSAGE, "overlap %lld (%d x %d): pass-through points inconsistent be = %d (expected %d)",
                n, o->aread, o->bread, be, o->path.bepos);
        }
      if (opt & DAMAR_CHECK_STRICT)
        strict_checks(ck, o, trace, tbytes);
    }
  ck->prev = *o;
  ck->prev.path.trace = NULL;
  ck->have_prev = 1;
  return 1;
}

int64 damar_lascheck_end(damar_lascheck *ck, int64 expected_novl)
{ if (expected_novl >= 0 && expected_novl != ck->seen && (ck->violations == 0 || (ck->options & DAMAR_CHECK_ALL)))
    say(ck, DAMAR_CHECK_MESSAGE, "novl of %lld doesn't match actual overlap count of %lld",
        (long long) expected_novl, (long long) ck->seen);
  return ck->violations;
}

/* ---- a whole file, read the way the reference's reader reads it ----------------------------------------------------
 *
 * The reference reads the records of one A read into an array of slots and their traces, widened to 16 bits, into one
 * buffer; it goes on until the count of the header is reached, whatever the file holds.  A header that announces more
 * records than there are makes it look at a slot it did not fill: the record that lay there from an earlier, larger
 * group (its trace, under -p, being whatever the front of the trace buffer holds, widened once more).  To say of such a
 * file what the reference says, slots and buffer are kept in the same way here; they start out zeroed. */

typedef struct { FILE *out, *err; } Sinks;

static void to_sinks(void *arg, int kind, const char *text)
{ Sinks *s = (Sinks *) arg;
  FILE  *f = (kind == DAMAR_CHECK_PAIR) ? s->out : s->err;
  if (f != NULL)
    fprintf(f, "%s\n", text);
}

#define ON_DISK  (sizeof(Overlap) - sizeof(void *))          /* 40 bytes: the record minus its leading pointer */

static int read_record(FILE *f, Overlap *slot)
{ return fread((char *) slot + sizeof(void *), ON_DISK, 1, f) == 1;
}

static void widen(uint16 *t, int n)                        /* n bytes at t become n 16-bit values, in place */
{ const uint8 *b = (const uint8 *) t;
  int j;
  for (j = n - 1; j >= 0; j--)
    t[j] = b[j];
}

int damar_lascheck_file(const char *dbname, const char *lasname, int options, FILE *out, FILE *err)
{ HITS_DB  db;
  FILE    *f;
  int64    novl = 0, done = 0;
  int      tspace = 0, tbytes, load;
  Overlap *slot;
  uint16  *tr = NULL;                /* the traces of the group in hand, 16 bits a value */
  size_t  *toff;                     /* where slot i's trace starts in tr */
  int64    tcap = 0, ttop;
  int      cap = 500, n = 0, i, go = 1;
  Sinks    sinks;
  damar_lascheck ck;

  sinks.out = out;  sinks.err = err;
  if ((f = fopen(lasname, "r")) == NULL)
    { if (err) fprintf(err, "could not open '%s'\n", lasname);
      return 2;
    }
  if (damar_read_block(dbname, &db))
    { if (err) fprintf(err, "could not open database '%s'\n", dbname);
      fclose(f);
      return 2;
    }
  if (fread(&novl, sizeof(novl), 1, f) != 1 || fread(&tspace, sizeof(tspace), 1, f) != 1)
    novl = 0;
  tbytes = (tspace <= TRACE_XOVR) ? 1 : 2;
  load   = (options & (DAMAR_CHECK_PTP | DAMAR_CHECK_STRICT)) != 0;
  if (options & DAMAR_CHECK_STRICT)
    options |= DAMAR_CHECK_PAD;
  damar_lascheck_begin(&ck, tspace, options, to_sinks, &sinks);

  slot = (Overlap *) calloc((size_t) cap, sizeof(Overlap));
  toff = (size_t *) calloc((size_t) cap, sizeof(size_t));
  if (slot == NULL || toff == NULL)
    { if (err) fprintf(err, "out of memory\n");
      return 2;
    }
  fseeko(f, (off_t) (sizeof(novl) + sizeof(tspace)), SEEK_SET);
  if (!read_record(f, slot))
    go = 0;
  while (go)
    { int a;
      slot[0] = slot[n];                                    /* the record that ended the last group, read or not */
      a = slot[0].aread;
      ttop = 0;
      for (n = 0; ; )
        { Overlap *o = slot + n;
          const int64 len = o->path.tlen > 0 ? o->path.tlen : 0;
          if (load)
            { if (ttop + len > tcap)
                { tcap = (int64) (1.2 * (double) tcap) + ttop + len + 1024;
                  tr = (uint16 *) realloc(tr, sizeof(uint16) * (size_t) tcap);
                  if (tr == NULL)
                    { if (err) fprintf(err, "out of memory\n");
                      return 2;
                    }
                }
              toff[n] = (size_t) ttop;
              if (len > 0)
                { size_t got = fread(tr + ttop, 1, (size_t) tbytes * (size_t) len, f);
                  (void) got;                               /* (a file that ends here: the values stay what they were) */
                  if (tbytes == 1)
                    widen(tr + ttop, (int) len);
                }
              ttop += len;
            }
          else if (len > 0)
            fseeko(f, (off_t) tbytes * (off_t) len, SEEK_CUR);
          n += 1;
          if (n >= cap)
            { const int more = (int) (1.2 * n) + 10;
              slot = (Overlap *) realloc(slot, sizeof(Overlap) * (size_t) more);
              toff = (size_t *) realloc(toff, sizeof(size_t) * (size_t) more);
              if (slot == NULL || toff == NULL)
                { if (err) fprintf(err, "out of memory\n");
                  return 2;
                }
              memset(slot + cap, 0, sizeof(Overlap) * (size_t) (more - cap));
              cap = more;
            }
          if (!read_record(f, slot + n) || slot[n].aread != a)
            break;
        }
      damar_lascheck_break(&ck);
      for (i = 0; i < n && go; i++)
        { const int ar = slot[i].aread - db.ufirst, br = slot[i].bread - db.ufirst;
          go = damar_lascheck_feed(&ck, slot + i, load ? (const void *) (tr + toff[i]) : NULL, 2,
                                   (ar >= 0 && ar < db.nreads) ? db.reads[ar].rlen : -1,
                                   (br >= 0 && br < db.nreads) ? db.reads[br].rlen : -1);
        }
      done += n;
      if (ck.violations > 0 || done >= novl)
        go = 0;
    }
  damar_lascheck_end(&ck, novl);
  free(slot);
  free(toff);
  free(tr);
  fclose(f);
  damar_close_block(&db);
  return ck.violations > 0 ? 1 : 0;
}
