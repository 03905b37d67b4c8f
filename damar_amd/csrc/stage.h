/* stage.h -- what the call families of the tool stages (stages/ *.hip) are built on: a device buffer that is kept
 * between calls, the stage record that owns a family's buffers, events and figures, the uploads onto the seed stream,
 * and two helpers of the host side.  DESIGN.md section 9k.
 */
#ifndef DAMAR_STAGE_H
#define DAMAR_STAGE_H

#include <initializer_list>
#include <stdlib.h>
#include <string.h>

#include "shim_internal.h"

struct DevStage;

struct DBuf                        /* a device buffer kept between calls, grown when a call needs more */
{ void  *p = nullptr;
  size_t cap = 0;
  DBuf  *next;                     /* of the stage's buffers */
  DBuf(DevStage &s);              /* a buffer is made with the stage it belongs to, so DevStage::release() needs no list */
  DBuf(const DBuf &) = delete;
  void *need(size_t n)
  { if (n > cap)
      { if (p) HIP_CHECK(hipFree(p));
        cap = n + n / 4 + 4096;
        HIP_CHECK(hipMalloc(&p, cap));
      }
    return p;
  }
  void drop() { if (p) HIP_CHECK(hipFree(p));  p = nullptr;  cap = 0; }
};

/* What one call family keeps between its calls: the device buffers, the events that time a call's phases on G_st, and the
   figures of the last call for its damar_*_last.  A family is a static of a struct derived from this one whose members are
   its buffers by name; damar_homog holds one per handle. */
struct DevStage
{ DBuf      *bufs = nullptr;
  hipEvent_t ev[5] = { NULL, NULL, NULL, NULL, NULL };       /* made on first use, kept like the buffers */
  double     ms[4] = { 0, 0, 0, 0 };
  int64      cnt[4] = { 0, 0, 0, 0 };
  double     w0 = 0;               /* the wall clock at begin() */

  /* The frame of a call whose ms are upload, kernel, download and the whole call by the wall clock: begin() first of all;
     device() before the device is touched, where the call gets that far; its work between mark(0) .. mark(3);
     sync_laps(0, 3); end() with the three counts of a call that succeeded.  (Hidden: the members below them that the
     compiler leaves out of line are among the library's dynamic symbols, and that set stays as it is.) */
  DAMAR_INTERNAL void begin()
  { for (double &m : ms) m = 0;
    w0 = now_ms();
  }
  DAMAR_INTERNAL void device()
  { ensure_init();
    /* a tool built on one of these calls is through a few milliseconds after the library comes up: its launch, its copies
       and the frees of the family's release would all run beside the start-up thread, which is inside HIP calls of its own
       for longer than that.  The process cannot end before that thread does (helpers_join), so waiting here costs nothing. */
    late_streams();
  }
  DAMAR_INTERNAL void sync_laps(int first, int n)       /* G_st drained, then laps() */
  { HIP_CHECK(hipStreamSynchronize(G_st));
    laps(first, n);
  }
  DAMAR_INTERNAL void end(int64 c0, int64 c1, int64 c2)
  { cnt[0] = c0;  cnt[1] = c1;  cnt[2] = c2;
    ms[3] = now_ms() - w0;
  }

  void mark(int i)                 /* event i, here on G_st */
  { if (ev[0] == NULL)
      for (hipEvent_t &e : ev) HIP_CHECK(hipEventCreate(&e));
    HIP_CHECK(hipEventRecord(ev[i], G_st));
  }
  void laps_add(int first, int n)  /* after the caller's synchronise: the time from event i to event i + 1 added to ms[i], n of them */
  { for (int i = first; i < first + n; i++)
      { float t = 0;
        HIP_CHECK(hipEventElapsedTime(&t, ev[i], ev[i + 1]));
        ms[i] += t;
      }
  }
  void laps(int first, int n)      /* the same, written over ms[i] */
  { for (int i = first; i < first + n; i++) ms[i] = 0;
    laps_add(first, n);
  }
  void last(double *m, int64 *c, int ncnt) const
  { for (int i = 0; i < 4; i++) m[i] = ms[i];
    for (int i = 0; i < ncnt; i++) c[i] = cnt[i];
  }
  void release()                   /* the buffers and the events; the figures stay */
  { for (DBuf *b = bufs; b != NULL; b = b->next) b->drop();
    if (ev[0] != NULL)
      for (hipEvent_t &e : ev)
        { (void) hipEventDestroy(e);
          e = NULL;
        }
  }
};

inline DBuf::DBuf(DevStage &s) : next(s.bufs) { s.bufs = this; }

/* src[0 .. n) into b on G_st: room for it and 16 bytes more (the kernels' wide loads may reach past the last value), the
   copy where there is something to copy */
template <typename T>
static inline T *up(DBuf &b, const T *src, size_t n)
{ T *d = (T *) b.need(sizeof(T) * n + 16);
  if (n > 0)
    HIP_CHECK(hipMemcpyAsync(d, src, sizeof(T) * n, hipMemcpyHostToDevice, G_st));
  return d;
}

/* a track of the database: anno[nreads + 1] byte offsets into data[ndata] */
struct DevTrack { const u64 *anno;  const int *data; };

static inline DevTrack up_track(DBuf &anno, DBuf &data, const uint64 *a, size_t nreads, const int *d, int64 ndata)
{ DevTrack k;
  k.anno = (const u64 *) up(anno, a, nreads + 1);
  k.data = up(data, d, (size_t) ndata);
  return k;
}

/* A stage whose calls take a damar_pile_batch or a damar_trace_batch, and the batch as pile_up() leaves it on the device:
   col[i] is the i-th of the record columns the caller named, toff and trace are there for a trace batch */
struct PileStage : DevStage
{ DBuf off{*this}, aread{*this}, col[8] = { *this, *this, *this, *this, *this, *this, *this, *this }, toff{*this}, trace{*this};
};

struct PileDev
{ const long long *off, *toff;
  const int *aread, *col[8];
  const u8  *trace;
};

static inline PileDev pile_up(PileStage &S, const damar_pile_batch *b, const damar_trace_batch *t, std::initializer_list<const int *> cols)
{ const size_t np = (size_t) b->npiles, nrec = (size_t) b->nrec;
  PileDev d;
  memset(&d, 0, sizeof(d));
  d.off = (const long long *) up(S.off, b->pile_off, np + 1);
  d.aread = up(S.aread, b->pile_aread, np);
  int i = 0;
  for (const int *c : cols)
    { d.col[i] = up(S.col[i], c, nrec);
      i += 1;
    }
  if (t != NULL)
    { d.toff = (const long long *) up(S.toff, t->trace_off, nrec);
      d.trace = up(S.trace, t->trace, (size_t) t->trace_bytes);
    }
  return d;
}

/* a limit the library was built with, lowered by a test through the environment: a value below `floor` or not below the
   limit leaves it as it is */
static inline int test_limit(const char *name, int built, int floor)
{ const char *e = getenv(name);
  const int v = (e != NULL) ? atoi(e) : built;
  return (v >= floor && v < built) ? v : built;
}

/* k more items of `per` values each at the end of a list that grows by realloc (a pile's results behind those of the piles
   before it); 1 after a message, the list freed */
template <typename T>
static inline int list_append(T **list, int64 *n, int64 *cap, size_t per, const T *src, int64 k, const char *what)
{ if (*n + k > *cap)
    { const int64 c = *n + k + *cap / 4 + 256;
      T *grown = (T *) realloc(*list, sizeof(T) * per * (size_t) c);
      if (grown == NULL)
        { fprintf(stderr, "damar: out of memory (%s)\n", what);
          free(*list);
          return 1;
        }
      *list = grown;
      *cap = c;
    }
  if (k > 0)
    memcpy(*list + per * (size_t) *n, src, sizeof(T) * per * (size_t) k);
  *n += k;
  return 0;
}

#endif
