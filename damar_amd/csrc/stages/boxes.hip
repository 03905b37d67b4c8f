/* stages/boxes.hip -- the C-ABI of exact alignment in boxes: damar_align_boxes, damar_align_reads, damar_trace_boxes */
#include <algorithm>
#include <vector>
#include <limits.h>

#include "stage.h"

/***** exact alignment of batches of boxes: what damar_align_boxes, damar_align_reads and damar_trace_boxes share **********/

/* A stage whose calls take a batch of boxes: the batch's columns, where a box's output begins (off), and what comes back:
   the differences, the length of a box's output (-1: the box is the host routine's) and the output itself.
   ms of the last call: upload, kernel, download (HIP events), whole call (wall);
   cnt: boxes, boxes the host routine did beside the kernel, values of output */
struct BoxStage : DevStage
{ DBuf m{*this}, n{*this}, aoff{*this}, boff{*this}, off{*this}, bases{*this}, diffs{*this}, len{*this}, out{*this};
  void *room(size_t nb, size_t out_bytes)      /* for what comes back, before the upload is timed: -> the output's */
  { diffs.need(sizeof(int) * nb);
    len.need(sizeof(int) * nb);
    return out.need(out_bytes);
  }
};

/* damar_box_batch and damar_tbox_batch as one (abpos is NULL for the first); no batch at all is one of -1 boxes */
struct BoxBatch
{ int64 nbox;
  const int *m, *n, *abpos;
  const int64 *aoff, *boff;
  const char *bases;
  int64 nbases;
};

static BoxBatch box_batch(const damar_box_batch *b)
{ return (b == NULL) ? BoxBatch{ -1 } : BoxBatch{ b->nbox, b->m, b->n, NULL, b->aoff, b->boff, b->bases, b->nbases }; }

static BoxBatch box_batch(const damar_tbox_batch *b)
{ return (b == NULL) ? BoxBatch{ -1 } : BoxBatch{ b->nbox, b->m, b->n, b->abpos, b->aoff, b->boff, b->bases, b->nbases }; }

/* false after a message when a call cannot take the batch.  what: the family's word in its messages; args_ok: what the call
   asks of its other arguments */
static bool box_batch_valid(const char *what, const BoxBatch &v, bool args_ok, const int *diffs)
{ if (!args_ok || v.nbox < 0 || (v.nbox > 0 && diffs == NULL))
    { fprintf(stderr, "damar: %s: malformed batch\n", what);
      return false;
    }
  if (v.nbox >= ((int64) 1 << 31))
    { fprintf(stderr, "damar: %s: a batch holds fewer than 2^31 boxes\n", what);
      return false;
    }
  for (size_t i = 0; i < (size_t) v.nbox; i++)
    if (v.m[i] < 1 || v.n[i] < 1 || (v.abpos != NULL && v.abpos[i] < 0) || v.aoff[i] < 0 || v.boff[i] < 0 || v.aoff[i] + v.m[i] > v.nbases ||
        v.boff[i] + v.n[i] > v.nbases)
      { char at[32] = "";
        if (v.abpos != NULL)
          snprintf(at, sizeof(at), " at %d", v.abpos[i]);
        fprintf(stderr, "damar: %s: box %zu (%d x %d%s) does not lie inside the %lld bases\n", what, i, v.m[i], v.n[i], at, (long long) v.nbases);
        return false;
      }
  return true;
}

struct BoxDev
{ const int *m, *n;
  const long long *aoff, *boff, *off;
  const u8 *bases;
  int *diffs, *len;
};

/* after S.room(): the batch onto the device on G_st, off[nbox + 1] with it, and every length that comes back -1 */
static BoxDev box_up(BoxStage &S, const BoxBatch &v, const long long *off)
{ const size_t nb = (size_t) v.nbox;
  BoxDev d;
  d.m = up(S.m, v.m, nb);
  d.n = up(S.n, v.n, nb);
  d.aoff = (const long long *) up(S.aoff, v.aoff, nb);
  d.boff = (const long long *) up(S.boff, v.boff, nb);
  d.off = up(S.off, off, nb + 1);
  d.bases = (const u8 *) up(S.bases, v.bases, (size_t) v.nbases);
  d.diffs = (int *) S.diffs.p;
  d.len = (int *) S.len.p;
  HIP_CHECK(hipMemsetAsync(d.len, 0xff, sizeof(int) * nb, G_st));
  return d;
}

static void box_down(const BoxDev &d, size_t nb, int *diffs, int *len)          /* the differences and the lengths back, on G_st */
{ HIP_CHECK(hipMemcpyAsync(diffs, d.diffs, sizeof(int) * nb, hipMemcpyDeviceToHost, G_st));
  HIP_CHECK(hipMemcpyAsync(len, d.len, sizeof(int) * nb, hipMemcpyDeviceToHost, G_st));
}

/* what the kernel left: boxes beyond its bounds (and all of them on the host route), through one(i), the host routine on
   box i, which sets len[i] and returns the differences; -> how many the host routine did beside the kernel */
template <typename One>
static int64 box_rest(std::vector<int> &len, int *diffs, bool host, One one)
{ int64 fallback = 0;
  for (size_t i = 0; i < len.size(); i++)
    if (len[i] < 0)
      { diffs[i] = one(i);
        fallback += host ? 0 : 1;
      }
  return fallback;
}

/* damar_align_boxes and damar_align_reads.  what: the family's word in its messages; host: its switch to the host routine;
   order: where the order goes in which the workgroups take the boxes, longest first, or NULL for the order of the batch;
   launch(a): the family's bound into a and its kernel on G_st */
template <typename Launch>
static int box_scripts(BoxStage &S, const char *what, const damar_box_batch *b, int *diffs, int64 *soff, int **script, bool host, DBuf *order,
                       Launch launch)
{ S.begin();
  const BoxBatch v = box_batch(b);
  if (!box_batch_valid(what, v, soff != NULL && script != NULL, diffs))
    return 1;
  const size_t nb = (size_t) v.nbox;
  /* every box gets max(m, n) values of room; the scripts are moved together at the end */
  std::vector<long long> room(nb + 1);
  room[0] = 0;
  for (size_t i = 0; i < nb; i++)
    room[i + 1] = room[i] + std::max(v.m[i], v.n[i]);
  std::vector<int> wide((size_t) room[nb] + 1), slen(nb, -1);

  if (!host && nb > 0)
    { S.device();
      /* longest first: the workgroups take the boxes in this order, and the longest box is the launch's critical path */
      std::vector<u32> longest;
      if (order != NULL)
        { longest.resize(nb);
          for (size_t i = 0; i < nb; i++) longest[i] = (u32) i;
          std::stable_sort(longest.begin(), longest.end(), [&](u32 x, u32 y) { return std::max(v.m[x], v.n[x]) > std::max(v.m[y], v.n[y]); });
        }
      BoxArgs a;
      memset(&a, 0, sizeof(a));
      a.nbox = (u32) nb;
      a.script = (int *) S.room(nb, sizeof(int) * ((size_t) room[nb] + 1));
      S.mark(0);
      const BoxDev d = box_up(S, v, room.data());
      if (order != NULL)
        a.order = up(*order, longest.data(), nb);
      S.mark(1);
      a.m = d.m;  a.n = d.n;  a.aoff = d.aoff;  a.boff = d.boff;  a.coff = d.off;  a.bases = d.bases;  a.diffs = d.diffs;  a.slen = d.len;
      launch(&a);
      HIP_CHECK(hipGetLastError());
      S.mark(2);
      box_down(d, nb, diffs, slen.data());
      if (room[nb] > 0)
        HIP_CHECK(hipMemcpyAsync(wide.data(), a.script, sizeof(int) * (size_t) room[nb], hipMemcpyDeviceToHost, G_st));
      S.mark(3);
      S.sync_laps(0, 3);
    }
  const int64 fallback = box_rest(slen, diffs, host, [&](size_t i)
    { return damar_exact_box(v.bases + v.aoff[i], v.m[i], v.bases + v.boff[i], v.n[i], wide.data() + room[i], &slen[i]); });
  soff[0] = 0;
  for (size_t i = 0; i < nb; i++)
    soff[i + 1] = soff[i] + slen[i];
  *script = (int *) malloc(sizeof(int) * (size_t) soff[nb] + 8);
  if (*script == NULL)
    { fprintf(stderr, "damar: out of memory (%s)\n", what);
      return 1;
    }
  for (size_t i = 0; i < nb; i++)
    if (slen[i] > 0)
      memcpy(*script + soff[i], wide.data() + room[i], sizeof(int) * (size_t) slen[i]);
  S.end(v.nbox, fallback, soff[nb]);
  return 0;
}

/***** exact alignment of a batch of boxes with their edit scripts: Compute_Alignment(DIFF_ALIGN) (kernels/box_align.hip) ******/

static BoxStage BX;

extern "C" void damar_box_release(void) { BX.release(); }

extern "C" unsigned int damar_box_grid(void) { return damar_box_align_grid(); }

extern "C" void damar_box_last(double *ms, int64 *cnt) { BX.last(ms, cnt, 3); }

extern "C" int damar_align_boxes(const damar_box_batch *b, int *diffs, int64 *soff, int **script)
{ return box_scripts(BX, "boxes", b, diffs, soff, script, damar_trim_on_host() != 0, NULL, [](BoxArgs *a)
    { a->maxlen = test_limit("DAMAR_TEST_BOX_LIMIT", DAMAR_BOX_MAXLEN, INT_MIN);
      damar_launch_box_align(a, G_st);
    });
}

/***** the same for boxes of read length, LAcorrect's postrace (kernels/read_align.hip) ******/

static struct : BoxStage { DBuf order{*this}; } RD;

extern "C" void damar_read_release(void) { RD.release(); }

extern "C" unsigned int damar_read_grid(void) { return damar_read_align_grid(); }

extern "C" void damar_read_last(double *ms, int64 *cnt) { RD.last(ms, cnt, 3); }

extern "C" int damar_postrace_on_host(void)
{ const char *e = getenv("DAMAR_POSTRACE");
  return e != NULL && strcmp(e, "host") == 0;
}

extern "C" int damar_align_reads(const damar_box_batch *b, int *diffs, int64 *soff, int **script)
{ return box_scripts(RD, "reads", b, diffs, soff, script, damar_postrace_on_host() != 0, &RD.order, [](BoxArgs *a)
    { a->maxdiff = test_limit("DAMAR_TEST_READ_DIFFS", DAMAR_READ_MAXDIFF, 0);
      damar_launch_read_align(a, (u32) test_limit("DAMAR_TEST_READ_GRID", (int) damar_read_align_grid(), 1), G_st);
    });
}

/***** exact alignment of a batch of boxes into trace pairs: Compute_Alignment(DIFF_TRACE) (kernels/box_trace.hip) ******/

static struct : BoxStage { DBuf large{*this}, abpos{*this}; } TB;

extern "C" void damar_tbox_release(void) { TB.release(); }

extern "C" unsigned int damar_tbox_grid(void) { return damar_box_trace_grid(); }

extern "C" void damar_tbox_last(double *ms, int64 *cnt) { TB.last(ms, cnt, 3); }

extern "C" int damar_trace_boxes(const damar_tbox_batch *b, int *diffs, int64 *toff, uint16 **trace)
{ TB.begin();
  const BoxBatch v = box_batch(b);
  if (!box_batch_valid("trace boxes", v, toff != NULL && trace != NULL && b != NULL && b->tspace >= 1, diffs))
    return 1;
  const size_t nb = (size_t) v.nbox;
  const int    ts = b->tspace;
  /* a box's number of values follows from where it lies on A's grid: the pairs go straight to their place */
  toff[0] = 0;
  for (size_t i = 0; i < nb; i++)
    toff[i + 1] = toff[i] + 2 * (int64) ((v.abpos[i] % ts + v.m[i] + ts - 1) / ts);
  *trace = (uint16 *) malloc(sizeof(uint16) * (size_t) toff[nb] + 8);
  if (*trace == NULL)
    { fprintf(stderr, "damar: out of memory (trace boxes)\n");
      return 1;
    }
  std::vector<int> tlen(nb, -1);

  const bool host = damar_stitch_on_host() != 0;
  if (!host && nb > 0)
    { TB.device();
      TBoxArgs a;
      memset(&a, 0, sizeof(a));
      a.nbox = (u32) nb;
      a.maxlen = test_limit("DAMAR_TEST_BOX_LIMIT", DAMAR_TBOX_MAXLEN, INT_MIN);
      a.tspace = ts;
      std::vector<u32> large;
      for (size_t i = 0; i < nb; i++)
        if ((u32) std::max(v.m[i], v.n[i]) > damar_box_trace_small())
          large.push_back((u32) i);
      a.nlarge = (u32) large.size();
      a.trace = (u16 *) TB.room(nb, sizeof(u16) * ((size_t) toff[nb] + 4));
      TB.mark(0);
      const BoxDev d = box_up(TB, v, (const long long *) toff);
      a.abpos = up(TB.abpos, v.abpos, nb);
      a.large = up(TB.large, large.data(), large.size());
      TB.mark(1);
      a.m = d.m;  a.n = d.n;  a.aoff = d.aoff;  a.boff = d.boff;  a.toff = d.off;  a.bases = d.bases;  a.diffs = d.diffs;  a.tlen = d.len;
      damar_launch_box_trace(&a, G_st);
      HIP_CHECK(hipGetLastError());
      TB.mark(2);
      box_down(d, nb, diffs, tlen.data());
      if (toff[nb] > 0)
        HIP_CHECK(hipMemcpyAsync(*trace, a.trace, sizeof(u16) * (size_t) toff[nb], hipMemcpyDeviceToHost, G_st));
      TB.mark(3);
      TB.sync_laps(0, 3);
    }
  const int64 fallback = box_rest(tlen, diffs, host, [&](size_t i)
    { return damar_trace_box(v.bases + v.aoff[i], v.m[i], v.bases + v.boff[i], v.n[i], v.abpos[i], ts, *trace + toff[i], &tlen[i]); });
  for (size_t i = 0; i < nb; i++)
    if (tlen[i] != toff[i + 1] - toff[i])
      { fprintf(stderr, "damar: trace boxes: box %zu came back with %d values for %lld\n", i, tlen[i], (long long) (toff[i + 1] - toff[i]));
        free(*trace);
        *trace = NULL;
        return 1;
      }
  TB.end(v.nbox, fallback, toff[nb]);
  return 0;
}
