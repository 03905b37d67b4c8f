/* stages/trace.hip -- the C-ABI of trace-point expansion: damar_trace_pts / _mid, Compute_Trace_PTS / _MID */
#include <algorithm>
#include <vector>

#include "stage.h"

/***** (f)4: trace-point expansion, align.c:5577-5692 Compute_Trace_PTS for batches of records *********/

static struct : DevStage         /* ms of the last damar_trace_pts: trace_waves kernel, layout..pack on the device, whole call, inside the
                                    batches (wall); cnt: records, segments, deferred segments, script values */
{ DBuf recs{*this}, pts{*this}, segs{*this}, count{*this}, dist{*this}, segoff{*this}, stage{*this}, vf{*this}, hf{*this}, over{*this},
       ctr{*this}, tlen{*this}, diffs{*this}, script{*this}, scan{*this}, bvf{*this}, bhf{*this}, mid{*this}, segs2{*this}, key{*this},
       val{*this}, key1{*this}, val1{*this}, sortw{*this};
} TR;

extern "C" void damar_trace_release(void) { TR.release(); }

extern "C" void damar_trace_last(double *ms, int64 *cnt) { TR.last(ms, cnt, 4); }

/* staging slots one record needs = sum over its segments of dmax + |M - N| (the script of a segment has at
   most D + |del| <= dmax + |del| values); also dmax and the segment count */
template <typename PT>
static void trace_record_shape(const Path *path, const PT *p, int tspace, int *dmax_out, int *nseg_out, int64 *slots_out)
{ const int tlen = path->tlen;
  int dmax = 0;
  for (int d = 0; d + 1 < tlen; d += 2)
    if ((int) p[d] > dmax) dmax = (int) p[d];
  const int nseg = tlen >= 2 ? tlen / 2 : 1;
  int ab = path->abpos, ae = (ab / tspace) * tspace, bb = path->bbpos;
  int64 slots = 0;
  for (int s = 0; s < nseg; s++)
    { int be;
      if (s + 1 < nseg) { ae += tspace; be = bb + (int) p[2 * s + 1]; }
      else              { ae = path->aepos; be = path->bepos; }
      const int del = (ae - ab) - (be - bb);
      slots += dmax + (del < 0 ? -del : del);
      ab = ae;
      bb = be;
    }
  *dmax_out = dmax;  *nseg_out = nseg;  *slots_out = slots;
}

/* One wave phase over `nwork` segments: the slot kernel, then the stripe kernel for what it deferred.
   kind 0 = scripts, 1 = mid points.  Returns the error flags, or ~0u after a message. */
static u32 trace_wave_phase(TraceArgs t, int mode, int kind, u32 nwork, u32 rows, u32 maxblocks, u32 *d_ctr,
                            u32 *d_key, u32 *d_val, hipEvent_t e1, hipEvent_t e2)
{ const u32 nblocks = std::min(maxblocks, (nwork + 63) / 64);
  /* work order: segments with equal difference counts side by side in a wavefront */
  static int ordered = -1;
  if (ordered < 0)
    { const char *e = getenv("DAMAR_TRACE_ORDER");
      ordered = e ? atoi(e) : 1;
    }
  const u32 *order = NULL;
  if (ordered)
    { u32 *k1 = (u32 *) TR.key1.need(sizeof(u32) * (size_t) nwork), *v1 = (u32 *) TR.val1.need(sizeof(u32) * (size_t) nwork);
      void *sw = TR.sortw.need(damar_sort_workspace_bytes(nwork));
      order = damar_radix_sort_u32(d_key, d_val, k1, v1, nwork, 8, sw, G_st) ? v1 : d_val;
      sort_check(sw);
    }
  const size_t area = damar_trace_slot_area_cells();
  t.vf = (short *) TR.vf.need((size_t) nblocks * damar_trace_slot_vf_bytes(mode, kind));
  t.hf = (signed char *) TR.hf.need((size_t) nblocks * area);
  t.cap = rows;
  t.list = order;  t.nwork = nwork;
  t.next = d_ctr + 4;
  HIP_CHECK(hipMemsetAsync(d_ctr, 0, 8, G_st));
  HIP_CHECK(hipMemsetAsync(d_ctr + 4, 0, 4, G_st));
  HIP_CHECK(hipEventRecord(e1, G_st));
  damar_launch_trace_waves_slots(&t, mode, kind, nblocks, G_st);
  HIP_CHECK(hipEventRecord(e2, G_st));
  u32 ctr[4];
  HIP_CHECK(hipMemcpyAsync(ctr, d_ctr, sizeof(ctr), hipMemcpyDeviceToHost, G_st));
  HIP_CHECK(hipStreamSynchronize(G_st));
  float wms = 0;
  HIP_CHECK(hipEventElapsedTime(&wms, e1, e2));
  TR.ms[0] += wms;
  if (ctr[0] > 0 && !(ctr[2] & DAMAR_TRACE_ERR_POINTS))
    { /* segments the slot kernel does not take: one lane each on stripes that hold dmax + 3 rows */
      const u32 need = ctr[1];
      size_t bthreads = ((size_t) ctr[0] + 63) / 64 * 64;
      const size_t budget = (size_t) 8 << 30;
      while (bthreads > 64 && bthreads * need * 3 > budget) bthreads /= 2;
      bthreads = (bthreads + 63) / 64 * 64;
      if (bthreads * need * 3 > ((size_t) 64 << 30))
        { fprintf(stderr, "damar: trace expansion: a segment needs %u wave cells, more than this build provides\n", need);
          return ~0u;
        }
      t.vf = (short *) TR.bvf.need(sizeof(short) * bthreads * need);
      t.hf = (signed char *) TR.bhf.need(bthreads * need);
      t.cap = need;
      t.list = t.over;  t.nwork = ctr[0];
      HIP_CHECK(hipMemsetAsync(d_ctr, 0, 8, G_st));
      HIP_CHECK(hipEventRecord(e1, G_st));
      damar_launch_trace_waves(&t, mode, kind, (u32) (bthreads / 64), G_st);
      HIP_CHECK(hipEventRecord(e2, G_st));
      u32 c2[4];
      HIP_CHECK(hipMemcpyAsync(c2, d_ctr, sizeof(c2), hipMemcpyDeviceToHost, G_st));
      HIP_CHECK(hipStreamSynchronize(G_st));
      HIP_CHECK(hipEventElapsedTime(&wms, e1, e2));
      TR.ms[0] += wms;
      TR.cnt[2] += ctr[0];
      if (c2[0] != 0)
        { fprintf(stderr, "damar: trace expansion: internal error, %u segments deferred twice\n", c2[0]);
          return ~0u;
        }
      ctr[2] |= c2[2];
    }
  if (ctr[2] & DAMAR_TRACE_ERR_POINTS)
    { fprintf(stderr, "damar: Trace point out of bounds (Compute_Trace), source DB likely incorrect\n");   /* align.c:5575 */
      return ~0u;
    }
  if (ctr[2] & DAMAR_TRACE_ERR_ALIGN)
    { fprintf(stderr, "damar: Bad alignment between trace points (Compute_Trace), source DB likely incorrect\n");   /* :4890 */
      return ~0u;
    }
  if (ctr[2] & DAMAR_TRACE_ERR_INTERNAL)
    { fprintf(stderr, "damar: trace expansion: internal error, staging bound of the mid-point pieces violated\n");
      return ~0u;
    }
  return ctr[2];
}

/* kind 0: Compute_Trace_PTS, the script of every trace-point segment.  kind 1: Compute_Trace_MID: a first
   wave phase finds the mid point of every segment, the pieces between successive mid points (one more
   than segments per record) are laid out anew and the script phase runs on those. */
static int trace_batch(const DevBlock *ad, const DevBlock *bd, int64 r0, int64 r1, int tbytes, int tspace, int mode, int kind,
                       const std::vector<TraceRecIn> &recs, const std::vector<u8> &pts,
                       u32 nsegs, u64 nslots, int64 *soff, int *diffs, int **script, int64 *nscript)
{ const u32 nrecs = (u32) (r1 - r0);
  static u32 rows = 0, maxblocks = 0;
  if (rows == 0)
    { const char *e = getenv("DAMAR_TRACE_ROWS");        /* test hook: fewer rows -> more segments deferred */
      rows = e ? (u32) atoi(e) : 64u;
      if (rows < 4) rows = 4;
      e = getenv("DAMAR_TRACE_BLOCKS");
      maxblocks = e ? (u32) atoi(e) : (u32) (G_prop.multiProcessorCount * 16);
      if (maxblocks < 1) maxblocks = 1;
    }
  const double h0 = now_ms();
  const u32 nwork = nsegs + (kind ? nrecs : 0u);             /* segments of the script phase */
  TraceRecIn *d_recs = (TraceRecIn *) TR.recs.need(sizeof(TraceRecIn) * (size_t) nrecs);
  void       *d_pts  = TR.pts.need(pts.size() + 64);
  TraceSeg   *d_segs = (TraceSeg *) TR.segs.need(sizeof(TraceSeg) * (size_t) nsegs);
  u32 *d_count  = (u32 *) TR.count.need(sizeof(u32) * (size_t) nwork);
  int *d_dist   = (int *) TR.dist.need(sizeof(int) * (size_t) nwork);
  u32 *d_segoff = (u32 *) TR.segoff.need(sizeof(u32) * (size_t) nwork);
  int *d_stage  = (int *) TR.stage.need(sizeof(int) * (size_t) (nslots + 16));
  u32 *d_over   = (u32 *) TR.over.need(sizeof(u32) * (size_t) nwork);
  u32 *d_ctr    = (u32 *) TR.ctr.need(256);                    /* [0] deferred, [1] cells needed, [2] error flags; u64 total at +64 */
  u32 *d_tlen   = (u32 *) TR.tlen.need(sizeof(u32) * (size_t) (nrecs + 1));
  int *d_diffs  = (int *) TR.diffs.need(sizeof(int) * (size_t) nrecs);
  void *d_scan  = TR.scan.need(damar_scan_workspace_bytes(nrecs));
  u32 *d_key    = (u32 *) TR.key.need(sizeof(u32) * (size_t) nwork);
  u32 *d_val    = (u32 *) TR.val.need(sizeof(u32) * (size_t) nwork);

  struct Events            /* destroyed on every return path */
  { hipEvent_t e[4];
    Events()  { for (int i = 0; i < 4; i++) HIP_CHECK(hipEventCreate(&e[i])); }
    ~Events() { for (int i = 0; i < 4; i++) (void) hipEventDestroy(e[i]); }
  } evs;
  hipEvent_t e0 = evs.e[0], e1 = evs.e[1], e2 = evs.e[2], e3 = evs.e[3];
  HIP_CHECK(hipMemcpyAsync(d_recs, recs.data(), sizeof(TraceRecIn) * (size_t) nrecs, hipMemcpyHostToDevice, G_st));
  if (!pts.empty())
    HIP_CHECK(hipMemcpyAsync(d_pts, pts.data(), pts.size(), hipMemcpyHostToDevice, G_st));
  HIP_CHECK(hipMemsetAsync(d_ctr, 0, 256, G_st));
  HIP_CHECK(hipEventRecord(e0, G_st));
  damar_launch_trace_layout(d_recs, nrecs, d_pts, tbytes, tspace, ad, bd, d_segs, d_key, d_val, d_ctr + 2, G_st);
  TraceArgs t;
  memset(&t, 0, sizeof(t));
  t.segs = d_segs;
  t.abases = ad->bases;  t.bbases = bd->bases;
  t.apk = ad->pk;  t.bpk = bd->pk;
  t.stage = d_stage;  t.count = d_count;  t.dist = d_dist;
  t.over = d_over;  t.over_cap = nwork;  t.nover = d_ctr;  t.need = d_ctr + 1;  t.err = d_ctr + 2;
  if (kind)
    { t.mid = (int *) TR.mid.need(sizeof(int) * 2 * (size_t) nsegs);
      if (trace_wave_phase(t, mode, 1, nsegs, rows, maxblocks, d_ctr, d_key, d_val, e1, e2) == ~0u)
        return 1;
      TraceSeg *d_segs2 = (TraceSeg *) TR.segs2.need(sizeof(TraceSeg) * (size_t) nwork);
      damar_launch_trace_mid_layout(d_recs, nrecs, d_segs, t.mid, ad, bd, d_segs2, d_key, d_val, d_ctr + 2, G_st);
      t.segs = d_segs = d_segs2;
    }
  if (trace_wave_phase(t, mode, 0, nwork, rows, maxblocks, d_ctr, d_key, d_val, e1, e2) == ~0u)
    return 1;
  damar_launch_trace_gather(d_recs, nrecs, kind, d_count, d_dist, d_segoff, d_tlen, d_diffs, G_st);
  u64 *d_tot = (u64 *) ((char *) d_ctr + 64);
  damar_exclusive_scan_u32(d_tlen, d_tlen, nrecs, d_scan, d_tot, G_st);
  u64 total = 0;
  HIP_CHECK(hipMemcpyAsync(&total, d_tot, sizeof(u64), hipMemcpyDeviceToHost, G_st));
  HIP_CHECK(hipStreamSynchronize(G_st));
  if (total >= 0xfffffff0ull)
    { fprintf(stderr, "damar: trace expansion: batch script exceeds 32-bit offsets\n");
      return 1;
    }
  int *d_script = (int *) TR.script.need(sizeof(int) * (size_t) (total + 16));
  damar_launch_trace_pack(d_segs, nwork, d_count, d_segoff, d_tlen, d_stage, d_script, G_st);
  HIP_CHECK(hipEventRecord(e3, G_st));
  std::vector<u32> hoff(nrecs);
  const size_t base = (size_t) *nscript;
  { int *grown = (int *) realloc(*script, sizeof(int) * (base + (size_t) total + 1));
    if (grown == NULL)
      { fprintf(stderr, "damar: out of memory (edit scripts)\n");
        return 1;
      }
    *script = grown;
    *nscript = (int64) (base + (size_t) total);
  }
  HIP_CHECK(hipMemcpyAsync(hoff.data(), d_tlen, sizeof(u32) * (size_t) nrecs, hipMemcpyDeviceToHost, G_st));
  HIP_CHECK(hipMemcpyAsync(diffs + r0, d_diffs, sizeof(int) * (size_t) nrecs, hipMemcpyDeviceToHost, G_st));
  if (total > 0)
    HIP_CHECK(hipMemcpyAsync(*script + base, d_script, sizeof(int) * (size_t) total, hipMemcpyDeviceToHost, G_st));
  HIP_CHECK(hipStreamSynchronize(G_st));
  float dms = 0;
  HIP_CHECK(hipEventElapsedTime(&dms, e0, e3));
  TR.ms[1] += dms;
  for (u32 i = 0; i < nrecs; i++)
    soff[r0 + i] = (int64) base + hoff[i];
  soff[r1] = (int64) base + (int64) total;
  TR.ms[3] += now_ms() - h0;
  TR.cnt[0] += nrecs;  TR.cnt[1] += nwork;  TR.cnt[3] += (int64) total;
  return 0;
}

/* ovls[i].path.trace = the record's trace points as read from the .las (tbytes 1 or 2 per value);
 * aread / bread are DB read ids, afirst / bfirst the ids of the blocks' first reads.  same != 0: A and B of
 * every record are one buffer (align.c:4933-4951; LAshow never is).  On return *script_out is a malloc'ed
 * array holding all edit scripts, record i at [soff[i], soff[i+1]), diffs[i] its summed distance. */
static int trace_expand(damar_dev_block *ablk, int afirst, damar_dev_block *bblk, int bfirst,
                        const Overlap *ovls, int64 novl, int tbytes, int tspace, int mode, int same, int kind,
                        int64 *soff, int *diffs, int **script_out)
{ ensure_init();
  const double t0 = now_ms();
  for (int i = 0; i < 4; i++) { TR.ms[i] = 0;  TR.cnt[i] = 0; }
  int  *script = NULL;
  int64 nscript = 0;
  *script_out = NULL;
  std::vector<TraceRecIn> recs;
  std::vector<u8> pts;
  u32 max_segs = 1u << 24;                                   /* per batch: segments, staging slots */
  const u64 max_slots = 1ull << 30;
  { const char *e = getenv("DAMAR_TRACE_MAXSEGS");           /* test hook: many small batches */
    if (e && atoi(e) > 0) max_segs = (u32) atoi(e);
  }
  int64 r0 = 0;
  u32   nsegs = 0;
  u64   nslots = 0;
  soff[0] = 0;
  for (int64 i = 0; i <= novl; i++)
    { int dmax = 0, nseg = 0;
      int64 slots = 0;
      if (i < novl)
        { const Overlap *o = ovls + i;
          const int64 ar = (int64) o->aread - afirst, br = (int64) o->bread - bfirst;
          if (ar < 0 || ar >= ablk->nreads || br < 0 || br >= bblk->nreads || o->path.tlen < 0 || (o->path.tlen & 1))
            { fprintf(stderr, "damar: trace expansion: record %lld does not belong to the two blocks\n", (long long) i);
              free(script);
              return 1;
            }
          if (tbytes == 1) trace_record_shape(&o->path, (const uint8 *) o->path.trace, tspace, &dmax, &nseg, &slots);
          else             trace_record_shape(&o->path, (const uint16 *) o->path.trace, tspace, &dmax, &nseg, &slots);
          if (kind)            /* pieces between mid points: |del'| <= |del| of the two segments + 2 (dmax + |del|) drift */
            slots = 3 * slots + 3 * (int64) dmax;
        }
      if (i == novl || nsegs + (u32) nseg > max_segs || nslots + (u64) slots > max_slots)
        { if (i > r0)
            { if (trace_batch(&ablk->d, &bblk->d, r0, i, tbytes, tspace, mode, kind, recs, pts,
                              nsegs, nslots, soff, diffs, &script, &nscript))
                { free(script);
                  return 1;
                }
            }
          recs.clear();  pts.clear();
          r0 = i;  nsegs = 0;  nslots = 0;
          if (i == novl) break;
          if ((u64) slots > max_slots || (u32) nseg > max_segs)
            { fprintf(stderr, "damar: trace expansion: record %lld is larger than a batch\n", (long long) i);
              free(script);
              return 1;
            }
        }
      const Overlap *o = ovls + i;
      TraceRecIn in;
      in.aread = (u32) (o->aread - afirst);  in.bread = (u32) (o->bread - bfirst);
      in.flags = (o->flags & COMP_FLAG ? 1u : 0u) | (same ? 2u : 0u);
      in.abpos = o->path.abpos;  in.bbpos = o->path.bbpos;  in.aepos = o->path.aepos;  in.bepos = o->path.bepos;
      in.poff = (u32) (pts.size() / (size_t) tbytes);
      in.tlen = o->path.tlen;
      in.seg0 = nsegs;
      in.stage0 = (u32) nslots;
      in.dmax = dmax;
      in.slots = (u32) slots;
      recs.push_back(in);
      const u8 *src = (const u8 *) o->path.trace;
      pts.insert(pts.end(), src, src + (size_t) o->path.tlen * (size_t) tbytes);
      nsegs += (u32) nseg;
      nslots += (u64) slots;
    }
  if (script == NULL)
    script = (int *) malloc(sizeof(int));
  *script_out = script;
  TR.ms[2] = now_ms() - t0;
  return 0;
}

extern "C" int damar_trace_pts(damar_dev_block *ablk, int afirst, damar_dev_block *bblk, int bfirst,
                               const Overlap *ovls, int64 novl, int tbytes, int tspace, int mode, int same,
                               int64 *soff, int *diffs, int **script_out)
{ return trace_expand(ablk, afirst, bblk, bfirst, ovls, novl, tbytes, tspace, mode, same, 0, soff, diffs, script_out);
}

/* the same arguments, Compute_Trace_MID (align.c:5694-5830): the script between the segments' mid points */
extern "C" int damar_trace_mid(damar_dev_block *ablk, int afirst, damar_dev_block *bblk, int bfirst,
                               const Overlap *ovls, int64 novl, int tbytes, int tspace, int mode, int same,
                               int64 *soff, int *diffs, int **script_out)
{ return trace_expand(ablk, afirst, bblk, bfirst, ovls, novl, tbytes, tspace, mode, same, 1, soff, diffs, script_out);
}

/* align.c:5577-5692 for one record, through the batch path (the two sequences travel to HBM per call: this
 * entry point is for callers that need the reference's API; LAshow-like loops over a .las belong on
 * damar_trace_pts).  As in the reference, align->path->trace holds 16-bit trace-point pairs on entry (after
 * Decompress_TraceTo16), bseq is already complemented where the record says so, and on return path->trace
 * points to the edit script inside `work`, tlen and diffs are updated.  Returns 0, or 1 after the
 * reference's message where the reference's EXIT(1) paths are. */
static int compute_trace(Alignment *align, Work_Data *work, int trace_spacing, int mode, int kind)
{ ensure_init();
  WorkData *w = (WorkData *) work;
  HITS_DB   db[2];
  HITS_READ rd[2][2];
  std::vector<char> buf[2];
  const char *seq[2] = { align->aseq, align->bseq };
  const int   len[2] = { align->alen, align->blen };
  const int   same = (align->aseq == align->bseq);
  for (int i = 0; i < 2; i++)
    { memset(&db[i], 0, sizeof(HITS_DB));
      memset(rd[i], 0, sizeof(rd[i]));
      buf[i].assign((size_t) len[i] + 2, 4);
      memcpy(buf[i].data() + 1, seq[i], (size_t) len[i]);
      rd[i][0].rlen = len[i];  rd[i][0].boff = 0;  rd[i][1].boff = len[i] + 1;
      db[i].nreads = db[i].ureads = 1;  db[i].maxlen = len[i];  db[i].totlen = len[i];
      db[i].bases = buf[i].data() + 1;  db[i].reads = rd[i];
    }
  damar_dev_block *ab = damar_block_upload(&db[0]);
  damar_dev_block *bb = same ? ab : damar_block_upload(&db[1]);
  Overlap o;
  memset(&o, 0, sizeof(o));
  o.path = *align->path;
  int64 soff[2];
  int   diffs = 0, *script = NULL;
  const int rc = trace_expand(ab, 0, bb, 0, &o, 1, 2, trace_spacing, mode, same, kind, soff, &diffs, &script);
  damar_block_free(ab);
  if (!same)
    damar_block_free(bb);
  if (rc)
    return 1;
  w->script.assign(script, script + soff[1]);
  free(script);
  align->path->trace = w->script.data();
  align->path->tlen  = (int) soff[1];
  align->path->diffs = diffs;
  return 0;
}

extern "C" int Compute_Trace_PTS(Alignment *align, Work_Data *work, int trace_spacing, int mode)   /* align.c:5577 */
{ return compute_trace(align, work, trace_spacing, mode, 0);
}

extern "C" int Compute_Trace_MID(Alignment *align, Work_Data *work, int trace_spacing, int mode)   /* align.c:5694 */
{ return compute_trace(align, work, trace_spacing, mode, 1);
}
