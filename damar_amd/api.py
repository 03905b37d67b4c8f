"""ctypes mirror of the overlap path's C interface.

Same names and argument meaning as the reference's ``dalign/filter.h:64-70``,
``dalign/align.h:223-259, 416-432`` and the subset of ``db/DB.h`` that
``dalign/daligner.c`` uses; see include/damar_*.h for the citations.  Every call goes
straight into libdamar_hip.so -- nothing is computed in Python.
"""
import ctypes as C
import os

from .lib import load, bin_path

c_int64 = C.c_int64


class HITS_READ(C.Structure):          # db/DB.h:319-326
    _fields_ = [("rlen", C.c_int), ("boff", c_int64), ("coff", c_int64), ("flags", C.c_int)]


class HITS_DB(C.Structure):            # db/DB.h:361-389
    _fields_ = [("ureads", C.c_int), ("freq", C.c_float * 4), ("maxlen", C.c_int),
                ("totlen", c_int64), ("nreads", C.c_int), ("part", C.c_int), ("ufirst", C.c_int),
                ("path", C.c_char_p), ("loaded", C.c_int), ("bases", C.c_void_p),
                ("reads", C.POINTER(HITS_READ)), ("tracks", C.c_void_p)]


class SimParams(C.Structure):          # include/damar_db.h damar_sim_params
    _fields_ = [("genome_mbp", C.c_double), ("coverage", C.c_double), ("bias", C.c_double),
                ("seed", C.c_int), ("rmean", C.c_int), ("rsdev", C.c_int), ("rshort", C.c_int),
                ("erate", C.c_double), ("block_mbp", C.c_int), ("min_len", C.c_int),
                ("tandem_frac", C.c_double), ("max_blocks", C.c_int)]


T_NAMES = ["tuples", "ksort", "table", "merge", "ssort", "work", "report", "d2h", "tail"]

class MatchJob(C.Structure):           # include/damar_hip.h damar_match_job
    _fields_ = [("ablock", C.POINTER(HITS_DB)), ("bblock", C.POINTER(HITS_DB)),
                ("aidx", C.c_void_p), ("bidx", C.c_void_p),
                ("self_", C.c_int), ("comp", C.c_int),
                ("spec", C.c_void_p), ("counts", c_int64 * 3)]


_PI = C.POINTER(C.c_int)


class PileBatch(C.Structure):          # include/damar_hip.h damar_pile_batch
    _fields_ = [("npiles", c_int64), ("nrec", c_int64), ("pile_off", C.POINTER(c_int64)), ("pile_aread", _PI),
                ("abpos", _PI), ("aepos", _PI), ("bbpos", _PI), ("bepos", _PI), ("bread", _PI), ("flags", _PI),
                ("read_len", _PI), ("read_flags", _PI), ("nreads", C.c_int), ("maxlen", C.c_int)]


class RepeatParams(C.Structure):       # damar_repeat_params
    _fields_ = [("xcov_enter", C.c_double), ("xcov_leave", C.c_double), ("cov", C.c_int), ("merge_dist", C.c_int),
                ("min_aln_len", C.c_int), ("inc_identity", C.c_int), ("inccov", C.c_int), ("max_cov", C.c_int)]


class PileTrack(C.Structure):          # damar_pile_track
    _fields_ = [("count", _PI), ("data", _PI), ("ndata", c_int64), ("merged", c_int64), ("repeat_bases", c_int64)]


class TraceBatch(C.Structure):         # include/damar_hip.h damar_trace_batch
    _fields_ = [("p", PileBatch), ("trace", C.POINTER(C.c_ubyte)), ("trace_off", C.POINTER(c_int64)), ("tlen", _PI),
                ("trace_bytes", c_int64), ("tbytes", C.c_int), ("tspace", C.c_int)]


class QParams(C.Structure):            # damar_q_params
    _fields_ = [("segmin", C.c_int), ("segmax", C.c_int), ("ccs", C.c_int)]


class QResult(C.Structure):            # host/damar_host.h damar_q_result
    _fields_ = [("q_anno", C.POINTER(C.c_uint64)), ("trim_anno", C.POINTER(C.c_uint64)), ("q_data", _PI), ("trim_data", _PI),
                ("nq", c_int64), ("ntrim", c_int64)]


class DbInfo(C.Structure):             # host/damar_host.h damar_dbinfo
    _fields_ = [("nreads", C.c_int), ("maxlen", C.c_int), ("read_len", _PI), ("read_flags", _PI), ("nblocks", C.c_int),
                ("block_first", _PI), ("path", C.c_char_p)]


class RepeatResult(C.Structure):       # damar_repeat_result
    _fields_ = [("histo", C.POINTER(c_int64)), ("cov_max", C.c_int), ("cov_bases", c_int64), ("cov_inactive", c_int64),
                ("avg_rlen", C.c_int), ("cov", C.c_int), ("anno", C.POINTER(C.c_uint64)), ("data", _PI), ("ndata", c_int64),
                ("merged", c_int64), ("bases_total", c_int64), ("bases_repeat", c_int64)]


class BoxBatch(C.Structure):           # include/damar_hip.h damar_box_batch
    _fields_ = [("nbox", c_int64), ("m", _PI), ("n", _PI), ("aoff", C.POINTER(c_int64)), ("boff", C.POINTER(c_int64)),
                ("bases", C.c_void_p), ("nbases", c_int64)]


class TBoxBatch(C.Structure):          # include/damar_hip.h damar_tbox_batch
    _fields_ = [("nbox", c_int64), ("m", _PI), ("n", _PI), ("abpos", _PI), ("aoff", C.POINTER(c_int64)), ("boff", C.POINTER(c_int64)),
                ("bases", C.c_void_p), ("nbases", c_int64), ("tspace", C.c_int)]


class StitchParams(C.Structure):       # host/damar_host.h damar_stitch_params
    _fields_ = [("fuzz", C.c_int), ("purge", C.c_int), ("anchor", C.c_int), ("merge", C.c_int), ("min_len", C.c_int),
                ("min_merge", C.c_int), ("gap_diff", C.c_double), ("lc_track", C.c_char_p), ("rep_track", C.c_char_p)]


class StitchStats(C.Structure):        # host/damar_host.h damar_stitch_stats
    _fields_ = [("novl", c_int64), ("written", c_int64), ("discarded", c_int64), ("stitched", c_int64), ("stitched_lc", c_int64),
                ("candidates", c_int64), ("no_box", c_int64), ("widened", c_int64), ("boxes", c_int64), ("box_a", c_int64), ("box_b", c_int64), ("refused", c_int64),
                ("rounds", c_int64), ("round_boxes", c_int64 * 16)]


class TrimStats(C.Structure):          # host/damar_host.h damar_trim_stats
    _fields_ = [("novl", c_int64), ("ntrimmed", c_int64), ("novl_bases", c_int64), ("ntrim_bases", c_int64),
                ("written", c_int64), ("discarded", c_int64), ("boxes", c_int64), ("box_a", c_int64), ("box_b", c_int64)]


class GapParams(C.Structure):          # include/damar_hip.h damar_gap_params
    _fields_ = [("stitch", C.c_int), ("ex_anno", C.POINTER(C.c_uint64)), ("ex_data", _PI), ("ex_ndata", c_int64), ("purge", C.c_int),
                ("trim_track", C.c_char_p)]


class GapEvents(C.Structure):          # include/damar_hip.h damar_gap_events
    _fields_ = [("count", _PI), ("ev", _PI), ("nev", c_int64), ("contained", c_int64), ("breaks", c_int64), ("dropped", c_int64)]


class GapStats(C.Structure):           # host/damar_host.h damar_gap_stats
    _fields_ = [("novl", c_int64), ("written", c_int64), ("discarded", c_int64), ("contained", c_int64), ("breaks", c_int64),
                ("dropped", c_int64), ("piles", c_int64), ("host_piles", c_int64), ("events", c_int64), ("trim", TrimStats)]


class HomogParams(C.Structure):        # host/damar_host.h damar_homog_params
    _fields_ = [("merge", C.c_int), ("ends", C.c_int), ("res", C.c_int), ("iv_anno", C.POINTER(C.c_uint64)), ("iv_data", _PI),
                ("iv_ndata", c_int64), ("trim_anno", C.POINTER(C.c_uint64)), ("trim_data", _PI)]


class HomogResult(C.Structure):        # host/damar_host.h damar_homog_result
    _fields_ = [("anno", C.POINTER(C.c_uint64)), ("data", _PI), ("ndata", c_int64), ("tagged", c_int64)]


_proto_done = False


def _lib():
    global _proto_done
    L = load()
    if not _proto_done:
        L.damar_read_block.argtypes = [C.c_char_p, C.POINTER(HITS_DB)]
        L.damar_read_block.restype = C.c_int
        L.damar_close_block.argtypes = [C.POINTER(HITS_DB)]
        L.damar_complement_block.argtypes = [C.POINTER(HITS_DB), C.c_int]
        L.damar_complement_block.restype = C.POINTER(HITS_DB)
        L.damar_sim_defaults.argtypes = [C.POINTER(SimParams)]
        L.damar_sim_write_db.argtypes = [C.POINTER(SimParams), C.c_char_p, C.c_char_p]
        L.damar_sim_write_db.restype = C.c_int
        L.damar_get_dir.argtypes = [C.c_int, C.c_int]
        L.damar_get_dir.restype = C.c_void_p
        L.Set_Filter_Params.argtypes = [C.c_int] * 5
        L.Set_Filter_Params.restype = C.c_int
        L.Sort_Kmers.argtypes = [C.POINTER(HITS_DB), C.POINTER(C.c_int)]
        L.Sort_Kmers.restype = C.c_void_p
        L.Match_Filter.argtypes = [C.c_char_p, C.POINTER(HITS_DB), C.c_char_p, C.POINTER(HITS_DB),
                                   C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.New_Align_Spec.argtypes = [C.c_double, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_int,
                                     C.c_int, C.c_int, C.c_int]
        L.New_Align_Spec.restype = C.c_void_p
        L.Free_Align_Spec.argtypes = [C.c_void_p]
        L.Write_Overlap_Buffer.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]
        L.Reset_Overlap_Buffer.argtypes = [C.c_void_p]
        L.damar_hip_init.argtypes = [C.c_int]
        L.damar_hip_init.restype = C.c_int
        L.damar_hip_device_name.restype = C.c_char_p
        L.damar_block_upload.argtypes = [C.POINTER(HITS_DB)]
        L.damar_block_upload.restype = C.c_void_p
        L.damar_block_free.argtypes = [C.c_void_p]
        L.damar_load_masks.argtypes = [C.POINTER(HITS_DB), C.POINTER(C.c_char_p), C.c_int]
        L.damar_load_masks.restype = C.c_int
        L.damar_async_d2h_ms.restype = C.c_double
        L.damar_index_build.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.damar_index_build.restype = C.c_void_p
        L.damar_index_free.argtypes = [C.c_void_p]
        L.damar_index_bytes.argtypes = [C.c_void_p]
        L.damar_index_bytes.restype = C.c_uint64
        L.damar_complement_copy.argtypes = [C.POINTER(HITS_DB), C.POINTER(HITS_DB)]
        L.damar_free_complement.argtypes = [C.POINTER(HITS_DB)]
        L.damar_async_drain.argtypes = []
        L.damar_set_bread_range.argtypes = [C.c_int, C.c_int]
        L.damar_index_download.argtypes = [C.c_void_p, C.c_void_p]
        L.damar_match.argtypes = [C.POINTER(HITS_DB), C.POINTER(HITS_DB), C.c_void_p, C.c_void_p,
                                  C.c_int, C.c_int, C.c_void_p, C.POINTER(c_int64)]
        L.damar_match_batch.argtypes = [C.POINTER(MatchJob), C.c_int]
        L.damar_set_async.argtypes = [C.c_int]
        L.damar_async_totals.argtypes = [C.POINTER(c_int64), C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.damar_async_counts.argtypes = [C.POINTER(c_int64), C.POINTER(C.c_double), C.POINTER(c_int64)]
        L.damar_wave_totals.argtypes = [C.POINTER(c_int64)] * 3
        L.damar_write_overlaps.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]
        L.damar_tandem_set_params.argtypes = [C.c_int] * 4
        L.damar_tandem_set_params.restype = C.c_int
        L.Match_Self.argtypes = [C.c_char_p, C.POINTER(HITS_DB), C.c_void_p]
        L.damar_match_self.argtypes = [C.POINTER(HITS_DB), C.c_void_p, C.c_void_p, C.POINTER(c_int64)]
        L.damar_last_seeds.argtypes = [C.c_void_p, c_int64]
        L.damar_last_seeds.restype = c_int64
        L.damar_order_runs_test.argtypes = [C.c_void_p, c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int]
        L.damar_order_runs_test.restype = C.c_int
        L.damar_pair_work_test.argtypes = [C.c_void_p, C.c_void_p, c_int64, c_int64, c_int64] + [C.c_int] * 8 + \
                                          [C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, c_int64, C.POINTER(c_int64)]
        L.damar_pair_work_test.restype = c_int64
        L.damar_local_alignment_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                                  C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int),
                                                  C.POINTER(c_int64), C.POINTER(C.c_uint16), c_int64]
        L.damar_local_alignment_batch.restype = C.c_int
        L.damar_local_alignment_batch_opts.argtypes = L.damar_local_alignment_batch.argtypes + [C.c_int, C.POINTER(C.c_int),
                                                                                               C.POINTER(C.c_int)]
        L.damar_local_alignment_batch_opts.restype = C.c_int
        L.damar_last_timings.argtypes = [C.POINTER(C.c_double)]
        L.damar_last_counters.argtypes = [C.POINTER(c_int64)]
        L.damar_last_slabs.argtypes = [C.POINTER(C.c_int), C.POINTER(c_int64), C.c_int]
        L.damar_last_slabs.restype = C.c_int
        L.damar_slab_totals.argtypes = [C.POINTER(c_int64)]
        L.damar_slab_cut.argtypes = [C.POINTER(C.c_uint64), C.c_int, C.c_uint64, C.POINTER(C.c_int), C.POINTER(c_int64), C.c_int]
        L.damar_slab_cut.restype = C.c_int
        L.damar_bench_sort_u32.argtypes = [C.c_uint32, C.c_int, C.c_int, C.c_uint32]
        L.damar_bench_sort_u32.restype = C.c_double
        L.damar_set_check.argtypes = [C.c_int]
        L.damar_check_totals.argtypes = [C.POINTER(c_int64)]
        L.damar_check_note_blocks.argtypes = [C.c_void_p, C.POINTER(HITS_DB), C.POINTER(HITS_DB)]
        L.damar_pile_coverage.argtypes = [C.POINTER(PileBatch), C.POINTER(RepeatParams), C.POINTER(c_int64), C.POINTER(c_int64), C.POINTER(c_int64)]
        L.damar_pile_repeats.argtypes = [C.POINTER(PileBatch), C.POINTER(RepeatParams), C.POINTER(PileTrack)]
        L.damar_pile_tandem.argtypes = [C.POINTER(PileBatch), C.c_int, C.POINTER(PileTrack)]
        L.damar_pile_last.argtypes = [C.POINTER(C.c_double), C.POINTER(c_int64)]
        L.damar_dbinfo_open.argtypes = [C.c_char_p, C.POINTER(DbInfo)]
        L.damar_dbinfo_close.argtypes = [C.POINTER(DbInfo)]
        L.damar_repeat_track.argtypes = [C.POINTER(DbInfo), C.c_char_p, C.POINTER(RepeatParams), C.c_int, C.c_int, C.POINTER(RepeatResult)]
        L.damar_repeat_result_free.argtypes = [C.POINTER(RepeatResult)]
        L.damar_tan_track.argtypes = [C.POINTER(DbInfo), C.c_char_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.POINTER(c_int64)),
                                      C.POINTER(C.POINTER(C.c_int)), C.POINTER(c_int64), C.POINTER(c_int64)]
        L.damar_piles_open.argtypes = [C.c_char_p, c_int64]
        L.damar_piles_open.restype = C.c_void_p
        L.damar_piles_next.argtypes = [C.c_void_p, C.POINTER(PileBatch)]
        L.damar_piles_close.argtypes = [C.c_void_p]
        L.damar_pile_quality.argtypes = [C.POINTER(TraceBatch), C.POINTER(QParams), _PI, C.POINTER(c_int64)]
        L.damar_q_last.argtypes = [C.POINTER(C.c_double), C.POINTER(c_int64)]
        L.damar_q_track.argtypes = [C.POINTER(DbInfo), C.c_char_p, C.POINTER(QParams), C.c_int, C.c_int, C.POINTER(QResult)]
        L.damar_trim_update.argtypes = [C.POINTER(DbInfo), C.c_char_p, C.POINTER(C.c_uint64), _PI, c_int64, C.POINTER(C.c_uint64), _PI,
                                        C.c_int, C.c_int, C.c_int, C.POINTER(QResult)]
        L.damar_q_result_free.argtypes = [C.POINTER(QResult)]
        L.damar_align_boxes.argtypes = [C.POINTER(BoxBatch), _PI, C.POINTER(c_int64), C.POINTER(_PI)]
        L.damar_box_grid.restype = C.c_uint
        L.damar_align_reads.argtypes = [C.POINTER(BoxBatch), _PI, C.POINTER(c_int64), C.POINTER(_PI)]
        L.damar_read_grid.restype = C.c_uint
        L.damar_box_last.argtypes = [C.POINTER(C.c_double), C.POINTER(c_int64)]
        L.damar_trace_boxes.argtypes = [C.POINTER(TBoxBatch), _PI, C.POINTER(c_int64), C.POINTER(C.POINTER(C.c_uint16))]
        L.damar_tbox_grid.restype = C.c_uint
        L.damar_tbox_last.argtypes = [C.POINTER(C.c_double), C.POINTER(c_int64)]
        L.damar_stitch_las.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(StitchParams), C.POINTER(StitchStats)]
        L.damar_trim_las.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(TrimStats)]
        u64p = C.POINTER(C.c_uint64)
        L.damar_homog_open.argtypes = [_PI, C.c_int, C.c_int]
        L.damar_homog_open.restype = C.c_void_p
        L.damar_homog_seed.argtypes = [C.c_void_p, u64p, _PI, c_int64]
        L.damar_homog_add.argtypes = [C.c_void_p, C.POINTER(TraceBatch), u64p, _PI, c_int64, C.c_int, _PI]
        L.damar_homog_finish.argtypes = [C.c_void_p, u64p, C.POINTER(_PI), C.POINTER(c_int64), C.POINTER(c_int64)]
        L.damar_homog_close.argtypes = [C.c_void_p]
        L.damar_homog_last.argtypes = [C.POINTER(C.c_double), C.POINTER(c_int64)]
        L.damar_homogenize_track.argtypes = [C.POINTER(DbInfo), C.c_char_p, C.POINTER(HomogParams), C.POINTER(HomogResult)]
        L.damar_homog_result_free.argtypes = [C.POINTER(HomogResult)]
        L.damar_track_read_a2.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(u64p), C.POINTER(_PI), C.POINTER(c_int64)]
        L.damar_track_read_any.argtypes = [C.POINTER(DbInfo), C.c_char_p, C.POINTER(u64p), C.POINTER(_PI), C.POINTER(c_int64)]
        L.damar_pile_gaps.argtypes = [C.POINTER(PileBatch), C.POINTER(GapParams), _PI, C.POINTER(GapEvents)]
        L.damar_gap_limits.argtypes = [_PI, _PI]
        L.damar_gap_last.argtypes = [C.POINTER(C.c_double), C.POINTER(c_int64)]
        L.damar_gap_las.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(GapParams), C.POINTER(GapStats)]
        _proto_done = True
    return L


def set_globals(verbose=0, minover=2000, symmetric=1, identity=0, hgap_min=0, biased=0):
    """The globals daligner.c:131-140 shares with filter.c (MINOVER is already doubled)."""
    L = _lib()
    C.c_int.in_dll(L, "VERBOSE").value = verbose
    C.c_int.in_dll(L, "MINOVER").value = minover
    C.c_int.in_dll(L, "SYMMETRIC").value = symmetric
    C.c_int.in_dll(L, "IDENTITY").value = identity
    C.c_int.in_dll(L, "HGAP_MIN").value = hgap_min
    C.c_int.in_dll(L, "BIASED").value = biased


def sim_write_db(directory, root, genome_mbp, coverage=20., seed=1, erate=.15, block_mbp=200,
                 rmean=10000, rsdev=2000, rshort=4000, tandem_frac=0., max_blocks=0):
    """db/simulator.c | FA2db | DBsplit equivalent (include/damar_db.h); returns #blocks."""
    L = _lib()
    p = SimParams()
    L.damar_sim_defaults(C.byref(p))
    p.genome_mbp, p.coverage, p.seed, p.erate, p.block_mbp = genome_mbp, coverage, seed, erate, block_mbp
    p.rmean, p.rsdev, p.rshort = rmean, rsdev, rshort
    p.tandem_frac = tandem_frac
    p.max_blocks = max_blocks
    nb = L.damar_sim_write_db(C.byref(p), directory.encode(), root.encode())
    if nb < 0:
        raise RuntimeError("damar_sim_write_db failed")
    return nb


def read_block(name):
    L = _lib()
    db = HITS_DB()
    if L.damar_read_block(name.encode(), C.byref(db)) != 0:
        raise RuntimeError("cannot read block %s" % name)
    return db


def get_dir(run, block):
    L = _lib()
    p = L.damar_get_dir(run, block)
    return C.string_at(p).decode()


def timings():
    L = _lib()
    a = (C.c_double * len(T_NAMES))()
    L.damar_last_timings(a)
    return dict(zip(T_NAMES, list(a)))


def counters():
    L = _lib()
    a = (c_int64 * 8)()
    L.damar_last_counters(a)
    return list(a)


def order_runs(keys, ppos, dbits, work):
    """The ordering step of the seed sort over the read pair only, alone (test hook damar_order_runs_test): a copy of the
    uint64 array `keys` with the runs whose heads `work` lists in order of their A positions."""
    import numpy as np
    L = _lib()
    k = np.ascontiguousarray(keys, dtype=np.uint64).copy()
    w = np.ascontiguousarray(work, dtype=np.uint32)
    if L.damar_order_runs_test(k.ctypes.data, len(k), ppos, dbits, w.ctypes.data, len(w)) != 0:
        raise RuntimeError("damar_order_runs_test failed")
    return k


def pair_work(keys, vals, off, gtotal, ppos, dbits, abits, minhit, nshift, binshift, kmer, hitmin, b_lo, b_hi, mode):
    """The work list of a comparison alone (test hook damar_pair_work_test) over the packed seeds `keys` (uint64; `vals` =
    their diagonals as uint32 where dbits == 0, None otherwise), the stretch [off, off + len(keys)) of a list of gtotal
    seeds.  mode 0: one pass over sorted seeds, 1: one pass over seeds sorted by read pair only, 2: heads, then screen.
    Returns (work, flag): the ascending seed indices of the work items (uint32) and, as an int64 array of one entry, whether
    mode 1 met a kept run too long to order."""
    import numpy as np
    L = _lib()
    k = np.ascontiguousarray(keys, dtype=np.uint64)
    v = None if vals is None else np.ascontiguousarray(vals, dtype=np.uint32)
    if v is not None and len(v) != len(k):
        raise ValueError("vals and keys differ in length")
    flag = c_int64(0)
    work = np.zeros(len(k) // max(1, minhit) + 1, dtype=np.uint32)          # (a work item heads a run of at least minhit seeds)
    n = L.damar_pair_work_test(k.ctypes.data if len(k) else None, None if v is None else v.ctypes.data, len(k), off, gtotal,
                               ppos, dbits, abits, minhit, nshift, binshift, kmer, hitmin, b_lo, b_hi, mode,
                               work.ctypes.data, len(work), C.byref(flag))
    if n < 0:
        raise ValueError("damar_pair_work_test refused its arguments")
    if n > len(work):
        raise RuntimeError("damar_pair_work_test: %d work items over %d seeds with minhit %d" % (n, len(k), minhit))
    return work[:n].copy(), np.array([flag.value], dtype=np.int64)


def last_slabs():
    """Slab table of the last damar_match: (b_lo[0 .. n], hits[0 .. n-1]); n = 1 for a comparison that was not split."""
    L = _lib()
    n = L.damar_last_slabs(None, None, 0)
    b = (C.c_int * (n + 1))()
    h = (c_int64 * n)()
    L.damar_last_slabs(b, h, n)
    return list(b), list(h)


def slab_totals():
    """(seed stages run, comparisons split) of the last damar_match / damar_match_batch."""
    L = _lib()
    a = (c_int64 * 2)()
    L.damar_slab_totals(a)
    return a[0], a[1]


def slab_cut(hits, cap):
    """The greedy cut of B reads into slabs (host arithmetic): (b_lo, sums), or the library's error code (< 0: read
    -(code + 1) alone exceeds cap)."""
    L = _lib()
    n = len(hits)
    h = (C.c_uint64 * max(n, 1))(*[int(x) for x in hits])
    b = (C.c_int * (n + 2))()
    s = (c_int64 * (n + 1))()
    got = L.damar_slab_cut(h, n, int(cap), b, s, n + 1)
    if got <= 0:
        return got
    return list(b[:got + 1]), list(s[:got])


def set_check(on):
    """daligner -C for the in-process run: every .las file is checked by the thread that writes it (include/damar_hip.h)."""
    _lib().damar_set_check(1 if on else 0)


def check_totals():
    """(files checked, records checked, violations, files checked but discarded by DAMAR_LAS_KEEP) since the process started;
    read it after the writers have drained (driver.Plan.finish)."""
    a = (c_int64 * 4)()
    _lib().damar_check_totals(a)
    return tuple(a)


def las_check(db, las, ptp=True, sort=True, dupes=True, strict=False, ignore_discarded=False):
    """bin/LAcheck on one file: -> (exit status, its stderr lines).  db: the WHOLE database (records carry its read numbers);
    ptp / sort / dupes / ignore_discarded are the reference tool's -p -s -d -i, strict is -x."""
    import subprocess
    exe = bin_path("LAcheck")
    if not os.path.exists(exe):
        raise RuntimeError("%s not built" % exe)
    opts = [o for o, on in (("-p", ptp), ("-s", sort), ("-d", dupes), ("-i", ignore_discarded), ("-x", strict)) if on]
    r = subprocess.run([exe] + opts + [db, las], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    return r.returncode, r.stderr.splitlines()


# ---- mask tracks from piles of overlaps (LArepeat, TANmask) -------------------------------------------------------

def repeat_params(cov=-1, xcov_enter=2.0, xcov_leave=1.7, merge_dist=-1, min_aln_len=0, inc_identity=0, inccov=0, max_cov=100):
    return RepeatParams(xcov_enter, xcov_leave, cov, merge_dist, min_aln_len, int(inc_identity), int(inccov), max_cov)


def _batch(piles, read_len, read_flags):
    """piles: dict of numpy arrays pile_off (int64, npiles + 1), pile_aread, abpos, aepos, bbpos, bepos, bread, flags."""
    import numpy as np
    keep = {}
    b = PileBatch()
    keep["pile_off"] = np.ascontiguousarray(piles["pile_off"], dtype=np.int64)
    b.npiles = len(keep["pile_off"]) - 1
    b.pile_off = keep["pile_off"].ctypes.data_as(C.POINTER(c_int64))
    for k in ("pile_aread", "abpos", "aepos", "bbpos", "bepos", "bread", "flags"):
        keep[k] = np.ascontiguousarray(piles[k], dtype=np.int32)
        setattr(b, k, keep[k].ctypes.data_as(_PI))
    b.nrec = len(keep["abpos"])
    keep["read_len"] = np.ascontiguousarray(read_len, dtype=np.int32)
    keep["read_flags"] = np.ascontiguousarray(read_flags, dtype=np.int32)
    b.read_len = keep["read_len"].ctypes.data_as(_PI)
    b.read_flags = keep["read_flags"].ctypes.data_as(_PI)
    b.nreads = len(keep["read_len"])
    b.maxlen = int(keep["read_len"].max()) if b.nreads else 0
    return b, keep


def _take_track(L, t, count):
    import numpy as np
    data = np.ctypeslib.as_array(t.data, shape=(max(int(t.ndata), 1),))[:int(t.ndata)].copy()
    C.CDLL(None).free(t.data)
    return count, data


def pile_coverage(piles, read_len, read_flags, params):
    """-> (histogram int64[max_cov], bases, inactive bases) of the batch (LArepeat's estimate pass)."""
    import numpy as np
    L = _lib()
    b, keep = _batch(piles, read_len, read_flags)
    histo = np.zeros(params.max_cov, dtype=np.int64)
    bases, inactive = c_int64(0), c_int64(0)
    if L.damar_pile_coverage(C.byref(b), C.byref(params), histo.ctypes.data_as(C.POINTER(c_int64)), C.byref(bases), C.byref(inactive)):
        raise RuntimeError("damar_pile_coverage failed")
    return histo, bases.value, inactive.value


def pile_repeats(piles, read_len, read_flags, params):
    """-> (count int32[npiles], data int32[], merged, repeat_bases) of the batch (LArepeat's repeat pass)."""
    import numpy as np
    L = _lib()
    b, keep = _batch(piles, read_len, read_flags)
    count = np.zeros(max(b.npiles, 1), dtype=np.int32)
    t = PileTrack(count.ctypes.data_as(_PI), None, 0, 0, 0)
    if L.damar_pile_repeats(C.byref(b), C.byref(params), C.byref(t)):
        raise RuntimeError("damar_pile_repeats failed")
    count, data = _take_track(L, t, count[:b.npiles])
    return count, data, int(t.merged), int(t.repeat_bases)


def pile_tandem(piles, read_len, read_flags, min_len=0):
    """-> (count int32[npiles], data int32[]) of the batch (TANmask's sweep with an honest threshold)."""
    import numpy as np
    L = _lib()
    b, keep = _batch(piles, read_len, read_flags)
    count = np.zeros(max(b.npiles, 1), dtype=np.int32)
    t = PileTrack(count.ctypes.data_as(_PI), None, 0, 0, 0)
    if L.damar_pile_tandem(C.byref(b), int(min_len), C.byref(t)):
        raise RuntimeError("damar_pile_tandem failed")
    return _take_track(L, t, count[:b.npiles])


_PHASES = ("upload", "kernel", "download", "call")
_STAGES = ("trace", "pile", "q", "box", "tbox", "gap", "fix", "filter", "correct", "read", "dust", "separate")


def _last(stage, ncnt, names=_PHASES):
    """damar_<stage>_last -> ({names: ms}, the ncnt counters...)."""
    ms, cnt = (C.c_double * 4)(), (c_int64 * ncnt)()
    f = getattr(_lib(), "damar_%s_last" % stage)
    f.argtypes, f.restype = [C.POINTER(C.c_double), C.POINTER(c_int64)], None
    f(ms, cnt)
    return (dict(zip(names, list(ms))),) + tuple(cnt)


def release(stage):
    """Frees the device buffers and events a call family keeps between calls: damar_<stage>_release, stage one of
    trace, pile, q, box, tbox, gap, fix, filter, correct, read, dust, separate (a homogenize session is released by closing it)."""
    if stage not in _STAGES:
        raise ValueError("no stage %r" % (stage,))
    f = getattr(_lib(), "damar_%s_release" % stage)
    f.argtypes, f.restype = [], None
    f()


def pile_last():
    """Of the last device call: ({upload, sort, sweep, download} ms, events sorted, regions written)."""
    return _last("pile", 2, ("upload", "sort", "sweep", "download"))


def db_info(db):
    """-> (read_len, read_flags, block_first or None) of a database, from its stub and index alone."""
    import numpy as np
    L = _lib()
    d = DbInfo()
    if L.damar_dbinfo_open(db.encode(), C.byref(d)):
        raise RuntimeError("cannot open database %s" % db)
    rl = np.ctypeslib.as_array(d.read_len, shape=(d.nreads,)).copy()
    rf = np.ctypeslib.as_array(d.read_flags, shape=(d.nreads,)).copy()
    bf = np.ctypeslib.as_array(d.block_first, shape=(d.nblocks + 1,)).copy() if d.nblocks else None
    L.damar_dbinfo_close(C.byref(d))
    return rl, rf, bf


def read_piles(las, bound=0):
    """The batches of whole piles of a .las file, as dicts of numpy arrays (host/piles.c)."""
    import numpy as np
    L = _lib()
    r = L.damar_piles_open(las.encode(), bound)
    if not r:
        raise RuntimeError("cannot open %s" % las)
    out = []
    try:
        while True:
            b = PileBatch()
            got = L.damar_piles_next(r, C.byref(b))
            if got < 0:
                raise RuntimeError("%s is damaged" % las)
            if got == 0:
                break
            d = {"pile_off": np.ctypeslib.as_array(b.pile_off, shape=(b.npiles + 1,)).copy(),
                 "pile_aread": np.ctypeslib.as_array(b.pile_aread, shape=(b.npiles,)).copy()}
            for k in ("abpos", "aepos", "bbpos", "bepos", "bread", "flags"):
                d[k] = np.ctypeslib.as_array(getattr(b, k), shape=(b.nrec,)).copy()
            out.append(d)
    finally:
        L.damar_piles_close(r)
    return out


def read_trace_piles(las, bound=0, tbound=0):
    """The batches of whole piles of a .las file with their traces (the traces-on reader of host/piles.c), as the dicts
    pile_quality takes; tbound: the trace bytes a batch holds at most (0: 1 GiB)."""
    import numpy as np
    L = _lib()
    L.damar_piles_open_traces.argtypes = [C.c_char_p, c_int64, c_int64]
    L.damar_piles_open_traces.restype = C.c_void_p
    L.damar_piles_next_traces.argtypes = [C.c_void_p, C.POINTER(TraceBatch)]
    r = L.damar_piles_open_traces(las.encode(), bound, tbound)
    if not r:
        raise RuntimeError("cannot open %s" % las)
    out = []
    try:
        while True:
            t = TraceBatch()
            got = L.damar_piles_next_traces(r, C.byref(t))
            if got < 0:
                raise RuntimeError("%s is damaged" % las)
            if got == 0:
                break
            b = t.p
            d = {"pile_off": np.ctypeslib.as_array(b.pile_off, shape=(b.npiles + 1,)).copy(),
                 "pile_aread": np.ctypeslib.as_array(b.pile_aread, shape=(b.npiles,)).copy()}
            for k in ("abpos", "aepos", "bbpos", "bepos", "bread", "flags"):
                d[k] = np.ctypeslib.as_array(getattr(b, k), shape=(b.nrec,)).copy()
            d["tlen"] = np.ctypeslib.as_array(t.tlen, shape=(b.nrec,)).copy()
            d["trace_off"] = np.ctypeslib.as_array(t.trace_off, shape=(b.nrec,)).copy()
            d["trace"] = np.ctypeslib.as_array(t.trace, shape=(max(t.trace_bytes, 1),))[:t.trace_bytes].copy()
            d["tbytes"], d["tspace"] = t.tbytes, t.tspace
            out.append(d)
    finally:
        L.damar_piles_close(r)
    return out


def repeat_track(db, las, max_areads=-1, cov_only=False, **opts):
    """LArepeat on one .las file: -> (anno uint64[nreads + 1], data int32[], stats); opts as repeat_params()."""
    import numpy as np
    L = _lib()
    d = DbInfo()
    if L.damar_dbinfo_open(db.encode(), C.byref(d)):
        raise RuntimeError("cannot open database %s" % db)
    p = repeat_params(**opts)
    res = RepeatResult()
    rc = L.damar_repeat_track(C.byref(d), las.encode(), C.byref(p), max_areads, 1 if cov_only else 0, C.byref(res))
    try:
        if rc:
            raise RuntimeError("damar_repeat_track failed (%d)" % rc)
        stats = dict(cov=res.cov, merged=int(res.merged), bases_total=int(res.bases_total), bases_repeat=int(res.bases_repeat))
        if res.histo:
            stats.update(histo=np.ctypeslib.as_array(res.histo, shape=(p.max_cov,)).copy(), cov_max=res.cov_max,
                         cov_bases=int(res.cov_bases), cov_inactive=int(res.cov_inactive), avg_rlen=res.avg_rlen)
        if cov_only:
            return None, None, stats
        anno = np.ctypeslib.as_array(res.anno, shape=(d.nreads + 1,)).copy()
        data = np.ctypeslib.as_array(res.data, shape=(max(int(res.ndata), 1),))[:int(res.ndata)].copy()
        return anno, data, stats
    finally:
        L.damar_repeat_result_free(C.byref(res))
        L.damar_dbinfo_close(C.byref(d))


def tan_track(db, las, min_len=0, block=0):
    """TANmask's track of one .las file: -> (offsets int64[reads + 1] in bytes, data int32[]) for the reads of `block`
    (0: the whole database)."""
    import numpy as np
    L = _lib()
    d = DbInfo()
    if L.damar_dbinfo_open(db.encode(), C.byref(d)):
        raise RuntimeError("cannot open database %s" % db)
    try:
        if block < 0 or block > d.nblocks:
            raise ValueError("block %d of a database of %d blocks" % (block, d.nblocks))
        first, last = (d.block_first[block - 1], d.block_first[block]) if block > 0 else (0, d.nreads)
        offs, data = C.POINTER(c_int64)(), _PI()
        nm, mk = c_int64(0), c_int64(0)
        rc = L.damar_tan_track(C.byref(d), las.encode(), first, last, int(min_len), C.byref(offs), C.byref(data), C.byref(nm), C.byref(mk))
        if rc:
            raise RuntimeError("damar_tan_track failed (%d)" % rc)
        o = np.ctypeslib.as_array(offs, shape=(last - first + 1,)).copy()
        n = int(o[-1]) // 4
        v = np.ctypeslib.as_array(data, shape=(max(n, 1),))[:n].copy()
        libc = C.CDLL(None)
        libc.free(offs)
        libc.free(data)
        return o, v
    finally:
        L.damar_dbinfo_close(C.byref(d))


# ---- quality and trim tracks from the overlaps' traces (LAq) --------------------------------------------------------

def pile_quality(batch, read_len, segmin=1, segmax=20, ccs=False):
    """-> q int32[tiles]: the quality value of every tile (segment of tspace bases) of the batch's piles, pile after pile,
    ceil(read length / tspace) tiles each.  batch: the arrays of a trace-less batch (_batch) plus `trace` (uint8, the
    records' trace bytes back to back), `trace_off` (int64, a byte offset per record), `tlen`, `tbytes` and `tspace`."""
    import numpy as np
    L = _lib()
    pb, keep = _batch(batch, read_len, np.zeros(len(read_len), dtype=np.int32))
    t = TraceBatch()
    t.p = pb
    keep["trace"] = np.ascontiguousarray(batch["trace"], dtype=np.uint8)
    keep["trace_off"] = np.ascontiguousarray(batch["trace_off"], dtype=np.int64)
    keep["tlen"] = np.ascontiguousarray(batch["tlen"], dtype=np.int32)
    if len(keep["trace_off"]) != pb.nrec or len(keep["tlen"]) != pb.nrec:
        raise ValueError("trace_off and tlen hold one entry per record")
    t.trace = keep["trace"].ctypes.data_as(C.POINTER(C.c_ubyte))
    t.trace_off = keep["trace_off"].ctypes.data_as(C.POINTER(c_int64))
    t.tlen = keep["tlen"].ctypes.data_as(_PI)
    t.trace_bytes = len(keep["trace"])
    t.tbytes, t.tspace = int(batch["tbytes"]), int(batch["tspace"])
    p = QParams(int(segmin), int(segmax), 1 if ccs else 0)
    nt = c_int64(0)
    if L.damar_pile_quality(C.byref(t), C.byref(p), None, C.byref(nt)):
        raise RuntimeError("damar_pile_quality failed")
    q = np.zeros(max(nt.value, 1), dtype=np.int32)
    if L.damar_pile_quality(C.byref(t), C.byref(p), q.ctypes.data_as(_PI), C.byref(nt)):
        raise RuntimeError("damar_pile_quality failed")
    return q[:nt.value]


def q_last():
    """Of the last device call of pile_quality / q_track: ({upload, count, select, download} ms, segments counted, tiles)."""
    return _last("q", 2, ("upload", "count", "select", "download"))


def _take_q(res, nreads, with_q):
    import numpy as np
    arr = lambda ptr, n, dt: np.ctypeslib.as_array(ptr, shape=(max(int(n), 1),))[:int(n)].astype(dt)
    out = ()
    if with_q:
        out = (arr(res.q_anno, nreads + 1, np.uint64), arr(res.q_data, res.nq, np.int32))
    return out + (arr(res.trim_anno, nreads + 1, np.uint64), arr(res.trim_data, res.ntrim, np.int32))


def q_track(db, las, segmin=1, segmax=20, trim_q=25, min_len=1000, ccs=False):
    """LAq on one .las file: -> (q_anno uint64[nreads + 1], q_data int32[], trim_anno, trim_data), the annos in bytes."""
    L = _lib()
    d = DbInfo()
    if L.damar_dbinfo_open(db.encode(), C.byref(d)):
        raise RuntimeError("cannot open database %s" % db)
    p = QParams(int(segmin), int(segmax), 1 if ccs else 0)
    res = QResult()
    try:
        if L.damar_q_track(C.byref(d), las.encode(), C.byref(p), int(trim_q), int(min_len), C.byref(res)):
            raise RuntimeError("damar_q_track failed")
        return _take_q(res, d.nreads, True)
    finally:
        L.damar_q_result_free(C.byref(res))
        L.damar_dbinfo_close(C.byref(d))


def trim_update(db, las, q, trim, trim_q=25, min_len=1000, ccs=False):
    """LAq -u: the trim track again from the records of `las` that are neither discarded nor identity overlaps.
    q, trim: (anno, data) as q_track returns them -> (trim_anno, trim_data); reads without a pile get no entry."""
    import numpy as np
    L = _lib()
    d = DbInfo()
    if L.damar_dbinfo_open(db.encode(), C.byref(d)):
        raise RuntimeError("cannot open database %s" % db)
    qa, ta = (np.ascontiguousarray(x[0], dtype=np.uint64) for x in (q, trim))
    qd, td = (np.ascontiguousarray(x[1], dtype=np.int32) for x in (q, trim))
    res = QResult()
    try:
        if len(qa) != d.nreads + 1 or len(ta) != d.nreads + 1 or int(qa[-1]) != 4 * len(qd) or int(ta[-1]) != 4 * len(td) \
                or np.any(qa[1:] < qa[:-1]) or np.any(ta[1:] < ta[:-1]) or np.any(qa % 4) or np.any(ta % 4):
            raise ValueError("the tracks do not fit the database")
        u64p = C.POINTER(C.c_uint64)
        if L.damar_trim_update(C.byref(d), las.encode(), qa.ctypes.data_as(u64p), qd.ctypes.data_as(_PI), len(qd),
                               ta.ctypes.data_as(u64p), td.ctypes.data_as(_PI), int(trim_q), int(min_len), 1 if ccs else 0, C.byref(res)):
            raise RuntimeError("damar_trim_update failed")
        return _take_q(res, d.nreads, False)
    finally:
        L.damar_q_result_free(C.byref(res))
        L.damar_dbinfo_close(C.byref(d))


# ---- overlaps cut back to the trim track (LAtrim) and the exact box alignment under it -----------------------------

def align_boxes(a_seqs, b_seqs):
    """Exact alignment of box i = a_seqs[i] against b_seqs[i] (sequences of base values, one per element, neither empty)
    as the reference's Compute_Alignment(DIFF_ALIGN) does it: -> (diffs int32[boxes], scripts: a list of int32 arrays, the
    indels in path order, -(a + 1) for a base of B alone in front of A position a, b + 1 for a base of A alone in front of
    B position b).  On the GPU, one wavefront per box, unless DAMAR_TRIM=host is set."""
    return _align(_lib().damar_align_boxes, "damar_align_boxes", a_seqs, b_seqs)


def _box_columns(a_seqs, b_seqs):
    """The sequences of a batch of boxes as the arrays behind a BoxBatch or TBoxBatch, to be kept alive while the batch is
    in use: -> (m, n, aoff, boff, bases, nbases), the bases of all boxes in one array, A before B."""
    import numpy as np
    nb = len(a_seqs)
    seqs = [np.ascontiguousarray(x, dtype=np.uint8) for pair in zip(a_seqs, b_seqs) for x in pair]
    if any(len(x) == 0 for x in seqs):
        raise ValueError("a box has at least one base on either side")
    lens = np.array([len(x) for x in seqs], dtype=np.int64).reshape(nb, 2)
    offs = np.concatenate([[0], np.cumsum(lens.reshape(-1))]).astype(np.int64)
    bases = np.concatenate(seqs) if nb else np.zeros(1, dtype=np.uint8)
    m, n = (np.ascontiguousarray(lens[:, k], dtype=np.int32) for k in (0, 1))
    return m, n, np.ascontiguousarray(offs[:-1:2]), np.ascontiguousarray(offs[1::2]), bases, int(offs[-1])


def _align(call, name, a_seqs, b_seqs):
    import numpy as np
    if len(a_seqs) != len(b_seqs):
        raise ValueError("one B sequence per A sequence")
    nb = len(a_seqs)
    m, n, aoff, boff, bases, nbases = _box_columns(a_seqs, b_seqs)
    bb = BoxBatch(nb, m.ctypes.data_as(_PI), n.ctypes.data_as(_PI), aoff.ctypes.data_as(C.POINTER(c_int64)),
                  boff.ctypes.data_as(C.POINTER(c_int64)), bases.ctypes.data, nbases)
    diffs, soff, script = np.zeros(max(nb, 1), dtype=np.int32), np.zeros(nb + 1, dtype=np.int64), _PI()
    if call(C.byref(bb), diffs.ctypes.data_as(_PI), soff.ctypes.data_as(C.POINTER(c_int64)), C.byref(script)):
        raise RuntimeError(name + " failed")
    try:
        total = int(soff[nb])
        flat = np.ctypeslib.as_array(script, shape=(max(total, 1),))[:total].copy()
    finally:
        C.CDLL(None).free(script)
    return diffs[:nb], [flat[soff[i]:soff[i + 1]] for i in range(nb)]


def box_last():
    """Of the last align_boxes / of the last batch of trim_las: ({upload, kernel, download, call} ms, boxes, boxes the host
    routine did beside the kernel, script values)."""
    return _last("box", 3)


def align_reads(a_seqs, b_seqs):
    """align_boxes for boxes of read length (a read against its correction, LAcorrect's postrace): the same arguments and
    the same result.  On the GPU, one workgroup of eight wavefronts per box and the boxes dealt longest first, unless
    DAMAR_POSTRACE=host is set; what bounds a box there is its differences (8000), not its length."""
    return _align(_lib().damar_align_reads, "damar_align_reads", a_seqs, b_seqs)


def read_last():
    """Of the last align_reads / of the last batch of correct_las: ({upload, kernel, download, call} ms, boxes, boxes the
    host routine did beside the kernel, script values)."""
    return _last("read", 3)


def trim_las(db, las, out, track="trim", purge=False):
    """LAtrim on one .las file: every record cut back to what `track` keeps of both reads, written to `out` (purge: without
    the records that end up discarded) -> the counters of the run."""
    st = TrimStats()
    if _lib().damar_trim_las(db.encode(), las.encode(), out.encode(), track.encode(), 1 if purge else 0, C.byref(st)):
        raise RuntimeError("damar_trim_las failed")
    return {k: int(getattr(st, k)) for k, _ in TrimStats._fields_}


# ---- split overlaps rejoined (LAstitch) and the exact box alignment into trace pairs under it -----------------------

def trace_boxes(a_seqs, b_seqs, a_starts, tspace):
    """Exact alignment of box i = a_seqs[i] against b_seqs[i] (sequences of base values, one per element, neither empty)
    into trace pairs as the reference's Compute_Alignment(DIFF_TRACE) does it, a_starts[i] being where the box begins in A
    (the pairs are cut on A's grid of tspace): -> (diffs int32[boxes], a list of uint16 arrays: differences and B length of
    every interval the box touches).  On the GPU, one wavefront per box, unless DAMAR_STITCH=host is set."""
    import numpy as np
    L = _lib()
    if len(a_seqs) != len(b_seqs) or len(a_seqs) != len(a_starts):
        raise ValueError("one B sequence and one start per A sequence")
    if int(tspace) < 1:
        raise ValueError("the trace spacing is at least 1")
    nb = len(a_seqs)
    m, n, aoff, boff, bases, nbases = _box_columns(a_seqs, b_seqs)
    ab = np.ascontiguousarray(a_starts, dtype=np.int32).reshape(nb)
    if nb and ab.min() < 0:
        raise ValueError("a box begins at or behind position 0 of A")
    i64p = C.POINTER(c_int64)
    tb = TBoxBatch(nb, m.ctypes.data_as(_PI), n.ctypes.data_as(_PI), ab.ctypes.data_as(_PI), aoff.ctypes.data_as(i64p),
                   boff.ctypes.data_as(i64p), bases.ctypes.data, nbases, int(tspace))
    diffs, toff, trace = np.zeros(max(nb, 1), dtype=np.int32), np.zeros(nb + 1, dtype=np.int64), C.POINTER(C.c_uint16)()
    if L.damar_trace_boxes(C.byref(tb), diffs.ctypes.data_as(_PI), toff.ctypes.data_as(i64p), C.byref(trace)):
        raise RuntimeError("damar_trace_boxes failed")
    try:
        total = int(toff[nb])
        flat = np.ctypeslib.as_array(trace, shape=(max(total, 1),))[:total].copy()
    finally:
        C.CDLL(None).free(trace)
    return diffs[:nb], [flat[toff[i]:toff[i + 1]] for i in range(nb)]


def tbox_last():
    """Of the last trace_boxes / of the last round of stitch_las: ({upload, kernel, download, call} ms, boxes, boxes the host
    routine did beside the kernel, trace values)."""
    return _last("tbox", 3)


def stitch_las(db, las, out, fuzz=40, purge=False, track=None, repeats=None, anchor=500, merge=10, min_len=500, min_merge=200,
               gap_diff=0.3):
    """LAstitch on one .las file: the records of one (A read, B read) that the overlapper split are rejoined, the joint
    realigned, the superfluous record flagged; written to `out` (purge: without the discarded records) -> the counters of
    the run, round_boxes a list of the boxes per round."""
    p = StitchParams(int(fuzz), 1 if purge else 0, int(anchor), int(merge), int(min_len), int(min_merge), float(gap_diff),
                     track.encode() if track else None, repeats.encode() if repeats else None)
    st = StitchStats()
    if int(fuzz) < 0:
        raise ValueError("invalid fuzzing value of %d" % int(fuzz))
    if _lib().damar_stitch_las(db.encode(), las.encode(), out.encode(), C.byref(p), C.byref(st)):
        raise RuntimeError("damar_stitch_las failed")
    res = {k: int(getattr(st, k)) for k, _ in StitchStats._fields_ if k != "round_boxes"}
    res["round_boxes"] = [int(x) for x in st.round_boxes][:max(res["rounds"], 1)]
    return res


# ---- containments, gaps and breaks of piles (LAgap) -----------------------------------------------------------------

GAP_KINDS = ("masked", "stitchable", "drop_L", "drop_R", "drop_none")
GAP_TRAILING = 0x100


def gap_limits():
    """(bins, events) a pile may have for kernels/pile_gaps.hip to do it: DAMAR_GAP_MAXBINS, DAMAR_GAP_MAXEVENTS"""
    bins, events = C.c_int(0), C.c_int(0)
    _lib().damar_gap_limits(C.byref(bins), C.byref(events))
    return bins.value, events.value


def _gap_params(stitch, exclude, keep):
    import numpy as np
    p = GapParams(int(stitch), None, None, 0, 0, None)
    if exclude is not None:
        keep["ex_anno"] = np.ascontiguousarray(exclude[0], dtype=np.uint64)
        keep["ex_data"] = np.ascontiguousarray(exclude[1], dtype=np.int32)
        p.ex_anno = keep["ex_anno"].ctypes.data_as(C.POINTER(C.c_uint64))
        p.ex_data = keep["ex_data"].ctypes.data_as(_PI)
        p.ex_ndata = len(keep["ex_data"])
    return p


def pile_gaps(piles, read_len, stitch=0, exclude=None):
    """LAgap's work on a batch of whole piles (the dict of _batch; exclude: (anno, data) of a track of the whole database,
    byte offsets and {begin, end} pairs): -> (flags int32[nrec], OVL_TEMP included, and per pile the list of its events
    (first bin, bin after the run, kind, v0, v1, records dropped), kind as include/damar_hip.h has it).  On the GPU, one
    wavefront per pile, unless DAMAR_PILES=host is set."""
    import numpy as np
    L = _lib()
    b, keep = _batch(piles, read_len, np.zeros(len(read_len), dtype=np.int32))
    p = _gap_params(stitch, exclude, keep)
    if exclude is not None and len(keep["ex_anno"]) != b.nreads + 1:
        raise ValueError("the exclude track holds one offset per read and one more")
    flags = np.zeros(max(b.nrec, 1), dtype=np.int32)
    count = np.zeros(max(b.npiles, 1), dtype=np.int32)
    ev = GapEvents(count.ctypes.data_as(_PI), None, 0, 0, 0, 0)
    if L.damar_pile_gaps(C.byref(b), C.byref(p), flags.ctypes.data_as(_PI), C.byref(ev)):
        raise RuntimeError("damar_pile_gaps failed")
    try:
        flat = np.ctypeslib.as_array(ev.ev, shape=(max(6 * int(ev.nev), 1),))[:6 * int(ev.nev)].copy().reshape(-1, 6)
    finally:
        C.CDLL(None).free(ev.ev)
    at, events = 0, []
    for n in count[:b.npiles]:
        events.append([tuple(int(x) for x in row) for row in flat[at:at + n]])
        at += int(n)
    return flags[:b.nrec], events


def gap_last():
    """Of the last pile_gaps / of the last batch of gap_las: ({upload, kernel, download, call} ms, piles, piles the host
    routine did beside the kernel, break events)."""
    return _last("gap", 3)


def gap_las(db, las, out, stitch=0, purge=False, trim=None, exclude=None, repeats=None):
    """LAgap on one .las file: contained records and the records across gaps and breaks flagged, written to `out` (purge:
    without the discarded records); trim: the trim track the records are cut to first, exclude: the track whose intervals
    mask breaks, repeats: loaded and not used, as in the reference.  The reference's lines go to stdout.  -> the counters of
    the run (host_piles: piles the host routine did beside the kernel)."""
    import numpy as np
    L = _lib()
    d = DbInfo()
    if L.damar_dbinfo_open(db.encode(), C.byref(d)):
        raise RuntimeError("cannot open database %s" % db)
    try:
        got = {}
        for name in (exclude, repeats):
            if name is None:
                continue
            anno, data, ndata = C.POINTER(C.c_uint64)(), _PI(), c_int64(0)
            if L.damar_track_read_any(C.byref(d), name.encode(), C.byref(anno), C.byref(data), C.byref(ndata)):
                raise RuntimeError("could not open track '%s'" % name)
            got[name] = (np.ctypeslib.as_array(anno, shape=(d.nreads + 1,)).copy(),
                         np.ctypeslib.as_array(data, shape=(max(ndata.value, 1),))[:ndata.value].copy())
            C.CDLL(None).free(anno)
            C.CDLL(None).free(data)
    finally:
        L.damar_dbinfo_close(C.byref(d))
    keep = {}
    p = _gap_params(stitch, got.get(exclude) if exclude is not None else None, keep)
    p.purge = 1 if purge else 0
    p.trim_track = trim.encode() if trim else None
    st = GapStats()
    if L.damar_gap_las(db.encode(), las.encode(), out.encode(), C.byref(p), C.byref(st)):
        raise RuntimeError("damar_gap_las failed")
    res = {k: int(getattr(st, k)) for k, _ in GapStats._fields_ if k != "trim"}
    res["trim"] = {k: int(getattr(st.trim, k)) for k, _ in TrimStats._fields_}
    return res


# ---- the overlaps of a block pair split by their chains (LAseparate) --------------------------------------------------

class SeparateParams(C.Structure):     # include/damar_hip.h damar_separate_params
    _fields_ = [("rep_anno", C.POINTER(C.c_uint64)), ("rep_data", _PI), ("rep_ndata", c_int64), ("kind", C.c_int), ("twidth", C.c_int), ("rep_checked", C.c_int)]


class ChainOut(C.Structure):           # include/damar_hip.h damar_chain_out
    _fields_ = [(k, _PI) for k in ("flags", "nchains", "proper", "nbest", "best")]


class SeparateStats(C.Structure):      # host/damar_host.h damar_separate_stats
    _fields_ = [(k, c_int64) for k in ("novl", "written", "written_discard", "kept", "discarded", "groups", "host_groups", "multi")]


def separate_limits():
    """(records, chains) a group may have for kernels/pile_chains.hip to do it: DAMAR_SEPARATE_MAXGROUP, DAMAR_SEPARATE_MAXCHAINS"""
    group, chains = C.c_int(0), C.c_int(0)
    f = _lib().damar_separate_limits
    f.argtypes, f.restype = [_PI, _PI], None
    f(C.byref(group), C.byref(chains))
    return group.value, chains.value


def pile_chains(batch, read_len, rep_anno, rep_data, twidth, kind):
    """LAseparate's work on a batch of whole piles (the dict of _batch; rep_anno, rep_data: the repeat track of the whole
    database, byte offsets and {begin, end} pairs, or None for no track): -> (flags int32[nrec] as the reference's first
    pass leaves them, OVL_TEMP included, and per group in file order (number of chains, members of the best chain in chain
    order as indices into the group, whether it was found proper)).  On the GPU, a lane per group, unless DAMAR_PILES=host
    is set."""
    import numpy as np
    L = _lib()
    b, keep = _batch(batch, read_len, np.zeros(len(read_len), dtype=np.int32))
    p = SeparateParams(None, None, 0, int(kind), int(twidth), 0)
    if rep_anno is not None:
        keep["rep_anno"] = np.ascontiguousarray(rep_anno, dtype=np.uint64)
        keep["rep_data"] = np.ascontiguousarray(rep_data, dtype=np.int32)
        if len(keep["rep_anno"]) != b.nreads + 1:
            raise ValueError("the repeat track holds one offset per read and one more")
        p.rep_anno = keep["rep_anno"].ctypes.data_as(C.POINTER(C.c_uint64))
        p.rep_data = keep["rep_data"].ctypes.data_as(_PI)
        p.rep_ndata = len(keep["rep_data"])
    cols = np.zeros((5, max(b.nrec, 1)), dtype=np.int32)
    out = ChainOut(*[cols[i].ctypes.data_as(_PI) for i in range(5)])
    L.damar_pile_chains.argtypes = [C.POINTER(PileBatch), C.POINTER(SeparateParams), C.POINTER(ChainOut)]
    if L.damar_pile_chains(C.byref(b), C.byref(p), C.byref(out)):
        raise RuntimeError("damar_pile_chains failed")
    flags, nchains, proper, nbest, best = (c[:b.nrec] for c in cols)
    heads = np.flatnonzero(nchains >= 0)
    ends = np.append(heads[1:], b.nrec)
    groups = [(int(nchains[g]), [int(x) for x in best[g:g + min(int(nbest[g]), int(e - g))]], bool(proper[g])) for g, e in zip(heads, ends)]
    return flags.copy(), groups


def separate_last():
    """Of the last pile_chains / of the last batch of separate_las: ({upload, kernel, download, call} ms, groups, groups the
    host routine did beside the kernel, groups of more than one record)."""
    return _last("separate", 3)


def separate_las(db, las, out, out_discard, kind=0, repeats="rep"):
    """LAseparate on one .las file: the records the verdict of `kind` (-T) keeps written to `out`, the others to
    `out_discard`; repeats: the track of repeat intervals.  The reference's lines go to stdout.  -> the counters of the run
    (host_groups: groups the host routine did beside the kernel)."""
    L = _lib()
    st = SeparateStats()
    L.damar_separate_las.argtypes = [C.c_char_p] * 5 + [C.c_int, C.POINTER(SeparateStats)]
    if L.damar_separate_las(db.encode(), las.encode(), out.encode(), out_discard.encode(), repeats.encode(), int(kind), C.byref(st)):
        raise RuntimeError("damar_separate_las failed")
    return {k: int(getattr(st, k)) for k, _ in SeparateStats._fields_}


# ---- reads patched from their piles (LAfix) -------------------------------------------------------------------------

class FixParams(C.Structure):          # include/damar_hip.h damar_fix_params
    _fields_ = [("q_anno", C.POINTER(C.c_uint64)), ("q_data", _PI), ("q_ndata", c_int64), ("rep_anno", C.POINTER(C.c_uint64)),
                ("rep_data", _PI), ("rep_ndata", c_int64), ("lowq", C.c_int), ("maxgap", C.c_int), ("maxspanners", C.c_int),
                ("minsupport", C.c_int), ("twidth", C.c_int)]


class FixGaps(C.Structure):            # include/damar_hip.h damar_fix_gaps
    _fields_ = [("count", _PI), ("gaps", _PI), ("ngaps", c_int64)]


class FixOpts(C.Structure):            # host/damar_host.h damar_fix_opts
    _fields_ = [("min_len", C.c_int), ("lowq", C.c_int), ("maxgap", C.c_int), ("low_coverage", C.c_int), ("q_track", C.c_char_p),
                ("trim_track", C.c_char_p), ("rep_track", C.c_char_p), ("convert", C.POINTER(C.c_char_p)), ("nconvert", C.c_int),
                ("trim_out", C.c_char_p)]


class FixStats(C.Structure):           # host/damar_host.h damar_fix_stats
    _fields_ = [(k, c_int64) for k in ("gaps", "flips", "chimers", "bases_before", "bases_after", "reads_trimmed", "reads_fixed",
                                       "piles", "host_piles", "repairs")]


FIX_GAP = ("ab", "ae", "bb", "be", "diff", "b", "support", "comp")


def fix_limits():
    """(segments, candidates) a pile may have for kernels/pile_patch.hip to do it: DAMAR_FIX_MAXSEGS, DAMAR_FIX_MAXCAND"""
    segs, cands = C.c_int(0), C.c_int(0)
    L = _lib()
    L.damar_fix_limits.argtypes = [_PI, _PI]
    L.damar_fix_limits(C.byref(segs), C.byref(cands))
    return segs.value, cands.value


def pile_patches(batch, read_len, trim, q, repeats=None, low_q=28, max_gap=500, low_coverage=False):
    """LAfix's search on a batch of whole piles with their traces (the dict pile_quality takes; trim: int32[piles, 2], the
    interval kept of every pile's A read, begin >= end: none; q and repeats: (anno, data) of a track of the whole database,
    byte offsets): -> per pile the list of its repairs in the order they are spliced in, each a dict of FIX_GAP.  On the
    GPU, one wavefront per pile, unless DAMAR_PILES=host is set."""
    import numpy as np
    L = _lib()
    t, keep = _trace_batch(batch, read_len)
    u64p = C.POINTER(C.c_uint64)
    p = FixParams()
    keep["qa"], keep["qd"] = np.ascontiguousarray(q[0], dtype=np.uint64), np.ascontiguousarray(q[1], dtype=np.int32)
    if len(keep["qa"]) != t.p.nreads + 1:
        raise ValueError("the q track holds one offset per read and one more")
    p.q_anno, p.q_data, p.q_ndata = keep["qa"].ctypes.data_as(u64p), keep["qd"].ctypes.data_as(_PI), len(keep["qd"])
    if repeats is not None:
        keep["ra"], keep["rd"] = np.ascontiguousarray(repeats[0], dtype=np.uint64), np.ascontiguousarray(repeats[1], dtype=np.int32)
        if len(keep["ra"]) != t.p.nreads + 1:
            raise ValueError("the repeat track holds one offset per read and one more")
        p.rep_anno, p.rep_data, p.rep_ndata = keep["ra"].ctypes.data_as(u64p), keep["rd"].ctypes.data_as(_PI), len(keep["rd"])
    p.lowq, p.maxgap = int(low_q), int(max_gap)
    p.maxspanners, p.minsupport = (3, 2) if low_coverage else (7, 4)
    p.twidth = t.tspace
    tr = np.ascontiguousarray(trim, dtype=np.int32).reshape(-1)
    if len(tr) != 2 * t.p.npiles:
        raise ValueError("trim holds a begin and an end per pile")
    count = np.zeros(max(t.p.npiles, 1), dtype=np.int32)
    out = FixGaps(count.ctypes.data_as(_PI), None, 0)
    L.damar_pile_patches.argtypes = [C.POINTER(TraceBatch), C.POINTER(FixParams), _PI, C.POINTER(FixGaps)]
    if L.damar_pile_patches(C.byref(t), C.byref(p), tr.ctypes.data_as(_PI), C.byref(out)):
        raise RuntimeError("damar_pile_patches failed")
    try:
        flat = np.ctypeslib.as_array(out.gaps, shape=(max(8 * int(out.ngaps), 1),))[:8 * int(out.ngaps)].copy().reshape(-1, 8)
    finally:
        C.CDLL(None).free(out.gaps)
    at, res = 0, []
    for n in count[:t.p.npiles]:
        res.append([dict(zip(FIX_GAP, (int(x) for x in row))) for row in flat[at:at + n]])
        at += int(n)
    return res


def fix_last():
    """Of the last pile_patches / of the last batch of fix_las: ({upload, kernel, download, call} ms, piles, piles the host
    routine did beside the kernel, repairs)."""
    return _last("fix", 3)


def fix_las(db, las, fasta, *, min_len=1000, low_q=28, max_gap=500, trim=None, q="q", repeats=None, convert=(), trim_out=None,
            low_coverage=False):
    """LAfix on one .las file: every read with a pile patched from the reads that overlap it and written to `fasta`; trim, q,
    repeats and convert name tracks of the database (LAfix's -t -q -r -c), trim_out is the file of -T.  The reference's
    lines go to stdout.  -> the counters of the run (host_piles: piles the host routine did beside the kernel)."""
    L = _lib()
    enc = lambda s: s.encode() if s else None
    names = (C.c_char_p * max(len(convert), 1))(*[c.encode() for c in convert])
    o = FixOpts(int(min_len), int(low_q), int(max_gap), 1 if low_coverage else 0, enc(q), enc(trim), enc(repeats), names,
                len(convert), enc(trim_out))
    st = FixStats()
    L.damar_fix_las.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(FixOpts), C.POINTER(FixStats)]
    if L.damar_fix_las(db.encode(), las.encode(), fasta.encode(), C.byref(o), C.byref(st)):
        raise RuntimeError("damar_fix_las failed")
    return {k: int(getattr(st, k)) for k, _ in FixStats._fields_}


# ---- repeat intervals carried across overlaps onto the B reads (TKhomogenize) ---------------------------------------

def _trace_batch(batch, read_len):
    """a batch of the read_trace_piles form as the C structure, and what keeps its arrays alive"""
    import numpy as np
    pb, keep = _batch(batch, read_len, np.zeros(len(read_len), dtype=np.int32))
    t = TraceBatch()
    t.p = pb
    keep["trace"] = np.ascontiguousarray(batch["trace"], dtype=np.uint8)
    keep["trace_off"] = np.ascontiguousarray(batch["trace_off"], dtype=np.int64)
    keep["tlen"] = np.ascontiguousarray(batch["tlen"], dtype=np.int32)
    if len(keep["trace_off"]) != pb.nrec or len(keep["tlen"]) != pb.nrec:
        raise ValueError("trace_off and tlen hold one entry per record")
    t.trace = keep["trace"].ctypes.data_as(C.POINTER(C.c_ubyte))
    t.trace_off = keep["trace_off"].ctypes.data_as(C.POINTER(c_int64))
    t.tlen = keep["tlen"].ctypes.data_as(_PI)
    t.trace_bytes = len(keep["trace"])
    t.tbytes, t.tspace = int(batch["tbytes"]), int(batch["tspace"])
    return t, keep


def trim_pairs(trim_anno, trim_data, nreads):
    """the trim track as one {begin, end} per read, the way the reference's get_trim reads it: (0, 0) for a read without an
    entry or with an empty or inverted one"""
    import numpy as np
    anno = np.asarray(trim_anno, dtype=np.int64) // 4
    data = np.asarray(trim_data, dtype=np.int32)
    n = np.diff(anno)
    if len(anno) != nreads + 1 or np.any((n != 0) & (n != 2)):
        raise ValueError("a trim track holds one interval per read at most")
    pairs = np.zeros((nreads, 2), dtype=np.int32)
    has = np.flatnonzero(n == 2)
    b, e = data[anno[has]], data[anno[has] + 1]
    ok = b < e
    pairs[has[ok], 0], pairs[has[ok], 1] = b[ok], e[ok]
    return pairs


def pile_homogenize(batches, read_len, rep_anno, rep_data, merge=False, ends=-1, trim=None, res=1):
    """TKhomogenize on arrays: the intervals of the track (rep_anno uint64[nreads + 1] byte offsets, rep_data {begin, end}
    pairs) carried across the records of `batches` -- a LIST of batches of the read_trace_piles form, added to one session
    in order -- onto the B reads.  merge: -m; ends: -e, with trim = (anno, data) of the trim track; res: -r.
    -> (anno uint64[nreads + 1], data int32[], tagged).  The mask lives on the GPU unless DAMAR_PILES=host is set."""
    import numpy as np
    L = _lib()
    rl = np.ascontiguousarray(read_len, dtype=np.int32)
    nreads = len(rl)
    ra = np.ascontiguousarray(rep_anno, dtype=np.uint64)
    rd = np.ascontiguousarray(rep_data, dtype=np.int32)
    if len(ra) != nreads + 1:
        raise ValueError("the interval track holds an offset per read and one more")
    pairs = None
    if ends != -1:
        if trim is None:
            raise ValueError("ends needs the trim track")
        pairs = np.ascontiguousarray(trim_pairs(trim[0], trim[1], nreads))
    u64p = C.POINTER(C.c_uint64)
    h = L.damar_homog_open(rl.ctypes.data_as(_PI), nreads, int(res))
    if not h:
        raise RuntimeError("damar_homog_open failed")
    try:
        if merge and L.damar_homog_seed(h, ra.ctypes.data_as(u64p), rd.ctypes.data_as(_PI), len(rd)):
            raise RuntimeError("damar_homog_seed failed")
        for batch in batches:
            t, keep = _trace_batch(batch, rl)
            if L.damar_homog_add(h, C.byref(t), ra.ctypes.data_as(u64p), rd.ctypes.data_as(_PI), len(rd), int(ends),
                                 pairs.ctypes.data_as(_PI) if pairs is not None else None):
                raise RuntimeError("damar_homog_add failed")
        anno = np.zeros(nreads + 1, dtype=np.uint64)
        data, ndata, tagged = _PI(), c_int64(0), c_int64(0)
        if L.damar_homog_finish(h, anno.ctypes.data_as(u64p), C.byref(data), C.byref(ndata), C.byref(tagged)):
            raise RuntimeError("damar_homog_finish failed")
        try:
            out = np.ctypeslib.as_array(data, shape=(max(ndata.value, 1),))[:ndata.value].copy()
        finally:
            C.CDLL(None).free(data)
        return anno, out, tagged.value
    finally:
        L.damar_homog_close(h)


def homog_last():
    """Of the last session of pile_homogenize / homogenize_track, summed over its calls: ({upload, mark, readout, download}
    ms, records seen, ranges set in the mask, intervals read out)."""
    return _last("homog", 3, ("upload", "mark", "readout", "download"))


def _load_a2(L, d, name):
    import numpy as np
    anno, data, n = C.POINTER(C.c_uint64)(), _PI(), c_int64(0)
    if L.damar_track_read_a2(d.path, name.encode(), d.nreads, C.byref(anno), C.byref(data), C.byref(n)):
        raise RuntimeError("cannot read track %s" % name)
    try:
        return (np.ctypeslib.as_array(anno, shape=(d.nreads + 1,)).copy(),
                np.ctypeslib.as_array(data, shape=(max(n.value, 1),))[:n.value].copy())
    finally:
        libc = C.CDLL(None)
        libc.free(anno)
        libc.free(data)


def homogenize_track(db, las, track_in="repeats", merge=False, ends=-1, trim="trim", res=1):
    """TKhomogenize on one .las file: the track `track_in` of the database carried across the overlaps
    -> (anno uint64[nreads + 1] in bytes, data int32[], tagged)."""
    import numpy as np
    L = _lib()
    d = DbInfo()
    if L.damar_dbinfo_open(db.encode(), C.byref(d)):
        raise RuntimeError("cannot open database %s" % db)
    res_c = HomogResult()
    try:
        ia, idt = _load_a2(L, d, track_in)
        u64p = C.POINTER(C.c_uint64)
        p = HomogParams(1 if merge else 0, int(ends), int(res), ia.ctypes.data_as(u64p), idt.ctypes.data_as(_PI), len(idt), None, None)
        if ends != -1:
            ta, td = _load_a2(L, d, trim)
            p.trim_anno, p.trim_data = ta.ctypes.data_as(u64p), td.ctypes.data_as(_PI)
        if L.damar_homogenize_track(C.byref(d), las.encode(), C.byref(p), C.byref(res_c)):
            raise RuntimeError("damar_homogenize_track failed")
        anno = np.ctypeslib.as_array(res_c.anno, shape=(d.nreads + 1,)).copy()
        data = np.ctypeslib.as_array(res_c.data, shape=(max(int(res_c.ndata), 1),))[:int(res_c.ndata)].copy()
        return anno, data, int(res_c.tagged)
    finally:
        L.damar_homog_result_free(C.byref(res_c))
        L.damar_dbinfo_close(C.byref(d))


def read_track(db, name, block=0):
    """A track as written: {"anno", "data"} and, for the .a2/.d2 form, the header's version, size and len.  The
    compressed form is tried first, like the loaders."""
    import numpy as np
    import struct
    import zlib
    d = os.path.dirname(os.path.abspath(db))
    root = os.path.basename(db)
    root = root[:-3] if root.endswith(".db") else root
    pre = os.path.join(d, ".%s.%s%s" % (root, "%d." % block if block > 0 else "", name))

    def inflate(buf):
        out, at = [], 0
        while at < len(buf):
            n = struct.unpack_from("<Q", buf, at)[0]
            out.append(zlib.decompress(buf[at + 8:at + 8 + n]))
            at += 8 + n
        return b"".join(out)
    if os.path.exists(pre + ".a2"):
        a = open(pre + ".a2", "rb").read()
        version, size, _pad, length, clen, cdlen = struct.unpack_from("<HHIQQQ", a, 0)
        dd = open(pre + ".d2", "rb").read()
        return dict(version=version, size=size, len=length, anno=np.frombuffer(inflate(a[64:64 + clen]), dtype="<u8"),
                    data=np.frombuffer(inflate(dd[:cdlen]), dtype="<i4"))
    a = open(pre + ".anno", "rb").read()
    length, size = struct.unpack_from("<ii", a, 0)
    return dict(len=length, size=size, anno=np.frombuffer(a[8:], dtype="<i8"), data=np.fromfile(pre + ".data", dtype="<i4"))


def daligner_binary():
    p = bin_path("daligner")
    if not os.path.exists(p):
        raise RuntimeError("%s not built" % p)
    return p


def lib():
    return _lib()


# ---- overlaps filtered per pile (LAfilter) ---------------------------------------------------------------------------

class FilterParams(C.Structure):       # include/damar_hip.h damar_filter_params
    _fields_ = [("steps", C.c_int), ("downsample", C.c_int), ("seg_rate", C.c_int), ("stitch", C.c_int), ("stitch_aggr", C.c_int),
                ("min_rlen", C.c_int), ("min_olen", C.c_int), ("max_unaligned", C.c_int), ("min_nonrep", C.c_int), ("max_diffs", C.c_float),
                ("merge_tips", C.c_int), ("multi", C.c_int), ("lowcov", C.c_int), ("remove", C.c_int), ("include", C.c_int),
                ("trim", _PI), ("rep_anno", C.POINTER(C.c_uint64)), ("rep_data", _PI), ("rep_ndata", c_int64),
                ("sym_off", _PI), ("sym_len", _PI), ("sym_data", _PI), ("sym_ndata", c_int64), ("read_state", C.POINTER(C.c_ubyte))]


class FilterOut(C.Structure):          # include/damar_hip.h damar_filter_out
    _fields_ = [(k, _PI) for k in ("flags", "aepos", "bepos", "diffs", "tlen", "reason", "cont_by", "cnt")]


class FilterOpts(C.Structure):         # host/damar_host.h damar_filter_opts
    _fields_ = [("p", FilterParams), ("verbose", C.c_int), ("purge", C.c_int), ("do_trim", C.c_int), ("trim_track", C.c_char_p),
                ("rep_track", C.c_char_p), ("exclude", C.c_char_p), ("include", C.c_char_p), ("discarded_out", C.c_char_p),
                ("discarded_in", C.c_char_p)]


FILTER_COUNTERS = ("diffs", "unaligned", "contained", "length", "repeat", "read_length", "low_coverage", "symmetric", "multi", "multi_bases",
                   "stitched")


class FilterStats(C.Structure):        # host/damar_host.h damar_filter_stats
    _fields_ = [("novl", c_int64), ("written", c_int64), ("discarded", c_int64), ("cnt", c_int64 * len(FILTER_COUNTERS)), ("piles", c_int64),
                ("host_piles", c_int64), ("trim", TrimStats)]


FILTER_PRE, FILTER_MAIN = 1, 2


def filter_limits():
    """(group, len): the records of one B read in a row and the bases of an A read (under -z with -u) a pile may have for
    kernels/pile_filter.hip to do it: DAMAR_FILTER_MAXGROUP, DAMAR_FILTER_MAXLEN"""
    g, n = C.c_int(), C.c_int()
    _lib().damar_filter_limits(C.byref(g), C.byref(n))
    return g.value, n.value


def filter_last():
    """Of the last pile_filter / of the last batch of filter_las: ({upload, kernel, download, call} ms, piles, piles the host
    routine did beside the kernel, records that left discarded)."""
    return _last("filter", 3)


def _filter_numbers(p, downsample=0, seg_rate=-1, stitch=-1, stitch_aggr=False, min_rlen=-1, min_olen=-1, max_unaligned=-1, min_nonrep=-1,
                    max_diffs=-1.0, merge_tips=0, multi=False, lowcov=0, remove=0):
    p.downsample, p.seg_rate, p.stitch, p.stitch_aggr = int(downsample), int(seg_rate), int(stitch), 1 if stitch_aggr else 0
    p.min_rlen, p.min_olen, p.max_unaligned, p.min_nonrep = int(min_rlen), int(min_olen), int(max_unaligned), int(min_nonrep)
    p.max_diffs, p.merge_tips, p.multi, p.lowcov, p.remove = float(max_diffs), int(merge_tips), 1 if multi else 0, int(lowcov), int(remove)


def pile_filter(batch, read_len, steps=FILTER_PRE | FILTER_MAIN, trim=None, repeats=None, sym=None, read_state=None, include=False, **numbers):
    """LAfilter's work on a batch of whole piles with their traces (the dict of _trace_batch, with `diffs`).  trim: get_trim
    of every read (2 * nreads ints) or None; repeats: (anno, data) of the repeat track, needed with min_nonrep; sym: (off,
    len, data) of the -A lists; read_state: 1 / 2 per read for -x / -I; numbers: the options of damar_filter_params by
    name.  -> dict of the per-record arrays flags, aepos, bepos, diffs, tlen, reason, cont_by, and cnt (npiles x counters).
    On the GPU unless DAMAR_PILES=host."""
    import numpy as np
    L = _lib()
    t, keep = _trace_batch(batch, read_len)
    p = FilterParams()
    _filter_numbers(p, **numbers)
    p.steps, p.include = int(steps), 1 if include else 0
    if trim is not None:
        keep["ftrim"] = np.ascontiguousarray(trim, dtype=np.int32)
        p.trim = keep["ftrim"].ctypes.data_as(_PI)
    if repeats is not None:
        keep["ranno"], keep["rdata"] = np.ascontiguousarray(repeats[0], dtype=np.uint64), np.ascontiguousarray(repeats[1], dtype=np.int32)
        p.rep_anno, p.rep_data, p.rep_ndata = keep["ranno"].ctypes.data_as(C.POINTER(C.c_uint64)), keep["rdata"].ctypes.data_as(_PI), len(keep["rdata"])
    if sym is not None:
        for k, v in zip(("soff", "slen", "sdata"), sym):
            keep[k] = np.ascontiguousarray(v, dtype=np.int32)
        p.sym_off, p.sym_len, p.sym_data = (keep[k].ctypes.data_as(_PI) for k in ("soff", "slen", "sdata"))
        p.sym_ndata = len(keep["sdata"])
    if read_state is not None:
        keep["state"] = np.ascontiguousarray(read_state, dtype=np.uint8)
        p.read_state = keep["state"].ctypes.data_as(C.POINTER(C.c_ubyte))
    diffs = np.ascontiguousarray(batch["diffs"], dtype=np.int32)
    nrec, npiles = int(t.p.nrec), int(t.p.npiles)
    names = ("flags", "aepos", "bepos", "diffs", "tlen", "reason", "cont_by")
    res = {k: np.zeros(max(nrec, 1), dtype=np.int32) for k in names}
    res["cnt"] = np.zeros(max(npiles, 1) * len(FILTER_COUNTERS), dtype=np.int32)
    out = FilterOut(*[res[k].ctypes.data_as(_PI) for k in names + ("cnt",)])
    L.damar_pile_filter.argtypes = [C.POINTER(TraceBatch), _PI, C.POINTER(FilterParams), C.POINTER(FilterOut)]
    if L.damar_pile_filter(C.byref(t), diffs.ctypes.data_as(_PI), C.byref(p), C.byref(out)):
        raise RuntimeError("damar_pile_filter failed")
    res = {k: v[:nrec] for k, v in res.items() if k != "cnt"} | {"cnt": res["cnt"][:npiles * len(FILTER_COUNTERS)].reshape(npiles, -1)}
    return res


def filter_las(db, las, out, *, verbose=False, purge=False, do_trim=False, trim="trim", repeats="repeats", exclude=None, include=None,
               discarded_out=None, discarded_in=None, **numbers):
    """LAfilter on one .las file, written to `out` (purge: without the discarded records).  trim / repeats: track names (-t
    -r), do_trim: -T, exclude / include: files of read ids (-x -I), discarded_out / discarded_in: the -a and -A files;
    numbers: the options of damar_filter_params by name (max_diffs as a fraction).  The reference's lines go to stdout.
    -> the counters of the run (host_piles: piles the host routine did beside the kernel)."""
    L = _lib()
    enc = lambda s: s.encode() if s is not None else None
    o = FilterOpts()
    _filter_numbers(o.p, **numbers)
    o.verbose, o.purge, o.do_trim = 1 if verbose else 0, 1 if purge else 0, 1 if do_trim else 0
    o.trim_track, o.rep_track, o.exclude, o.include = enc(trim), enc(repeats), enc(exclude), enc(include)
    o.discarded_out, o.discarded_in = enc(discarded_out), enc(discarded_in)
    st = FilterStats()
    L.damar_filter_las.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(FilterOpts), C.POINTER(FilterStats)]
    if L.damar_filter_las(db.encode(), las.encode(), out.encode(), C.byref(o), C.byref(st)):
        raise RuntimeError("damar_filter_las failed")
    res = {k: int(getattr(st, k)) for k in ("novl", "written", "discarded", "piles", "host_piles")}
    res.update(zip(FILTER_COUNTERS, (int(x) for x in st.cnt)))
    return res


# ---- reads corrected from the consensus of their tiles (LAcorrect) ----------------------------------------------------

class TileBatch(C.Structure):          # include/damar_hip.h damar_tile_batch
    _fields_ = [("ntiles", c_int64), ("ent_off", C.POINTER(c_int64)), ("seq_off", C.POINTER(c_int64)), ("seq_len", _PI),
                ("bases", C.POINTER(C.c_ubyte)), ("nbases", c_int64), ("weight", _PI)]


class CorrectOpts(C.Structure):        # host/damar_host.h damar_correct_opts
    _fields_ = [("verbose", C.c_int), ("nthreads", C.c_int), ("block", C.c_int), ("q_track", C.c_char_p), ("read_ids", C.c_char_p)]


class CorrectStats(C.Structure):       # host/damar_host.h damar_correct_stats
    _fields_ = [(k, c_int64) for k in ("reads", "copies", "tiles", "host_tiles", "bases")] + \
               [(k, C.c_double) for k in ("ms_consensus", "ms_kernel", "ms_postrace", "ms_postrace_wait", "ms_total")] + \
               [(k, c_int64) for k in ("postrace_boxes", "postrace_host")] + \
               [(k, C.c_double) for k in ("ms_postrace_kernel", "ms_postrace_call")]


def correct_limits():
    """(seg, cols, cells): the bases of one sequence, the profile columns and the wave cells a tile may need for
    kernels/tile_consensus.hip to do it: DAMAR_CORRECT_MAXSEG, DAMAR_CORRECT_MAXCOLS, DAMAR_CORRECT_CELLS"""
    v = [C.c_int() for _ in range(3)]
    _lib().damar_correct_limits(*[C.byref(x) for x in v])
    return tuple(x.value for x in v)


def correct_last():
    """Of the last tile_consensus / of the last batch of correct_las: ({upload, kernel, download, call} ms, tiles, tiles the
    host routine did beside the kernel, bases called)."""
    return _last("correct", 3)


def tile_consensus(tiles, weight=None):
    """The consensus of a batch of tiles: `tiles` is a list of tiles, a tile a list of at most 20 sequences (arrays of bases
    0..3; a complemented read's already turned), added in order as LAcorrect's single_tile_consensus adds them.
    -> (list of the tiles' called bases as uint8 arrays, array of the sequences each tile took).  On the GPU unless
    DAMAR_PILES=host."""
    import numpy as np
    L = _lib()
    seqs = [np.ascontiguousarray(s, dtype=np.uint8) for t in tiles for s in t]
    ent_off = np.zeros(len(tiles) + 1, dtype=np.int64)
    ent_off[1:] = np.cumsum([len(t) for t in tiles])
    seq_len = np.array([len(s) for s in seqs] + [0], dtype=np.int32)
    seq_off = np.zeros(len(seqs) + 1, dtype=np.int64)
    seq_off[1:] = np.cumsum(seq_len[:len(seqs)])
    bases = np.concatenate(seqs + [np.zeros(1, dtype=np.uint8)])
    b = TileBatch(len(tiles), ent_off.ctypes.data_as(C.POINTER(c_int64)), seq_off.ctypes.data_as(C.POINTER(c_int64)),
                  seq_len.ctypes.data_as(_PI), bases.ctypes.data_as(C.POINTER(C.c_ubyte)), int(seq_off[len(seqs)]), None)
    if weight is not None:
        w = np.ascontiguousarray(weight, dtype=np.int32)
        b.weight = w.ctypes.data_as(_PI)
    cons_off = np.zeros(len(tiles) + 1, dtype=np.int64)
    added = np.zeros(max(len(tiles), 1), dtype=np.int32)
    cons = C.POINTER(C.c_ubyte)()
    L.damar_tile_consensus.argtypes = [C.POINTER(TileBatch), C.POINTER(c_int64), C.POINTER(C.POINTER(C.c_ubyte)), _PI]
    if L.damar_tile_consensus(C.byref(b), cons_off.ctypes.data_as(C.POINTER(c_int64)), C.byref(cons), added.ctypes.data_as(_PI)):
        raise RuntimeError("damar_tile_consensus failed")
    flat = np.ctypeslib.as_array(cons, shape=(max(int(cons_off[-1]), 1),))[:int(cons_off[-1])].copy()
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    libc.free(C.cast(cons, C.c_void_p))
    return [flat[cons_off[i]:cons_off[i + 1]] for i in range(len(tiles))], added[:len(tiles)]


def correct_las(db, las, out, *, verbose=False, parts=1, block=-1, q="q", read_ids=None):
    """LAcorrect on one .las file: the corrected reads written to <out>.NN.fasta, one file per part (-j).  q: the quality
    track's name (-q), read_ids: a file of read numbers (-r), block: -b.  The reference's lines go to stdout.
    -> the counters and timings of the run (host_tiles: tiles the host routine did beside the kernel)."""
    L = _lib()
    o = CorrectOpts(1 if verbose else 0, int(parts), int(block), q.encode(), read_ids.encode() if read_ids is not None else None)
    st = CorrectStats()
    L.damar_correct_las.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(CorrectOpts), C.POINTER(CorrectStats)]
    if L.damar_correct_las(db.encode(), las.encode(), out.encode(), C.byref(o), C.byref(st)):
        raise RuntimeError("damar_correct_las failed")
    return {k: getattr(st, k) for k, _ in CorrectStats._fields_}


# ---- the low-complexity mask of reads (DBdust) --------------------------------------------------------------------

class DustParams(C.Structure):         # include/damar_hip.h damar_dust_params
    _fields_ = [("window", C.c_int), ("thresh", C.c_double), ("minlen", C.c_int), ("biased", C.c_int), ("freq", C.c_float * 4)]


class DustList(C.Structure):           # host/damar_host.h damar_dust_list
    _fields_ = [("iv", _PI), ("n", c_int64), ("cap", c_int64)]


def _dust_params(window, thresh, minlen, biased, freq):
    p = DustParams(int(window), float(thresh), int(minlen), 1 if biased else 0)
    if biased:
        if freq is None:
            raise ValueError("biased needs the four base frequencies")
        for i in range(4):
            p.freq[i] = freq[i]
    return p


def dust_limits():
    """(piece, halo, stripe, window): the triplet starts of a piece, the triplets run in front of it, the candidates a piece
    may retire and the widest window of kernels/dust.hip: DAMAR_DUST_PIECE, _HALO, _STRIPE, _MAXWINDOW"""
    v = [C.c_int() for _ in range(4)]
    L = _lib()
    L.damar_dust_limits.argtypes = [_PI] * 4
    L.damar_dust_limits(*[C.byref(x) for x in v])
    return tuple(x.value for x in v)


def dust_last():
    """Of the last dust_reads / of the last batch of dust_track: ({upload, kernel, download, call} ms, reads, reads the host
    routine did beside the kernel, intervals, steps taken, steps that entered the walk over the window's starts)."""
    st = (c_int64 * 2)()
    L = _lib()
    L.damar_dust_steps.argtypes = [C.POINTER(c_int64)]
    L.damar_dust_steps(st)
    return _last("dust", 3) + (st[0], st[1])


def dust_reads(seqs, window=64, thresh=2.0, minlen=10, biased=False, freq=None):
    """DBdust's mask of each read of `seqs` (arrays of bases 0..3): -> a list of int32 arrays [n, 2] of [beg, end) pairs.
    On the GPU (kernels/dust.hip) unless DAMAR_DUST=host; biased reads and windows the kernel does not hold go to the host
    routine and are counted (dust_last)."""
    import numpy as np
    L = _lib()
    p = _dust_params(window, thresh, minlen, biased, freq)
    arrs = [np.ascontiguousarray(s, dtype=np.uint8) for s in seqs]
    off = np.zeros(len(arrs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(s) for s in arrs])
    bases = np.concatenate(arrs + [np.zeros(1, dtype=np.uint8)])
    out_off = np.zeros(len(arrs) + 1, dtype=np.int64)
    out = _PI()
    L.damar_dust_reads.argtypes = [C.POINTER(C.c_ubyte), C.POINTER(c_int64), c_int64, C.POINTER(DustParams), C.POINTER(c_int64),
                                   C.POINTER(_PI)]
    if L.damar_dust_reads(bases.ctypes.data_as(C.POINTER(C.c_ubyte)), off.ctypes.data_as(C.POINTER(c_int64)), len(arrs), C.byref(p),
                          out_off.ctypes.data_as(C.POINTER(c_int64)), C.byref(out)):
        raise RuntimeError("damar_dust_reads failed")
    n = int(out_off[-1])
    flat = np.ctypeslib.as_array(out, shape=(max(n, 1),))[:n].copy()
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    libc.free(C.cast(out, C.c_void_p))
    return [flat[out_off[i]:out_off[i + 1]].reshape(-1, 2) for i in range(len(arrs))]


def dust_host_read(seq, window=64, thresh=2.0, minlen=10, biased=False, freq=None, piece=0, halo=0):
    """One read through the routine of host/dust.c alone: whole (piece = 0), or cut into pieces of `piece` triplet starts with
    `halo` triplets run in front of each.  -> (int32 [n, 2] of [beg, end) pairs, the longest the candidate list became
    -- of the whole read only, else 0)."""
    import numpy as np
    L = _lib()
    p = _dust_params(window, thresh, minlen, biased, freq)
    s = np.ascontiguousarray(seq, dtype=np.uint8)
    s = np.concatenate([s, np.zeros(4, dtype=np.uint8)])
    n = len(s) - 4
    out = np.zeros(2 * max(n, 1), dtype=np.int32)
    work = DustList()
    L.damar_host_dust_read.argtypes = [C.POINTER(C.c_ubyte), C.c_int, C.POINTER(DustParams), C.c_int, C.c_int, _PI, C.POINTER(DustList),
                                       C.POINTER(c_int64)]
    L.damar_host_dust_read.restype = c_int64
    L.damar_host_dust_piece.argtypes = [C.POINTER(C.c_ubyte), C.c_int, C.POINTER(DustParams), C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.POINTER(DustList), C.POINTER(c_int64)]
    sp = s.ctypes.data_as(C.POINTER(C.c_ubyte))
    m = L.damar_host_dust_read(sp, n, C.byref(p), int(piece), int(halo), out.ctypes.data_as(_PI), C.byref(work), None)
    longest = 0
    if piece <= 0 and n > 2:
        work.n = 0
        longest = L.damar_host_dust_piece(sp, n, C.byref(p), 0, 0, n - 2, n - 2, C.byref(work), None)
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    libc.free(C.cast(work.iv, C.c_void_p))
    return out[:2 * m].reshape(-1, 2).copy(), longest


def dust_host_candidates(seq, window=64, thresh=2.0, start=0, own=None, stop=None):
    """The candidates the routine of host/dust.c retires over the triplets [start, stop) of one read, those that start in
    own = (beg, end): -> (int32 [n, 2] of (start, last triplet), the longest the candidate list became)."""
    import numpy as np
    L = _lib()
    p = _dust_params(window, thresh, 2, False, None)
    s = np.concatenate([np.ascontiguousarray(seq, dtype=np.uint8), np.zeros(4, dtype=np.uint8)])
    n = len(s) - 4
    own = (0, n) if own is None else own
    work = DustList()
    L.damar_host_dust_piece.argtypes = [C.POINTER(C.c_ubyte), C.c_int, C.POINTER(DustParams), C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.POINTER(DustList), C.POINTER(c_int64)]
    longest = L.damar_host_dust_piece(s.ctypes.data_as(C.POINTER(C.c_ubyte)), n, C.byref(p), int(start), int(own[0]), int(own[1]),
                                      int(n if stop is None else stop), C.byref(work), None)
    out = np.ctypeslib.as_array(work.iv, shape=(max(2 * work.n, 1),))[:2 * work.n].copy().reshape(-1, 2) if work.n else \
        np.zeros((0, 2), dtype=np.int32)
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    libc.free(C.cast(work.iv, C.c_void_p))
    return out, longest


def dust_track(db, window=64, thresh=2.0, minlen=10, biased=False):
    """DBdust on a database or one of its blocks: .dust.anno / .dust.data written beside it (appended to for a whole database
    that has them).  -> {reads, host_reads, intervals, bases, steps, walk_steps} of the run."""
    L = _lib()
    p = _dust_params(window, thresh, minlen, False, None)
    p.biased = 1 if biased else 0
    st = (c_int64 * 6)()
    L.damar_dust_track.argtypes = [C.c_char_p, C.POINTER(DustParams), C.POINTER(c_int64)]
    if L.damar_dust_track(db.encode(), C.byref(p), st):
        raise RuntimeError("damar_dust_track failed")
    return dict(zip(("reads", "host_reads", "intervals", "bases", "steps", "walk_steps"), list(st)))


# ---- the overlap graph of a filtered file (OGbuild) ------------------------------------------------------------------

class GraphResult(C.Structure):         # include/damar_graph.h damar_graph_result
    _fields_ = [("nreads", C.c_int), ("loff", C.POINTER(c_int64)), ("roff", C.POINTER(c_int64)), ("left", _PI), ("right", _PI),
                ("status", C.POINTER(C.c_ubyte)), ("cnt_left", c_int64), ("cnt_right", c_int64), ("edges", c_int64), ("redges", c_int64),
                ("symdiscard", c_int64), ("parallel", c_int64), ("removed", c_int64), ("neg_rec", c_int64), ("nneg", c_int64),
                ("neg", C.POINTER(c_int64))]


class OgOpts(C.Structure):              # include/damar_graph.h damar_og_opts
    _fields_ = [("split", C.c_int), ("contained", C.c_int), ("track", C.c_char_p), ("format", C.c_char_p), ("prio", C.c_char_p)]


OG_EDGE_INTS = 9                        # a b ab ae bb be flags ovh diffs


def og_build(db, las, out, split=False, contained=0, trim="trim", fmt="graphml", prio="ovl"):
    """OGbuild on one filtered .las file: the overlap graph written to `out` (split: one file per component), the reference's
    lines on stdout.  -> its exit status."""
    L = _lib()
    L.damar_og_build.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(OgOpts)]
    o = OgOpts(1 if split else 0, int(contained), trim.encode(), fmt.encode(), prio.encode())
    return int(L.damar_og_build(db.encode(), las.encode(), out.encode(), C.byref(o)))


def og_edges(db, las, trim="trim"):
    """The edges OGbuild makes of a file before -c: dict of loff, roff (int64[nreads + 1]), left, right (int32[n, 9]: a b ab ae
    bb be flags ovh diffs), status (uint8[nreads]) and the counters of the run."""
    import numpy as np
    L = _lib()
    L.damar_og_edges.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(GraphResult)]
    L.damar_graph_result_free.argtypes = [C.POINTER(GraphResult)]
    r = GraphResult()
    if L.damar_og_edges(db.encode(), las.encode(), trim.encode(), C.byref(r)):
        raise RuntimeError("damar_og_edges failed")
    try:
        n = r.nreads
        out = dict(loff=np.ctypeslib.as_array(r.loff, shape=(n + 1,)).copy(), roff=np.ctypeslib.as_array(r.roff, shape=(n + 1,)).copy(),
                   status=np.ctypeslib.as_array(r.status, shape=(n,)).copy())
        for k, off in (("left", out["loff"]), ("right", out["roff"])):
            m = int(off[n])
            out[k] = (np.ctypeslib.as_array(getattr(r, k), shape=(max(m, 1) * OG_EDGE_INTS,))[:m * OG_EDGE_INTS].copy().reshape(m, OG_EDGE_INTS))
        for k in ("cnt_left", "cnt_right", "edges", "redges", "symdiscard", "parallel", "removed", "neg_rec"):
            out[k] = int(getattr(r, k))
        return out
    finally:
        L.damar_graph_result_free(C.byref(r))


def og_last():
    """Of the last OGbuild session, summed over its batches: ({upload, piles, finish, download} ms, records, candidate edges,
    reads the host routine finished beside the kernel, edges kept)."""
    return _last("graph", 4, ("upload", "piles", "finish", "download"))
