"""ctypes binding of the C ABI declared in include/nanorepeat_amd.h.

There is no CPU path: if libnanorepeat_amd.so is missing, or no HIP device is visible,
the compute entry points raise.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libnanorepeat_amd.so")
_LIB = None

READ_OK, READ_FALLBACK, READ_NO_RECORD, READ_SKIPPED = 0, 1, 2, 3
F_ALL_EXTENTS = 1     # explicit extents DP for every candidate (brute force)
F_TIE_EXTENTS = 2     # explicit extents DP for every top-score tie (fills cand_tstart/cand_tend)
F_BRUTE_FORCE = 4     # K independent alignments per read instead of the junction decomposition
F_TEST_CHAIN = 8      # testing only: every read in chained 128-row blocks
F_DPP_SWEEP = 16      # testing / comparison: k_sweep_pk16 instead of k_sweep_ring for unchained reads
F_NO_HALF_WAVE = 32   # testing / comparison: one read pair per wave also for reads of up to 768 bases
F_NO_JOINT_PACK = 64  # testing / comparison, 2D: int32 payload cells also outside the scoring window
F_JOINT_TAILS = 256   # testing / comparison, 2D routed grids: tail sweeps (junction at R[0]) instead of the junction at the end of mid
F_JOINT_NO_KEEP = 1024  # testing / comparison, 2D routed grids: a finer grid sweeps its reads again instead of using the column states kept from the coarse one
F_JOINT_NO_CHAIN = 512  # testing / comparison, 2D routed grids: the MID part as one systolic sweep per (read, k1) instead of column-parallel scans
F_NO_QUANTA = 2048    # testing / comparison, 1D: reverse and forward sweeps as two launches instead of one launch of quanta taken by ticket
F_QUANTA_2L = 4096    # accepted and ignored (round 4's first form of the quanta as two launches)
F_SERIAL_CHAIN = 128  # testing / comparison, 1D: a long read's row blocks one after the other in one wave
MIX_STREAM = 1        # testing / comparison, nra_mixture_fit: every problem streams its points from memory
CENS_F_STREAM = 1     # testing / comparison, nra_censored_fit: every problem streams its values from memory
MIX_ONE_CLASS = 2     # testing / comparison, nra_mixture_fit: no separate kernel for problems of up to 1024 points
F_FULL_ANCHORS = 8192  # testing / comparison, 1D: the exact cell over every anchor column (no relaxed cells, no re-sweep)

# every symbol include/nanorepeat_amd.h declares
EXPORTS = ("nra_abi_version", "nra_version", "nra_last_error", "nra_device_count",
           "nra_default_scoring", "nra_release_cached_memory", "nra_round3_1d", "nra_joint_2d", "nra_align_pairs", "nra_align_pairs_cigar", "nra_align_paths", "nra_batch1d_create",
           "nra_batch2d_create", "nra_batch2d_create_reads", "nra_batch2d_set_cells", "nra_joint_grid_cells", "nra_batch2d_set_grid", "nra_batch2d_invalidate", "nra_batch2d_sweep_flanks", "nra_batch2d_refine", "nra_batch_run", "nra_batch_sync", "nra_batch_stats",
           "nra_batch1d_fetch", "nra_batch1d_resweeps", "nra_batch1d_saturation", "nra_batch1d_clears", "nra_plan1d_digest", "nra_plan2d_digest", "nra_batch2d_fetch", "nra_batch_destroy",
           "nra_screen_create", "nra_screen_reads", "nra_screen_stats", "nra_screen_destroy",
           "nra_screen_set_motifs", "nra_screen_reads_partial",
           "nra_read_structure", "nra_tract_motifs", "nra_extend_tracts", "nra_mixture_fit", "nra_mixture_bootstrap",
           "nra_tract_consensus", "nra_allele_split", "nra_flank_phase", "nra_tract_segments", "nra_tract_periods",
           "nra_censored_fit", "nra_censored_posteriors", "nra_censored_bootstrap", "nra_read_methylation",
           "nra_scan_repeats", "nra_sketch_pairs",
           "nra_place_create", "nra_place_scan", "nra_place_candidates", "nra_place_stats", "nra_place_destroy")


E_RANGE = -3      # NRA_E_RANGE
E_STATE = -5      # NRA_E_STATE


class NraError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"nanorepeat_amd error {code}: {msg}")
        self.code = code


class Scoring(C.Structure):
    _fields_ = [(n, C.c_int32) for n in
                ("match", "mismatch", "gap_open1", "gap_ext1", "gap_open2", "gap_ext2",
                 "sc_ambi", "min_dp_score")]


class Region(C.Structure):
    _fields_ = [("left", C.c_char_p), ("unit", C.c_char_p), ("right", C.c_char_p),
                ("left_len", C.c_int32), ("unit_len", C.c_int32), ("right_len", C.c_int32)]


class JointRegion(C.Structure):
    _fields_ = [("left", C.c_char_p), ("unit1", C.c_char_p), ("mid", C.c_char_p),
                ("unit2", C.c_char_p), ("right", C.c_char_p),
                ("left_len", C.c_int32), ("unit1_len", C.c_int32), ("mid_len", C.c_int32),
                ("unit2_len", C.c_int32), ("right_len", C.c_int32)]


class Plan2DStep(C.Structure):
    _fields_ = [("kind", C.c_int32), ("read_strand", C.POINTER(C.c_int8)), ("n_cells", C.c_int64),
                ("cell_read", C.POINTER(C.c_int32)), ("cell_k1", C.POINTER(C.c_int32)), ("cell_k2", C.POINTER(C.c_int32)),
                ("start1", C.c_int32), ("step1", C.c_int32), ("count1", C.c_int32),
                ("start2", C.c_int32), ("step2", C.c_int32), ("count2", C.c_int32),
                ("lo1", C.POINTER(C.c_double)), ("hi1", C.POINTER(C.c_double)),
                ("lo2", C.POINTER(C.c_double)), ("hi2", C.POINTER(C.c_double)),
                ("buf1", C.c_int32), ("buf2", C.c_int32), ("keep_budget", C.c_int64), ("device_free", C.c_int64)]


class Stats(C.Structure):
    _fields_ = [("n_alignments", C.c_int64), ("algorithmic_cells", C.c_int64),
                ("executed_cells", C.c_int64), ("algorithmic_bytes", C.c_int64),
                ("n_extent_tasks", C.c_int64), ("score_kernel_ms", C.c_double),
                ("extent_kernel_ms", C.c_double), ("total_ms", C.c_double),
                ("n_score_launches", C.c_int32), ("n_runs", C.c_int32),
                ("score_phase_ms", C.c_double),
                ("sum_score_kernel_ms", C.c_double), ("sum_extent_kernel_ms", C.c_double),
                ("sum_total_ms", C.c_double), ("sum_score_phase_ms", C.c_double),
                ("intermediate_bytes", C.c_int64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class ScreenStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_keys", "n_postings", "n_masked_periodic", "n_masked_max_occ",
                                         "n_empty_regions", "index_bytes", "bases_screened", "n_calls")] + \
               [(n, C.c_double) for n in ("build_ms", "kernel_ms", "sum_kernel_ms")] + \
               [("n_classes", C.c_int64), ("motif_kernel_ms", C.c_double), ("sum_motif_kernel_ms", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class ScanStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_windows", "n_periodic", "n_segments", "n_chunks")] + \
               [("kernel_ms", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class SketchStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_windows", "n_kmers", "n_compared", "n_tiles")] + \
               [(n, C.c_double) for n in ("kernel_ms", "sketch_ms", "pairs_ms", "upload_ms", "sort_ms")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class PlaceStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_keys", "n_postings", "n_masked_periodic", "n_masked_max_occ", "index_bytes",
                                         "target_bases", "n_target_windows", "n_hits_kept", "n_keys_over", "n_chunks",
                                         "tile_windows")] + \
               [(n, C.c_double) for n in ("build_ms", "kernel_ms", "upload_ms", "reduce_ms")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


def load():
    """Load the shared library (raises if it has not been built)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python -m nanorepeat_amd.build` "
            "(hipcc --offload-arch=gfx950).  nanorepeat_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    p8 = C.POINTER(C.c_uint8)
    pi8 = C.POINTER(C.c_int8)
    pi32 = C.POINTER(C.c_int32)
    pi64 = C.POINTER(C.c_int64)
    vp = C.c_void_p
    lib.nra_abi_version.restype = C.c_int
    lib.nra_version.restype = C.c_char_p
    lib.nra_last_error.restype = C.c_char_p
    lib.nra_device_count.restype = C.c_int
    lib.nra_default_scoring.argtypes = [C.POINTER(Scoring)]
    lib.nra_release_cached_memory.restype = C.c_int
    lib.nra_release_cached_memory.argtypes = [C.c_int]
    lib.nra_round3_1d.restype = C.c_int
    lib.nra_round3_1d.argtypes = [C.c_int, C.POINTER(Region), C.c_int32, C.c_int32, C.c_char_p, pi64,
                                  pi32, pi32, pi32, C.POINTER(Scoring), C.c_int32,
                                  pi32, pi64, pi32, p8, pi32, pi32, pi32]
    lib.nra_joint_2d.restype = C.c_int
    lib.nra_joint_2d.argtypes = [C.c_int, C.POINTER(JointRegion), C.c_int32, C.c_char_p, pi64, pi8,
                                 C.c_int64, pi32, pi32, pi32, C.POINTER(Scoring), C.c_int32,
                                 pi32, pi32, pi32, pi64, pi64, pi32, p8]
    lib.nra_align_pairs.restype = C.c_int
    lib.nra_align_pairs.argtypes = [C.c_int, C.c_int32, C.c_char_p, pi64, C.c_int64, pi32, pi32,
                                    C.POINTER(Scoring), C.c_int32, pi32, pi32, pi32]
    lib.nra_align_pairs_cigar.restype = C.c_int
    lib.nra_align_pairs_cigar.argtypes = [C.c_int, C.c_int32, C.c_char_p, pi64, C.c_int64, pi32, pi32,
                                          C.POINTER(Scoring), C.c_int32, pi32, pi32, pi32, pi32, pi32,
                                          C.c_char_p, C.c_int64, pi64]
    lib.nra_align_paths.restype = C.c_int
    lib.nra_align_paths.argtypes = lib.nra_align_pairs_cigar.argtypes
    lib.nra_batch1d_create.restype = C.c_int
    lib.nra_batch1d_create.argtypes = [C.c_int, C.POINTER(Region), C.c_int32, C.c_int32, C.c_char_p,
                                       pi64, pi32, pi32, pi32, C.POINTER(Scoring), C.c_int32,
                                       C.POINTER(vp)]
    lib.nra_batch2d_create.restype = C.c_int
    lib.nra_batch2d_create.argtypes = [C.c_int, C.POINTER(JointRegion), C.c_int32, C.c_char_p, pi64,
                                       pi8, C.c_int64, pi32, pi32, pi32, C.POINTER(Scoring),
                                       C.c_int32, C.POINTER(vp)]
    lib.nra_batch2d_create_reads.restype = C.c_int
    lib.nra_batch2d_create_reads.argtypes = [C.c_int, C.POINTER(JointRegion), C.c_int32, C.c_char_p, pi64,
                                             C.POINTER(Scoring), C.c_int32, C.POINTER(vp)]
    lib.nra_batch2d_set_cells.restype = C.c_int
    lib.nra_batch2d_set_cells.argtypes = [vp, pi8, C.c_int64, pi32, pi32, pi32]
    pf64 = C.POINTER(C.c_double)
    grid_args = [C.c_int32, C.c_int32, C.c_int32, pf64, pf64, C.c_int32, C.c_int32, C.c_int32, pf64, pf64]
    lib.nra_joint_grid_cells.restype = C.c_int64
    lib.nra_joint_grid_cells.argtypes = [C.c_int32] + grid_args + [C.c_int64, pi32, pi32, pi32]
    lib.nra_batch2d_set_grid.restype = C.c_int
    lib.nra_batch2d_set_grid.argtypes = [vp, pi8] + grid_args + [pi64]
    lib.nra_batch2d_sweep_flanks.restype = C.c_int
    lib.nra_batch2d_sweep_flanks.argtypes = [vp, pi8]
    lib.nra_batch2d_refine.restype = C.c_int
    lib.nra_batch2d_refine.argtypes = [vp, C.c_int32, C.c_int32, pf64, pf64, pf64, pf64]
    for f in (lib.nra_batch_run, lib.nra_batch_sync, lib.nra_batch2d_invalidate):
        f.restype = C.c_int
        f.argtypes = [vp]
    lib.nra_batch_stats.restype = C.c_int
    lib.nra_batch_stats.argtypes = [vp, C.POINTER(Stats)]
    lib.nra_batch1d_fetch.restype = C.c_int
    lib.nra_batch1d_resweeps.restype = C.c_int
    lib.nra_batch1d_resweeps.argtypes = [vp, pi64, pi64, pi64, pi64]
    lib.nra_batch1d_saturation.restype = C.c_int
    lib.nra_batch1d_saturation.argtypes = [vp, pi64, pi64, pi64, pi64]
    lib.nra_batch1d_clears.restype = C.c_int
    lib.nra_batch1d_clears.argtypes = [vp, pi32, pi32]
    lib.nra_plan1d_digest.restype = C.c_int64
    lib.nra_plan1d_digest.argtypes = lib.nra_batch1d_create.argtypes[1:-1] + [C.c_int32, C.c_char_p, C.c_int64]
    lib.nra_plan2d_digest.restype = C.c_int64
    lib.nra_plan2d_digest.argtypes = [C.POINTER(JointRegion), C.c_int32, C.c_char_p, pi64, C.POINTER(Scoring), C.c_int32,
                                      C.POINTER(Plan2DStep), C.c_int32, C.c_char_p, C.c_int64]
    lib.nra_batch1d_fetch.argtypes = [vp, pi32, pi64, pi32, p8, pi32, pi32, pi32]
    lib.nra_batch2d_fetch.restype = C.c_int
    lib.nra_batch2d_fetch.argtypes = [vp, pi8, pi32, pi32, pi32, pi64, pi64, pi32, p8]
    lib.nra_batch_destroy.restype = None
    lib.nra_batch_destroy.argtypes = [vp]
    lib.nra_screen_create.restype = C.c_int
    lib.nra_screen_create.argtypes = [C.c_int, C.c_int32, C.c_char_p, pi64, C.c_int32, C.c_int32, C.POINTER(vp)]
    lib.nra_screen_reads.restype = C.c_int
    lib.nra_screen_reads.argtypes = [vp, C.c_int32, C.c_char_p, pi64, C.c_int32, pi64, pi32, pi32, pi32, pi32]
    lib.nra_screen_set_motifs.restype = C.c_int
    lib.nra_screen_set_motifs.argtypes = [vp, C.c_int32, C.c_char_p, pi64]
    lib.nra_screen_reads_partial.restype = C.c_int
    lib.nra_screen_reads_partial.argtypes = [vp, C.c_int32, C.c_char_p, pi64, C.c_int32, C.c_int32, pi64, pi32, pi32,
                                             pi32, pi32, pi32, p8]
    lib.nra_screen_stats.restype = C.c_int
    lib.nra_screen_stats.argtypes = [vp, C.POINTER(ScreenStats)]
    lib.nra_screen_destroy.restype = C.c_int
    lib.nra_screen_destroy.argtypes = [vp]
    lib.nra_read_structure.restype = C.c_int
    lib.nra_read_structure.argtypes = [C.c_int, C.c_int32, C.c_char_p, pi64, C.c_int32, C.c_char_p, pi64, pi32,
                                       pi32, pi32, p8]
    lib.nra_tract_motifs.restype = C.c_int
    lib.nra_tract_motifs.argtypes = [C.c_int, C.c_int32, C.c_char_p, pi64, C.c_int32, C.c_int32, pi32,
                                     C.POINTER(C.c_int8), pi32, pi32]
    lib.nra_extend_tracts.restype = C.c_int
    lib.nra_extend_tracts.argtypes = [C.c_int, C.c_int32, C.c_char_p, pi64, C.c_int32, C.c_char_p, pi64, pi32,
                                      C.c_int32, C.c_int32, C.c_int32, pi32, pi32, pi32, pi32]
    lib.nra_mixture_bootstrap.restype = C.c_int
    lib.nra_mixture_bootstrap.argtypes = [C.c_int, C.c_int64, pf64, C.c_int64, pf64, C.c_int32, pi32, pi32, pi64, pi64,
                                          pf64, pf64, pi32, pi32, pi32, pi64, C.c_int64, pi32, C.c_int32, pi32,
                                          C.c_int32, pi32, pi32, pi32, pf64, pf64, pf64, pf64]
    lib.nra_mixture_fit.restype = C.c_int
    lib.nra_mixture_fit.argtypes = [C.c_int, C.c_int64, pf64, C.c_int32, pi64, pi32, pi32, C.c_int32, pi32, pi32, pi32,
                                    C.c_int32, pf64, pf64, pf64, pf64, pi32, pi32]
    lib.nra_censored_fit.restype = C.c_int
    lib.nra_censored_fit.argtypes = [C.c_int, C.c_int64, pf64, C.c_int32, pi64, pi32, pi32, pf64, C.c_int32, pi32, pi32,
                                     pi32, pf64, C.c_int32, C.c_double, C.c_int32, pf64, pf64, pf64, pi32, pi32]
    lib.nra_censored_posteriors.restype = C.c_int
    lib.nra_censored_posteriors.argtypes = [C.c_int, C.c_int64, pf64, C.c_int32, pi64, pi32, pi32, pf64, pi32, pi32,
                                            pf64, pf64, C.c_int64, pf64]
    lib.nra_censored_bootstrap.restype = C.c_int
    lib.nra_censored_bootstrap.argtypes = [C.c_int, C.c_int64, pf64, C.c_int32, pi64, pi32, pi32, pf64, pf64, C.c_int32,
                                           pi32, pi32, C.c_int32, C.c_int32, C.c_double, C.c_int32, pi32, pi32, pi32,
                                           pi32, pi32, pf64, pf64, pf64, pf64]
    lib.nra_allele_split.restype = C.c_int
    lib.nra_allele_split.argtypes = [C.c_int, C.c_int32, pi64, C.c_int32, C.c_char_p, pi64, C.c_char_p, pi64] + \
                                    [C.c_int32] * 7 + [pi32, pi32, pi32, C.c_int64, pi32, pi64, C.c_int64, p8, pi64, pi64]
    lib.nra_flank_phase.restype = C.c_int
    lib.nra_flank_phase.argtypes = [C.c_int, C.c_int32, pi64, C.c_int32, C.c_char_p, pi64, C.c_char_p, pi64] + \
                                   [C.c_int32] * 8 + [pi32, pi32, pi32, pi32, C.c_int64, pi32, pi64, C.c_int64, p8, pi64,
                                                      pi64]
    lib.nra_tract_consensus.restype = C.c_int
    lib.nra_tract_consensus.argtypes = [C.c_int, C.c_int32, pi64, C.c_int32, C.c_char_p, pi64, C.c_int32, C.c_int32,
                                        C.c_int64, C.c_char_p, pi32, pi64, pi32, pi64]
    lib.nra_tract_segments.restype = C.c_int
    lib.nra_tract_segments.argtypes = [C.c_int, C.c_int32, pi32, C.c_char_p, pi64, C.c_int32, C.c_char_p, pi64, pi32,
                                       C.c_int32, pi32, pi32, pi32, p8, p8]
    lib.nra_read_methylation.restype = C.c_int
    lib.nra_read_methylation.argtypes = [C.c_int, C.c_int32, C.c_char_p, pi64, pi32, p8, pi64, p8, pi32, pi32,
                                         C.c_int32, C.c_int32, C.c_int32, C.c_int32, pi32, pi32, pi32]
    lib.nra_scan_repeats.restype = C.c_int
    lib.nra_scan_repeats.argtypes = [C.c_int, C.c_int32, C.c_char_p, pi64, C.c_int32, C.c_int32, C.c_int32, pi64,
                                     pi32, pi32, pi32, pi32, pi32, pi32, C.POINTER(ScanStats)]
    lib.nra_sketch_pairs.restype = C.c_int
    lib.nra_sketch_pairs.argtypes = [C.c_int, C.c_int32, C.c_char_p, pi64, pi32, C.c_int32, C.c_int32, pi64, pi32, pi32,
                                     pi32, pi32, C.POINTER(SketchStats)]
    lib.nra_place_create.restype = C.c_int
    lib.nra_place_create.argtypes = [C.c_int, C.c_int32, C.c_char_p, pi64, C.c_int32, C.c_int32, C.POINTER(vp)]
    lib.nra_place_scan.restype = C.c_int
    lib.nra_place_scan.argtypes = [vp, C.c_int32, C.c_int64, C.c_char_p, C.c_int64]
    lib.nra_place_candidates.restype = C.c_int
    lib.nra_place_candidates.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, pi64, pi32, pi32, pi32, pi32, pi32]
    lib.nra_place_stats.restype = C.c_int
    lib.nra_place_stats.argtypes = [vp, C.POINTER(PlaceStats)]
    lib.nra_place_destroy.restype = C.c_int
    lib.nra_place_destroy.argtypes = [vp]
    lib.nra_tract_periods.restype = C.c_int
    lib.nra_tract_periods.argtypes = [C.c_int, C.c_int32, C.c_char_p, pi64, C.c_int32, pi32, pi32]
    _LIB = lib
    return lib


def _check(rc):
    if rc != 0:
        raise NraError(rc, load().nra_last_error().decode(errors="replace"))


def default_scoring(**over):
    sc = Scoring()
    load().nra_default_scoring(C.byref(sc))
    for k, v in over.items():
        setattr(sc, k, v)
    return sc


def device_count():
    n = load().nra_device_count()
    if n < 0:
        raise NraError(n, load().nra_last_error().decode(errors="replace"))
    return n


def release_cached_memory(device=-1):
    """Give the library's cached device chunks and pinned buffers back to the runtime (all devices by default)."""
    _check(load().nra_release_cached_memory(device))


def _ptr(a, ty):
    return None if a is None else a.ctypes.data_as(C.POINTER(ty))


def pack_reads(reads):
    """Concatenated sequence bytes + offsets.  All-str input (the usual case) is joined once and encoded once."""
    n = len(reads)
    off = np.zeros(n + 1, dtype=np.int64)
    if n == 0:
        return b"", off
    if all(type(r) is str for r in reads):
        blob = "".join(reads)
        if blob.isascii():                      # one byte per character: lengths carry over
            np.cumsum(np.fromiter(map(len, reads), np.int64, n), out=off[1:])
            return blob.encode("ascii"), off
    bs = [r.encode() if isinstance(r, str) else bytes(r) for r in reads]
    off[1:] = np.cumsum([len(b) for b in bs])
    return b"".join(bs), off


def _regions(regions):
    arr = (Region * max(len(regions), 1))()
    keep = []
    for i, (l, u, r) in enumerate(regions):
        lb, ub, rb = l.encode(), u.encode(), r.encode()
        keep += [lb, ub, rb]
        arr[i] = Region(lb, ub, rb, len(lb), len(ub), len(rb))
    return arr, keep


def _joint_region(region):
    parts = [x.encode() for x in region]
    return JointRegion(*parts, *[len(x) for x in parts]), parts


def _outputs_1d(n, ncand):
    return dict(best_score=np.zeros(n, np.int32), sum_k=np.zeros(n, np.int64),
                n_ties=np.zeros(n, np.int32), status=np.zeros(n, np.uint8),
                cand_score=np.zeros(ncand, np.int32), cand_tstart=np.zeros(ncand, np.int32),
                cand_tend=np.zeros(ncand, np.int32))


def _outputs_2d(n, nc):
    return dict(read_strand=np.zeros(n, np.int8), cell_score=np.zeros(nc, np.int32),
                cell_wscore=np.zeros(nc, np.int32), best_wscore=np.zeros(n, np.int32),
                sum_k1=np.zeros(n, np.int64), sum_k2=np.zeros(n, np.int64),
                n_ties=np.zeros(n, np.int32), status=np.zeros(n, np.uint8))


def round3_1d(regions, reads, kmin, kmax, read_region=None, sc=None, flags=0, device=0,
              per_candidate=True):
    """One-shot nra_round3_1d.  regions = [(left, unit, right)], reads = [str]."""
    lib = load()
    sc = sc or default_scoring()
    n = len(reads)
    seqs, off = pack_reads(reads)
    kmin = np.ascontiguousarray(kmin, np.int32)
    kmax = np.ascontiguousarray(kmax, np.int32)
    rr = None if read_region is None else np.ascontiguousarray(read_region, np.int32)
    regs, keep = _regions(regions)
    ncand = int(np.maximum(kmax.astype(np.int64) - kmin + 1, 0).sum()) if per_candidate else 0
    out = _outputs_1d(n, ncand)
    pc = per_candidate
    _check(lib.nra_round3_1d(device, regs, len(regions), n, seqs, _ptr(off, C.c_int64),
                             _ptr(rr, C.c_int32), _ptr(kmin, C.c_int32), _ptr(kmax, C.c_int32),
                             C.byref(sc), flags,
                             _ptr(out["best_score"], C.c_int32), _ptr(out["sum_k"], C.c_int64),
                             _ptr(out["n_ties"], C.c_int32), _ptr(out["status"], C.c_uint8),
                             _ptr(out["cand_score"], C.c_int32) if pc else None,
                             _ptr(out["cand_tstart"], C.c_int32) if pc else None,
                             _ptr(out["cand_tend"], C.c_int32) if pc else None))
    return out


def plan1d_digest(regions, reads, kmin, kmax, read_region=None, sc=None, flags=0, simds=1024):
    """nra_plan1d_digest: the plan nra_batch1d_create would make on a device of `simds` SIMDs, as text (no device needed)."""
    lib = load()
    sc = sc or default_scoring()
    seqs, off = pack_reads(reads)
    kmin = np.ascontiguousarray(kmin, np.int32)
    kmax = np.ascontiguousarray(kmax, np.int32)
    rr = None if read_region is None else np.ascontiguousarray(read_region, np.int32)
    regs, keep = _regions(regions)
    args = (regs, len(regions), len(reads), seqs, _ptr(off, C.c_int64), _ptr(rr, C.c_int32),
            _ptr(kmin, C.c_int32), _ptr(kmax, C.c_int32), C.byref(sc), flags, simds)
    need = lib.nra_plan1d_digest(*args, None, 0)
    if need < 0:
        _check(int(need))
    buf = C.create_string_buffer(int(need))
    _check(min(0, int(lib.nra_plan1d_digest(*args, buf, need))))
    return buf.value.decode()


PLAN2D_KINDS = {"cells": 0, "grid": 1, "sweep_flanks": 2, "refine": 3, "invalidate": 4}
JOINT_KEEP_BUDGET = 96 << 30     # NRA_JOINT_KEEP_BUDGET


def plan2d_digest(region, reads, steps, sc=None, flags=0):
    """nra_plan2d_digest: the plans a joint batch of `reads` would make for `steps`, played in order, as text (no device
    needed).  A step is a dict: kind (a key of PLAN2D_KINDS), strand (or None), cells = (cell_read, k1, k2), grid = Grid,
    bounds = (lo1, hi1, lo2, hi2) and buf = (buf1, buf2) of a refinement, budget / free in bytes."""
    lib = load()
    sc = sc or default_scoring()
    seqs, off = pack_reads(reads)
    jr, keep = _joint_region(region)
    arr = (Plan2DStep * max(len(steps), 1))()
    for i, s in enumerate(steps):
        t = arr[i]
        t.kind = PLAN2D_KINDS[s["kind"]]
        t.keep_budget = s.get("budget", JOINT_KEEP_BUDGET)
        t.device_free = s.get("free", 256 << 30)
        if s.get("strand") is not None:
            st = np.ascontiguousarray(s["strand"], np.int8)
            keep.append(st)
            t.read_strand = _ptr(st, C.c_int8)
        if "cells" in s:
            cr, k1, k2 = (np.ascontiguousarray(a, np.int32) for a in s["cells"])
            keep += [cr, k1, k2]
            t.n_cells = len(cr)
            t.cell_read, t.cell_k1, t.cell_k2 = (_ptr(a, C.c_int32) for a in (cr, k1, k2))
        if "grid" in s:
            g = s["grid"]
            keep.append(g)
            (t.start1, t.step1, t.count1), (t.start2, t.step2, t.count2) = g.axes
            t.lo1, t.hi1, t.lo2, t.hi2 = (_ptr(a, C.c_double) for a in g.bounds)
        if "bounds" in s:
            b = [np.ascontiguousarray(a, np.float64) for a in s["bounds"]]
            keep += b
            t.lo1, t.hi1, t.lo2, t.hi2 = (_ptr(a, C.c_double) for a in b)
            t.buf1, t.buf2 = s["buf"]
    args = (C.byref(jr), len(reads), seqs, _ptr(off, C.c_int64), C.byref(sc), flags, arr, len(steps))
    need = lib.nra_plan2d_digest(*args, None, 0)
    if need < 0:
        _check(int(need))
    buf = C.create_string_buffer(int(need))
    _check(min(0, int(lib.nra_plan2d_digest(*args, buf, need))))
    return buf.value.decode()


def prepared_round3_1d(regions, reads, kmin, kmax, read_region=None, sc=None, flags=0, device=0):
    """-> (call, out): `call()` is exactly one nra_round3_1d over prebuilt host buffers (ASCII reads in,
    per-read results out), so that a benchmark times the C ABI and not the Python list handling."""
    lib = load()
    sc = sc or default_scoring()
    n = len(reads)
    seqs, off = pack_reads(reads)
    kmin = np.ascontiguousarray(kmin, np.int32)
    kmax = np.ascontiguousarray(kmax, np.int32)
    rr = None if read_region is None else np.ascontiguousarray(read_region, np.int32)
    regs, keep = _regions(regions)
    out = _outputs_1d(n, 0)
    args = (device, regs, len(regions), n, seqs, _ptr(off, C.c_int64), _ptr(rr, C.c_int32),
            _ptr(kmin, C.c_int32), _ptr(kmax, C.c_int32), C.byref(sc), flags,
            _ptr(out["best_score"], C.c_int32), _ptr(out["sum_k"], C.c_int64),
            _ptr(out["n_ties"], C.c_int32), _ptr(out["status"], C.c_uint8), None, None, None)
    hold = (seqs, off, kmin, kmax, rr, regs, keep, sc)

    def call():
        _check(lib.nra_round3_1d(*args))
        return hold and out
    return call, out


def joint_2d(region, reads, cell_read, cell_k1, cell_k2, read_strand=None, sc=None, flags=0,
             device=0):
    """One-shot nra_joint_2d.  region = (left, unit1, mid, unit2, right)."""
    lib = load()
    sc = sc or default_scoring()
    n = len(reads)
    seqs, off = pack_reads(reads)
    jr, keep = _joint_region(region)
    cr = np.ascontiguousarray(cell_read, np.int32)
    k1 = np.ascontiguousarray(cell_k1, np.int32)
    k2 = np.ascontiguousarray(cell_k2, np.int32)
    out = _outputs_2d(n, len(cr))
    if read_strand is not None:
        out["read_strand"][:] = np.asarray(read_strand, np.int8)
    _check(lib.nra_joint_2d(device, C.byref(jr), n, seqs, _ptr(off, C.c_int64),
                            _ptr(out["read_strand"], C.c_int8), len(cr), _ptr(cr, C.c_int32),
                            _ptr(k1, C.c_int32), _ptr(k2, C.c_int32), C.byref(sc), flags,
                            _ptr(out["cell_score"], C.c_int32), _ptr(out["cell_wscore"], C.c_int32),
                            _ptr(out["best_wscore"], C.c_int32), _ptr(out["sum_k1"], C.c_int64),
                            _ptr(out["sum_k2"], C.c_int64), _ptr(out["n_ties"], C.c_int32),
                            _ptr(out["status"], C.c_uint8)))
    return out


class Grid:
    """One routed grid round (nra_batch2d_set_grid): per axis the grid values start + i * step, i < count, and per
    read the half-open bounds [lo, hi) (doubles) of the values it takes."""

    def __init__(self, axis1, lo1, hi1, axis2, lo2, hi2):
        self.axes = (tuple(int(x) for x in axis1), tuple(int(x) for x in axis2))      # (start, step, count)
        self.bounds = [np.ascontiguousarray(a, np.float64) for a in (lo1, hi1, lo2, hi2)]
        self.n_reads = len(self.bounds[0])
        assert all(len(a) == self.n_reads for a in self.bounds)

    def c_args(self):
        lo1, hi1, lo2, hi2 = (_ptr(a, C.c_double) for a in self.bounds)
        return (*self.axes[0], lo1, hi1, *self.axes[1], lo2, hi2)


def joint_grid_cells(grid):
    """nra_joint_grid_cells: the cells of a routed grid, (cell_read, k1, k2), on the host."""
    lib = load()
    n = lib.nra_joint_grid_cells(grid.n_reads, *grid.c_args(), 0, None, None, None)
    if n < 0:
        _check(int(n))
    cr, k1, k2 = (np.zeros(n, np.int32) for _ in range(3))
    got = lib.nra_joint_grid_cells(grid.n_reads, *grid.c_args(), n, _ptr(cr, C.c_int32), _ptr(k1, C.c_int32), _ptr(k2, C.c_int32))
    if got < 0:
        _check(int(got))
    return cr, k1, k2


def align_pairs(seqs, pair_query, pair_target, sc=None, flags=0, device=0):
    """nra_align_pairs: optimal local alignment of seqs[pair_query[i]] (query) against
    seqs[pair_target[i]] (target) -> dict(score, tstart, tend) in target coordinates."""
    lib = load()
    sc = sc or default_scoring()
    data, off = pack_reads(seqs)
    pq = np.ascontiguousarray(pair_query, np.int32)
    pt = np.ascontiguousarray(pair_target, np.int32)
    n = len(pq)
    out = dict(score=np.zeros(n, np.int32), tstart=np.zeros(n, np.int32), tend=np.zeros(n, np.int32))
    _check(lib.nra_align_pairs(device, len(seqs), data, _ptr(off, C.c_int64), n, _ptr(pq, C.c_int32),
                               _ptr(pt, C.c_int32), C.byref(sc), flags, _ptr(out["score"], C.c_int32),
                               _ptr(out["tstart"], C.c_int32), _ptr(out["tend"], C.c_int32)))
    return out


def align_pairs_cigar(seqs, pair_query, pair_target, sc=None, flags=0, device=0, entry="nra_align_pairs_cigar"):
    """nra_align_pairs_cigar: like align_pairs, plus qstart/qend and the --eqx CIGAR of each pair."""
    lib = load()
    sc = sc or default_scoring()
    data, off = pack_reads(seqs)
    pq = np.ascontiguousarray(pair_query, np.int32)
    pt = np.ascontiguousarray(pair_target, np.int32)
    n = len(pq)
    out = {k: np.zeros(n, np.int32) for k in ("score", "tstart", "tend", "qstart", "qend")}
    lens = np.diff(off)
    cap = int(sum(12 * (int(lens[q]) + int(lens[t])) + 16 for q, t in zip(pq, pt))) + 16
    buf = C.create_string_buffer(cap)
    coff = np.zeros(n + 1, np.int64)
    _check(getattr(lib, entry)(device, len(seqs), data, _ptr(off, C.c_int64), n, _ptr(pq, C.c_int32),
                               _ptr(pt, C.c_int32), C.byref(sc), flags,
                               *[_ptr(out[k], C.c_int32) for k in ("score", "tstart", "tend", "qstart", "qend")],
                               buf, cap, _ptr(coff, C.c_int64)))
    raw = buf.raw
    out["cigar"] = [raw[coff[i]:coff[i + 1] - 1].decode() for i in range(n)]
    return out


TRACE_CHUNK_BYTES = 6 << 30        # nra_align_pairs_cigar keeps one trace byte per DP cell, <= 8 GiB per call


def align_paths(seqs, pair_query, pair_target, sc=None, flags=0, device=0):
    """nra_align_paths: align_pairs_cigar for queries of up to 200 000 bases (targets of up to 65 000)."""
    return align_pairs_cigar(seqs, pair_query, pair_target, sc=sc, flags=flags, device=device, entry="nra_align_paths")


PATHS_MAX_QUERY = 200000           # nra_align_paths: NRA_E_RANGE beyond these
PATHS_MAX_TARGET = 65000
PATHS_MAX_TRACE = 8 << 30


def align_paths_chunked(seqs, pair_query, pair_target, sc=None, flags=0, device=0, chunk_bytes=TRACE_CHUNK_BYTES):
    """align_paths for any number of pairs, split like align_pairs_cigar_chunked."""
    return align_pairs_cigar_chunked(seqs, pair_query, pair_target, sc=sc, flags=flags, device=device,
                                     chunk_bytes=chunk_bytes, call=align_paths)


def align_pairs_cigar_chunked(seqs, pair_query, pair_target, sc=None, flags=0, device=0,
                              chunk_bytes=TRACE_CHUNK_BYTES, call=align_pairs_cigar):
    """align_pairs_cigar for any number of pairs: splits the list so that each call's trace
    (query length x target length bytes per pair) stays below `chunk_bytes`, and sends each call
    only the sequences it uses."""
    n = len(pair_query)
    out = {k: np.full(n, -1, np.int32) for k in ("score", "tstart", "tend", "qstart", "qend")}
    out["cigar"] = [""] * n
    lo = 0
    while lo < n:
        hi, used = lo, 0
        while hi < n:
            cost = len(seqs[pair_query[hi]]) * len(seqs[pair_target[hi]])
            if hi > lo and used + cost > chunk_bytes:
                break
            used += cost; hi += 1
        ids = sorted({int(x) for x in pair_query[lo:hi]} | {int(x) for x in pair_target[lo:hi]})
        local = {g: i for i, g in enumerate(ids)}
        part = call([seqs[g] for g in ids], [local[int(x)] for x in pair_query[lo:hi]],
                    [local[int(x)] for x in pair_target[lo:hi]], sc=sc, flags=flags, device=device)
        for k in ("score", "tstart", "tend", "qstart", "qend"):
            out[k][lo:hi] = part[k]
        out["cigar"][lo:hi] = part["cigar"]
        lo = hi
    return out


class Batch:
    """Device-resident batch: create = encode + H2D, run = kernels only, fetch = D2H."""

    def __init__(self, handle, kind, n_reads, n_cand):
        self._h = handle
        self.kind = kind
        self.n_reads = n_reads
        self.n_cand = n_cand

    @classmethod
    def create_1d(cls, regions, reads, kmin, kmax, read_region=None, sc=None, flags=0, device=0):
        lib = load()
        sc = sc or default_scoring()
        seqs, off = pack_reads(reads)
        kmin = np.ascontiguousarray(kmin, np.int32)
        kmax = np.ascontiguousarray(kmax, np.int32)
        rr = None if read_region is None else np.ascontiguousarray(read_region, np.int32)
        regs, keep = _regions(regions)
        h = C.c_void_p()
        _check(lib.nra_batch1d_create(device, regs, len(regions), len(reads), seqs,
                                      _ptr(off, C.c_int64), _ptr(rr, C.c_int32),
                                      _ptr(kmin, C.c_int32), _ptr(kmax, C.c_int32), C.byref(sc),
                                      flags, C.byref(h)))
        ncand = int(np.maximum(kmax.astype(np.int64) - kmin + 1, 0).sum())
        return cls(h, 1, len(reads), ncand)

    @classmethod
    def create_2d(cls, region, reads, cell_read, cell_k1, cell_k2, read_strand=None, sc=None,
                  flags=0, device=0):
        lib = load()
        sc = sc or default_scoring()
        seqs, off = pack_reads(reads)
        jr, keep = _joint_region(region)
        cr = np.ascontiguousarray(cell_read, np.int32)
        k1 = np.ascontiguousarray(cell_k1, np.int32)
        k2 = np.ascontiguousarray(cell_k2, np.int32)
        st = None if read_strand is None else np.ascontiguousarray(read_strand, np.int8)
        h = C.c_void_p()
        _check(lib.nra_batch2d_create(device, C.byref(jr), len(reads), seqs, _ptr(off, C.c_int64),
                                      _ptr(st, C.c_int8), len(cr), _ptr(cr, C.c_int32),
                                      _ptr(k1, C.c_int32), _ptr(k2, C.c_int32), C.byref(sc), flags,
                                      C.byref(h)))
        return cls(h, 2, len(reads), len(cr))

    @classmethod
    def create_2d_reads(cls, region, reads, sc=None, flags=0, device=0):
        """The reads of a joint run, packed and resident; give it a cell list with set_cells()."""
        lib = load()
        sc = sc or default_scoring()
        seqs, off = pack_reads(reads)
        jr, keep = _joint_region(region)
        h = C.c_void_p()
        _check(lib.nra_batch2d_create_reads(device, C.byref(jr), len(reads), seqs, _ptr(off, C.c_int64),
                                            C.byref(sc), flags, C.byref(h)))
        return cls(h, 2, len(reads), 0)

    def set_cells(self, cell_read, cell_k1, cell_k2, read_strand=None):
        """The (read, k1, k2) cells of the next run (grouped by read); the previous list is dropped."""
        cr = np.ascontiguousarray(cell_read, np.int32)
        k1 = np.ascontiguousarray(cell_k1, np.int32)
        k2 = np.ascontiguousarray(cell_k2, np.int32)
        st = None if read_strand is None else np.ascontiguousarray(read_strand, np.int8)
        _check(load().nra_batch2d_set_cells(self._h, _ptr(st, C.c_int8), len(cr), _ptr(cr, C.c_int32),
                                            _ptr(k1, C.c_int32), _ptr(k2, C.c_int32)))
        self.n_cand = self._n_cells = len(cr)

    def set_grid(self, grid, read_strand=None):
        """A whole routed grid round (Grid): the library lists the cells itself.  Returns the number of cells."""
        if grid.n_reads != self.n_reads:
            raise ValueError("grid bounds must have one entry per read of the batch")
        st = None if read_strand is None else np.ascontiguousarray(read_strand, np.int8)
        n = C.c_int64(0)
        _check(load().nra_batch2d_set_grid(self._h, _ptr(st, C.c_int8), *grid.c_args(), C.byref(n)))
        self.n_cand = self._n_cells = int(n.value)
        return self.n_cand

    def sweep_flanks(self, read_strand):
        """nra_batch2d_sweep_flanks: enqueue the strand-only flank sweeps now, ahead of the cell list."""
        st = np.ascontiguousarray(read_strand, np.int8)
        if len(st) != self.n_reads:
            raise ValueError("one strand per read of the batch")
        _check(load().nra_batch2d_sweep_flanks(self._h, _ptr(st, C.c_int8)))

    def refine(self, buf1, buf2, lo1, hi1, lo2, hi2):
        """nra_batch2d_refine: the reference's round 3 enqueued behind the routed grid whose run() was just called, routed
        on the device.  False when the batch cannot (E_STATE: the caller fetches and sets the finer grid itself)."""
        b = [np.ascontiguousarray(a, np.float64) for a in (lo1, hi1, lo2, hi2)]
        if any(len(a) != self.n_reads for a in b):
            raise ValueError("refinement bounds must have one entry per read of the batch")
        rc = load().nra_batch2d_refine(self._h, int(buf1), int(buf2), *(_ptr(a, C.c_double) for a in b))
        if rc == E_STATE:
            return False
        _check(rc)
        self.n_cand = self.n_reads * 4 * int(buf1) * int(buf2)
        return True

    def invalidate(self):
        """Drop what earlier cell lists left for later ones (reverse sweeps): the next list starts like the first."""
        _check(load().nra_batch2d_invalidate(self._h))

    def run(self):
        _check(load().nra_batch_run(self._h))
        if self.kind == 2 and getattr(self, "_n_cells", None) is not None:
            self.n_cand = self._n_cells          # (a refinement of the previous run had its own per-cell layout)

    def sync(self):
        _check(load().nra_batch_sync(self._h))

    def stats(self):
        st = Stats()
        _check(load().nra_batch_stats(self._h, C.byref(st)))
        return st.as_dict()

    def resweeps(self):
        """1D, after the run: the sweep tasks and reads the relaxed anchor columns sent to the exact re-sweep, of how many."""
        v = [C.c_int64(0) for _ in range(4)]
        _check(load().nra_batch1d_resweeps(self._h, *[C.byref(x) for x in v]))
        return {"tasks": v[0].value, "reads": v[1].value, "tasks_total": v[2].value, "reads_total": v[3].value}

    def saturation(self):
        """1D, after the run: the forward sweeps in quanta that left through the saturation exit and the steps they skipped,
        of how many sweeps and planned steps."""
        v = [C.c_int64(0) for _ in range(4)]
        _check(load().nra_batch1d_saturation(self._h, *[C.byref(x) for x in v]))
        return {"sweeps": v[0].value, "steps": v[1].value, "sweeps_total": v[2].value, "steps_total": v[3].value}

    def clears(self):
        """1D: which per-candidate arrays a run of this batch clears before its kernels start."""
        v = [C.c_int32(0) for _ in range(2)]
        _check(load().nra_batch1d_clears(self._h, *[C.byref(x) for x in v]))
        return {"scores": bool(v[0].value), "extents": bool(v[1].value)}

    def fetch(self, per_candidate=True):
        lib = load()
        if self.kind == 1:
            out = _outputs_1d(self.n_reads, self.n_cand if per_candidate else 0)
            pc = per_candidate
            _check(lib.nra_batch1d_fetch(self._h, _ptr(out["best_score"], C.c_int32),
                                         _ptr(out["sum_k"], C.c_int64), _ptr(out["n_ties"], C.c_int32),
                                         _ptr(out["status"], C.c_uint8),
                                         _ptr(out["cand_score"], C.c_int32) if pc else None,
                                         _ptr(out["cand_tstart"], C.c_int32) if pc else None,
                                         _ptr(out["cand_tend"], C.c_int32) if pc else None))
            return out
        out = _outputs_2d(self.n_reads, self.n_cand if per_candidate else 0)
        pc = per_candidate
        _check(lib.nra_batch2d_fetch(self._h, _ptr(out["read_strand"], C.c_int8),
                                     _ptr(out["cell_score"], C.c_int32) if pc else None,
                                     _ptr(out["cell_wscore"], C.c_int32) if pc else None,
                                     _ptr(out["best_wscore"], C.c_int32), _ptr(out["sum_k1"], C.c_int64),
                                     _ptr(out["sum_k2"], C.c_int64), _ptr(out["n_ties"], C.c_int32),
                                     _ptr(out["status"], C.c_uint8)))
        return out

    def close(self):
        if self._h:
            load().nra_batch_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def screen_create(anchors, k=15, max_occ=16, device=0):
    """nra_screen_create.  anchors = [(left, right)] per region -> an opaque handle (screen_destroy frees it)."""
    data, off = pack_reads([a for pair in anchors for a in pair])
    h = C.c_void_p()
    _check(load().nra_screen_create(device, len(anchors), data, _ptr(off, C.c_int64), k, max_occ, C.byref(h)))
    return h


def screen_stats(handle):
    st = ScreenStats()
    _check(load().nra_screen_stats(handle, C.byref(st)))
    return st.as_dict()


def screen_reads(handle, reads, min_hits=4, capacity=None):
    """nra_screen_reads -> dict(read, region, hits_left, hits_right) of the passing pairs, sorted by read then
    region.  When the pairs exceed `capacity` (default: a few per read), the call is repeated once with the
    capacity the library asked for."""
    lib = load()
    seqs, off = pack_reads(reads)
    n = len(reads)
    if capacity is None:
        capacity = n * (4 + screen_stats(handle)["n_empty_regions"]) + 1024
    while True:
        out = {key: np.zeros(capacity, np.int32) for key in ("read", "region", "hits_left", "hits_right")}
        n_pairs = C.c_int64(capacity)
        rc = lib.nra_screen_reads(handle, n, seqs, _ptr(off, C.c_int64), min_hits, C.byref(n_pairs),
                                  *(_ptr(out[key], C.c_int32) for key in ("read", "region", "hits_left", "hits_right")))
        if rc == E_RANGE and n_pairs.value > capacity:
            capacity = int(n_pairs.value)
            continue
        _check(rc)
        return {key: v[:n_pairs.value] for key, v in out.items()}


def screen_set_motifs(handle, motifs):
    """nra_screen_set_motifs: one motif per region of the handle (a second call replaces the first)."""
    data, off = pack_reads(list(motifs))
    _check(load().nra_screen_set_motifs(handle, len(motifs), data, _ptr(off, C.c_int64)))


def screen_reads_partial(handle, reads, min_hits=4, motif_share_pct=5, capacity=None):
    """nra_screen_reads_partial -> dict(read, region, hits_left, hits_right, motif_windows, kind) of the pairs of the
    four kinds (0 both anchors, 1 left only, 2 right only, 3 in repeat), sorted by read then region.  When the pairs
    exceed `capacity`, the call is repeated once with the capacity the library asked for."""
    lib = load()
    seqs, off = pack_reads(reads)
    n = len(reads)
    if capacity is None:
        capacity = n * (8 + screen_stats(handle)["n_empty_regions"]) + 1024
    keys = ("read", "region", "hits_left", "hits_right", "motif_windows")
    while True:
        out = {key: np.zeros(capacity, np.int32) for key in keys}
        out["kind"] = np.zeros(capacity, np.uint8)
        n_pairs = C.c_int64(capacity)
        rc = lib.nra_screen_reads_partial(handle, n, seqs, _ptr(off, C.c_int64), min_hits, motif_share_pct,
                                          C.byref(n_pairs), *(_ptr(out[key], C.c_int32) for key in keys),
                                          _ptr(out["kind"], C.c_uint8))
        if rc == E_RANGE and n_pairs.value > capacity:
            capacity = int(n_pairs.value)
            continue
        _check(rc)
        return {key: v[:n_pairs.value] for key, v in out.items()}


def screen_destroy(handle):
    if handle:
        _check(load().nra_screen_destroy(handle))


def read_structure(motifs, tracts, read_motif, device=0):
    """nra_read_structure: the wraparound alignment of every tract against its motif (motifs[read_motif[i]]) ->
    dict(edits, start_phase, path, path_off): the path bytes of tract i are path[path_off[i]:path_off[i + 1]]."""
    lib = load()
    mdata, moff = pack_reads(list(motifs))
    data, off = pack_reads(tracts)
    rm = np.ascontiguousarray(read_motif, np.int32)
    n = len(tracts)
    if len(rm) != n:
        raise ValueError("one motif index per tract")
    out = dict(edits=np.zeros(n, np.int32), start_phase=np.zeros(n, np.int32),
               path=np.zeros(int(off[-1]), np.uint8), path_off=off)
    _check(lib.nra_read_structure(device, len(motifs), mdata, _ptr(moff, C.c_int64), n, data, _ptr(off, C.c_int64),
                                  _ptr(rm, C.c_int32), _ptr(out["edits"], C.c_int32),
                                  _ptr(out["start_phase"], C.c_int32), _ptr(out["path"], C.c_uint8)))
    return out


def tract_motifs(tracts, max_period=6, top_n=4, device=0):
    """nra_tract_motifs: the tandem positions of every tract per period 1..max_period and its top_n motif classes ->
    dict(n_tandem [n, max_period], top_p [n, top_n] int8, top_code, top_count [n, top_n] int32); (0, -1, 0) in
    unused slots."""
    lib = load()
    data, off = pack_reads(list(tracts))
    n = len(off) - 1
    out = dict(n_tandem=np.zeros((n, max(max_period, 0)), np.int32), top_p=np.zeros((n, max(top_n, 0)), np.int8),
               top_code=np.zeros((n, max(top_n, 0)), np.int32), top_count=np.zeros((n, max(top_n, 0)), np.int32))
    _check(lib.nra_tract_motifs(device, n, data, _ptr(off, C.c_int64), max_period, top_n,
                                _ptr(out["n_tandem"], C.c_int32), _ptr(out["top_p"], C.c_int8),
                                _ptr(out["top_code"], C.c_int32), _ptr(out["top_count"], C.c_int32)))
    return out


def tract_periods(tracts, max_period=64, device=0):
    """nra_tract_periods: per tract and lag p = 1..max_period, the positions i with s[i] and s[i + p] both ACGT
    (valid) and those of them with s[i] == s[i + p] (match) -> dict(match, valid), int32 [n, max_period]."""
    lib = load()
    data, off = pack_reads(list(tracts))
    n = len(off) - 1
    out = dict(match=np.zeros((n, max(max_period, 0)), np.int32), valid=np.zeros((n, max(max_period, 0)), np.int32))
    _check(lib.nra_tract_periods(device, n, data, _ptr(off, C.c_int64), max_period, _ptr(out["match"], C.c_int32),
                                 _ptr(out["valid"], C.c_int32)))
    return out


def read_methylation(reads, mods, flags, tract_lo, tract_hi, flank=2000, bin=200, lo_byte=63, hi_byte=192, device=0):
    """nra_read_methylation: the CpG calls of every read counted over its tract and flank bins.  reads: the stored
    sequences; mods[i] = (deltas, probs) of read i's list; flags[i]: bit 0 stored reversed, bit 1 implicit; the tract
    of read i is stored [tract_lo[i], tract_hi[i]).  -> dict(counts int32 [n, 2 nb + 1, 5] with nb = ceil(flank / bin)
    and the segments before[0..nb), tract, after[0..nb), n_c [n], status [n])."""
    lib = load()
    data, off = pack_reads(list(reads))
    n = len(off) - 1
    if not (len(mods) == len(flags) == len(tract_lo) == len(tract_hi) == n):
        raise ValueError("one list, flag byte and tract per read")
    mod_off = np.zeros(n + 1, np.int64)
    mod_off[1:] = np.cumsum([len(d) for d, _ in mods])
    if any(len(d) != len(p) for d, p in mods):
        raise ValueError("one call byte per delta")
    deltas = np.ascontiguousarray(np.concatenate([np.asarray(d, np.int32) for d, _ in mods] or
                                                 [np.zeros(0, np.int32)]), np.int32)
    probs = np.ascontiguousarray(np.concatenate([np.asarray(p, np.uint8) for _, p in mods] or
                                                [np.zeros(0, np.uint8)]), np.uint8)
    flags = np.ascontiguousarray(flags, np.uint8)
    lo, hi = np.ascontiguousarray(tract_lo, np.int32), np.ascontiguousarray(tract_hi, np.int32)
    nb = (flank + bin - 1) // bin if flank >= 1 and bin >= 1 else 0
    out = dict(counts=np.zeros((n, 2 * min(nb, 64) + 1, 5), np.int32), n_c=np.zeros(n, np.int32),
               status=np.zeros(n, np.int32))
    _check(lib.nra_read_methylation(device, n, data, _ptr(off, C.c_int64), _ptr(deltas, C.c_int32),
                                    _ptr(probs, C.c_uint8), _ptr(mod_off, C.c_int64), _ptr(flags, C.c_uint8),
                                    _ptr(lo, C.c_int32), _ptr(hi, C.c_int32), flank, bin, lo_byte, hi_byte,
                                    _ptr(out["counts"], C.c_int32), _ptr(out["n_c"], C.c_int32),
                                    _ptr(out["status"], C.c_int32)))
    return out


SCAN_KEYS = ("read", "start", "end", "cls", "windows", "fwd_windows")


def scan_repeats(seqs, k=11, max_gap=100, min_span=200, device=0, capacity=None):
    """nra_scan_repeats: the tandem runs of every read, no region or motif given -> dict(read, start, end, cls, windows,
    fwd_windows: int32 per run, ordered by (read, start, end, cls); stats: dict).  When the runs exceed `capacity`, the
    call is repeated once with the capacity the library asked for."""
    lib = load()
    data, off = pack_reads(list(seqs))
    n = len(off) - 1
    if capacity is None:
        capacity = 4 * n + 1024
    while True:
        out = {key: np.zeros(capacity, np.int32) for key in SCAN_KEYS}
        n_runs = C.c_int64(capacity)
        st = ScanStats()
        rc = lib.nra_scan_repeats(device, n, data, _ptr(off, C.c_int64), k, max_gap, min_span, C.byref(n_runs),
                                  *(_ptr(out[key], C.c_int32) for key in SCAN_KEYS), C.byref(st))
        if rc == E_RANGE and n_runs.value > capacity:
            capacity = int(n_runs.value)
            continue
        _check(rc)
        out = {key: v[:n_runs.value] for key, v in out.items()}
        out["stats"] = st.as_dict()
        return out


SKETCH_KEYS = ("a", "b", "shared")
SKETCH_MAX_LEN = 2048      # NRA_SKETCH_MAX_N
SKETCH_MAX_GROUP = 65536   # NRA_SKETCH_MAX_GROUP


def sketch_pairs(seqs, groups, k=13, min_shared=1, device=0, capacity=None):
    """nra_sketch_pairs: the pairs of sequences of one group (groups[i], negative: none) that share at least min_shared
    canonical non-periodic k-mers -> dict(a, b, shared: int32 per pair, a < b, ordered by (a, b); sketch_size: int32
    per sequence; stats: dict).  When the pairs exceed `capacity`, the call is repeated once with the capacity the
    library asked for."""
    lib = load()
    data, off = pack_reads(list(seqs))
    n = len(off) - 1
    grp = np.ascontiguousarray(groups, np.int32)
    if grp.shape != (n,):
        raise ValueError("one group id per sequence")
    if capacity is None:
        capacity = 16 * n + 1024
    while True:
        out = {key: np.zeros(capacity, np.int32) for key in SKETCH_KEYS}
        size = np.zeros(n, np.int32)
        n_pairs = C.c_int64(capacity)
        st = SketchStats()
        rc = lib.nra_sketch_pairs(device, n, data, _ptr(off, C.c_int64), _ptr(grp, C.c_int32), k, min_shared,
                                  C.byref(n_pairs), *(_ptr(out[key], C.c_int32) for key in SKETCH_KEYS),
                                  _ptr(size, C.c_int32), C.byref(st))
        if rc == E_RANGE and n_pairs.value > capacity:
            capacity = int(n_pairs.value)
            continue
        _check(rc)
        out = {key: v[:n_pairs.value] for key, v in out.items()}
        out["sketch_size"] = size
        out["stats"] = st.as_dict()
        return out


PLACE_KEYS = ("query", "contig", "strand", "bin", "votes")
PLACE_MAX_QUERY = 2048        # NRA_PLACE_MAX_QUERY
PLACE_MAX_QUERIES = 1 << 20   # NRA_PLACE_MAX_QUERIES
PLACE_MAX_POS = 1 << 30       # NRA_PLACE_MAX_POS
PLACE_OCC_CEILING = 1024      # NRA_PLACE_OCC_CEILING


def place_create(queries, k=15, max_occ=16, device=0):
    """nra_place_create: the index of the queries -> an opaque handle (place_destroy frees it)."""
    data, off = pack_reads(list(queries))
    h = C.c_void_p()
    _check(load().nra_place_create(device, len(off) - 1, data, _ptr(off, C.c_int64), k, max_occ, C.byref(h)))
    return h


def place_scan(handle, contig, pos0, bases):
    """nra_place_scan: bases [pos0, pos0 + len(bases)) of contig `contig` (a label >= 0).  Successive chunks of a contig
    overlap by k - 1 bases; a window given twice counts twice."""
    data = bases.encode() if isinstance(bases, str) else bytes(bases)
    _check(load().nra_place_scan(handle, contig, pos0, data, len(data)))


def place_candidates(handle, bin=64, max_target_occ=64, min_votes=8, capacity=None):
    """nra_place_candidates -> dict(query, contig, strand, bin, votes: int32 per candidate, ordered by (query, contig,
    strand, bin)).  When the candidates exceed `capacity`, the call is repeated once with the capacity the library
    asked for."""
    lib = load()
    if capacity is None:
        capacity = 4096
    while True:
        out = {key: np.zeros(capacity, np.int32) for key in PLACE_KEYS}
        n_cand = C.c_int64(capacity)
        rc = lib.nra_place_candidates(handle, bin, max_target_occ, min_votes, C.byref(n_cand),
                                      *(_ptr(out[key], C.c_int32) for key in PLACE_KEYS))
        if rc == E_RANGE and n_cand.value > capacity:
            capacity = int(n_cand.value)
            continue
        _check(rc)
        return {key: v[:n_cand.value] for key, v in out.items()}


def place_stats(handle):
    st = PlaceStats()
    _check(load().nra_place_stats(handle, C.byref(st)))
    return st.as_dict()


def place_destroy(handle):
    if handle:
        _check(load().nra_place_destroy(handle))


def extend_tracts(motifs, tracts, read_motif, match=2, mismatch=4, gap=6, device=0):
    """nra_extend_tracts: the anchored wraparound extension of every tract along its motif (motifs[read_motif[i]]) ->
    dict(score, end, end_phase, motif_bases), int32 per tract."""
    lib = load()
    mdata, moff = pack_reads(list(motifs))
    data, off = pack_reads(tracts)
    rm = np.ascontiguousarray(read_motif, np.int32)
    n = len(tracts)
    if len(rm) != n:
        raise ValueError("one motif index per tract")
    out = {key: np.zeros(n, np.int32) for key in ("score", "end", "end_phase", "motif_bases")}
    _check(lib.nra_extend_tracts(device, len(motifs), mdata, _ptr(moff, C.c_int64), n, data, _ptr(off, C.c_int64),
                                 _ptr(rm, C.c_int32), match, mismatch, gap,
                                 *(_ptr(out[key], C.c_int32) for key in ("score", "end", "end_phase", "motif_bases"))))
    return out


def mixture_fit(samples, prob_off, prob_n, prob_d, fit_problem, fit_n, starts, flags=0, device=0):
    """nra_mixture_fit: fit f = fit_n[f] components on problem fit_problem[f] (prob_n[p] rows of prob_d[p] float64 from
    samples[prob_off[p]]) from the next fit_n[f] rows of `starts` -> dict(lb, n_iter, converged per fit; off = where a
    fit's components begin; w [components], mu and var [components, 2])."""
    lib = load()
    x = np.ascontiguousarray(samples, np.float64).ravel()
    po = np.ascontiguousarray(prob_off, np.int64)
    pn = np.ascontiguousarray(prob_n, np.int32)
    pd = np.ascontiguousarray(prob_d, np.int32)
    fp = np.ascontiguousarray(fit_problem, np.int32)
    fn = np.ascontiguousarray(fit_n, np.int32)
    st = np.ascontiguousarray(starts, np.int32)
    if not (len(po) == len(pn) == len(pd)) or len(fp) != len(fn):
        raise ValueError("one offset, row count and axis count per problem; one problem and order per fit")
    if len(st) != int(np.maximum(fn, 0).sum()):
        raise ValueError("one start row per component of every fit")
    nf = len(fn)
    off = np.zeros(nf + 1, np.int64)
    np.cumsum(np.maximum(fn, 0), out=off[1:])
    t = int(off[-1])
    out = dict(lb=np.zeros(nf), n_iter=np.zeros(nf, np.int32), converged=np.zeros(nf, np.int32), off=off,
               w=np.zeros(t), mu=np.zeros((t, 2)), var=np.zeros((t, 2)))
    _check(lib.nra_mixture_fit(device, len(x), _ptr(x, C.c_double), len(po), _ptr(po, C.c_int64), _ptr(pn, C.c_int32),
                               _ptr(pd, C.c_int32), nf, _ptr(fp, C.c_int32), _ptr(fn, C.c_int32), _ptr(st, C.c_int32),
                               flags, _ptr(out["lb"], C.c_double), _ptr(out["w"], C.c_double),
                               _ptr(out["mu"], C.c_double), _ptr(out["var"], C.c_double),
                               _ptr(out["n_iter"], C.c_int32), _ptr(out["converged"], C.c_int32)))
    return out


CENS_MAX_COMPONENTS = 8      # NRA_CENS_MAX_COMPONENTS
CENS_MAX_ITER = 500          # NRA_CENS_MAX_ITER


def _censored_problems(values, prob_off, prob_n, prob_n_exact, prob_tau):
    y = np.ascontiguousarray(values, np.float64).ravel()
    po = np.ascontiguousarray(prob_off, np.int64)
    pn = np.ascontiguousarray(prob_n, np.int32)
    pe = np.ascontiguousarray(prob_n_exact, np.int32)
    pt = np.ascontiguousarray(prob_tau, np.float64)
    if not (len(po) == len(pn) == len(pe) == len(pt)):
        raise ValueError("one offset, value count, exact count and tau per problem")
    return y, po, pn, pe, pt


def censored_fit(values, prob_off, prob_n, prob_n_exact, prob_tau, fit_problem, fit_n, fit_open, starts, max_iter=500,
                 tol=1e-9, flags=0, device=0):
    """nra_censored_fit: problem p = prob_n[p] log-domain values from values[prob_off[p]], the first prob_n_exact[p]
    exact, the others lower bounds, sd prob_tau[p]; fit f = fit_n[f] closed components (+ an open one where fit_open[f])
    on problem fit_problem[f] from the next fit_n[f] means of `starts` -> dict(ll, n_iter, converged per fit; nu_off,
    w_off = where a fit's means and weights begin; nu [closed components]; w [components, the open weight last])."""
    lib = load()
    y, po, pn, pe, pt = _censored_problems(values, prob_off, prob_n, prob_n_exact, prob_tau)
    fp = np.ascontiguousarray(fit_problem, np.int32)
    fn = np.ascontiguousarray(fit_n, np.int32)
    fo = np.ascontiguousarray(fit_open, np.int32)
    st = np.ascontiguousarray(starts, np.float64)
    if not (len(fp) == len(fn) == len(fo)):
        raise ValueError("one problem, order and open switch per fit")
    if len(st) != int(np.maximum(fn, 0).sum()):
        raise ValueError("one start mean per closed component of every fit")
    nf = len(fn)
    nu_off = np.zeros(nf + 1, np.int64)
    np.cumsum(np.maximum(fn, 0), out=nu_off[1:])
    w_off = np.zeros(nf + 1, np.int64)
    np.cumsum(np.maximum(fn, 0) + np.clip(fo, 0, 1), out=w_off[1:])
    out = dict(ll=np.zeros(nf), n_iter=np.zeros(nf, np.int32), converged=np.zeros(nf, np.int32), nu_off=nu_off,
               w_off=w_off, nu=np.zeros(int(nu_off[-1])), w=np.zeros(int(w_off[-1])))
    _check(lib.nra_censored_fit(device, len(y), _ptr(y, C.c_double), len(po), _ptr(po, C.c_int64), _ptr(pn, C.c_int32),
                                _ptr(pe, C.c_int32), _ptr(pt, C.c_double), nf, _ptr(fp, C.c_int32), _ptr(fn, C.c_int32),
                                _ptr(fo, C.c_int32), _ptr(st, C.c_double), int(max_iter), float(tol), flags,
                                _ptr(out["ll"], C.c_double), _ptr(out["w"], C.c_double), _ptr(out["nu"], C.c_double),
                                _ptr(out["n_iter"], C.c_int32), _ptr(out["converged"], C.c_int32)))
    return out


def censored_posteriors(values, prob_off, prob_n, prob_n_exact, prob_tau, model_n, model_open, w, nu, device=0):
    """nra_censored_posteriors: one model (model_n[p] closed components, model_open[p]) per problem, its weights and
    means laid out as censored_fit returns them -> a list with one [prob_n[p], n + open] array of posteriors per
    problem (the open column last)."""
    lib = load()
    y, po, pn, pe, pt = _censored_problems(values, prob_off, prob_n, prob_n_exact, prob_tau)
    mn = np.ascontiguousarray(model_n, np.int32)
    mo = np.ascontiguousarray(model_open, np.int32)
    ww = np.ascontiguousarray(w, np.float64)
    mu = np.ascontiguousarray(nu, np.float64)
    if not (len(mn) == len(mo) == len(po)):
        raise ValueError("one model per problem")
    nc = np.maximum(mn, 0).astype(np.int64) + np.clip(mo, 0, 1)
    if len(mu) != int(np.maximum(mn, 0).sum()) or len(ww) != int(nc.sum()):
        raise ValueError("one mean per closed component and one weight per component of every model")
    r_off = np.zeros(len(po) + 1, np.int64)
    np.cumsum(np.maximum(pn, 0).astype(np.int64) * nc, out=r_off[1:])
    resp = np.zeros(int(r_off[-1]))
    _check(lib.nra_censored_posteriors(device, len(y), _ptr(y, C.c_double), len(po), _ptr(po, C.c_int64),
                                       _ptr(pn, C.c_int32), _ptr(pe, C.c_int32), _ptr(pt, C.c_double),
                                       _ptr(mn, C.c_int32), _ptr(mo, C.c_int32), _ptr(ww, C.c_double),
                                       _ptr(mu, C.c_double), len(resp), _ptr(resp, C.c_double)))
    return [resp[r_off[p]:r_off[p + 1]].reshape(int(pn[p]), int(nc[p])) for p in range(len(po))]


CENS_BOOT_FITTED, CENS_BOOT_NO_EXACT = 0, 1      # NRA_CENS_BOOT_FITTED, NRA_CENS_BOOT_NO_EXACT


def censored_bootstrap(values, prob_off, prob_n, prob_n_exact, prob_tau, prob_ln_n, n_rep, idx, rep_m, max_alleles,
                       max_iter=500, tol=1e-9, flags=0, device=0):
    """nra_censored_bootstrap: the model search of n_rep replicates of every problem.  Problems as for censored_fit, each
    in sorted layout (exact values ascending, then bounds ascending), prob_ln_n[p] = math.log(prob_n[p]); idx: the
    problems' ascending index rows (n_rep * prob_n[p] each) concatenated in problem order, rep_m [problems, n_rep] the
    exact positions of every row -> dict(status, model_n, model_open, best_start, n_iter, ll, bic [problems, n_rep];
    nu [problems, n_rep, 8]; w [problems, n_rep, 9], the open weight at index model_n)."""
    lib = load()
    y, po, pn, pe, pt = _censored_problems(values, prob_off, prob_n, prob_n_exact, prob_tau)
    pl = np.ascontiguousarray(prob_ln_n, np.float64)
    ix = np.ascontiguousarray(idx, np.int32).ravel()
    rm = np.ascontiguousarray(rep_m, np.int32).ravel()
    n_rep, n = int(n_rep), len(po)
    if len(pl) != n:
        raise ValueError("one lnN per problem")
    if len(ix) != max(n_rep, 0) * int(np.maximum(pn, 0).astype(np.int64).sum()) or len(rm) != max(n_rep, 0) * n:
        raise ValueError("n_rep * N indices and n_rep exact counts per problem")
    r = (n, max(n_rep, 0))
    out = dict(status=np.zeros(r, np.int32), model_n=np.zeros(r, np.int32), model_open=np.zeros(r, np.int32),
               best_start=np.zeros(r, np.int32), n_iter=np.zeros(r, np.int32), ll=np.zeros(r), bic=np.zeros(r),
               nu=np.zeros(r + (CENS_MAX_COMPONENTS,)), w=np.zeros(r + (CENS_MAX_COMPONENTS + 1,)))
    _check(lib.nra_censored_bootstrap(
        device, len(y), _ptr(y, C.c_double), n, _ptr(po, C.c_int64), _ptr(pn, C.c_int32), _ptr(pe, C.c_int32),
        _ptr(pt, C.c_double), _ptr(pl, C.c_double), n_rep, _ptr(ix, C.c_int32), _ptr(rm, C.c_int32), int(max_alleles),
        int(max_iter), float(tol), flags, _ptr(out["status"], C.c_int32), _ptr(out["model_n"], C.c_int32),
        _ptr(out["model_open"], C.c_int32), _ptr(out["best_start"], C.c_int32), _ptr(out["n_iter"], C.c_int32),
        _ptr(out["ll"], C.c_double), _ptr(out["bic"], C.c_double), _ptr(out["nu"], C.c_double),
        _ptr(out["w"], C.c_double)))
    return out


BOOT_DECIDED, BOOT_NEEDS_MORE = 0, 1      # NRA_BOOT_DECIDED, NRA_BOOT_NEEDS_MORE
BOOT_STARTS = 10
BOOT_COPIES = 100


def boot_start_rows(first_n, n_cap):
    """The start rows nra_mixture_bootstrap reads for a problem: ten starts of n rows for every order it may fit."""
    return sum(BOOT_STARTS * n for n in range(max(int(first_n), 2), int(n_cap) + 1))


def mixture_bootstrap(x, z, prob_m, prob_d, prob_e, prob_zo, prob_first_n, prob_n_cap, prob_max_n, starts, n_rep, idx,
                      flags=0, device=0):
    """nra_mixture_bootstrap: the order search of n_rep replicates of every problem.  x, z, starts, idx: the problems'
    kept sizes (m * d each), noise (100 m d), start rows (boot_start_rows) and resampling indices (n_rep * m), each
    concatenated in problem order -> dict(status, order, best_start, lb [problems, n_rep]; off = where a problem's
    components begin (n_rep * n_cap each, replicate-major); w [components], mu and var [components, 2])."""
    lib = load()
    xs = np.ascontiguousarray(x, np.float64).ravel()
    zs = np.ascontiguousarray(z, np.float64).ravel()
    pm = np.ascontiguousarray(prob_m, np.int32)
    pd = np.ascontiguousarray(prob_d, np.int32)
    pe = np.ascontiguousarray(prob_e, np.float64)
    pz = np.ascontiguousarray(prob_zo, np.float64)
    pf = np.ascontiguousarray(prob_first_n, np.int32)
    pc = np.ascontiguousarray(prob_n_cap, np.int32)
    px = np.ascontiguousarray(prob_max_n, np.int32)
    st = np.ascontiguousarray(starts, np.int32).ravel()
    ix = np.ascontiguousarray(idx, np.int32).ravel()
    n_rep = int(n_rep)
    n = len(pm)
    if not all(len(v) == n for v in (pd, pe, pz, pf, pc, px)):
        raise ValueError("one entry per problem in every problem array")
    md = np.maximum(pm, 0).astype(np.int64) * np.maximum(pd, 0)

    def offsets(sizes):
        off = np.zeros(n + 1, np.int64)
        np.cumsum(sizes, out=off[1:])
        return off

    x_off, z_off = offsets(md), offsets(md * BOOT_COPIES)
    s_off = offsets([boot_start_rows(f, c) for f, c in zip(pf, pc)])
    off = offsets(max(n_rep, 0) * np.maximum(pc, 0).astype(np.int64))
    if len(xs) != x_off[-1] or len(zs) != z_off[-1] or len(st) != s_off[-1]:
        raise ValueError("x, z and starts must hold exactly what the problems need")
    if len(ix) != max(n_rep, 0) * int(np.maximum(pm, 0).sum()):
        raise ValueError("n_rep * m indices per problem")
    r, t = (n, max(n_rep, 0)), int(off[-1])
    out = dict(status=np.zeros(r, np.int32), order=np.zeros(r, np.int32), best_start=np.zeros(r, np.int32),
               lb=np.zeros(r), off=off, w=np.zeros(t), mu=np.zeros((t, 2)), var=np.zeros((t, 2)))
    _check(lib.nra_mixture_bootstrap(
        device, len(xs), _ptr(xs, C.c_double), len(zs), _ptr(zs, C.c_double), n, _ptr(pm, C.c_int32),
        _ptr(pd, C.c_int32), _ptr(x_off, C.c_int64), _ptr(z_off, C.c_int64), _ptr(pe, C.c_double), _ptr(pz, C.c_double),
        _ptr(pf, C.c_int32), _ptr(pc, C.c_int32), _ptr(px, C.c_int32), _ptr(s_off, C.c_int64), len(st),
        _ptr(st, C.c_int32), n_rep, _ptr(ix, C.c_int32), flags, _ptr(out["status"], C.c_int32),
        _ptr(out["order"], C.c_int32), _ptr(out["best_start"], C.c_int32), _ptr(out["lb"], C.c_double),
        _ptr(out["w"], C.c_double), _ptr(out["mu"], C.c_double), _ptr(out["var"], C.c_double)))
    return out


CONS_MAX_DIST = 1000      # NRA_CONS_MAX_DIST: the largest, and the default, max_dist of nra_tract_consensus
CONS_STATS = ("aligned_64", "aligned_128", "aligned_256", "aligned_512", "aligned_1024", "rows_64", "rows_128",
              "rows_256", "rows_512", "rows_1024", "rounds", "launches", "widened", "left_out_by_length",
              "max_pointer_bytes")


def tract_consensus(groups, max_dist=CONS_MAX_DIST, max_rounds=8, device=0):
    """nra_tract_consensus: the consensus of every group (a list of tracts) -> dict(consensus [str per group], support
    [int32 array per group], n_rounds, converged, voted, left_out [int32 per group], stats {name: count})."""
    lib = load()
    groups = [list(g) for g in groups]
    ng = len(groups)
    goff = np.zeros(ng + 1, np.int64)
    if ng:
        np.cumsum([len(g) for g in groups], out=goff[1:])
    tracts = [t for g in groups for t in g]
    data, off = pack_reads(tracts)
    cap = int(sum(2 * max((len(t) for t in g), default=0) + 64 for g in groups))
    cons = C.create_string_buffer(max(cap, 1))
    support = np.zeros(max(cap, 1), np.int32)
    coff = np.zeros(ng + 1, np.int64)
    res = np.zeros((ng, 4), np.int32)
    stats = np.zeros(16, np.int64)
    _check(lib.nra_tract_consensus(device, ng, _ptr(goff, C.c_int64), len(tracts), data, _ptr(off, C.c_int64),
                                   max_dist, max_rounds, cap, cons, _ptr(support, C.c_int32), _ptr(coff, C.c_int64),
                                   _ptr(res, C.c_int32), _ptr(stats, C.c_int64)))
    raw = cons.raw
    return dict(consensus=[raw[coff[g]:coff[g + 1]].decode("ascii") for g in range(ng)],
                support=[support[coff[g]:coff[g + 1]].copy() for g in range(ng)],
                n_rounds=res[:, 0].copy(), converged=res[:, 1].copy(), voted=res[:, 2].copy(),
                left_out=res[:, 3].copy(), stats={k: int(v) for k, v in zip(CONS_STATS, stats)})


SPLIT_DEFAULTS = dict(max_dist=CONS_MAX_DIST, min_count=3, min_share_pct=25, min_purity_pct=75, min_sites=1,
                      max_sites=256, max_iter=16)      # min_sites: chosen from the table of DESIGN.md section 19.3
SPLIT_STATS = CONS_STATS[:10] + ("sites", "launches", "widened", "left_out_by_length", "max_pointer_bytes",
                                 "groups_split")
SPLIT_RES = ("split", "n0", "n1", "undecided", "left_out", "n_sites", "n_supported", "iterations")


def allele_split(groups, backbones, device=0, **thresholds):
    """nra_allele_split: the tracts of every group piled up on its backbone, the variant sites and the two haplotypes
    (thresholds: SPLIT_DEFAULTS) -> dict(label, dist [int32 array per group: per tract], sites [int32 [n_sites, 12]
    per group: column, symbol of haplotype 0, of 1, A C G T counts of 0, of 1, supported], site_sym [uint8
    [n_sites, tracts] per group], split, n0, n1, undecided, left_out, n_sites, n_supported, iterations [int32 per
    group], stats {name: count})."""
    lib = load()
    unknown = set(thresholds) - set(SPLIT_DEFAULTS)
    if unknown:
        raise TypeError(f"allele_split: unknown threshold(s) {sorted(unknown)}")
    p = dict(SPLIT_DEFAULTS, **thresholds)
    groups = [list(g) for g in groups]
    backbones = list(backbones)
    ng = len(groups)
    if len(backbones) != ng:
        raise ValueError("one backbone per group")
    sizes = np.array([len(g) for g in groups], np.int64)
    goff = np.zeros(ng + 1, np.int64)
    np.cumsum(sizes, out=goff[1:])
    tracts = [t for g in groups for t in g]
    data, off = pack_reads(tracts)
    bdata, boff = pack_reads(backbones)
    nt = len(tracts)
    most = np.minimum(np.diff(boff), max(1, min(int(p["max_sites"]), 4096)))
    site_cap, sym_cap = int(most.sum()), int((most * sizes).sum())
    label, dist = np.zeros(max(nt, 1), np.int32), np.zeros(max(nt, 1), np.int32)
    res = np.zeros((ng, 8), np.int32)
    sites = np.zeros((max(site_cap, 1), 12), np.int32)
    sym = np.zeros(max(sym_cap, 1), np.uint8)
    soff, yoff = np.zeros(ng + 1, np.int64), np.zeros(ng + 1, np.int64)
    stats = np.zeros(16, np.int64)
    _check(lib.nra_allele_split(device, ng, _ptr(goff, C.c_int64), nt, data, _ptr(off, C.c_int64), bdata,
                                _ptr(boff, C.c_int64), *(int(p[k]) for k in SPLIT_DEFAULTS), _ptr(label, C.c_int32),
                                _ptr(dist, C.c_int32), _ptr(res, C.c_int32), site_cap, _ptr(sites, C.c_int32),
                                _ptr(soff, C.c_int64), sym_cap, _ptr(sym, C.c_uint8), _ptr(yoff, C.c_int64),
                                _ptr(stats, C.c_int64)))
    out = dict(label=[label[goff[g]:goff[g + 1]].copy() for g in range(ng)],
               dist=[dist[goff[g]:goff[g + 1]].copy() for g in range(ng)],
               sites=[sites[soff[g]:soff[g + 1]].copy() for g in range(ng)],
               site_sym=[sym[yoff[g]:yoff[g + 1]].reshape(int(soff[g + 1] - soff[g]), int(sizes[g])).copy()
                         for g in range(ng)],
               stats={k: int(v) for k, v in zip(SPLIT_STATS, stats)})
    for q, name in enumerate(SPLIT_RES):
        out[name] = res[:, q].copy()
    return out


FLANK_MAX_DIST = 500      # NRA_FLANK_MAX_DIST: the largest, and the default, max_dist of nra_flank_phase
FLANK_DEFAULTS = dict(max_dist=FLANK_MAX_DIST, skip=20, min_count=3, min_share_pct=25, min_purity_pct=75, min_sites=2,
                      max_sites=256, max_iter=16)
FLANK_RES = ("phased", "n0", "n1", "undecided", "left_out", "n_sites", "n_supported", "iterations")
FLANK_STATS = SPLIT_STATS[:15] + ("groups_phased",)


def flank_phase(groups, backbones, device=0, **thresholds):
    """nra_flank_phase: groups = per region a list of rows (left segment, right segment), backbones = per region
    (left side, right side), everything written from the repeat outward; an empty or None segment is absent
    (thresholds: FLANK_DEFAULTS) -> dict(label [int32 per row], dist, end [int32 [rows, 2]], sites [int32 [n_sites, 12]:
    group column, symbol of haplotype 0, of 1, A C G T counts of 0, of 1, supported], site_sym [uint8 [n_sites, rows]]
    per group, phased, n0, n1, undecided, left_out, n_sites, n_supported, iterations [int32 per group], stats)."""
    lib = load()
    unknown = set(thresholds) - set(FLANK_DEFAULTS)
    if unknown:
        raise TypeError(f"flank_phase: unknown threshold(s) {sorted(unknown)}")
    p = dict(FLANK_DEFAULTS, **thresholds)
    groups = [[(a or "", b or "") for a, b in g] for g in groups]
    backbones = [(a or "", b or "") for a, b in backbones]
    ng = len(groups)
    if len(backbones) != ng:
        raise ValueError("one pair of backbone sides per group")
    sizes = np.array([len(g) for g in groups], np.int64)
    goff = np.zeros(ng + 1, np.int64)
    np.cumsum(sizes, out=goff[1:])
    data, off = pack_reads([s for g in groups for row in g for s in row])
    bdata, boff = pack_reads([s for bb in backbones for s in bb])
    nr = int(goff[-1])
    most = np.minimum(boff[2::2] - boff[:-1:2], max(1, min(int(p["max_sites"]), 4096)))
    site_cap, sym_cap = int(most.sum()), int((most * sizes).sum())
    label = np.zeros(max(nr, 1), np.int32)
    dist, end = np.zeros((max(nr, 1), 2), np.int32), np.zeros((max(nr, 1), 2), np.int32)
    res = np.zeros((ng, 8), np.int32)
    sites = np.zeros((max(site_cap, 1), 12), np.int32)
    sym = np.zeros(max(sym_cap, 1), np.uint8)
    soff, yoff = np.zeros(ng + 1, np.int64), np.zeros(ng + 1, np.int64)
    stats = np.zeros(16, np.int64)
    _check(lib.nra_flank_phase(device, ng, _ptr(goff, C.c_int64), nr, data, _ptr(off, C.c_int64), bdata,
                               _ptr(boff, C.c_int64), *(int(p[k]) for k in FLANK_DEFAULTS), _ptr(label, C.c_int32),
                               _ptr(dist, C.c_int32), _ptr(end, C.c_int32), _ptr(res, C.c_int32), site_cap,
                               _ptr(sites, C.c_int32), _ptr(soff, C.c_int64), sym_cap, _ptr(sym, C.c_uint8),
                               _ptr(yoff, C.c_int64), _ptr(stats, C.c_int64)))
    out = dict(label=[label[goff[g]:goff[g + 1]].copy() for g in range(ng)],
               dist=[dist[goff[g]:goff[g + 1]].copy() for g in range(ng)],
               end=[end[goff[g]:goff[g + 1]].copy() for g in range(ng)],
               sites=[sites[soff[g]:soff[g + 1]].copy() for g in range(ng)],
               site_sym=[sym[yoff[g]:yoff[g + 1]].reshape(int(soff[g + 1] - soff[g]), int(sizes[g])).copy()
                         for g in range(ng)],
               stats={k: int(v) for k, v in zip(FLANK_STATS, stats)})
    for q, name in enumerate(FLANK_RES):
        out[name] = res[:, q].copy()
    return out


def tract_segments(sets, tracts, tract_set, switch_cost, device=0):
    """nra_tract_segments: the alignment of every tract against its motif set (sets[tract_set[i]], a list of motifs)
    with `switch_cost` for changing motif -> dict(edits, start_phase, start_motif, path, motif_of, path_off): the path
    bytes and the motif index per base of tract i are path / motif_of[path_off[i]:path_off[i + 1]]."""
    lib = load()
    sets = [list(x) for x in sets]
    soff = np.zeros(len(sets) + 1, np.int32)
    if sets:
        np.cumsum([len(x) for x in sets], out=soff[1:])
    mdata, moff = pack_reads([u for x in sets for u in x])
    data, off = pack_reads(list(tracts))
    ts = np.ascontiguousarray(tract_set, np.int32)
    n = len(off) - 1
    if len(ts) != n:
        raise ValueError("one set index per tract")
    out = dict(edits=np.zeros(n, np.int32), start_phase=np.zeros(n, np.int32), start_motif=np.zeros(n, np.int32),
               path=np.zeros(int(off[-1]), np.uint8), motif_of=np.zeros(int(off[-1]), np.uint8), path_off=off)
    _check(lib.nra_tract_segments(device, len(sets), _ptr(soff, C.c_int32), mdata, _ptr(moff, C.c_int64), n, data,
                                  _ptr(off, C.c_int64), _ptr(ts, C.c_int32), int(switch_cost),
                                  _ptr(out["edits"], C.c_int32), _ptr(out["start_phase"], C.c_int32),
                                  _ptr(out["start_motif"], C.c_int32), _ptr(out["path"], C.c_uint8),
                                  _ptr(out["motif_of"], C.c_uint8)))
    return out
