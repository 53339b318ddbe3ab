"""Host-side mirror of the reference's interface for the hot path, over the C ABI.

Class / method names follow the reference (SNAPLib/BaseAligner.h:44-90, GenomeIndex.h:33-80,
LandauVishkin.h:100): `BaseAligner.AlignRead` here takes a *batch* of reads because a GPU
aligner is fed batches, but argument meaning, result fields (SingleAlignmentResult) and error
behaviour follow the reference.  All computation happens in libsnapgpu.so (HIP, gfx950);
there is no CPU path -- if the library or a GPU is missing, construction raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .abi import (Counters, IndexView, Params, RESULT_DTYPE, W_TEXT_TRUNCATED, default_params, ptr)
from .index import GENOME_PAD, GenomeIndex

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsnapgpu.so")      # the product opens this file and nothing else

_lib = None


class SnapGpuError(RuntimeError):
    pass


def load_library():
    """dlopen libsnapgpu.so (built by __graft_entry__.build()); fails loudly if missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SnapGpuError("%s not built: run `python -c 'import __graft_entry__ as g; g.build()'`" % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        lib.snapgpu_last_error.restype = C.c_char_p
        lib.snapgpu_last_error.argtypes = [C.c_void_p]
        lib.snapgpu_create.argtypes = [C.POINTER(IndexView), C.POINTER(Params), C.c_int, C.POINTER(C.c_void_p)]
        lib.snapgpu_destroy.argtypes = [C.c_void_p]
        lib.snapgpu_destroy.restype = None
        lib.snapgpu_align_single_device.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 6
        _lib = lib
    return _lib


W_RECORDS_TRUNCATED = 2          # SNAPGPU_W_RECORDS_TRUNCATED (include/snapgpu.h)

EXPORTED_SYMBOLS = [
    "snapgpu_abi_version", "snapgpu_last_error", "snapgpu_default_params", "snapgpu_create",
    "snapgpu_destroy", "snapgpu_create_from_directory", "snapgpu_device_count", "snapgpu_create_replica", "snapgpu_broadcast_index", "snapgpu_default_paired_params", "snapgpu_enable_paired",
    "snapgpu_align_paired", "snapgpu_align_paired_device", "snapgpu_index_device_ptrs", "snapgpu_lookup_seeds",
    "snapgpu_lookup_seeds_device", "snapgpu_landau_vishkin", "snapgpu_affine_gap", "snapgpu_align_single",
    "snapgpu_align_single_device", "snapgpu_get_counters", "snapgpu_kernel_time",
    "snapgpu_enable_secondary", "snapgpu_align_single_secondary", "snapgpu_align_single_secondary_device",
    "snapgpu_align_paired_secondary", "snapgpu_align_paired_secondary_device",
    "snapgpu_compute_cigar_lv", "snapgpu_compute_cigar_ag", "snapgpu_adjust_alignments", "snapgpu_set_aligner_flags", "snapgpu_affine_gap_sequence", "snapgpu_sam_fields_single", "snapgpu_sam_fields_single_device", "snapgpu_sam_fields_paired", "snapgpu_sam_fields_paired_device", "snapgpu_align_sam_single", "snapgpu_align_sam_single_records", "snapgpu_align_sam_single_records_device", "snapgpu_set_contig_names", "snapgpu_sam_text_single", "snapgpu_sam_text_single_device", "snapgpu_align_sam_single_text", "snapgpu_align_sam_paired", "snapgpu_sam_text_paired", "snapgpu_sam_text_paired_device", "snapgpu_align_sam_paired_text","snapgpu_create_replica_with_params",
    "snapgpu_set_contig_bam_ids", "snapgpu_bam_records_single", "snapgpu_bam_records_single_device", "snapgpu_align_sam_single_bam",
    "snapgpu_bam_records_paired", "snapgpu_bam_records_paired_device", "snapgpu_align_sam_paired_bam",
    "snapgpu_bgzf_compress", "snapgpu_bgzf_compress_device", "snapgpu_align_sam_single_bgzf", "snapgpu_align_sam_paired_bgzf",
    "snapgpu_bam_sort", "snapgpu_bam_sort_device", "snapgpu_align_sam_single_bam_sorted", "snapgpu_align_sam_paired_bam_sorted",
    "snapgpu_default_index_build_params", "snapgpu_index_build", "snapgpu_index_build_from_fasta", "snapgpu_index_build_shaped",
    "snapgpu_index_build_from_fasta_shaped", "snapgpu_built_index_view",
    "snapgpu_built_index_save", "snapgpu_built_index_stats", "snapgpu_built_index_destroy",
]


def _pack(strings):
    lens = np.array([len(s) for s in strings], dtype=np.int32)
    offs = np.zeros(len(strings), dtype=np.uint32)
    if len(strings):
        offs[1:] = np.cumsum(lens[:-1])
    buf = np.frombuffer(b"".join(strings) + b"\0" * 16, dtype=np.uint8).copy()
    return buf, offs, lens


def make_index_view(index: GenomeIndex, device_index_ptrs=None):
    """snapgpu_index_view over the arrays of a loaded index; returns (view, arrays to keep alive)."""
    keep = []
    v = IndexView()
    v.seed_len = index.seed_len
    v.key_bytes = index.key_bytes
    v.n_hash_tables = index.n_hash_tables
    v.large_hash_table = 1 if index.large else 0
    v.location_size = index.location_size
    v.chromosome_padding = index.chromosome_padding
    sizes = getattr(index, "_device_sizes", None)      # set by dist.broadcast_index on every rank
    v.overflow_table_size = sizes[1] if sizes else index.overflow.size
    v.hash_blob_bytes = sizes[0] if sizes else index.hash_blob.size
    toff = np.ascontiguousarray(index.table_offset, dtype=np.uint64)
    tsz = np.ascontiguousarray(index.table_size, dtype=np.uint64)
    cb = np.ascontiguousarray(index.contig_begin, dtype=np.uint64)
    keep += [toff, tsz, cb]
    v.table_offset = toff.ctypes.data
    v.table_size = tsz.ctypes.data
    v.contig_begin = cb.ctypes.data
    v.n_contigs = len(index.contigs)
    v.n_bases = index.n_bases
    v.genome_pad = GENOME_PAD
    v.first_alt_location = index.first_alt_location
    pb, prc, cst, cops = index.projection_arrays()
    keep += [pb, prc, cst, cops]
    v.contig_proj_begin = pb.ctypes.data
    v.contig_proj_rc = prc.ctypes.data
    v.contig_cigar_start = cst.ctypes.data
    v.cigar_ops = cops.ctypes.data
    if device_index_ptrs is None:
        v.hash_blob = index.hash_blob.ctypes.data
        v.overflow = index.overflow.ctypes.data
        v.genome = index.genome_padded.ctypes.data + GENOME_PAD
        v.on_device = 0
    else:                                   # (hash, overflow, genome_padded) device addresses
        v.hash_blob, v.overflow = int(device_index_ptrs[0]), int(device_index_ptrs[1])
        v.genome = int(device_index_ptrs[2]) + GENOME_PAD
        v.on_device = 1
    return v, keep


class BaseAligner:
    """One aligner context on one GPU (the analogue of one BaseAligner per CPU thread)."""

    def __init__(self, index: GenomeIndex, params: Params | None = None, device: int = 0,
                 device_index_ptrs=None):
        self.lib = load_library()
        self.index = index
        self.params = params if params is not None else default_params()
        self._keep = []
        v, keep = make_index_view(index, device_index_ptrs)
        self._keep += keep
        handle = C.c_void_p()
        rc = self.lib.snapgpu_create(C.byref(v), C.byref(self.params), device, C.byref(handle))
        if rc != 0:
            raise SnapGpuError("snapgpu_create failed (%d): %s" % (rc, self.lib.snapgpu_last_error(None).decode()))
        self.handle = handle
        self.device = device

    @classmethod
    def from_built_index(cls, built, index: GenomeIndex | None = None, params: Params | None = None, device: int = 0, paired_params=None):
        """A context over an index that snapgpu_index_build* left in HBM (snap_amd.index.BuiltIndex): the view is adopted as it is
        (on_device = 1), nothing is copied and no file is read.  `built` must outlive the aligner."""
        self = cls.__new__(cls)
        self.lib = load_library()
        self.index = index
        self.params = params if params is not None else default_params()
        self._keep = [built]
        v = built.view()
        handle = C.c_void_p()
        rc = self.lib.snapgpu_create(C.byref(v), C.byref(self.params), device, C.byref(handle))
        if rc != 0:
            raise SnapGpuError("snapgpu_create over a built index failed (%d): %s" % (rc, self.lib.snapgpu_last_error(None).decode()))
        self.handle = handle
        self.device = device
        self._after_built(paired_params)
        return self

    @classmethod
    def from_directory(cls, directory: str, params: Params | None = None, device: int = 0):
        """snapgpu_create_from_directory: the library's own loader of the reference's four index files (what the shim and snapgpu-sam use)."""
        self = cls.__new__(cls)
        self.lib = load_library()
        self.index = None
        self.params = params if params is not None else default_params()
        self._keep = []
        self.lib.snapgpu_create_from_directory.argtypes = [C.c_char_p, C.POINTER(Params), C.c_int, C.POINTER(C.c_void_p)]
        handle = C.c_void_p()
        rc = self.lib.snapgpu_create_from_directory(directory.encode(), C.byref(self.params), device, C.byref(handle))
        if rc != 0:
            raise SnapGpuError("snapgpu_create_from_directory failed (%d): %s" % (rc, self.lib.snapgpu_last_error(None).decode()))
        self.handle = handle
        self.device = device
        return self

    def _after_built(self, paired_params):
        pass

    def replica(self, device: int | None = None, share_index: bool = True, params: Params | None = None):
        """Another context over the same index (include/snapgpu.h: snapgpu_create_replica): on this GPU sharing the resident blobs -- a
        second feeder, so that two batches can be in flight -- or on another GPU with blobs of its own (to be filled by
        snapgpu_broadcast_index).  The analogue of the reference's one-aligner-per-thread over one shared GenomeIndex
        (SNAPLib/AlignerContext.cpp: runTask).  `params`: options of its own for the new context (snapgpu_create_replica_with_params),
        e.g. another -d over the one resident index."""
        self.lib.snapgpu_create_replica_with_params.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(Params), C.POINTER(C.c_void_p)]
        h = C.c_void_p()
        dev = self.device if device is None else device
        rc = self.lib.snapgpu_create_replica_with_params(self.handle, C.c_int(dev), C.c_int(1 if share_index else 0),
                                                         C.byref(params) if params is not None else None, C.byref(h))
        if rc != 0:
            raise SnapGpuError("snapgpu_create_replica failed (%d): %s" % (rc, self.lib.snapgpu_last_error(self.handle).decode()))
        other = type(self).__new__(type(self))
        other.__dict__.update(self.__dict__)
        other.handle = h
        other.device = dev
        if params is not None:
            other.params = params
        other._after_replica()
        return other

    def _after_replica(self):
        pass

    def close(self):
        if getattr(self, "handle", None):
            self.lib.snapgpu_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise SnapGpuError("%s failed (%d): %s" % (what, rc, self.lib.snapgpu_last_error(self.handle).decode()))

    # ---- GenomeIndex::lookupSeed32 ------------------------------------------------------
    def lookupSeed32(self, seeds: np.ndarray, max_hits_out: int = 512):
        seeds = np.ascontiguousarray(seeds, dtype=np.uint8)
        n = seeds.shape[0]
        n_hits = np.zeros((n, 2), dtype=np.int64)
        hits = np.zeros((n, 2, max_hits_out), dtype=np.uint32)
        self._check(self.lib.snapgpu_lookup_seeds(self.handle, C.c_uint32(n), ptr(seeds), ptr(n_hits), ptr(hits),
                                                  C.c_uint32(max_hits_out)), "snapgpu_lookup_seeds")
        return n_hits, hits

    def lookup_device(self, n: int, d_seeds: int, d_n_hits: int, d_hits: int = 0, max_hits_out: int = 300, stream: int = 0):
        """GenomeIndex::lookupSeed32 for n seeds already in HBM (device pointers); d_hits = 0: hit counts only (lists read, not stored).
        Timed and counted like the align kernels: the stand-alone index-probe kernel."""
        self._check(self.lib.snapgpu_lookup_seeds_device(self.handle, C.c_uint32(n), C.c_void_p(d_seeds), C.c_void_p(d_n_hits),
                                                         C.c_void_p(d_hits) if d_hits else None, C.c_uint32(max_hits_out),
                                                         C.c_void_p(stream) if stream else None), "snapgpu_lookup_seeds_device")

    # ---- LandauVishkin<dir>::computeEditDistance ---------------------------------------
    def computeEditDistance(self, direction: int, texts, patterns, quals, k):
        n = len(texts)
        tbuf, toff, tlen = _pack(texts)
        if direction == -1:
            toff = (toff + tlen.astype(np.uint32)).astype(np.uint32)
        pbuf, poff, plen = _pack(patterns)
        qbuf, _, _ = _pack(quals)
        k = np.ascontiguousarray(k, dtype=np.int32)
        score = np.zeros(n, np.int32); prob = np.zeros(n, np.float64)
        net = np.zeros(n, np.int32); tot = np.zeros(n, np.int32); span = np.zeros(n, np.int32)
        self._check(self.lib.snapgpu_landau_vishkin(
            self.handle, C.c_int(direction), C.c_uint32(n), ptr(tbuf), C.c_uint64(tbuf.size), ptr(toff), ptr(tlen),
            ptr(pbuf), ptr(qbuf), C.c_uint64(pbuf.size), ptr(poff), ptr(plen), ptr(k),
            ptr(score), ptr(prob), ptr(net), ptr(tot), ptr(span)), "snapgpu_landau_vishkin")
        return dict(score=score, match_probability=prob, net_indel=net, total_indels=tot, text_span=span)

    # ---- AffineGapVectorized<dir>::computeScore[Banded] --------------------------------
    def computeScoreAffine(self, direction: int, texts, patterns, quals, w, score_init, is_rc, banded, use_clip=None, sequence: bool = False):
        """sequence=True: the problems are calls in order on ONE newly constructed object (snapgpu_affine_gap_sequence); the result then
        also has stale_steps."""
        n = len(texts)
        tbuf, toff, tlen = _pack(texts)
        if direction == -1:
            toff = (toff + tlen.astype(np.uint32)).astype(np.uint32)
        pbuf, poff, plen = _pack(patterns)
        qbuf, _, _ = _pack(quals)
        w = np.ascontiguousarray(w, dtype=np.int32)
        score_init = np.ascontiguousarray(score_init, dtype=np.int32)
        is_rc = np.ascontiguousarray(is_rc, dtype=np.uint8)
        banded = np.ascontiguousarray(banded, dtype=np.uint8)
        use_clip = np.zeros(n, np.uint8) if use_clip is None else np.ascontiguousarray(use_clip, dtype=np.uint8)
        ag = np.zeros(n, np.int32); to = np.zeros(n, np.int32); po = np.zeros(n, np.int32)
        ne = np.zeros(n, np.int32); prob = np.zeros(n, np.float64)
        if sequence:
            stale = np.zeros(n, np.int32)
            self._check(self.lib.snapgpu_affine_gap_sequence(
                self.handle, C.c_int(direction), C.c_uint32(n), ptr(tbuf), C.c_uint64(tbuf.size), ptr(toff), ptr(tlen),
                ptr(pbuf), ptr(qbuf), C.c_uint64(pbuf.size), ptr(poff), ptr(plen), ptr(w), ptr(score_init),
                ptr(is_rc), ptr(banded), ptr(use_clip), ptr(ag), ptr(to), ptr(po), ptr(ne), ptr(prob), ptr(stale)), "snapgpu_affine_gap_sequence")
            return dict(ag_score=ag, text_offset=to, pattern_offset=po, n_edits=ne, match_probability=prob, stale_steps=stale)
        self._check(self.lib.snapgpu_affine_gap(
            self.handle, C.c_int(direction), C.c_uint32(n), ptr(tbuf), C.c_uint64(tbuf.size), ptr(toff), ptr(tlen),
            ptr(pbuf), ptr(qbuf), C.c_uint64(pbuf.size), ptr(poff), ptr(plen), ptr(w), ptr(score_init),
            ptr(is_rc), ptr(banded), ptr(use_clip), ptr(ag), ptr(to), ptr(po), ptr(ne), ptr(prob)), "snapgpu_affine_gap")
        return dict(ag_score=ag, text_offset=to, pattern_offset=po, n_edits=ne, match_probability=prob)

    # ---- SAMFormat::computeCigar (Landau-Vishkin variant) over a batch ------------------
    def computeCigar(self, data, off, length, loc, extra_before, use_m: bool = False, ops_stride: int = 64):
        """SAM.cpp:2354-2467 for a batch of written reads (see snapgpu_compute_cigar_lv in include/snapgpu.h): data = the clipped
        reads in reference orientation (one uint8 buffer), item i = data[off[i] : off[i] + length[i]] at genome location loc[i].
        Returns dict(ops uint32[n, ops_stride], n_ops, edit_distance, add_front_clipping, extra_clipped_after)."""
        data = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
        off = np.ascontiguousarray(off, dtype=np.uint64); length = np.ascontiguousarray(length, dtype=np.int32)
        loc = np.ascontiguousarray(loc, dtype=np.int64); extra_before = np.ascontiguousarray(extra_before, dtype=np.int32)
        n = off.size
        ops = np.zeros((n, ops_stride), dtype=np.uint32); n_ops = np.zeros(n, np.int32); ed = np.zeros(n, np.int32)
        afc = np.zeros(n, np.int32); after = np.zeros(n, np.int64)
        self._check(self.lib.snapgpu_compute_cigar_lv(
            self.handle, C.c_uint32(n), ptr(data), C.c_uint64(data.size), ptr(off), ptr(length), ptr(loc), ptr(extra_before),
            C.c_int(1 if use_m else 0), ptr(ops), C.c_uint32(ops_stride), ptr(n_ops), ptr(ed), ptr(afc), ptr(after)),
            "snapgpu_compute_cigar_lv")
        return dict(ops=ops, n_ops=n_ops, edit_distance=ed, add_front_clipping=afc, extra_clipped_after=after)

    def AdjustAlignments(self, data, off, length, results):
        """AlignmentAdjuster::AdjustAlignment (AlignmentAdjuster.cpp:33-190) for a batch (snapgpu_adjust_alignments): read i =
        data[off[i] : off[i] + length[i]] as given to AlignRead; results (RESULT_DTYPE) carry status / direction / location / score in and
        come back with status / location / score / clipping_for_read_adjustment adjusted.  Returns the adjusted copy."""
        data = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
        off = np.ascontiguousarray(off, dtype=np.uint64); length = np.ascontiguousarray(length, dtype=np.int32)
        out = np.ascontiguousarray(results, dtype=RESULT_DTYPE).copy()
        self._check(self.lib.snapgpu_adjust_alignments(self.handle, C.c_uint32(off.size), ptr(data), C.c_uint64(data.size), ptr(off), ptr(length), ptr(out)),
                    "snapgpu_adjust_alignments")
        return out

    def computeCigarAffineGap(self, data, quals, off, length, loc, extra_before, score, use_m: bool = False, ops_stride: int = 64):
        """SAM.cpp:2470-2588 (the CIGAR of a read scored with affine gap) for a batch; see snapgpu_compute_cigar_ag.  score = the
        alignment's edit distance.  Returns the fields of computeCigar plus back_clipping_missed and stale (the reference's answer
        for that item depends on what its object computed before)."""
        data = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
        quals = np.ascontiguousarray(quals, dtype=np.uint8).reshape(-1)
        off = np.ascontiguousarray(off, dtype=np.uint64); length = np.ascontiguousarray(length, dtype=np.int32)
        loc = np.ascontiguousarray(loc, dtype=np.int64); extra_before = np.ascontiguousarray(extra_before, dtype=np.int32)
        score = np.ascontiguousarray(score, dtype=np.int32)
        n = off.size
        ops = np.zeros((n, ops_stride), dtype=np.uint32); n_ops = np.zeros(n, np.int32); ed = np.zeros(n, np.int32)
        afc = np.zeros(n, np.int32); after = np.zeros(n, np.int64); tail = np.zeros(n, np.int32); stale = np.zeros(n, np.int32)
        self._check(self.lib.snapgpu_compute_cigar_ag(
            self.handle, C.c_uint32(n), ptr(data), ptr(quals), C.c_uint64(data.size), ptr(off), ptr(length), ptr(loc), ptr(extra_before),
            ptr(score), C.c_int(1 if use_m else 0), ptr(ops), C.c_uint32(ops_stride), ptr(n_ops), ptr(ed), ptr(afc), ptr(after),
            ptr(tail), ptr(stale)), "snapgpu_compute_cigar_ag")
        return dict(ops=ops, n_ops=n_ops, edit_distance=ed, add_front_clipping=afc, extra_clipped_after=after,
                    back_clipping_missed=tail, stale=stale)

    def samFields(self, bases, quals, offsets, front_clip, data_len, results, use_m: bool = False, ops_stride: int = 64):
        """SimpleReadWriter::writeReads + SAMFormat::writeRead up to the point of printing, for the primary results of a batch of
        single-end reads (see snapgpu_sam_fields_single).  bases / quals / offsets: the unclipped reads; front_clip / data_len:
        Read::clip's outcome; results: RESULT_DTYPE array.  Returns dict(flag, contig, pos, mapq, ops, n_ops, nm, stale)."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8).reshape(-1); quals = np.ascontiguousarray(quals, dtype=np.uint8).reshape(-1)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        front_clip = np.ascontiguousarray(front_clip, dtype=np.int32); data_len = np.ascontiguousarray(data_len, dtype=np.int32)
        results = np.ascontiguousarray(results, dtype=RESULT_DTYPE)
        n = offsets.size - 1
        flag = np.zeros(n, np.int32); contig = np.zeros(n, np.int32); pos = np.zeros(n, np.int64); mapq = np.zeros(n, np.int32)
        ops = np.zeros((n, ops_stride), dtype=np.uint32); n_ops = np.zeros(n, np.int32); nm = np.zeros(n, np.int32); stale = np.zeros(n, np.int32)
        self._check(self.lib.snapgpu_sam_fields_single(
            self.handle, C.c_uint32(n), ptr(bases), ptr(quals), ptr(offsets), ptr(front_clip), ptr(data_len), ptr(results),
            C.c_int(1 if use_m else 0), ptr(flag), ptr(contig), ptr(pos), ptr(mapq), ptr(ops), C.c_uint32(ops_stride), ptr(n_ops), ptr(nm),
            ptr(stale)), "snapgpu_sam_fields_single")
        return dict(flag=flag, contig=contig, pos=pos, mapq=mapq, ops=ops, n_ops=n_ops, nm=nm, stale=stale)

    def alignSam(self, bases, quals, offsets, front_clip, data_len, skip, use_m: bool = False, ops_stride: int = 64):
        """The single-end path of a SAM writer in one call (snapgpu_align_sam_single): BaseAligner::AlignRead over the clipped reads
        (SingleAligner.cpp:250) and SimpleReadWriter::writeReads' computed fields for each primary result, the batch uploaded once.
        bases / quals / offsets: the unclipped reads; front_clip / data_len: Read::clip's outcome; skip[i] != 0: the read is not given to
        the aligner (SingleAligner.cpp:211-232).  Returns (results, first_alt, dict(flag, contig, pos, mapq, ops, n_ops, nm, stale))."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8).reshape(-1); quals = np.ascontiguousarray(quals, dtype=np.uint8).reshape(-1)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        front_clip = np.ascontiguousarray(front_clip, dtype=np.int32); data_len = np.ascontiguousarray(data_len, dtype=np.int32)
        skip = np.ascontiguousarray(skip, dtype=np.uint8)
        n = offsets.size - 1
        results = np.zeros(n, dtype=RESULT_DTYPE); first_alt = np.zeros(n, dtype=RESULT_DTYPE)
        flag = np.zeros(n, np.int32); contig = np.zeros(n, np.int32); pos = np.zeros(n, np.int64); mapq = np.zeros(n, np.int32)
        ops = np.zeros((n, ops_stride), dtype=np.uint32); n_ops = np.zeros(n, np.int32); nm = np.zeros(n, np.int32); stale = np.zeros(n, np.int32)
        self._check(self.lib.snapgpu_align_sam_single(
            self.handle, C.c_uint32(n), ptr(bases), ptr(quals), ptr(offsets), ptr(front_clip), ptr(data_len), ptr(skip),
            C.c_int(1 if use_m else 0), ptr(results), ptr(first_alt), ptr(flag), ptr(contig), ptr(pos), ptr(mapq), ptr(ops),
            C.c_uint32(ops_stride), ptr(n_ops), ptr(nm), ptr(stale)), "snapgpu_align_sam_single")
        return results, first_alt, dict(flag=flag, contig=contig, pos=pos, mapq=mapq, ops=ops, n_ops=n_ops, nm=nm, stale=stale)

    def alignSamRecords(self, bases, quals, offsets, front_clip, data_len, skip, use_m: bool = False, ops_stride: int = 64,
                        adjust_primary: bool = False, capacity: int | None = None, secondary_stride: int = 0, grow: bool = True):
        """Single-end reads to ALL their SAM records in one call (snapgpu_align_sam_single_records): -om / -omax / -mpc through
        enable_secondary on this context, -ae through its adjust argument (or adjust_primary on a context without secondary results), -ea
        through params.emit_alt_alignments.  Inputs as alignSam.  capacity: records the per-record arrays have room for (default: one
        and a half per read); grow: call again with the count the library asks for when that was too few -- otherwise the truncated
        answer is returned with truncated=True.  secondary_stride > 0: also return the strided secondary results.
        Returns dict(n_records, truncated, rec_begin, rec_read, rec_kind, flag, contig, pos, mapq, ops, n_ops, nm, stale, results,
        first_alt, n_secondary[, secondary]); the per-record arrays are cut to the records that were written."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8).reshape(-1); quals = np.ascontiguousarray(quals, dtype=np.uint8).reshape(-1)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        front_clip = np.ascontiguousarray(front_clip, dtype=np.int32); data_len = np.ascontiguousarray(data_len, dtype=np.int32)
        skip = np.ascontiguousarray(skip, dtype=np.uint8)
        n = offsets.size - 1
        cap = int(capacity) if capacity is not None else n + n // 2 + 16
        results = np.zeros(n, dtype=RESULT_DTYPE); first_alt = np.zeros(n, dtype=RESULT_DTYPE); n_secondary = np.zeros(n, np.uint32)
        secondary = np.zeros((n, secondary_stride), dtype=RESULT_DTYPE) if secondary_stride else None
        rec_begin = np.zeros(n + 1, np.uint64)
        f = self.lib.snapgpu_align_sam_single_records
        f.argtypes = ([C.c_void_p, C.c_uint32] + [C.c_void_p] * 6 + [C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_uint32, C.c_void_p, C.c_uint64] +
                      [C.c_void_p] * 9 + [C.c_uint32] + [C.c_void_p] * 3)
        while True:
            rec_read = np.zeros(cap, np.uint32); rec_kind = np.zeros(cap, np.uint8)
            flag = np.zeros(cap, np.int32); contig = np.zeros(cap, np.int32); pos = np.zeros(cap, np.int64); mapq = np.zeros(cap, np.int32)
            ops = np.zeros((cap, ops_stride), dtype=np.uint32); n_ops = np.zeros(cap, np.int32); nm = np.zeros(cap, np.int32); stale = np.zeros(cap, np.int32)
            n_rec = C.c_uint64(0)
            rc = f(self.handle, n, ptr(bases), ptr(quals), ptr(offsets), ptr(front_clip), ptr(data_len), ptr(skip), 1 if use_m else 0,
                   1 if adjust_primary else 0, ptr(results), ptr(first_alt), ptr(secondary) if secondary is not None else None, secondary_stride,
                   ptr(n_secondary), cap, C.addressof(n_rec), ptr(rec_begin), ptr(rec_read), ptr(rec_kind), ptr(flag), ptr(contig), ptr(pos),
                   ptr(mapq), ptr(ops), ops_stride, ptr(n_ops), ptr(nm), ptr(stale))
            if rc == W_RECORDS_TRUNCATED and grow:
                cap = int(n_rec.value)
                continue
            if rc != W_RECORDS_TRUNCATED:
                self._check(rc, "snapgpu_align_sam_single_records")
            break
        m = min(int(n_rec.value), cap)
        out = dict(n_records=int(n_rec.value), truncated=rc == W_RECORDS_TRUNCATED, rec_begin=rec_begin, rec_read=rec_read[:m], rec_kind=rec_kind[:m],
                   flag=flag[:m], contig=contig[:m], pos=pos[:m], mapq=mapq[:m], ops=ops[:m], n_ops=n_ops[:m], nm=nm[:m], stale=stale[:m],
                   results=results, first_alt=first_alt, n_secondary=n_secondary)
        if secondary is not None:
            out["secondary"] = secondary
        return out

    def alignSamRecords_device(self, n: int, max_read_len: int, d_bases: int, d_quals: int, d_offsets: int, d_front_clip: int, d_data_len: int, d_skip: int,
                               capacity: int, d_rec_begin: int, d_rec_read: int, d_rec_kind: int, d_flag: int, d_contig: int, d_pos: int, d_mapq: int,
                               d_ops: int, ops_stride: int, d_n_ops: int, d_nm: int, d_stale: int, use_m: bool = False, adjust_primary: bool = False,
                               d_results: int = 0, d_first_alt: int = 0, d_secondary: int = 0, secondary_stride: int = 0, d_n_secondary: int = 0, stream: int = 0):
        """Device-pointer form of alignSamRecords (snapgpu_align_sam_single_records_device): the reads, Read::clip's outcome, skip and every
        output array already in HBM (the result arrays are optional: 0).  Synchronous on `stream` (0: the context's).
        Returns (n_records, truncated)."""
        vp = lambda x: C.c_void_p(x) if x else None
        f = self.lib.snapgpu_align_sam_single_records_device
        f.argtypes = ([C.c_void_p, C.c_uint32, C.c_uint32] + [C.c_void_p] * 6 + [C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_uint32, C.c_void_p, C.c_uint64] +
                      [C.c_void_p] * 9 + [C.c_uint32] + [C.c_void_p] * 4)
        n_rec = C.c_uint64(0)
        rc = f(self.handle, n, max_read_len, vp(d_bases), vp(d_quals), vp(d_offsets), vp(d_front_clip), vp(d_data_len), vp(d_skip), 1 if use_m else 0,
               1 if adjust_primary else 0, vp(d_results), vp(d_first_alt), vp(d_secondary), secondary_stride, vp(d_n_secondary), capacity, C.addressof(n_rec),
               vp(d_rec_begin), vp(d_rec_read), vp(d_rec_kind), vp(d_flag), vp(d_contig), vp(d_pos), vp(d_mapq), vp(d_ops), ops_stride, vp(d_n_ops), vp(d_nm),
               vp(d_stale), vp(stream))
        if rc != W_RECORDS_TRUNCATED:
            self._check(rc, "snapgpu_align_sam_single_records_device")
        return int(n_rec.value), rc == W_RECORDS_TRUNCATED

    # ---- records -> the bytes of their SAM lines (SAMFormat::createSAMLine / writeRead) ----
    def setContigNames(self, names):
        """snapgpu_set_contig_names: the RNAME of contig c is names[c] (str or bytes), one name per contig of the index."""
        enc = [n if isinstance(n, bytes) else str(n).encode() for n in names]
        arr = (C.c_char_p * max(len(enc), 1))(*enc)
        self.lib.snapgpu_set_contig_names.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        self._check(self.lib.snapgpu_set_contig_names(self.handle, C.c_uint32(len(enc)), C.cast(arr, C.c_void_p)), "snapgpu_set_contig_names")

    def samText(self, bases, quals, offsets, names, name_off, flag, contig, pos, mapq, ops, n_ops, nm, rec_read=None, capacity: int | None = None,
                grow: bool = True, text=None, _fn: str = "snapgpu_sam_text_single"):
        """The SAM lines of a batch's records (snapgpu_sam_text_single): bases / quals / offsets the unclipped reads, names / name_off
        (uint64[n_reads + 1]) their names, flag .. nm the records' fields as samFields / alignSamRecords return them (ops: [n_records,
        ops_stride]); rec_read: the read of each record (None: record i is read i).  capacity: bytes of text to make room for (default:
        an estimate); grow: call again with the size the library asks for when that was too few.  text: a uint8 array to write into
        (its size is the capacity).  Returns dict(text uint8[capacity], line_begin uint64[n_records + 1], text_bytes, truncated)."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8).reshape(-1); quals = np.ascontiguousarray(quals, dtype=np.uint8).reshape(-1)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        names = np.ascontiguousarray(names, dtype=np.uint8).reshape(-1); name_off = np.ascontiguousarray(name_off, dtype=np.uint64)
        flag = np.ascontiguousarray(flag, dtype=np.int32); contig = np.ascontiguousarray(contig, dtype=np.int32)
        pos = np.ascontiguousarray(pos, dtype=np.int64); mapq = np.ascontiguousarray(mapq, dtype=np.int32)
        ops = np.ascontiguousarray(ops, dtype=np.uint32); n_ops = np.ascontiguousarray(n_ops, dtype=np.int32); nm = np.ascontiguousarray(nm, dtype=np.int32)
        n_rec = flag.size
        ops_stride = ops.shape[1] if ops.ndim == 2 else (ops.size // n_rec if n_rec else 1)
        if rec_read is not None:
            rec_read = np.ascontiguousarray(rec_read, dtype=np.uint32)
        n_reads = offsets.size - 1
        cap = text.size if text is not None else (int(capacity) if capacity is not None else 2 * int(bases.size) + 256 * n_rec + 64)
        line_begin = np.zeros(n_rec + 1, np.uint64)
        f = getattr(self.lib, _fn)
        f.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32] + [C.c_void_p] * 11 + [C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64] + [C.c_void_p] * 3
        while True:
            if text is None or text.size != cap:
                text = np.zeros(cap, np.uint8)
            tb = C.c_uint64(0)
            rc = f(self.handle, n_rec, n_reads, ptr(bases), ptr(quals), ptr(offsets), ptr(names), ptr(name_off), ptr(rec_read) if rec_read is not None else None,
                   ptr(flag), ptr(contig), ptr(pos), ptr(mapq), ptr(ops), ops_stride, ptr(n_ops), ptr(nm), cap, ptr(text), ptr(line_begin), C.addressof(tb))
            if rc == W_TEXT_TRUNCATED and grow:
                cap = int(tb.value)
                continue
            if rc != W_TEXT_TRUNCATED:
                self._check(rc, _fn)
            return dict(text=text, line_begin=line_begin, text_bytes=int(tb.value), truncated=rc == W_TEXT_TRUNCATED)

    def samText_device(self, n_records: int, d_bases: int, d_quals: int, d_offsets: int, d_names: int, d_name_off: int, d_rec_read: int, d_flag: int,
                       d_contig: int, d_pos: int, d_mapq: int, d_ops: int, ops_stride: int, d_n_ops: int, d_nm: int, capacity: int, d_text: int,
                       d_line_begin: int, stream: int = 0, _fn: str = "snapgpu_sam_text_single_device"):
        """Device-pointer form of samText (snapgpu_sam_text_single_device): every array in HBM (d_rec_read 0: record i is read i), the text
        and line_begin left there.  Synchronous on `stream` (0: the context's).  Returns (text_bytes, truncated)."""
        vp = lambda x: C.c_void_p(x) if x else None
        f = getattr(self.lib, _fn)
        f.argtypes = [C.c_void_p, C.c_uint64] + [C.c_void_p] * 11 + [C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64] + [C.c_void_p] * 4
        tb = C.c_uint64(0)
        rc = f(self.handle, n_records, vp(d_bases), vp(d_quals), vp(d_offsets), vp(d_names), vp(d_name_off), vp(d_rec_read), vp(d_flag), vp(d_contig), vp(d_pos),
               vp(d_mapq), vp(d_ops), ops_stride, vp(d_n_ops), vp(d_nm), capacity, vp(d_text), vp(d_line_begin), C.addressof(tb), vp(stream))
        if rc != W_TEXT_TRUNCATED:
            self._check(rc, _fn)
        return int(tb.value), rc == W_TEXT_TRUNCATED

    def alignSamText(self, bases, quals, offsets, front_clip, data_len, skip, names, name_off, use_m: bool = False, ops_stride: int = 64,
                     adjust_primary: bool = False, capacity: int | None = None, text_capacity: int | None = None, grow: bool = True,
                     _fn: str = "snapgpu_align_sam_single_text", _sorted: bool = False):
        """Single-end reads to the text of all their SAM records in one call (snapgpu_align_sam_single_text): alignSamRecords' inputs plus the
        reads' names; capacity / text_capacity: records / bytes to make room for (defaults: estimates); grow: call again with what the
        library asks for when one was too small.  Returns dict(text, line_begin, text_bytes, truncated, n_records, records_truncated,
        rec_begin, flag); line_begin and flag are cut to the records that were formatted."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8).reshape(-1); quals = np.ascontiguousarray(quals, dtype=np.uint8).reshape(-1)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        front_clip = np.ascontiguousarray(front_clip, dtype=np.int32); data_len = np.ascontiguousarray(data_len, dtype=np.int32)
        skip = np.ascontiguousarray(skip, dtype=np.uint8)
        names = np.ascontiguousarray(names, dtype=np.uint8).reshape(-1); name_off = np.ascontiguousarray(name_off, dtype=np.uint64)
        n = offsets.size - 1
        cap = int(capacity) if capacity is not None else n + n // 2 + 16
        tcap = int(text_capacity) if text_capacity is not None else 3 * int(bases.size) + 256 * cap + 64
        rec_begin = np.zeros(n + 1, np.uint64)
        f = getattr(self.lib, _fn)
        f.argtypes = ([C.c_void_p, C.c_uint32] + [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64] + [C.c_void_p] * 3 +
                      [C.c_uint64] + [C.c_void_p] * (5 if _sorted else 3))
        while True:
            flag = np.zeros(cap, np.int32); line_begin = np.zeros(cap + 1, np.uint64); text = np.zeros(tcap, np.uint8)
            if _sorted:
                key = np.zeros(cap, np.uint64); perm = np.zeros(cap, np.uint32)
            n_rec = C.c_uint64(0); tb = C.c_uint64(0)
            rc = f(self.handle, n, ptr(bases), ptr(quals), ptr(offsets), ptr(front_clip), ptr(data_len), ptr(skip), 1 if use_m else 0, 1 if adjust_primary else 0,
                   ptr(names), ptr(name_off), ops_stride, cap, C.addressof(n_rec), ptr(rec_begin), ptr(flag), tcap, ptr(text), ptr(line_begin), C.addressof(tb),
                   *((ptr(key), ptr(perm)) if _sorted else ()))
            if rc == W_RECORDS_TRUNCATED and grow:
                cap = int(n_rec.value)
                continue
            if rc == W_TEXT_TRUNCATED and grow:
                tcap = int(tb.value)
                continue
            if rc not in (W_RECORDS_TRUNCATED, W_TEXT_TRUNCATED):
                self._check(rc, _fn)
            break
        m = min(int(n_rec.value), cap)
        d = dict(text=text, line_begin=line_begin[:m + 1], text_bytes=int(tb.value), truncated=rc == W_TEXT_TRUNCATED, n_records=int(n_rec.value),
                 records_truncated=rc == W_RECORDS_TRUNCATED, rec_begin=rec_begin, flag=flag[:m])
        if _sorted:
            d.update(key=key[:m], perm=perm[:m])
        return d

    # ---- records -> the bytes of their BAM records (BAMFormat::writeRead) ----
    def setContigBamIds(self, ref_id=None, n_contigs: int | None = None):
        """snapgpu_set_contig_bam_ids: the BAM reference number of contig c is ref_id[c] (int32, one per contig of the index); None: contig c
        is number c (n_contigs: the index's count, for an aligner that has no GenomeIndex of its own)."""
        f = self.lib.snapgpu_set_contig_bam_ids
        f.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        if ref_id is None:
            self._check(f(self.handle, len(self.index.contigs) if n_contigs is None else int(n_contigs), None), "snapgpu_set_contig_bam_ids")
            return
        ids = np.ascontiguousarray(ref_id, dtype=np.int32)
        self._check(f(self.handle, ids.size, ptr(ids) if ids.size else None), "snapgpu_set_contig_bam_ids")

    @staticmethod
    def _as_bam(d):
        """a text call's dict under the BAM calls' names"""
        d["bytes"] = d.pop("text"); d["block_begin"] = d.pop("line_begin"); d["bam_bytes"] = d.pop("text_bytes")
        return d

    def bamRecords(self, bases, quals, offsets, names, name_off, flag, contig, pos, mapq, ops, n_ops, nm, rec_read=None, capacity: int | None = None,
                   grow: bool = True, bytes_out=None):
        """The uncompressed BAM records of a batch's records (snapgpu_bam_records_single): samText's arguments (bytes_out: a uint8 array to
        write into).  Returns dict(bytes uint8[capacity], block_begin uint64[n_records + 1], bam_bytes, truncated)."""
        return self._as_bam(self.samText(bases, quals, offsets, names, name_off, flag, contig, pos, mapq, ops, n_ops, nm, rec_read=rec_read, capacity=capacity,
                                         grow=grow, text=bytes_out, _fn="snapgpu_bam_records_single"))

    def bamRecords_device(self, n_records: int, d_bases: int, d_quals: int, d_offsets: int, d_names: int, d_name_off: int, d_rec_read: int, d_flag: int,
                          d_contig: int, d_pos: int, d_mapq: int, d_ops: int, ops_stride: int, d_n_ops: int, d_nm: int, capacity: int, d_bytes: int,
                          d_block_begin: int, stream: int = 0):
        """Device-pointer form of bamRecords (snapgpu_bam_records_single_device), as samText_device.  Returns (bam_bytes, truncated)."""
        return self.samText_device(n_records, d_bases, d_quals, d_offsets, d_names, d_name_off, d_rec_read, d_flag, d_contig, d_pos, d_mapq, d_ops, ops_stride,
                                   d_n_ops, d_nm, capacity, d_bytes, d_block_begin, stream, _fn="snapgpu_bam_records_single_device")

    def alignSamBam(self, bases, quals, offsets, front_clip, data_len, skip, names, name_off, use_m: bool = False, ops_stride: int = 64,
                    adjust_primary: bool = False, capacity: int | None = None, byte_capacity: int | None = None, grow: bool = True):
        """Single-end reads to the BAM records of all their SAM records in one call (snapgpu_align_sam_single_bam), as alignSamText.  Returns
        dict(bytes, block_begin, bam_bytes, truncated, n_records, records_truncated, rec_begin, flag)."""
        return self._as_bam(self.alignSamText(bases, quals, offsets, front_clip, data_len, skip, names, name_off, use_m=use_m, ops_stride=ops_stride,
                                              adjust_primary=adjust_primary, capacity=capacity, text_capacity=byte_capacity, grow=grow,
                                              _fn="snapgpu_align_sam_single_bam"))

    # ---- BAM records -> coordinate order (the reference's -so, per batch) ----
    def bamSort(self, data, block_begin, want_key: bool = True, want_perm: bool = True, out=None):
        """The BAM records data[block_begin[i] : block_begin[i + 1]] in coordinate order (snapgpu_bam_sort): the stable sort by
        (uint32 refID) << 32 | uint32(pos + 1), the two words read from the records themselves.  out: a uint8 array of at least the records'
        bytes to write into.  Returns dict(sorted uint8, sorted_begin uint64[n + 1], key uint64[n] or None, perm uint32[n] or None);
        perm[r] is the input index of the record at place r."""
        data = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.asarray(data)
        if data.dtype != np.uint8 or (data.size and not data.flags.c_contiguous):
            data = np.ascontiguousarray(data, dtype=np.uint8)
        data = data.reshape(-1)
        block_begin = np.ascontiguousarray(block_begin, dtype=np.uint64)
        n = block_begin.size - 1
        nb = int(block_begin[n] - block_begin[0]) if n > 0 and block_begin[n] >= block_begin[0] else 0
        if out is None:
            out = np.zeros(nb, np.uint8)
        sorted_begin = np.zeros(n + 1, np.uint64)
        key = np.zeros(n, np.uint64) if want_key else None
        perm = np.zeros(n, np.uint32) if want_perm else None
        f = self.lib.snapgpu_bam_sort
        f.argtypes = [C.c_void_p, C.c_uint64] + [C.c_void_p] * 6
        self._check(f(self.handle, n, ptr(data) if data.size else None, ptr(block_begin), ptr(out) if out.size else None, ptr(sorted_begin),
                      ptr(key) if want_key else None, ptr(perm) if want_perm else None), "snapgpu_bam_sort")
        return dict(sorted=out, sorted_begin=sorted_begin, key=key, perm=perm)

    def bamSort_device(self, n_records: int, d_bytes: int, d_block_begin: int, d_sorted: int, d_sorted_begin: int, d_key: int = 0, d_perm: int = 0,
                       stream: int = 0):
        """Device-pointer form of bamSort (snapgpu_bam_sort_device): the records, block_begin (uint64[n + 1]) and every output in HBM, the bytes
        at any byte address; d_key / d_perm 0: not wanted.  Synchronous on `stream` (0: the context's)."""
        vp = lambda x: C.c_void_p(x) if x else None
        f = self.lib.snapgpu_bam_sort_device
        f.argtypes = [C.c_void_p, C.c_uint64] + [C.c_void_p] * 7
        self._check(f(self.handle, n_records, vp(d_bytes), vp(d_block_begin), vp(d_sorted), vp(d_sorted_begin), vp(d_key), vp(d_perm), vp(stream)),
                    "snapgpu_bam_sort_device")

    def alignSamBamSorted(self, bases, quals, offsets, front_clip, data_len, skip, names, name_off, use_m: bool = False, ops_stride: int = 64,
                          adjust_primary: bool = False, capacity: int | None = None, byte_capacity: int | None = None, grow: bool = True):
        """alignSamBam with the sort behind it on the device (snapgpu_align_sam_single_bam_sorted): bytes / block_begin come back in coordinate
        order, rec_begin and flag stay in record order.  Returns alignSamBam's dict plus key uint64[records] and perm uint32[records]."""
        return self._as_bam(self.alignSamText(bases, quals, offsets, front_clip, data_len, skip, names, name_off, use_m=use_m, ops_stride=ops_stride,
                                              adjust_primary=adjust_primary, capacity=capacity, text_capacity=byte_capacity, grow=grow,
                                              _fn="snapgpu_align_sam_single_bam_sorted", _sorted=True))

    # ---- bytes -> BGZF blocks (the BGZF writer behind BAMFormat, DataWriter's gzip filter) ----
    @staticmethod
    def _bgzf_members(n_bytes: int, block_input: int = 0xff00) -> int:
        """how many BGZF blocks n_bytes make when every block takes block_input of them (an empty input makes one empty block)"""
        return max(1, -(-int(n_bytes) // int(block_input))) if block_input else 1

    def bgzfCompress(self, data, block_input: int = 0xff00, capacity: int | None = None, grow: bool = True, out=None):
        """BGZF blocks of `data` (uint8 / bytes), one per block_input bytes (snapgpu_bgzf_compress).  capacity: bytes to make room for (default:
        what always suffices, n_members * (block_input + 31)); grow: call again with the size the library asks for when that was too few; out:
        a uint8 array to write into (its size is the capacity).  Returns dict(bgzf uint8[capacity], member_begin uint64[n_members + 1],
        n_members, bgzf_bytes, truncated)."""
        data = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else data, dtype=np.uint8).reshape(-1)
        nm = self._bgzf_members(data.size, block_input)
        cap = out.size if out is not None else (int(capacity) if capacity is not None else nm * (int(block_input) + 31))
        member_begin = np.zeros(nm + 1, np.uint64)
        f = self.lib.snapgpu_bgzf_compress
        f.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint64] + [C.c_void_p] * 4
        while True:
            if out is None or out.size != cap:
                out = np.zeros(cap, np.uint8)
            n_mem = C.c_uint64(0); ob = C.c_uint64(0)
            rc = f(self.handle, data.size, ptr(data) if data.size else None, block_input, cap, ptr(out) if cap else None, ptr(member_begin),
                   C.addressof(n_mem), C.addressof(ob))
            if rc == W_TEXT_TRUNCATED and grow:
                cap = int(ob.value)
                continue
            if rc != W_TEXT_TRUNCATED:
                self._check(rc, "snapgpu_bgzf_compress")
            return dict(bgzf=out, member_begin=member_begin, n_members=int(n_mem.value), bgzf_bytes=int(ob.value), truncated=rc == W_TEXT_TRUNCATED)

    def bgzfCompress_device(self, n_bytes: int, d_in: int, block_input: int, capacity: int, d_out: int, d_member_begin: int, stream: int = 0):
        """Device-pointer form of bgzfCompress (snapgpu_bgzf_compress_device): the input, the blocks and member_begin (uint64[n_members + 1]) in
        HBM, at any byte address.  Synchronous on `stream` (0: the context's).  Returns (n_members, bgzf_bytes, truncated)."""
        vp = lambda x: C.c_void_p(x) if x else None
        f = self.lib.snapgpu_bgzf_compress_device
        f.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint64] + [C.c_void_p] * 5
        n_mem = C.c_uint64(0); ob = C.c_uint64(0)
        rc = f(self.handle, n_bytes, vp(d_in), block_input, capacity, vp(d_out), vp(d_member_begin), C.addressof(n_mem), C.addressof(ob), vp(stream))
        if rc != W_TEXT_TRUNCATED:
            self._check(rc, "snapgpu_bgzf_compress_device")
        return int(n_mem.value), int(ob.value), rc == W_TEXT_TRUNCATED

    def alignSamBgzf(self, bases, quals, offsets, front_clip, data_len, skip, names, name_off, use_m: bool = False, ops_stride: int = 64,
                     adjust_primary: bool = False, capacity: int | None = None, block_input: int = 0xff00, bgzf_capacity: int | None = None,
                     member_capacity: int | None = None, grow: bool = True):
        """alignSamBam with the BGZF stage behind it on the device (snapgpu_align_sam_single_bgzf): the record bytes stay in HBM and their
        blocks come down.  bgzf_capacity / member_capacity: bytes / blocks to make room for (defaults: estimates); grow: call again with
        what the library asks for.  Returns dict(bgzf, member_begin, n_members, bgzf_bytes, bam_bytes, truncated, n_records,
        records_truncated, rec_begin, flag); member_begin is cut to the blocks it has room for."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8).reshape(-1); quals = np.ascontiguousarray(quals, dtype=np.uint8).reshape(-1)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        front_clip = np.ascontiguousarray(front_clip, dtype=np.int32); data_len = np.ascontiguousarray(data_len, dtype=np.int32)
        skip = np.ascontiguousarray(skip, dtype=np.uint8)
        names = np.ascontiguousarray(names, dtype=np.uint8).reshape(-1); name_off = np.ascontiguousarray(name_off, dtype=np.uint64)
        n = offsets.size - 1
        cap = int(capacity) if capacity is not None else n + n // 2 + 16
        zcap = int(bgzf_capacity) if bgzf_capacity is not None else 2 * int(bases.size) + 128 * cap + 64
        mcap = int(member_capacity) if member_capacity is not None else (zcap // block_input if block_input else 0) + 2
        rec_begin = np.zeros(n + 1, np.uint64)
        f = self.lib.snapgpu_align_sam_single_bgzf
        f.argtypes = ([C.c_void_p, C.c_uint32] + [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64] + [C.c_void_p] * 3 +
                      [C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64] + [C.c_void_p] * 3)
        while True:
            flag = np.zeros(cap, np.int32); member_begin = np.zeros(mcap + 1, np.uint64); bgzf = np.zeros(zcap, np.uint8)
            n_rec = C.c_uint64(0); n_mem = C.c_uint64(0); zb = C.c_uint64(0); bb = C.c_uint64(0)
            rc = f(self.handle, n, ptr(bases), ptr(quals), ptr(offsets), ptr(front_clip), ptr(data_len), ptr(skip), 1 if use_m else 0, 1 if adjust_primary else 0,
                   ptr(names), ptr(name_off), ops_stride, cap, C.addressof(n_rec), ptr(rec_begin), ptr(flag), block_input, zcap, ptr(bgzf) if zcap else None,
                   ptr(member_begin), mcap, C.addressof(n_mem), C.addressof(zb), C.addressof(bb))
            if rc == W_RECORDS_TRUNCATED and grow:
                cap = int(n_rec.value)
                continue
            if rc == W_TEXT_TRUNCATED and grow:
                zcap = max(zcap, int(zb.value)); mcap = max(mcap, int(n_mem.value))
                continue
            if rc not in (W_RECORDS_TRUNCATED, W_TEXT_TRUNCATED):
                self._check(rc, "snapgpu_align_sam_single_bgzf")
            break
        m = min(int(n_rec.value), cap)
        return dict(bgzf=bgzf, member_begin=member_begin[:min(int(n_mem.value), mcap) + 1], n_members=int(n_mem.value), bgzf_bytes=int(zb.value),
                    bam_bytes=int(bb.value), truncated=rc == W_TEXT_TRUNCATED, n_records=int(n_rec.value), records_truncated=rc == W_RECORDS_TRUNCATED,
                    rec_begin=rec_begin, flag=flag[:m])

    def samFieldsPaired(self, bases, quals, offsets, front_clip, data_len, results, use_m: bool = False, ops_stride: int = 64):
        """SAMFormat::writePairs + fillMateInfo up to the point of printing (see snapgpu_sam_fields_paired).  offsets has 2 n + 1
        entries (read 0 and read 1 of each pair); results: PAIRED_RESULT_DTYPE array of n."""
        from .abi import PAIRED_RESULT_DTYPE
        bases = np.ascontiguousarray(bases, dtype=np.uint8).reshape(-1); quals = np.ascontiguousarray(quals, dtype=np.uint8).reshape(-1)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        front_clip = np.ascontiguousarray(front_clip, dtype=np.int32); data_len = np.ascontiguousarray(data_len, dtype=np.int32)
        results = np.ascontiguousarray(results, dtype=PAIRED_RESULT_DTYPE)
        n = offsets.size - 1; npairs = n // 2
        flag = np.zeros(n, np.int32); contig = np.zeros(n, np.int32); pos = np.zeros(n, np.int64); mapq = np.zeros(n, np.int32)
        ops = np.zeros((n, ops_stride), dtype=np.uint32); n_ops = np.zeros(n, np.int32); nm = np.zeros(n, np.int32); stale = np.zeros(n, np.int32)
        rnext = np.zeros(n, np.int32); pnext = np.zeros(n, np.int64); tlen = np.zeros(n, np.int64); first = np.zeros(npairs, np.int32)
        self._check(self.lib.snapgpu_sam_fields_paired(
            self.handle, C.c_uint32(npairs), ptr(bases), ptr(quals), ptr(offsets), ptr(front_clip), ptr(data_len), ptr(results),
            C.c_int(1 if use_m else 0), ptr(flag), ptr(contig), ptr(pos), ptr(mapq), ptr(ops), C.c_uint32(ops_stride), ptr(n_ops), ptr(nm),
            ptr(rnext), ptr(pnext), ptr(tlen), ptr(first), ptr(stale)), "snapgpu_sam_fields_paired")
        return dict(flag=flag, contig=contig, pos=pos, mapq=mapq, ops=ops, n_ops=n_ops, nm=nm, rnext=rnext, pnext=pnext, tlen=tlen,
                    first_written=first, stale=stale)

    def samFieldsPaired_device(self, n_pairs: int, max_read_len: int, d_bases: int, d_quals: int, d_offsets: int, d_front_clip: int, d_data_len: int,
                               d_results: int, d_flag: int, d_contig: int, d_pos: int, d_mapq: int, d_ops: int, ops_stride: int, d_n_ops: int, d_nm: int,
                               d_rnext: int, d_pnext: int, d_tlen: int, d_first_written: int, d_stale: int, use_m: bool = False, stream: int = 0):
        """Device-pointer form of samFieldsPaired (snapgpu_sam_fields_paired_device): every array already in HBM -- e.g. the results where
        ChimericPairedEndAligner.align_device left them -- and the outputs left there.  Synchronous on `stream` (0: the context's)."""
        vp = lambda x: C.c_void_p(x) if x else None
        self.lib.snapgpu_sam_fields_paired_device.argtypes = ([C.c_void_p, C.c_uint32, C.c_uint32] + [C.c_void_p] * 6 + [C.c_int] + [C.c_void_p] * 5 +
                                                              [C.c_uint32] + [C.c_void_p] * 8)
        self._check(self.lib.snapgpu_sam_fields_paired_device(
            self.handle, C.c_uint32(n_pairs), C.c_uint32(max_read_len), vp(d_bases), vp(d_quals), vp(d_offsets), vp(d_front_clip), vp(d_data_len),
            vp(d_results), C.c_int(1 if use_m else 0), vp(d_flag), vp(d_contig), vp(d_pos), vp(d_mapq), vp(d_ops), C.c_uint32(ops_stride), vp(d_n_ops),
            vp(d_nm), vp(d_rnext), vp(d_pnext), vp(d_tlen), vp(d_first_written), vp(d_stale), vp(stream)), "snapgpu_sam_fields_paired_device")

    def samf_pre_valid(self) -> int:
        """Diagnostics: SamfPre records the row-loop pre-pass of this context's last SAM-field launch left valid (0: no pre-pass ran)."""
        v = C.c_uint64(0)
        self.lib.snapgpu_debug_samf_pre_valid.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        self._check(self.lib.snapgpu_debug_samf_pre_valid(self.handle, C.byref(v)), "snapgpu_debug_samf_pre_valid")
        return int(v.value)

    # ---- BaseAligner::AlignRead over a batch -------------------------------------------
    def AlignRead(self, bases: np.ndarray, quals: np.ndarray, offsets: np.ndarray):
        """Returns (primaryResult[n], firstALTResult[n]) as RESULT_DTYPE arrays."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8).reshape(-1)
        quals = np.ascontiguousarray(quals, dtype=np.uint8).reshape(-1)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = offsets.size - 1
        primary = np.zeros(n, dtype=RESULT_DTYPE)
        first_alt = np.zeros(n, dtype=RESULT_DTYPE)
        self._check(self.lib.snapgpu_align_single(self.handle, C.c_uint32(n), ptr(bases), ptr(quals), ptr(offsets),
                                                  ptr(primary), ptr(first_alt)), "snapgpu_align_single")
        return primary, first_alt

    # ---- BaseAligner::AlignRead with secondary results (-om / -omax / -mpc) --------------
    def set_flags(self, stop_on_first_hit: bool = False, explore_popular_seeds: bool = False):
        """-f / -x: BaseAligner::setStopOnFirstHit / setExplorePopularSeeds (SingleAligner.cpp:179-180) for this context's single-end calls."""
        self.lib.snapgpu_set_aligner_flags.argtypes = [C.c_void_p, C.c_int, C.c_int]
        self._check(self.lib.snapgpu_set_aligner_flags(self.handle, C.c_int(1 if stop_on_first_hit else 0), C.c_int(1 if explore_popular_seeds else 0)),
                    "snapgpu_set_aligner_flags")

    def enable_secondary(self, max_edit_distance: int, max_results: int = 0x7fffffff, max_per_contig: int = -1,
                         adjust_alignments: int = 0):
        from .abi import secondary_params
        sp = secondary_params(max_edit_distance, max_results, max_per_contig, adjust_alignments)
        self._check(self.lib.snapgpu_enable_secondary(self.handle, C.byref(sp)), "snapgpu_enable_secondary")
        self._sec_max = max_results

    def AlignReadSecondary(self, bases: np.ndarray, quals: np.ndarray, offsets: np.ndarray, stride: int = 16):
        """Returns (primary[n], firstALT[n], secondary[n, stride'], nSecondary[n]); like the reference's caller
        (SingleAligner.cpp:250-263) it grows the buffer and calls again when a read has more results than fit."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8).reshape(-1)
        quals = np.ascontiguousarray(quals, dtype=np.uint8).reshape(-1)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = offsets.size - 1
        primary = np.zeros(n, dtype=RESULT_DTYPE)
        first_alt = np.zeros(n, dtype=RESULT_DTYPE)
        while True:
            secondary = np.zeros((n, stride), dtype=RESULT_DTYPE)
            n_sec = np.zeros(n, dtype=np.uint32)
            rc = self.lib.snapgpu_align_single_secondary(self.handle, C.c_uint32(n), ptr(bases), ptr(quals), ptr(offsets),
                                                         ptr(primary), ptr(first_alt), ptr(secondary), C.c_uint32(stride), ptr(n_sec))
            if rc == 1:                                   # SNAPGPU_W_SECONDARY_TRUNCATED
                stride = int(n_sec.max())
                continue
            self._check(rc, "snapgpu_align_single_secondary")
            return primary, first_alt, secondary, n_sec

    def align_device(self, n: int, d_bases: int, d_quals: int, d_offsets: int, d_primary: int, d_first_alt: int = 0,
                     stream: int = 0):
        """Device-pointer form (inputs already in HBM, results left in HBM)."""
        self._check(self.lib.snapgpu_align_single_device(self.handle, C.c_uint32(n), C.c_void_p(d_bases),
                                                         C.c_void_p(d_quals), C.c_void_p(d_offsets), C.c_void_p(d_primary),
                                                         C.c_void_p(d_first_alt) if d_first_alt else None,
                                                         C.c_void_p(stream) if stream else None),
                    "snapgpu_align_single_device")

    def counters(self, reset: bool = False) -> dict:
        c = Counters()
        self._check(self.lib.snapgpu_get_counters(self.handle, C.byref(c), C.c_int(1 if reset else 0)), "snapgpu_get_counters")
        return c.as_dict()

    def launch_profile(self):
        """Diagnostics of the last single-end launch of a context created under SNAPGPU_PHASE_TIMERS=1: dict(read_cycles_log2_hist[64],
        wave_start[S], wave_finish[S], wave_worst_read_cycles[S], wave_worst_read_ag_calls[S])."""
        cap = 64 + 3 * 65536
        buf = np.zeros(cap, dtype=np.uint64)
        ns = C.c_uint32(0)
        self.lib.snapgpu_debug_launch_profile.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32)]
        self._check(self.lib.snapgpu_debug_launch_profile(self.handle, buf.ctypes.data, C.c_uint64(cap), C.byref(ns)), "snapgpu_debug_launch_profile")
        S = int(ns.value)
        w = buf[64 + 2 * S:64 + 3 * S]
        return dict(read_cycles_log2_hist=buf[:64].copy(), wave_start=buf[64:64 + S].copy(), wave_finish=buf[64 + S:64 + 2 * S].copy(),
                    wave_worst_read_cycles=(w >> np.uint64(24)).copy(), wave_worst_read_ag_calls=(w & np.uint64(0xffffff)).copy())

    def kernel_time(self, reset: bool = False):
        ms = C.c_double(0); nl = C.c_uint64(0)
        self._check(self.lib.snapgpu_kernel_time(self.handle, C.byref(ms), C.byref(nl), C.c_int(1 if reset else 0)),
                    "snapgpu_kernel_time")
        return ms.value, int(nl.value)

    def device_index_ptrs(self):
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._check(self.lib.snapgpu_index_device_ptrs(self.handle, C.byref(a), C.byref(b), C.byref(c)),
                    "snapgpu_index_device_ptrs")
        return a.value, b.value, c.value

    def debug_tables(self):
        phred = np.zeros(256); indel = np.zeros(1001); perfect = np.zeros(1001)
        sp = C.c_double(0); thr = np.zeros(72); wrapped = np.zeros(33, dtype=np.uint32)
        self._check(self.lib.snapgpu_debug_tables(self.handle, ptr(phred), ptr(indel), C.c_uint32(1001), ptr(perfect),
                                                  C.c_uint32(1001), C.byref(sp), ptr(thr), ptr(wrapped)), "snapgpu_debug_tables")
        return dict(phred=phred, indel=indel, perfect=perfect, seed_prob=sp.value, mapq_threshold=thr, wrapped=wrapped)


class ChimericPairedEndAligner(BaseAligner):
    """Paired-end host mirror: ChimericPairedEndAligner over IntersectingPairedEndAligner
    (SNAPLib/ChimericPairedEndAligner.cpp:126, SNAPLib/IntersectingPairedEndAligner.cpp:169), built the way
    PairedAlignerContext builds them (SNAPLib/PairedAligner.cpp:556-625).  `params` are the options shared with the
    single-end aligner (maxHits, maxDist, affine-gap scores ...), `paired_params` the PairedAlignerOptions."""

    def __init__(self, index: GenomeIndex, params: Params | None = None, paired_params=None, device: int = 0,
                 device_index_ptrs=None):
        from .abi import PairedParams, default_paired_params
        super().__init__(index, params, device, device_index_ptrs)
        self.paired_params = paired_params if paired_params is not None else default_paired_params()
        self.lib.snapgpu_enable_paired.argtypes = [C.c_void_p, C.POINTER(PairedParams)]
        self.lib.snapgpu_align_paired_device.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 6
        self._check(self.lib.snapgpu_enable_paired(self.handle, C.byref(self.paired_params)), "snapgpu_enable_paired")

    def _after_replica(self):               # (a replica starts as a single-end context)
        self._check(self.lib.snapgpu_enable_paired(self.handle, C.byref(self.paired_params)), "snapgpu_enable_paired")

    @classmethod
    def over(cls, base: "BaseAligner", paired_params=None, params: Params | None = None):
        """A paired-end context over the index another context (single-end or paired) already has resident on its GPU:
        snapgpu_create_replica(share_index = 1) + snapgpu_enable_paired.  `base` must outlive it (it owns the blobs)."""
        from .abi import PairedParams, default_paired_params
        proto = cls.__new__(cls)
        proto.__dict__.update(base.__dict__)
        proto.paired_params = paired_params if paired_params is not None else default_paired_params()
        proto.lib.snapgpu_enable_paired.argtypes = [C.c_void_p, C.POINTER(PairedParams)]
        proto.lib.snapgpu_align_paired_device.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 6
        try:
            other = BaseAligner.replica(proto, params=params)
        finally:
            proto.handle = None             # (the prototype borrowed base's handle: it must never destroy it, whatever the replica call did)
        return other

    def _after_built(self, paired_params):
        from .abi import PairedParams, default_paired_params
        self.paired_params = paired_params if paired_params is not None else default_paired_params()
        self.lib.snapgpu_enable_paired.argtypes = [C.c_void_p, C.POINTER(PairedParams)]
        self.lib.snapgpu_align_paired_device.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 6
        self._check(self.lib.snapgpu_enable_paired(self.handle, C.byref(self.paired_params)), "snapgpu_enable_paired")

    def align(self, bases: np.ndarray, quals: np.ndarray, offsets: np.ndarray):
        """ChimericPairedEndAligner::align over a batch: offsets has 2n+1 entries (read 0 / read 1 of each pair
        interleaved).  Returns (result[n], firstALTResult[n]) as PAIRED_RESULT_DTYPE arrays."""
        from .abi import PAIRED_RESULT_DTYPE
        bases = np.ascontiguousarray(bases, dtype=np.uint8).reshape(-1)
        quals = np.ascontiguousarray(quals, dtype=np.uint8).reshape(-1)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        if (offsets.size - 1) % 2:
            raise ValueError("offsets must have 2*n_pairs + 1 entries")
        n = (offsets.size - 1) // 2
        primary = np.zeros(n, dtype=PAIRED_RESULT_DTYPE)
        first_alt = np.zeros(n, dtype=PAIRED_RESULT_DTYPE)
        self._check(self.lib.snapgpu_align_paired(self.handle, C.c_uint32(n), ptr(bases), ptr(quals), ptr(offsets),
                                                  ptr(primary), ptr(first_alt)), "snapgpu_align_paired")
        return primary, first_alt

    def alignSamPaired(self, bases, quals, offsets, front_clip, data_len, skip, use_m: bool = False, ops_stride: int = 64, want_results: bool = True):
        """The paired-end path of a SAM writer in one call (snapgpu_align_sam_paired): ChimericPairedEndAligner::align over Read::clip's
        windows (PairedAligner.cpp:700) and SAMFormat::writePairs' computed fields for each pair's result, the batch uploaded once.
        bases / quals / offsets (2 n + 1 entries): the unclipped mates; front_clip / data_len [2 n]: Read::clip's outcome; skip[i] != 0:
        pair i is not given to the aligner (neither mate useful, PairedAligner.cpp:680-682).  Returns (results, first_alt, dict(flag,
        contig, pos, mapq, ops, n_ops, nm, rnext, pnext, tlen, first_written, stale)); want_results = False: (None, None, dict)."""
        from .abi import PAIRED_RESULT_DTYPE
        bases = np.ascontiguousarray(bases, dtype=np.uint8).reshape(-1); quals = np.ascontiguousarray(quals, dtype=np.uint8).reshape(-1)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        front_clip = np.ascontiguousarray(front_clip, dtype=np.int32); data_len = np.ascontiguousarray(data_len, dtype=np.int32)
        skip = np.ascontiguousarray(skip, dtype=np.uint8)
        if (offsets.size - 1) % 2:
            raise ValueError("offsets must have 2*n_pairs + 1 entries")
        n = offsets.size - 1; npairs = n // 2
        results = np.zeros(npairs, dtype=PAIRED_RESULT_DTYPE) if want_results else None
        first_alt = np.zeros(npairs, dtype=PAIRED_RESULT_DTYPE) if want_results else None
        flag = np.zeros(n, np.int32); contig = np.zeros(n, np.int32); pos = np.zeros(n, np.int64); mapq = np.zeros(n, np.int32)
        ops = np.zeros((n, ops_stride), dtype=np.uint32); n_ops = np.zeros(n, np.int32); nm = np.zeros(n, np.int32); stale = np.zeros(n, np.int32)
        rnext = np.zeros(n, np.int32); pnext = np.zeros(n, np.int64); tlen = np.zeros(n, np.int64); first = np.zeros(npairs, np.int32)
        self._check(self.lib.snapgpu_align_sam_paired(
            self.handle, C.c_uint32(npairs), ptr(bases), ptr(quals), ptr(offsets), ptr(front_clip), ptr(data_len), ptr(skip),
            C.c_int(1 if use_m else 0), ptr(results) if want_results else None, ptr(first_alt) if want_results else None,
            ptr(flag), ptr(contig), ptr(pos), ptr(mapq), ptr(ops), C.c_uint32(ops_stride), ptr(n_ops), ptr(nm),
            ptr(rnext), ptr(pnext), ptr(tlen), ptr(first), ptr(stale)), "snapgpu_align_sam_paired")
        return results, first_alt, dict(flag=flag, contig=contig, pos=pos, mapq=mapq, ops=ops, n_ops=n_ops, nm=nm, rnext=rnext, pnext=pnext,
                                        tlen=tlen, first_written=first, stale=stale)

    # ---- pair units -> the bytes of their SAM lines (SAMFormat::writePairs' printed lines) ----
    def samTextPaired(self, bases, quals, offsets, names, name_off, flag, contig, pos, mapq, ops, n_ops, nm, rnext, pnext, tlen, first_written,
                      unit_pair=None, capacity: int | None = None, grow: bool = True, text=None, _fn: str = "snapgpu_sam_text_paired"):
        """The SAM lines of a batch's pair units (snapgpu_sam_text_paired): bases / quals / offsets (2 n_pairs + 1 entries) the unclipped
        mates, names / name_off (uint64[2 n_pairs + 1]) their names, flag .. tlen the fields of both mates of every unit as samFieldsPaired /
        alignSamPaired return them ([2 n_units]; ops: [2 n_units, ops_stride]), first_written [n_units]; unit_pair: the pair of each unit
        (None: unit i is pair i).  capacity / grow / text: as samText.  Returns dict(text uint8[capacity], line_begin uint64[2 n_units + 1],
        text_bytes, truncated); lines 2 u and 2 u + 1 are unit u's, in the order they are printed."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8).reshape(-1); quals = np.ascontiguousarray(quals, dtype=np.uint8).reshape(-1)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        names = np.ascontiguousarray(names, dtype=np.uint8).reshape(-1); name_off = np.ascontiguousarray(name_off, dtype=np.uint64)
        flag = np.ascontiguousarray(flag, dtype=np.int32); contig = np.ascontiguousarray(contig, dtype=np.int32)
        pos = np.ascontiguousarray(pos, dtype=np.int64); mapq = np.ascontiguousarray(mapq, dtype=np.int32)
        ops = np.ascontiguousarray(ops, dtype=np.uint32); n_ops = np.ascontiguousarray(n_ops, dtype=np.int32); nm = np.ascontiguousarray(nm, dtype=np.int32)
        rnext = np.ascontiguousarray(rnext, dtype=np.int32); pnext = np.ascontiguousarray(pnext, dtype=np.int64); tlen = np.ascontiguousarray(tlen, dtype=np.int64)
        first_written = np.ascontiguousarray(first_written, dtype=np.int32)
        n_units = first_written.size
        if flag.size != 2 * n_units or (offsets.size - 1) % 2:
            raise ValueError("two records per unit and two mates per pair are needed")
        ops_stride = ops.shape[1] if ops.ndim == 2 else (ops.size // flag.size if flag.size else 1)
        if unit_pair is not None:
            unit_pair = np.ascontiguousarray(unit_pair, dtype=np.uint32)
        n_pairs = (offsets.size - 1) // 2
        cap = text.size if text is not None else (int(capacity) if capacity is not None else 4 * int(bases.size) + 600 * n_units + 64)
        line_begin = np.zeros(2 * n_units + 1, np.uint64)
        f = getattr(self.lib, _fn)
        f.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32] + [C.c_void_p] * 11 + [C.c_uint32] + [C.c_void_p] * 6 + [C.c_uint64] + [C.c_void_p] * 3
        while True:
            if text is None or text.size != cap:
                text = np.zeros(cap, np.uint8)
            tb = C.c_uint64(0)
            rc = f(self.handle, n_units, n_pairs, ptr(bases), ptr(quals), ptr(offsets), ptr(names), ptr(name_off), ptr(unit_pair) if unit_pair is not None else None,
                   ptr(flag), ptr(contig), ptr(pos), ptr(mapq), ptr(ops), ops_stride, ptr(n_ops), ptr(nm), ptr(rnext), ptr(pnext), ptr(tlen), ptr(first_written),
                   cap, ptr(text), ptr(line_begin), C.addressof(tb))
            if rc == W_TEXT_TRUNCATED and grow:
                cap = int(tb.value)
                continue
            if rc != W_TEXT_TRUNCATED:
                self._check(rc, _fn)
            return dict(text=text, line_begin=line_begin, text_bytes=int(tb.value), truncated=rc == W_TEXT_TRUNCATED)

    def samTextPaired_device(self, n_units: int, d_bases: int, d_quals: int, d_offsets: int, d_names: int, d_name_off: int, d_unit_pair: int, d_flag: int,
                             d_contig: int, d_pos: int, d_mapq: int, d_ops: int, ops_stride: int, d_n_ops: int, d_nm: int, d_rnext: int, d_pnext: int,
                             d_tlen: int, d_first_written: int, capacity: int, d_text: int, d_line_begin: int, stream: int = 0,
                             _fn: str = "snapgpu_sam_text_paired_device"):
        """Device-pointer form of samTextPaired (snapgpu_sam_text_paired_device): every array in HBM (d_unit_pair 0: unit i is pair i), the
        text and line_begin left there.  Synchronous on `stream` (0: the context's).  Returns (text_bytes, truncated)."""
        vp = lambda x: C.c_void_p(x) if x else None
        f = getattr(self.lib, _fn)
        f.argtypes = [C.c_void_p, C.c_uint64] + [C.c_void_p] * 11 + [C.c_uint32] + [C.c_void_p] * 6 + [C.c_uint64] + [C.c_void_p] * 4
        tb = C.c_uint64(0)
        rc = f(self.handle, n_units, vp(d_bases), vp(d_quals), vp(d_offsets), vp(d_names), vp(d_name_off), vp(d_unit_pair), vp(d_flag), vp(d_contig), vp(d_pos),
               vp(d_mapq), vp(d_ops), ops_stride, vp(d_n_ops), vp(d_nm), vp(d_rnext), vp(d_pnext), vp(d_tlen), vp(d_first_written), capacity, vp(d_text),
               vp(d_line_begin), C.addressof(tb), vp(stream))
        if rc != W_TEXT_TRUNCATED:
            self._check(rc, _fn)
        return int(tb.value), rc == W_TEXT_TRUNCATED

    def alignSamTextPaired(self, bases, quals, offsets, front_clip, data_len, skip, names, name_off, use_m: bool = False, ops_stride: int = 64,
                           text_capacity: int | None = None, grow: bool = True, want_results: bool = False, _fn: str = "snapgpu_align_sam_paired_text",
                           _sorted: bool = False):
        """Paired-end reads to the text of their SAM records in one call (snapgpu_align_sam_paired_text): alignSamPaired's inputs plus the
        mates' names; text_capacity: bytes to make room for (default: an estimate); grow: call again with what the library asks for when
        that was too few.  Returns dict(text, line_begin uint64[2 n_pairs + 1], text_bytes, truncated, flag [2 n_pairs], first_written
        [n_pairs], results, first_alt); the last two None unless want_results."""
        from .abi import PAIRED_RESULT_DTYPE
        bases = np.ascontiguousarray(bases, dtype=np.uint8).reshape(-1); quals = np.ascontiguousarray(quals, dtype=np.uint8).reshape(-1)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        front_clip = np.ascontiguousarray(front_clip, dtype=np.int32); data_len = np.ascontiguousarray(data_len, dtype=np.int32)
        skip = np.ascontiguousarray(skip, dtype=np.uint8)
        names = np.ascontiguousarray(names, dtype=np.uint8).reshape(-1); name_off = np.ascontiguousarray(name_off, dtype=np.uint64)
        if (offsets.size - 1) % 2:
            raise ValueError("offsets must have 2*n_pairs + 1 entries")
        n = offsets.size - 1; npairs = n // 2
        tcap = int(text_capacity) if text_capacity is not None else 3 * int(bases.size) + 300 * n + 64
        results = np.zeros(npairs, dtype=PAIRED_RESULT_DTYPE) if want_results else None
        first_alt = np.zeros(npairs, dtype=PAIRED_RESULT_DTYPE) if want_results else None
        f = getattr(self.lib, _fn)
        f.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 6 + [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_void_p] * 4 + [C.c_uint64] + [C.c_void_p] * (5 if _sorted else 3)
        while True:
            flag = np.zeros(n, np.int32); first = np.zeros(npairs, np.int32); line_begin = np.zeros(n + 1, np.uint64); text = np.zeros(tcap, np.uint8)
            if _sorted:
                key = np.zeros(n, np.uint64); perm = np.zeros(n, np.uint32)
            tb = C.c_uint64(0)
            rc = f(self.handle, npairs, ptr(bases), ptr(quals), ptr(offsets), ptr(front_clip), ptr(data_len), ptr(skip), 1 if use_m else 0, ptr(names), ptr(name_off),
                   ops_stride, ptr(results) if want_results else None, ptr(first_alt) if want_results else None, ptr(flag), ptr(first), tcap, ptr(text),
                   ptr(line_begin), C.addressof(tb), *((ptr(key), ptr(perm)) if _sorted else ()))
            if rc == W_TEXT_TRUNCATED and grow:
                tcap = int(tb.value)
                continue
            if rc != W_TEXT_TRUNCATED:
                self._check(rc, _fn)
            break
        d = dict(text=text, line_begin=line_begin, text_bytes=int(tb.value), truncated=rc == W_TEXT_TRUNCATED, flag=flag, first_written=first,
                 results=results, first_alt=first_alt)
        if _sorted:
            d.update(key=key, perm=perm)
        return d

    # ---- pair units -> the bytes of their BAM records (BAMFormat::writePairs) ----
    def bamRecordsPaired(self, bases, quals, offsets, names, name_off, flag, contig, pos, mapq, ops, n_ops, nm, rnext, pnext, tlen, first_written,
                         unit_pair=None, capacity: int | None = None, grow: bool = True, bytes_out=None):
        """The uncompressed BAM records of a batch's pair units (snapgpu_bam_records_paired): samTextPaired's arguments.  Returns dict(bytes
        uint8[capacity], block_begin uint64[2 n_units + 1], bam_bytes, truncated); records 2 u and 2 u + 1 are unit u's, in file order."""
        return self._as_bam(self.samTextPaired(bases, quals, offsets, names, name_off, flag, contig, pos, mapq, ops, n_ops, nm, rnext, pnext, tlen, first_written,
                                               unit_pair=unit_pair, capacity=capacity, grow=grow, text=bytes_out, _fn="snapgpu_bam_records_paired"))

    def bamRecordsPaired_device(self, n_units: int, d_bases: int, d_quals: int, d_offsets: int, d_names: int, d_name_off: int, d_unit_pair: int, d_flag: int,
                                d_contig: int, d_pos: int, d_mapq: int, d_ops: int, ops_stride: int, d_n_ops: int, d_nm: int, d_rnext: int, d_pnext: int,
                                d_tlen: int, d_first_written: int, capacity: int, d_bytes: int, d_block_begin: int, stream: int = 0):
        """Device-pointer form of bamRecordsPaired (snapgpu_bam_records_paired_device), as samTextPaired_device.  Returns (bam_bytes, truncated)."""
        return self.samTextPaired_device(n_units, d_bases, d_quals, d_offsets, d_names, d_name_off, d_unit_pair, d_flag, d_contig, d_pos, d_mapq, d_ops, ops_stride,
                                         d_n_ops, d_nm, d_rnext, d_pnext, d_tlen, d_first_written, capacity, d_bytes, d_block_begin, stream,
                                         _fn="snapgpu_bam_records_paired_device")

    def alignSamBamPaired(self, bases, quals, offsets, front_clip, data_len, skip, names, name_off, use_m: bool = False, ops_stride: int = 64,
                          byte_capacity: int | None = None, grow: bool = True, want_results: bool = False):
        """Paired-end reads to the BAM records of their SAM records in one call (snapgpu_align_sam_paired_bam), as alignSamTextPaired.  Returns
        dict(bytes, block_begin uint64[2 n_pairs + 1], bam_bytes, truncated, flag, first_written, results, first_alt)."""
        return self._as_bam(self.alignSamTextPaired(bases, quals, offsets, front_clip, data_len, skip, names, name_off, use_m=use_m, ops_stride=ops_stride,
                                                    text_capacity=byte_capacity, grow=grow, want_results=want_results, _fn="snapgpu_align_sam_paired_bam"))

    def alignSamBamSortedPaired(self, bases, quals, offsets, front_clip, data_len, skip, names, name_off, use_m: bool = False, ops_stride: int = 64,
                                byte_capacity: int | None = None, grow: bool = True, want_results: bool = False):
        """alignSamBamPaired with the sort behind it on the device (snapgpu_align_sam_paired_bam_sorted): bytes / block_begin in coordinate
        order (every record on its own, so mates separate), flag / first_written / results in record order.  Returns alignSamBamPaired's dict
        plus key uint64[2 n_pairs] and perm uint32[2 n_pairs]."""
        return self._as_bam(self.alignSamTextPaired(bases, quals, offsets, front_clip, data_len, skip, names, name_off, use_m=use_m, ops_stride=ops_stride,
                                                    text_capacity=byte_capacity, grow=grow, want_results=want_results,
                                                    _fn="snapgpu_align_sam_paired_bam_sorted", _sorted=True))

    def alignSamBgzfPaired(self, bases, quals, offsets, front_clip, data_len, skip, names, name_off, use_m: bool = False, ops_stride: int = 64,
                           block_input: int = 0xff00, bgzf_capacity: int | None = None, member_capacity: int | None = None, grow: bool = True,
                           want_results: bool = False):
        """alignSamBamPaired with the BGZF stage behind it on the device (snapgpu_align_sam_paired_bgzf), as alignSamBgzf.  Returns dict(bgzf,
        member_begin, n_members, bgzf_bytes, bam_bytes, truncated, flag, first_written, results, first_alt)."""
        from .abi import PAIRED_RESULT_DTYPE
        bases = np.ascontiguousarray(bases, dtype=np.uint8).reshape(-1); quals = np.ascontiguousarray(quals, dtype=np.uint8).reshape(-1)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        front_clip = np.ascontiguousarray(front_clip, dtype=np.int32); data_len = np.ascontiguousarray(data_len, dtype=np.int32)
        skip = np.ascontiguousarray(skip, dtype=np.uint8)
        names = np.ascontiguousarray(names, dtype=np.uint8).reshape(-1); name_off = np.ascontiguousarray(name_off, dtype=np.uint64)
        if (offsets.size - 1) % 2:
            raise ValueError("offsets must have 2*n_pairs + 1 entries")
        n = offsets.size - 1; npairs = n // 2
        zcap = int(bgzf_capacity) if bgzf_capacity is not None else 2 * int(bases.size) + 128 * n + 64
        mcap = int(member_capacity) if member_capacity is not None else (zcap // block_input if block_input else 0) + 2
        results = np.zeros(npairs, dtype=PAIRED_RESULT_DTYPE) if want_results else None
        first_alt = np.zeros(npairs, dtype=PAIRED_RESULT_DTYPE) if want_results else None
        f = self.lib.snapgpu_align_sam_paired_bgzf
        f.argtypes = ([C.c_void_p, C.c_uint32] + [C.c_void_p] * 6 + [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_void_p] * 4 +
                      [C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64] + [C.c_void_p] * 3)
        while True:
            flag = np.zeros(n, np.int32); first = np.zeros(npairs, np.int32); member_begin = np.zeros(mcap + 1, np.uint64); bgzf = np.zeros(zcap, np.uint8)
            n_mem = C.c_uint64(0); zb = C.c_uint64(0); bb = C.c_uint64(0)
            rc = f(self.handle, npairs, ptr(bases), ptr(quals), ptr(offsets), ptr(front_clip), ptr(data_len), ptr(skip), 1 if use_m else 0, ptr(names), ptr(name_off),
                   ops_stride, ptr(results) if want_results else None, ptr(first_alt) if want_results else None, ptr(flag), ptr(first), block_input, zcap,
                   ptr(bgzf) if zcap else None, ptr(member_begin), mcap, C.addressof(n_mem), C.addressof(zb), C.addressof(bb))
            if rc == W_TEXT_TRUNCATED and grow:
                zcap = max(zcap, int(zb.value)); mcap = max(mcap, int(n_mem.value))
                continue
            if rc != W_TEXT_TRUNCATED:
                self._check(rc, "snapgpu_align_sam_paired_bgzf")
            break
        return dict(bgzf=bgzf, member_begin=member_begin[:min(int(n_mem.value), mcap) + 1], n_members=int(n_mem.value), bgzf_bytes=int(zb.value),
                    bam_bytes=int(bb.value), truncated=rc == W_TEXT_TRUNCATED, flag=flag, first_written=first, results=results, first_alt=first_alt)

    def align_secondary(self, bases: np.ndarray, quals: np.ndarray, offsets: np.ndarray, stride: int = 8, single_stride: int = 16):
        """ChimericPairedEndAligner::align with secondary results (after enable_secondary(...)): returns
        (result[n], firstALT[n], secondary[n, stride'], nSecondary[n], singleSecondary[n, single_stride'], nSingleSecondary[n, 2]).
        Like PairedAligner.cpp:727-779 it grows a buffer and calls again when a pair has more results than fit."""
        from .abi import PAIRED_RESULT_DTYPE
        bases = np.ascontiguousarray(bases, dtype=np.uint8).reshape(-1)
        quals = np.ascontiguousarray(quals, dtype=np.uint8).reshape(-1)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        if (offsets.size - 1) % 2:
            raise ValueError("offsets must have 2*n_pairs + 1 entries")
        n = (offsets.size - 1) // 2
        primary = np.zeros(n, dtype=PAIRED_RESULT_DTYPE)
        first_alt = np.zeros(n, dtype=PAIRED_RESULT_DTYPE)
        while True:
            sec = np.zeros((n, stride), dtype=PAIRED_RESULT_DTYPE)
            nsec = np.zeros(n, dtype=np.uint32)
            ssec = np.zeros((n, single_stride), dtype=RESULT_DTYPE)
            nssec = np.zeros((n, 2), dtype=np.uint32)
            rc = self.lib.snapgpu_align_paired_secondary(self.handle, C.c_uint32(n), ptr(bases), ptr(quals), ptr(offsets), ptr(primary),
                                                         ptr(first_alt), ptr(sec), C.c_uint32(stride), ptr(nsec),
                                                         ptr(ssec), C.c_uint32(single_stride), ptr(nssec))
            if rc == 1:                                   # SNAPGPU_W_SECONDARY_TRUNCATED
                stride = max(stride, int(nsec.max()))
                single_stride = max(single_stride, int(nssec.sum(axis=1).max()))
                continue
            self._check(rc, "snapgpu_align_paired_secondary")
            return primary, first_alt, sec, nsec, ssec, nssec

    def align_device(self, n_pairs: int, d_bases: int, d_quals: int, d_offsets: int, d_primary: int, d_first_alt: int = 0,
                     stream: int = 0):
        self._check(self.lib.snapgpu_align_paired_device(self.handle, C.c_uint32(n_pairs), C.c_void_p(d_bases),
                                                         C.c_void_p(d_quals), C.c_void_p(d_offsets), C.c_void_p(d_primary),
                                                         C.c_void_p(d_first_alt) if d_first_alt else None,
                                                         C.c_void_p(stream) if stream else None),
                    "snapgpu_align_paired_device")
