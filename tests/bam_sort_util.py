"""TEST INFRASTRUCTURE: the yardstick of snapgpu_bam_sort / _device and the _bam_sorted fused calls (snap_amd/csrc/bam_sort.h), and the cases
that tests/test_emu_bam_sort.py (the wavefront emulator) and tests/test_zz_gpu_bam_sort.py (the GPU) run alike.

The restatement is the whole definition of the output: a key per record from the record's own bytes,
    key = (uint32 refID at offset 4) << 32 | uint32(int32 pos at offset 8, plus 1)
then sorted(range(n), key=lambda i: (key[i], i)) -- the stable sort -- and the concatenation of the records in that order.  The sort reads
only a record's extent and those two words, so handcrafted records with arbitrary payload bytes are valid inputs and keep the cases tiny."""
import ctypes as C
import os
import struct

import numpy as np

from tests import bam_util as bu
from tests import samrec_util as su
from tests import util
from tests.samtext_util import pack

SYMBOLS = ("snapgpu_bam_sort", "snapgpu_bam_sort_device", "snapgpu_align_sam_single_bam_sorted", "snapgpu_align_sam_paired_bam_sorted")
RADIX_TILE = 1024                # IB_TILE of snap_amd/csrc/radix_pass.h: the elements a wavefront takes per pass (SAMREC_CHUNK, the scan's tile, is the same)
LAST_CONTIG = 6                  # a refID the cases use as "the last contig": the sort does not know the contigs
GUARD = 0xCD


# ---------------------------------------------------------------------------------------- the restatement
def key_of(rec):
    ref, pos = struct.unpack_from("<ii", rec, 4)
    return ((ref & 0xFFFFFFFF) << 32) | ((pos + 1) & 0xFFFFFFFF)


def restate(records):
    """records (a list of bytes) -> (sorted bytes, sorted_begin, key, perm) as the calls must return them"""
    keys = [key_of(r) for r in records]
    perm = sorted(range(len(records)), key=lambda i: (keys[i], i))
    begin = np.zeros(len(records) + 1, np.uint64)
    if records:
        begin[1:] = np.cumsum([len(records[i]) for i in perm], dtype=np.uint64)
    return (b"".join(records[i] for i in perm), begin, np.array([keys[i] for i in perm], np.uint64), np.array(perm, np.uint32))


def make_records(refs, poss, lens, seed=5):
    """one record per (refID, pos, length >= 12): a block_size word, the two words of the key, payload bytes no test gives a meaning to"""
    rng = np.random.default_rng(seed)
    out = []
    for ref, pos, n in zip(refs, poss, lens):
        assert n >= 12
        out.append(struct.pack("<Iii", n - 4, int(ref), int(pos)) + rng.integers(0, 256, n - 12, dtype=np.uint8).tobytes())
    return out


def blob_of(records):
    bb = np.zeros(len(records) + 1, np.uint64)
    if records:
        bb[1:] = np.cumsum([len(r) for r in records], dtype=np.uint64)
    return np.frombuffer(b"".join(records), np.uint8), bb


def at_residue(n_bytes, residue, fill=GUARD, guard=64):
    """(a uint8 array, where in it n_bytes start at an address that is `residue` mod 16, with `guard` bytes of `fill` on both sides)"""
    buf = np.full(n_bytes + 2 * guard + 32, fill, np.uint8)
    at = guard + (residue - (buf.ctypes.data + guard)) % 16
    return buf, at


# ---------------------------------------------------------------------------------------- the cases
COUNTS = [0, 1, 2, 63, 64, 65, 255, 256, 257, RADIX_TILE - 1, RADIX_TILE, RADIX_TILE + 1, 2 * RADIX_TILE + 37]


def lens_for(n, seed):
    """every residue mod 16, from 12 bytes up"""
    return 12 + (np.arange(n) * 7 + seed) % 37


def count_case(n):
    rng = np.random.default_rng(100 + n)
    refs = rng.integers(-1, LAST_CONTIG + 1, n)
    poss = np.where(rng.integers(0, 4, n) == 0, rng.integers(-1, 40, n), rng.integers(-1, 2 ** 31 - 1, n))      # (ties among the small ones)
    return make_records(refs, poss, lens_for(n, n), seed=n)


def key_shape_cases():
    """name -> records; 130 records each: more than two rounds of a wavefront, less than a tile"""
    n = 130
    i = np.arange(n)
    lens = lens_for(n, 3)
    scatter = (i * 37) % n                                                   # a permutation of 0 .. n - 1
    c = {}
    c["all_equal"] = make_records(np.full(n, 2), np.full(n, 777), lens)
    c["descending"] = make_records((n - 1 - i) // 40, 5000 - 7 * i, lens)
    c["lowest_bit"] = make_records(np.full(n, 1), 1000 + (scatter & 1), lens)
    c["highest_pos_bit"] = make_records(np.full(n, 1), np.where(scatter & 1, 2 ** 30 + 5, 5), lens)
    c["refid_only"] = make_records(scatter % (LAST_CONTIG + 1), np.full(n, 12345), lens)
    c["unmapped_scattered"] = make_records(np.where(scatter % 5 == 0, -1, scatter % 3), np.where(scatter % 5 == 0, -1, 100 + scatter % 9), lens)
    c["last_contig_far_end"] = make_records(np.where(scatter % 4 == 0, LAST_CONTIG, scatter % LAST_CONTIG),
                                            np.where(scatter % 4 == 0, 2 ** 31 - 2, scatter * 1000), lens)
    c["only_unmapped"] = make_records(np.full(n, -1), np.full(n, -1), lens)
    c["unmapped_with_mate_coordinates"] = make_records(np.where(scatter % 3 == 0, -1, 2), np.where(scatter % 7 == 0, -1, 50 + scatter % 11), lens)
    c["all_ones_key"] = make_records(np.where(scatter % 2, -1, 0), np.where(scatter % 2, -2, 9), lens)      # refID -1, pos -2: the key is 2^64 - 1
    return c


def long_record_case():
    """a record longer than 64 KB beside 12-byte ones"""
    return make_records([3, 0, -1, 3, 0, 2], [50, 9, -1, 49, 9, 1], [12, 12, 12, 70001, 12, 12])


RESIDUE_PAIRS = [(s, (5 * s + 3) % 16) for s in range(16)]                  # every source residue, every destination residue
assert sorted(d for _, d in RESIDUE_PAIRS) == list(range(16))


def all_cases():
    c = {"count_%d" % n: count_case(n) for n in COUNTS}
    c.update(key_shape_cases())
    c["long_record"] = long_record_case()
    return c


# ---------------------------------------------------------------------------------------- the checks
def make_aligner(index):
    return bu.make_aligner(index)


def assert_equals_restatement(got, records, nb=None, what=""):
    exp_bytes, exp_begin, exp_key, exp_perm = restate(records)
    assert (got["sorted_begin"] == exp_begin).all(), what
    if got.get("perm") is not None:
        assert (got["perm"] == exp_perm).all(), (what, np.flatnonzero(got["perm"] != exp_perm)[:5])
    if got.get("key") is not None:
        assert (got["key"] == exp_key).all(), what
    assert got["sorted"][:len(exp_bytes)].tobytes() == exp_bytes, what


def check_case(a, records, what=""):
    data, bb = blob_of(records)
    assert_equals_restatement(a.bamSort(data, bb), records, what=what)


def check_optional_outputs(a):
    recs = key_shape_cases()["descending"]
    data, bb = blob_of(recs)
    for wk, wp in ((False, True), (True, False), (False, False)):
        got = a.bamSort(data, bb, want_key=wk, want_perm=wp)
        assert (got["key"] is None) == (not wk) and (got["perm"] is None) == (not wp)
        assert_equals_restatement(got, recs, what=(wk, wp))


def check_host_residues(a):
    """input and output at each of RESIDUE_PAIRS (the host form stages both at the residues they have on the host), guard bytes around the output"""
    recs = count_case(65) + long_record_case()[3:4]
    blob = b"".join(recs)
    exp = restate(recs)
    for s, d in RESIDUE_PAIRS:
        ibuf, iat = at_residue(len(blob), s)
        ibuf[iat:iat + len(blob)] = np.frombuffer(blob, np.uint8)
        obuf, oat = at_residue(len(blob), d)
        bb = blob_of(recs)[1] + np.uint64(iat)                               # (block_begin[0]: where the first record starts)
        got = a.bamSort(ibuf, bb, out=obuf[oat:oat + len(blob)])
        assert (ibuf.ctypes.data + iat) % 16 == s and (obuf.ctypes.data + oat) % 16 == d
        assert (obuf[:oat] == GUARD).all() and (obuf[oat + len(blob):] == GUARD).all(), (s, d)
        assert obuf[oat:oat + len(blob)].tobytes() == exp[0] and (got["perm"] == exp[3]).all() and (got["sorted_begin"] == exp[1]).all(), (s, d)


def check_device_form(a, hb):
    """bamSort_device over HBM: both byte arrays at each of RESIDUE_PAIRS with guard bytes on both sides of the output (no store leaves the
    records' bytes), d_key / d_perm 0, and no records"""
    recs = count_case(257) + long_record_case()[3:4]
    blob = np.frombuffer(b"".join(recs), np.uint8)
    nb, n = blob.size, len(recs)
    exp = restate(recs)
    try:
        d_bb = hb.upload(blob_of(recs)[1])
        for s, d in RESIDUE_PAIRS:
            ibuf = np.full(nb + 64, GUARD, np.uint8); ibuf[16 + s:16 + s + nb] = blob
            obuf0 = np.full(nb + 64, GUARD, np.uint8)
            sb0, key0, perm0 = np.full(n + 1, 7, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint32)
            d_in, d_out, d_sb, d_key, d_perm = hb.upload(ibuf), hb.upload(obuf0), hb.upload(sb0), hb.upload(key0), hb.upload(perm0)
            assert d_in % 16 == 0 and d_out % 16 == 0
            want = (s % 3 != 1, s % 3 != 2)
            a.bamSort_device(n, d_in + 16 + s, d_bb, d_out + 16 + d, d_sb, d_key if want[0] else 0, d_perm if want[1] else 0)
            obuf = hb.download(d_out, obuf0)
            assert (obuf[:16 + d] == GUARD).all() and (obuf[16 + d + nb:] == GUARD).all(), (s, d)
            assert obuf[16 + d:16 + d + nb].tobytes() == exp[0], (s, d)
            assert (hb.download(d_sb, sb0) == exp[1]).all()
            assert (hb.download(d_key, key0) == (exp[2] if want[0] else 0)).all() and (hb.download(d_perm, perm0) == (exp[3] if want[1] else 0)).all()
        d0 = hb.upload(np.full(1, 7, np.uint64))
        a.bamSort_device(0, 0, 0, 0, d0)
        assert int(hb.download(d0, np.zeros(1, np.uint64))[0]) == 0
    finally:
        hb.free_all()


def check_refusals(a, hb):
    """every refusal of include/snapgpu.h's list: SNAPGPU_E_INVALID (-1), the last-error text, the outputs untouched"""
    import pytest
    from snap_amd.aligner import SnapGpuError
    recs = make_records([1, 0, 2, 0], [5, 4, 3, 2], [20, 30, 12, 40])
    data, bb = blob_of(recs)
    n, nb = len(recs), data.size
    host = a.lib.snapgpu_bam_sort
    host.argtypes = [C.c_void_p, C.c_uint64] + [C.c_void_p] * 6
    last = a.lib.snapgpu_last_error
    last.restype = C.c_char_p

    def outputs():
        return np.full(nb, GUARD, np.uint8), np.full(n + 1, 0x77, np.uint64), np.full(n, 0x55, np.uint64), np.full(n, 0x33, np.uint32)

    def untouched(o):
        return (o[0] == GUARD).all() and (o[1] == 0x77).all() and (o[2] == 0x55).all() and (o[3] == 0x33).all()

    p = lambda x: x.ctypes.data_as(C.c_void_p)
    # ---- NULL where a pointer is needed
    for missing in ("bytes", "block_begin", "sorted", "sorted_begin"):
        o = outputs()
        args = dict(bytes=p(data), block_begin=p(bb), sorted=p(o[0]), sorted_begin=p(o[1]))
        args[missing] = None
        assert host(a.handle, n, args["bytes"], args["block_begin"], args["sorted"], args["sorted_begin"], p(o[2]), p(o[3])) == -1, missing
        assert b"snapgpu_bam_sort: null argument" in last(a.handle) and untouched(o), missing
    o = outputs()
    assert host(a.handle, 0, None, None, None, None, None, None) == -1 and b"null argument" in last(a.handle)
    # ---- more than 2^32 - 1 records (refused before anything is read)
    assert host(a.handle, 2 ** 32, p(data), p(bb), p(o[0]), p(o[1]), p(o[2]), p(o[3])) == -1
    assert b"2^32 - 1 records" in last(a.handle) and untouched(o)
    # ---- a decreasing block_begin, a record shorter than 12 bytes: the host form, then the device form (found by the key pass, in HBM)
    down = bb.copy(); down[2] = down[1] - 1
    short_recs = list(recs); short_recs[2] = short_recs[2][:11]
    sdata, sbb = blob_of(short_recs)
    for what, d_, b_, text in (("decreasing", data, down, r"record 1: block_begin must be non-decreasing"), ("short", sdata, sbb, r"record 2: a BAM record is at least 12 bytes")):
        o = outputs()
        with pytest.raises(SnapGpuError, match=r"failed \(-1\).*" + text):
            a.bamSort(d_, b_, out=o[0])
        assert host(a.handle, n, p(d_), p(b_), p(o[0]), p(o[1]), p(o[2]), p(o[3])) == -1 and untouched(o), what
        try:
            d_in, d_bb = hb.upload(np.concatenate([d_, np.zeros(64, np.uint8)])), hb.upload(b_)
            d_o = [hb.upload(x) for x in o]
            with pytest.raises(SnapGpuError, match=r"failed \(-1\).*snapgpu_bam_sort_device: " + text):
                a.bamSort_device(n, d_in, d_bb, *d_o)
            assert untouched([hb.download(dp, x) for dp, x in zip(d_o, o)]), what
            with pytest.raises(SnapGpuError, match=r"failed \(-1\).*null argument"):
                a.bamSort_device(n, d_in, d_bb, 0, d_o[1])
        finally:
            hb.free_all()
    # ---- two faults in one call: the message names the first bad record with its own reason (record 1 is short, record 2 ends before it begins)
    mixed_recs = [recs[0], recs[1][:11], recs[2], recs[3]]
    mdata, mbb = blob_of(mixed_recs)
    mbb = mbb.copy(); mbb[3] = mbb[2] - 1
    try:
        d_in, d_bb = hb.upload(np.concatenate([mdata, np.zeros(64, np.uint8)])), hb.upload(mbb)
        d_o = [hb.upload(x) for x in outputs()]
        with pytest.raises(SnapGpuError, match=r"failed \(-1\).*snapgpu_bam_sort_device: record 1: a BAM record is at least 12 bytes"):
            a.bamSort_device(n, d_in, d_bb, *d_o)
    finally:
        hb.free_all()
    with pytest.raises(SnapGpuError, match=r"failed \(-1\).*snapgpu_bam_sort: record 1: a BAM record is at least 12 bytes"):
        a.bamSort(mdata, mbb)
    # ---- and the context still sorts
    check_case(a, recs)


# ---------------------------------------------------------------------------------------- the fused calls
def sorted_of_unsorted(one):
    """the restatement over what a _bam call returned"""
    return restate(bu.records_of(one))


def assert_fused(srt, one, n_rec):
    exp_bytes, exp_begin, exp_key, exp_perm = sorted_of_unsorted(one)
    assert not srt["truncated"] and srt["bam_bytes"] == one["bam_bytes"] == len(exp_bytes)
    assert (srt["block_begin"][:n_rec + 1] == exp_begin).all() and (srt["perm"][:n_rec] == exp_perm).all() and (srt["key"][:n_rec] == exp_key).all()
    assert srt["bytes"][:len(exp_bytes)].tobytes() == exp_bytes
    assert (srt["flag"] == one["flag"]).all()
    assert len(set(exp_key.tolist())) > 1 and (exp_perm != np.arange(n_rec)).any()          # (the batch is not in order already)


def check_fused_single(index, tag, n=150):
    """alignSamBamSorted == the restatement over alignSamBam's bytes; rec_begin and flag in record order; a byte capacity that is too small
    (nothing promised but the counts), then enlarged by `grow`; a record capacity that is too small"""
    reads, f, _, recs, ids = bu.golden_case("single", tag)
    z = su.fixture()
    o = reads["offsets"][:n + 1]
    bases, quals, fc, dl = reads["bases"][:int(o[-1])], reads["quals"][:int(o[-1])], z["front_clip"][:n], z["data_len"][:n]
    nb, noff = pack([b"r%d" % i for i in range(n)])
    cli, kw, sec, ae, use_m = su.SETS[tag]
    a = su.make_aligner(index, tag)
    try:
        a.setContigBamIds(ids)
        skip = su.skip_mask(bases, o, fc, dl, int(a.params.max_k))
        call = dict(use_m=bool(use_m), adjust_primary=bool(ae and sec is None))
        one = a.alignSamBam(bases, quals, o, fc, dl, skip, nb, noff, **call)
        srt = a.alignSamBamSorted(bases, quals, o, fc, dl, skip, nb, noff, **call)
        n_rec = one["n_records"]
        assert srt["n_records"] == n_rec and (srt["rec_begin"] == one["rec_begin"]).all() and not srt["records_truncated"]
        assert_fused(srt, one, n_rec)
        tight = a.alignSamBamSorted(bases, quals, o, fc, dl, skip, nb, noff, capacity=n_rec, byte_capacity=one["bam_bytes"] - 1, grow=False, **call)
        assert tight["truncated"] and tight["bam_bytes"] == one["bam_bytes"] and tight["n_records"] == n_rec and (tight["flag"] == one["flag"]).all()
        grown = a.alignSamBamSorted(bases, quals, o, fc, dl, skip, nb, noff, capacity=n_rec, byte_capacity=one["bam_bytes"] - 1, grow=True, **call)
        assert_fused(grown, one, n_rec)
        few = a.alignSamBamSorted(bases, quals, o, fc, dl, skip, nb, noff, capacity=n // 2, byte_capacity=16, grow=False, **call)
        assert few["records_truncated"] and few["n_records"] == n_rec
    finally:
        a.close()
    return n_rec


def check_fused_tiny_reads(index, n=120):
    """the tiny_reads fixture (100-base reads, the defaults): one record per read"""
    from snap_amd import abi
    from snap_amd.aligner import BaseAligner
    z = np.load(os.path.join(util.GOLDEN, "tiny_reads.npz"))
    bases, quals = z["b100"][:n].reshape(-1), z["q100"][:n].reshape(-1)
    o = np.arange(n + 1, dtype=np.uint64) * 100
    fc = np.zeros(n, np.int32); dl = np.full(n, 100, np.int32); skip = np.zeros(n, np.uint8)
    nb, noff = pack([b"t%d" % i for i in range(n)])
    a = BaseAligner(index, abi.default_params(max_k=8, max_read_len=160))
    try:
        a.setContigBamIds(bu.ref_ids(len(index.contigs)))
        one = a.alignSamBam(bases, quals, o, fc, dl, skip, nb, noff)
        srt = a.alignSamBamSorted(bases, quals, o, fc, dl, skip, nb, noff)
        assert one["n_records"] == srt["n_records"] == n
        assert_fused(srt, one, n)
    finally:
        a.close()


def check_fused_paired(index, n_pairs=150):
    """alignSamBamSortedPaired == the restatement over alignSamBamPaired's bytes on the paired_reads fixture: every record on its own (mates
    separate); flag, first_written and the results in record order; a capacity one byte short, then enlarged"""
    from snap_amd import abi
    from snap_amd.aligner import ChimericPairedEndAligner
    zp = np.load(os.path.join(util.GOLDEN, "paired_reads.npz"))
    o = zp["o150"][:2 * n_pairs + 1].astype(np.uint64)
    bases, quals = zp["b150"][:int(o[-1])], zp["q150"][:int(o[-1])]
    n = 2 * n_pairs
    fc = np.zeros(n, np.int32); dl = np.diff(o.astype(np.int64)).astype(np.int32); skip = np.zeros(n_pairs, np.uint8)
    skip[3] = 1                                                              # one pair that is not given to the aligner: two unmapped records
    nb, noff = pack([b"p%d/%d" % (i // 2, 1 + i % 2) for i in range(n)])
    a = ChimericPairedEndAligner(index, abi.default_params(max_k=8, max_read_len=160), abi.default_paired_params())
    try:
        a.setContigBamIds(bu.ref_ids(len(index.contigs)))
        one = a.alignSamBamPaired(bases, quals, o, fc, dl, skip, nb, noff, want_results=True)
        srt = a.alignSamBamSortedPaired(bases, quals, o, fc, dl, skip, nb, noff, want_results=True)
        assert_fused(srt, one, n)
        assert (srt["first_written"] == one["first_written"]).all() and srt["results"].tobytes() == one["results"].tobytes()
        assert (np.abs(np.diff(np.argsort(srt["perm"])[:n].reshape(-1, 2), axis=1)) > 1).any()          # (some mates are apart)
        tight = a.alignSamBamSortedPaired(bases, quals, o, fc, dl, skip, nb, noff, byte_capacity=one["bam_bytes"] - 1, grow=False)
        assert tight["truncated"] and tight["bam_bytes"] == one["bam_bytes"] and (tight["flag"] == one["flag"]).all()
        grown = a.alignSamBamSortedPaired(bases, quals, o, fc, dl, skip, nb, noff, byte_capacity=one["bam_bytes"] - 1, grow=True)
        assert_fused(grown, one, n)
    finally:
        a.close()


# ---------------------------------------------------------------------------------------- the tool: snapgpu-sam -so
TOOL_CASES = [("single", ()), ("single", ("-om", "1")), ("single", ("-ea",)), ("paired", ()), ("paired", ("-om", "1")), ("paired", ("-ea",))]
TOOL_BATCH = {"single": ("32", "50"), "paired": ("20", "36")}                # -b: at least five runs of the 160-read / 56-pair inputs; a second value
CLOSING_LINE = r"snapgpu-sam: sorted on the device: (\d+) runs, (\d+) records, (\d+) spilled"


def make_tool_workload(d, mode):
    """the 160-read / 56-pair inputs (a genome with an ALT contig, so that -ea has first-ALT records and, for pairs, batches that leave the device path)"""
    from tests.test_zz_gpu_native_sam import make_paired_alt_workload, make_workload
    if mode == "single":
        index_dir, fastq = make_workload(d, 160, genome_bases=300_000)
        return index_dir, [fastq]
    return make_paired_alt_workload(d, 56, genome_bases=300_000)


def run_tool(tool, mode, index_dir, fqs, out, opts, env=None, unset=(), expect=0):
    import subprocess
    e = dict(os.environ if env is None else env)
    for k in ("SNAPGPU_SAM_DEVICE_BAM", "SNAPGPU_SAM_DEVICE_BGZF") + tuple(unset):
        e.pop(k, None)
    e.update(env or {})
    r = subprocess.run([tool, mode, index_dir] + list(fqs) + ["-o", out] + list(opts), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, stdin=subprocess.DEVNULL, timeout=3000, env=e)
    log = r.stdout.decode(errors="replace")
    assert (r.returncode == 0) == (expect == 0), "snapgpu-sam exited with %d:\n%s" % (r.returncode, log[-3000:])
    return log


def check_tool(tool, d, mode, opts, env=None, workload=None):
    """`snapgpu-sam ... -so -o x.bam`: the decompressed record stream is the restatement over the stream of the same command without -so; the
    header differs in the sort-order line alone; the stream is the same under -sm 0 (every run spills), the default -sm, two values of -b, -q 1
    and -q 3, and SNAPGPU_SAM_DEVICE_BGZF unset and 1; the temporary file is gone.  Returns (records, runs)."""
    import re
    from tests.test_zz_gpu_native_sam import bam_parts
    index_dir, fqs = workload or make_tool_workload(d, mode)
    b0, b1 = TOOL_BATCH[mode]
    out = os.path.join(d, "x.bam")                                           # (the same output path every time: it is part of @PG)
    run_tool(tool, mode, index_dir, fqs, out, list(opts) + ["-b", b0], env)
    u_text, u_refs, u_recs = bam_parts(out)
    exp = restate(u_recs)[0]
    assert len(set(map(key_of, u_recs))) > 10 and exp != b"".join(u_recs)    # (the input is not in order already)
    variants = [(["-b", b0], {}), (["-b", b0, "-sm", "0"], {}), (["-b", b1], {}), (["-b", b0, "-q", "1"], {}), (["-b", b0, "-q", "3"], {}),
                (["-b", b0], {"SNAPGPU_SAM_DEVICE_BGZF": "1"}), (["-b", b0, "-sm", "0"], {"SNAPGPU_SAM_DEVICE_BGZF": "1"})]
    runs0 = None
    for extra, switch in variants:
        e = dict(env or {}); e.update(switch)
        log = run_tool(tool, mode, index_dir, fqs, out, list(opts) + ["-so"] + extra, e)
        m = re.search(CLOSING_LINE, log)
        assert m, log[-800:]
        runs, records, spilled = map(int, m.groups())
        assert records == len(u_recs) and spilled == (runs if "-sm" in extra else 0), (extra, switch, m.group(0))
        if extra == ["-b", b0]:
            assert runs >= 5 and (runs0 is None or runs == runs0)
            runs0 = runs
        assert not os.path.exists(out + ".sort.tmp") and not os.path.exists(out + ".partial")
        text, refs, recs = bam_parts(out)
        assert b"".join(recs) == exp, "the -so stream is not the stable sort of the stream without -so (%r, %r)" % (extra, switch)
        assert refs == u_refs
        a, b = text.split(b"\n"), u_text.split(b"\n")
        assert len(a) == len(b) and [i for i in range(len(a)) if a[i] != b[i]] == [0], (a[:2], b[:2])
        assert a[0] == b"@HD\tVN:1.6\tSO:coordinate" and b[0] == b"@HD\tVN:1.6\tGO:query"
    return len(u_recs), runs0


def check_tool_refuses_sorted_sam(tool, d, workload):
    index_dir, fqs = workload
    out = os.path.join(d, "x.sam")
    log = run_tool(tool, "single", index_dir, fqs, out, ["-so"], expect=1)
    assert "-so writes a coordinate-sorted BAM file: -o must end in .bam" in log and not os.path.exists(out)


def check_tool_against_reference(tool, d, mode, opts, workload):
    """the live reference CLI's `-so -o x.bam` (without its index and its duplicate marking, which are not built here) on the same inputs: the same
    header line, the same multiset of records, the same key sequence over the records with refID >= 0.  Its order among ties depends on its
    threads and where it puts refID -1 is its own business: neither is compared.  Returns where it put the refID -1 records ("last", "first" or "mixed")."""
    import subprocess
    from oracle import ref
    from tests.test_zz_gpu_native_sam import bam_parts
    index_dir, fqs = workload
    out_ref, out_new = os.path.join(d, "ref_so.bam"), os.path.join(d, "new_so.bam")
    r = subprocess.run([ref.CLI_PATH, mode, index_dir] + list(fqs) + ["-o", out_ref, "-so", "-S", "id", "-t", "1"] + list(opts), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       stdin=subprocess.DEVNULL, timeout=3000)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    run_tool(tool, mode, index_dir, fqs, out_new, list(opts) + ["-so", "-b", TOOL_BATCH[mode][0]])
    a, b = bam_parts(out_ref), bam_parts(out_new)
    assert a[0] == b[0] and a[1] == b[1]                                     # (the header text but @PG: the sort-order line is the reference's)
    if "-ea" in opts:
        # with -ea the reference writes its first-ALT result as a secondary record whose `supplementary` member nothing ever sets (a stack object,
        # SingleAligner.cpp:249): bit 0x800 of such a record is whatever the stack held (tests/test_zz_gpu_native_sam.sam_lines).  Not compared.
        def unset_0x800(x):
            flag = struct.unpack_from("<H", x, 18)[0]
            return x[:18] + struct.pack("<H", flag & ~0x800) + x[20:] if flag & 0x100 else x
        a, b = (a[0], a[1], list(map(unset_0x800, a[2]))), (b[0], b[1], list(map(unset_0x800, b[2])))
    # (-t 1, as in run_and_compare_bam: with several aligner threads the reference's own records depend on which thread saw which read first)
    only_ref, only_new = sorted(set(a[2]) - set(b[2])), sorted(set(b[2]) - set(a[2]))
    print("records: reference %d, here %d; only in the reference's file %d, only here %d" % (len(a[2]), len(b[2]), len(only_ref), len(only_new)))
    assert sorted(a[2]) == sorted(b[2]), (only_ref[:1], only_new[:1])
    mapped = lambda recs: [key_of(x) for x in recs if key_of(x) >> 32 != 0xFFFFFFFF]
    assert mapped(a[2]) == mapped(b[2]) and len(mapped(a[2])) > len(a[2]) // 2
    un = [i for i, x in enumerate(a[2]) if key_of(x) >> 32 == 0xFFFFFFFF]
    if not un:
        return "none"
    return "last" if un[0] == len(a[2]) - len(un) else "first" if un[-1] == len(un) - 1 else "mixed"
