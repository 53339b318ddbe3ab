"""Shared by the BAM-record tests (snapgpu_bam_records_single* / _paired*, snapgpu_align_sam_single_bam / _paired_bam): a plain-Python
restatement of the bytes one record gets in a BAM file before BGZF compression (BAMFormat::writeRead / writePairs, Bam.cpp:1312-1508 /
1033-1309; reg2bin :523-535; SeqToCode :505-510, which starts at code 1, so '=' is 15 like every unknown byte; CigarCodeToRefBase :270,
which counts M D N P = X; the aux fields :1510-1650), the handcrafted records and pair units that cover the layout's edges, and the checks
the emulator's and the device's test files both run.  The restatement knows nothing of the library."""
import os
import struct

import numpy as np

from tests import samrec_util as su
from tests import util
from tests.samtext_paired_util import make_quals, qs_of, strip_suffixes
from tests.samtext_util import RC, pack

SYMBOLS = ("snapgpu_set_contig_bam_ids", "snapgpu_bam_records_single", "snapgpu_bam_records_single_device", "snapgpu_align_sam_single_bam",
           "snapgpu_bam_records_paired", "snapgpu_bam_records_paired_device", "snapgpu_align_sam_paired_bam")
W_TEXT_TRUNCATED = 3
OPS_STRIDE = 66
FIELDS = ("flag", "contig", "pos", "mapq", "ops", "n_ops", "nm")
PAIR_FIELDS = FIELDS + ("rnext", "pnext", "tlen")
READS = ("bases", "quals", "offsets", "names", "name_off")
GOLDEN = os.path.join(util.GOLDEN, "bam_records.npz")
PAIRED_TAGS = ("default", "lvonly", "eqx")                                 # samtext_paired_util.FIXTURE_TAGS: the sets of sam_fields_paired.npz

SEQ_CODE = bytearray([15] * 256)
for _i in range(1, 16):
    SEQ_CODE[b"=ACMGRSVTWYHKDBN"[_i]] = _i
REF_BASE = (1, 0, 1, 1, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0)
AUX = b"RGZFASTQ\0PLZIllumina\0PUZpu\0LBZlb\0SMZsm\0PGZSNAP\0NMC"


def i32(x):
    return (int(x) + 2 ** 31) % 2 ** 32 - 2 ** 31


def reg2bin(beg, end):
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def bam_record(name, flag, ref, pos, mapq, ops, n_ops, next_ref, pnext, tlen, seq, qual, nm, qs=None):
    """One record, its block_size word included.  name: bytes, already without a pair's suffix; ref / next_ref: BAM reference numbers (-1:
    none); pos / pnext 1-based as the SAM fields have them; qs: None for a single-end record (no QS:i, no bin from the mate)."""
    qn = name.split(b" ", 1)[0]
    n_cig = max(int(n_ops), 0)
    row = [int(x) for x in ops[:n_cig]]
    ref_len = sum(REF_BASE[op & 15] * (op >> 4) for op in row) % 2 ** 32 if n_cig else len(seq)
    pos0, pnext0 = i32(pos - 1), i32(pnext - 1)
    if not flag & 0x4:
        b = reg2bin(pos0, i32(pos0 + ref_len))
    elif qs is not None and not flag & 0x8:
        b = reg2bin(pnext0, i32(pnext0 + 1))
    else:
        b = reg2bin(-1, 0)
    t = int(tlen)
    t = t & 0x7fffffff if t >= 0 else -((-t) & 0x7fffffff)
    if flag & 0x10:
        seq, qual = seq.translate(RC)[::-1], qual[::-1]
    codes = [SEQ_CODE[c] for c in seq] + [0]
    body = struct.pack("<iiIIIiii", ref, pos0, ((b << 16) | ((mapq & 0xff) << 8) | (len(qn) + 1)) & 0xffffffff, ((flag << 16) | n_cig) & 0xffffffff,
                       len(seq), next_ref, pnext0, t)
    body += qn + b"\0" + struct.pack("<%dI" % n_cig, *row)
    body += bytes((codes[2 * j] << 4) | codes[2 * j + 1] for j in range((len(seq) + 1) // 2)) + bytes((c - 33) & 255 for c in qual)
    body += AUX + bytes([nm & 255]) + (b"QSi" + struct.pack("<i", qs) if qs is not None else b"")
    return struct.pack("<I", len(body)) + body


def _read(h, rd):
    b, e = int(h["offsets"][rd]), int(h["offsets"][rd + 1])
    return (h["bases"][b:e].tobytes(), h["quals"][b:e].tobytes(), h["names"][int(h["name_off"][rd]):int(h["name_off"][rd + 1])].tobytes())


def expected_single(ref_id, h, f=None, rec_read="own"):
    """The records of a single-end call: h the reads, f the fields (default: h's), rec_read None: record i is read i."""
    f = h if f is None else f
    rr = h["rec_read"] if isinstance(rec_read, str) else rec_read
    out = []
    for r in range(len(f["flag"])):
        s, q, nm = _read(h, r if rr is None else int(rr[r]))
        c = int(f["contig"][r])
        out.append(bam_record(nm, int(f["flag"][r]), -1 if c < 0 else int(ref_id[c]), int(f["pos"][r]), int(f["mapq"][r]), f["ops"][r], int(f["n_ops"][r]),
                              -1, 0, 0, s, q, int(f["nm"][r])))
    return out


def expected_pairs(ref_id, h, f, first_written, unit_pair):
    """The 2 * n_units records of a paired call, in file order."""
    out = []
    for u in range(len(first_written)):
        k = u if unit_pair is None else int(unit_pair[u])
        rd = [_read(h, 2 * k + v) for v in (0, 1)]
        nm = strip_suffixes(rd[0][2], rd[1][2])
        fw = int(first_written[u])
        for v in (fw, 1 - fw):
            i = 2 * u + v
            c, rn = int(f["contig"][i]), int(f["rnext"][i])
            ref = -1 if c < 0 else int(ref_id[c])
            out.append(bam_record(nm[v], int(f["flag"][i]), ref, int(f["pos"][i]), int(f["mapq"][i]), f["ops"][i], int(f["n_ops"][i]),
                                  ref if rn == -2 else -1 if rn == -1 else int(ref_id[rn]), int(f["pnext"][i]), int(f["tlen"][i]), rd[v][0], rd[v][1],
                                  int(f["nm"][i]), qs_of(rd[1 - v][1])))
    return out


def records_of(got, n=None):
    bb = got["block_begin"].astype(np.int64)
    n = bb.size - 1 if n is None else n
    return [got["bytes"][bb[i]:bb[i + 1]].tobytes() for i in range(n)]


def first_difference(got, exp):
    assert len(got) == len(exp), (len(got), len(exp))
    bad = [i for i, (x, y) in enumerate(zip(got, exp)) if x != y]
    assert not bad, "%d records differ, record %d:\n%r\n%r" % (len(bad), bad[0], got[bad[0]], exp[bad[0]])


# ---------------------------------------------------------------------------------------- handcrafted records
US = [1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000]
NAMES = [b" spacefirst", b"x", b"abc rest", b"abcd", b"abcde", b"q" * 63, b"r" * 64 + b" tail", b"s" * 65, b"t" * 254]       # cut lengths 0 1 3 4 5 63 64 65 254
ALPHABET = np.frombuffer(b"ACGTNacgtnMRWSYKVHDB=\xff.", np.uint8)
QUALS = np.array([33, 126, 10, 0xFF, 48, 64], np.uint8)
BIN_EDGES = [2 ** k for k in (14, 17, 20, 23, 26)]
NOPS = [-1, 0, 1, 63, 64, 65, OPS_STRIDE]
OPLENS = [1, 15, 16, 2 ** 28 - 1, 1000, 100]
TLENS = [0, 1, -1, 2 ** 31 - 1, -(2 ** 31 - 1), 2 ** 31, -2 ** 31, 2 ** 31 + 5, -(2 ** 31 + 5)]


def ref_ids(n_contigs):
    """a permutation of the contig numbers that is not the identity"""
    return np.roll(np.arange(n_contigs, dtype=np.int32), 1)[::-1].copy() if n_contigs > 2 else np.arange(n_contigs, dtype=np.int32)[::-1].copy()


def _reads(rng, n_reads, names, qual_kind=None):
    reads, quals = [], []
    for i in range(n_reads):
        U = US[i % len(US)]
        reads.append(rng.choice(ALPHABET, size=U).tobytes())
        quals.append(rng.choice(QUALS, size=U).tobytes() if qual_kind is None else make_quals(qual_kind(i), U, rng))
    b, off = pack(reads); q, _ = pack(quals); nb, noff = pack(names)
    return dict(bases=b, quals=q, offsets=off, names=nb, name_off=noff)


def _fields(n, n_contigs, paired):
    def cyc(vals, dtype): return np.array([vals[r % len(vals)] for r in range(n)], dtype)
    contigs = [-1, 0, n_contigs - 1] + list(range(1, n_contigs - 1))
    f = dict(contig=cyc(contigs, np.int32), mapq=cyc([0, 70, 255, 9], np.int32), nm=cyc([-1, 0, 255, 256, 7], np.int32), n_ops=cyc(NOPS, np.int32),
             pos=cyc([1, 9, 2 ** 29 + 100, 99_999_999, 2 ** 31 - 1 - 2 ** 29], np.int64))
    ops = np.zeros((n, OPS_STRIDE), np.uint32)
    for r in range(n):
        for j in range(OPS_STRIDE):
            ops[r, j] = (OPLENS[(r + j) % len(OPLENS)] << 4) | ((r + j) % 9)
    f["ops"] = ops
    # the spans inside and across every reg2bin boundary, and beyond 2^29: one 10M operation that ends 10 before / 5 behind the edge
    at = 30
    for edge in BIN_EDGES + [2 ** 29 + 2 ** 14]:
        for start in (edge - 20, edge - 5):
            f["pos"][at] = start + 1; f["n_ops"][at] = 1; f["ops"][at, 0] = (10 << 4) | 0
            at += 1
    if paired:
        f["rnext"] = cyc([-2, -1, 0, n_contigs - 1], np.int32); f["pnext"] = cyc([0, 1, 2 ** 14, 2 ** 29 + 7, 123456], np.int64); f["tlen"] = cyc(TLENS, np.int64)
    return f, at


def handcrafted(n_contigs, seed=11):
    """About 150 records over 26 reads: every length of US with both orientations first (records 0..25 on reads 0..12), every cut name length
    against several lengths, then every list against every other by their different periods; records 30..41 are the reg2bin spans."""
    rng = np.random.default_rng(seed)
    n_reads = 2 * len(US)
    h = _reads(rng, n_reads, [NAMES[i % len(NAMES)] for i in range(n_reads)])
    rec_read = [i // 2 for i in range(2 * len(US))] + [int(x) for x in rng.integers(0, n_reads, size=130)]
    rec_read += list(range(len(US), n_reads))                                # (every read has a record: the rec_read = NULL run uses them all)
    n = len(rec_read)
    f, _ = _fields(n, n_contigs, False)
    flags = [0, 16, 256, 272, 2064, 2048]
    flag = np.array([flags[r % 2] if r < 26 else flags[r % len(flags)] for r in range(n)], np.int32)
    for r in range(42, n, 9):                                                # unmapped, alone
        flag[r] = 4; f["pos"][r] = 0; f["contig"][r] = -1; f["n_ops"][r] = -1
    h.update(f, flag=flag, rec_read=np.array(rec_read, np.uint32))
    return h


PAIR_NAMES = [(b"a/1", b"a/2"), (b"a/2", b"a/1"), (b"a/1", b"a/1"), (b"a/1", b"ab/2"), (b"/1", b"/2"), (b"a/3", b"a/1"), (b"x y/1", b"x y/2"), (b"x/1 c", b"x/2 c"),
              (b"n" * 254 + b"/1", b"n" * 254 + b"/2"), (b"plainname", b"plainname"), (b"left right", b"left other"), (b"r/1", b"r/1x"), (b" /1", b" /2")]


def handcrafted_pairs(n_contigs, seed=12):
    """39 pairs and 100 pair units over them (every pair first, then repeats: several units to a pair): the /1 /2 rule both ways and refused,
    both print orders, every TLENS value, QS over every kind of quality string, and the three unmapped cases (units 20..22)."""
    rng = np.random.default_rng(seed)
    n_pairs = 3 * len(PAIR_NAMES)
    h = _reads(rng, 2 * n_pairs, [PAIR_NAMES[(m // 2) % len(PAIR_NAMES)][m % 2] for m in range(2 * n_pairs)], qual_kind=lambda m: (m + m // 7) % 6)
    unit_pair = list(range(n_pairs)) + [7, 7, 7, 8, 8] + [int(x) for x in rng.integers(0, n_pairs, size=56)]
    n_units = len(unit_pair); n = 2 * n_units
    f, _ = _fields(n, n_contigs, True)
    flags = [0x41, 0x85, 0x51, 0xA1, 0x63, 0x93, 0x871]
    f["flag"] = np.array([flags[r % len(flags)] for r in range(n)], np.int32)
    f["flag"][1::4] ^= 0x10
    for u, (fl0, fl1) in ((20, (0x45, 0x89)), (21, (0x49, 0x85)), (22, (0x4D, 0x8D))):      # mate 0 unmapped, mate 1 unmapped, both unmapped
        for v, fl in ((0, fl0), (1, fl1)):
            i = 2 * u + v
            f["flag"][i] = fl
            if fl & 0x4:
                f["pos"][i] = 0; f["contig"][i] = -1; f["n_ops"][i] = -1
            f["pnext"][i] = 0 if fl & 0x8 else 2 ** 17 + 3
    first_written = np.array([(u // 2 + u // 7) % 2 for u in range(n_units)], np.int32)
    h.update(f, first_written=first_written, unit_pair=np.array(unit_pair, np.uint32))
    return h


def make_aligner(index, ids="perm", paired=False, **kw):
    from snap_amd import abi
    from snap_amd.aligner import BaseAligner, ChimericPairedEndAligner
    p = abi.default_params(max_read_len=400, **kw)
    a = ChimericPairedEndAligner(index, p, abi.default_paired_params()) if paired else BaseAligner(index, p)
    if isinstance(ids, str):
        a.setContigBamIds(ref_ids(len(index.contigs)))
    elif ids is not None:
        a.setContigBamIds(ids)
    return a


def run_single(a, h, rec=None, **kw):
    sel = slice(None) if rec is None else rec
    return a.bamRecords(*[h[k] for k in READS], *[h[f][sel] for f in FIELDS], rec_read=h["rec_read"][sel], **kw)


def _rows(h, units):
    sel = slice(None) if units is None else units
    rows = np.arange(h["first_written"].size)[sel]
    return sel, np.stack([2 * rows, 2 * rows + 1], axis=1).reshape(-1)


def run_pairs(a, h, units=None, unit_pair=True, **kw):
    sel, rec = _rows(h, units)
    return a.bamRecordsPaired(*[h[k] for k in READS], *[h[k][rec] for k in PAIR_FIELDS], h["first_written"][sel],
                              unit_pair=h["unit_pair"][sel] if unit_pair else None, **kw)


def expected_of_pairs(ids, h, units=None):
    sel, rec = _rows(h, units)
    return expected_pairs(ids, h, {k: h[k][rec] for k in PAIR_FIELDS}, h["first_written"][sel], h["unit_pair"][sel])


def check_handcrafted(index):
    """Every handcrafted record through bamRecords -- all in one call, the first and the last on their own, without a record list, with the
    identity numbering -- and a name of 255 bytes after the cut refused with the record's number."""
    import pytest
    from snap_amd.aligner import SnapGpuError
    ids = ref_ids(len(index.contigs))
    h = handcrafted(len(ids))
    exp = expected_single(ids, h)
    assert {len(_read(h, int(r))[2].split(b" ", 1)[0]) for r in h["rec_read"]} >= {0, 1, 3, 4, 5, 63, 64, 65, 254}
    a = make_aligner(index)
    try:
        got = run_single(a, h)
        assert not got["truncated"] and got["bam_bytes"] == sum(map(len, exp))
        first_difference(records_of(got), exp)
        for r in (0, len(exp) - 1):
            assert records_of(run_single(a, h, rec=slice(r, r + 1))) == [exp[r]], r
        n = h["offsets"].size - 1
        first = [int(np.flatnonzero(h["rec_read"] == i)[0]) for i in range(n)]
        sub = {f: h[f][first] for f in FIELDS}
        plain = a.bamRecords(*[h[k] for k in READS], *[sub[f] for f in FIELDS])
        first_difference(records_of(plain), expected_single(ids, h, sub, rec_read=None))
        a.setContigBamIds(None)                                               # NULL: the identity
        first_difference(records_of(run_single(a, h, rec=slice(0, 40))), expected_single(np.arange(len(ids)), h)[:40])
        a.setContigBamIds(ids)
        long = dict(h)
        names = [_read(h, i)[2] for i in range(n)]
        names[5] = b"u" * 255 + b" rest"
        long["names"], long["name_off"] = pack(names)
        r5 = int(np.flatnonzero(h["rec_read"] == 5)[0])
        with pytest.raises(SnapGpuError, match=r"failed \(-1\).*record %d\b.*QNAME" % r5):
            run_single(a, long)
        names[5] = b"u" * 254 + b" rest"
        long["names"], long["name_off"] = pack(names)
        assert len(records_of(run_single(a, long))) == len(exp)
    finally:
        a.close()
    return h, exp


def check_handcrafted_pairs(index):
    ids = ref_ids(len(index.contigs))
    h = handcrafted_pairs(len(ids))
    exp = expected_of_pairs(ids, h)
    a = make_aligner(index, paired=True)
    try:
        got = run_pairs(a, h)
        assert not got["truncated"] and got["bam_bytes"] == sum(map(len, exp))
        first_difference(records_of(got), exp)
        for u in (0, h["first_written"].size - 1):
            first_difference(records_of(run_pairs(a, h, units=slice(u, u + 1))), exp[2 * u:2 * u + 2])
        n_pairs = (h["offsets"].size - 1) // 2
        plain = run_pairs(a, h, units=slice(0, n_pairs), unit_pair=False)        # unit_pair NULL: unit u is pair u (the first units are the pairs in order)
        first_difference(records_of(plain), exp[:2 * n_pairs])
    finally:
        a.close()
    return h, exp


def _check_capacities(run, full, guard=32):
    """An exact capacity, one byte short and none, into the middle of a buffer of 0xCD: nothing before the bytes, at or beyond the capacity is
    written; the records that fit are the full run's; block_begin and bam_bytes are complete."""
    tb = full["bam_bytes"]
    ref = records_of(full)
    bb = full["block_begin"].astype(np.int64)
    for cap in (tb, tb - 1, 0):
        buf = np.full(guard + tb + guard, 0xCD, np.uint8)
        got = run(bytes_out=buf[guard:guard + cap], grow=False)
        assert got["truncated"] == (cap < tb) and got["bam_bytes"] == tb and (got["block_begin"] == full["block_begin"]).all(), cap
        fit = int(np.searchsorted(bb[1:], cap, side="right"))
        assert fit == (len(ref) if cap == tb else len(ref) - 1 if cap else 0)
        body = buf[guard:]
        assert [body[bb[i]:bb[i + 1]].tobytes() for i in range(fit)] == ref[:fit], cap
        assert (buf[:guard] == 0xCD).all() and (body[bb[fit]:] == 0xCD).all(), cap


def check_memory_discipline(index):
    ids = ref_ids(len(index.contigs))
    h = handcrafted(len(ids))
    a = make_aligner(index)
    try:
        _check_capacities(lambda **kw: run_single(a, h, **kw), run_single(a, h))
        none = a.bamRecords(*[h[k] for k in READS], *[h[f][:0] for f in FIELDS], rec_read=h["rec_read"][:0], bytes_out=np.full(16, 0xCD, np.uint8))
        assert none["bam_bytes"] == 0 and int(none["block_begin"][0]) == 0 and (none["bytes"] == 0xCD).all()
    finally:
        a.close()
    hp = handcrafted_pairs(len(ids))
    a = make_aligner(index, paired=True)
    try:
        _check_capacities(lambda **kw: run_pairs(a, hp, **kw), run_pairs(a, hp))
    finally:
        a.close()


def scan_counts():
    """n_records at the edges of the scan's tiles (sam_text.h: tiles of 1024 records, whose sums one lane scans) and one tile more than 64 tiles"""
    return (1, 1023, 1024, 1025, 65 * 1024)


def check_scan_levels(index):
    """block_begin is the running sum of the restatement's record lengths, and the bytes are the records, 1- and 2-base reads."""
    ids = ref_ids(len(index.contigs))
    a = make_aligner(index)
    rng = np.random.default_rng(5)
    try:
        for n in scan_counts():
            U = rng.integers(1, 3, size=n)
            offsets = np.concatenate([[0], np.cumsum(U)]).astype(np.uint64)
            h = dict(bases=rng.choice(np.frombuffer(b"ACGT", np.uint8), size=int(offsets[-1])), quals=rng.integers(33, 127, size=int(offsets[-1])).astype(np.uint8),
                     offsets=offsets)
            h["names"], h["name_off"] = pack([b"r%d" % i for i in range(n)])
            f = dict(flag=(rng.integers(0, 2, size=n) * 16).astype(np.int32), contig=rng.integers(-1, len(ids), size=n).astype(np.int32),
                     pos=rng.integers(1, 10 ** 8, size=n).astype(np.int64), mapq=rng.integers(0, 71, size=n).astype(np.int32),
                     n_ops=rng.integers(-1, 3, size=n).astype(np.int32), nm=rng.integers(-1, 30, size=n).astype(np.int32),
                     ops=((rng.integers(1, 2000, size=(n, 2)) << 4) | rng.integers(0, 9, size=(n, 2))).astype(np.uint32))
            got = a.bamRecords(*[h[k] for k in READS], *[f[k] for k in FIELDS])
            exp = expected_single(ids, h, f, rec_read=None)
            assert got["block_begin"].dtype == np.uint64
            assert (got["block_begin"].astype(np.int64) == np.concatenate([[0], np.cumsum([len(x) for x in exp])])).all(), n
            assert got["bytes"][:got["bam_bytes"]].tobytes() == b"".join(exp), n
    finally:
        a.close()
    hp = handcrafted_pairs(len(ids))
    a = make_aligner(index, paired=True)
    try:
        n_pairs = (hp["offsets"].size - 1) // 2
        for n_units in (511, 512, 513):                                      # two records a unit: the same tile edges from the pair side
            big = {k: hp[k] for k in READS}
            rep = np.arange(n_units) % hp["first_written"].size
            rec = np.stack([2 * rep, 2 * rep + 1], axis=1).reshape(-1)
            big.update({k: hp[k][rec] for k in PAIR_FIELDS}, first_written=hp["first_written"][rep], unit_pair=hp["unit_pair"][rep])
            got = run_pairs(a, big)
            first_difference(records_of(got), expected_of_pairs(ids, big))
        assert n_pairs > 0
    finally:
        a.close()


def check_errors(index):
    """No BAM numbers; a wrong count of them; n_ops beyond ops_stride; a contig or an rnext the index does not have; a first_written that is
    neither 0 nor 1: SNAPGPU_E_INVALID each."""
    import pytest
    from snap_amd.aligner import SnapGpuError
    ids = ref_ids(len(index.contigs))
    h = handcrafted(len(ids))
    a = make_aligner(index, ids=None)
    try:
        with pytest.raises(SnapGpuError, match=r"failed \(-1\).*snapgpu_set_contig_bam_ids"):
            run_single(a, h)
        for wrong in (ids[:-1], np.concatenate([ids, [0]])):
            with pytest.raises(SnapGpuError, match=r"failed \(-1\)"):
                a.setContigBamIds(wrong)
        a.setContigBamIds(ids)
        for key, val in (("n_ops", OPS_STRIDE + 1), ("contig", len(ids))):
            bad = dict(h); bad[key] = h[key].copy(); bad[key][17] = val
            with pytest.raises(SnapGpuError, match=r"failed \(-1\).*ops_stride"):
                run_single(a, bad)
        first_difference(records_of(run_single(a, h, rec=slice(0, 30))), expected_single(ids, h)[:30])
    finally:
        a.close()
    hp = handcrafted_pairs(len(ids))
    a = make_aligner(index, ids=None, paired=True)
    try:
        with pytest.raises(SnapGpuError, match=r"failed \(-1\).*snapgpu_set_contig_bam_ids"):
            run_pairs(a, hp)
        a.setContigBamIds(ids)
        for key, val in (("n_ops", OPS_STRIDE + 1), ("contig", len(ids)), ("rnext", len(ids)), ("rnext", -3), ("first_written", 2), ("first_written", -1)):
            bad = dict(hp); bad[key] = hp[key].copy(); bad[key][9] = val
            with pytest.raises(SnapGpuError, match=r"failed \(-1\).*first_written"):
                run_pairs(a, bad)
    finally:
        a.close()


def check_device_form(index, hb):
    """bamRecords_device / bamRecordsPaired_device == the host forms, with d_bytes 0, 1, 2 and 3 bytes behind a dword boundary, guard bytes
    on both sides, a capacity that is too small, and no records."""
    ids = ref_ids(len(index.contigs))
    for paired in (False, True):
        h = handcrafted_pairs(len(ids)) if paired else handcrafted(len(ids))
        a = make_aligner(index, paired=paired)
        try:
            host = run_pairs(a, h) if paired else run_single(a, h)
            tb = host["bam_bytes"]
            keys = READS + (("unit_pair",) if paired else ("rec_read",)) + (PAIR_FIELDS + ("first_written",) if paired else FIELDS)
            d = {k: hb.upload(h[k]) for k in keys}
            n = h["first_written"].size if paired else h["flag"].size
            n_rec = 2 * n if paired else n
            for shift, cap in ((0, tb), (1, tb), (2, tb), (3, tb), (1, tb // 2)):
                buf0 = np.full(tb + 64, 0xCD, np.uint8); bb0 = np.zeros(n_rec + 1, np.uint64)
                d_buf, d_bb = hb.upload(buf0), hb.upload(bb0)
                assert d_buf % 4 == 0
                at = 16 + shift
                if paired:
                    got = a.bamRecordsPaired_device(n, *[d[k] for k in READS], d["unit_pair"], *[d[k] for k in FIELDS[:5]], OPS_STRIDE, d["n_ops"], d["nm"],
                                                    d["rnext"], d["pnext"], d["tlen"], d["first_written"], cap, d_buf + at, d_bb)
                else:
                    got = a.bamRecords_device(n, *[d[k] for k in READS], d["rec_read"], *[d[k] for k in FIELDS[:5]], OPS_STRIDE, d["n_ops"], d["nm"], cap,
                                              d_buf + at, d_bb)
                assert got == (tb, cap < tb), (paired, shift, cap)
                bb = hb.download(d_bb, bb0); buf = hb.download(d_buf, buf0)
                assert (bb == host["block_begin"]).all()
                fit = int(np.searchsorted(bb[1:].astype(np.int64), cap, side="right"))
                assert (buf[:at] == 0xCD).all() and (buf[at + int(bb[fit]):] == 0xCD).all(), (paired, shift, cap)
                assert buf[at:at + int(bb[fit])].tobytes() == host["bytes"][:int(bb[fit])].tobytes(), (paired, shift, cap)
            d0 = hb.upload(np.full(1, 7, np.uint64))
            if paired:
                assert a.bamRecordsPaired_device(0, *([0] * 11), OPS_STRIDE, *([0] * 6), 0, 0, d0) == (0, False)
            else:
                assert a.bamRecords_device(0, *([0] * 11), OPS_STRIDE, 0, 0, 0, 0, d0) == (0, False)
            assert int(hb.download(d0, np.zeros(1, np.uint64))[0]) == 0
        finally:
            a.close()
            hb.free_all()


# ---------------------------------------------------------------------------------------- the reference CLI's bytes, the fused forms, the tool
def golden():
    return np.load(GOLDEN)


def split_records(blob):
    out, at = [], 0
    while at < len(blob):
        n = 4 + struct.unpack_from("<I", blob, at)[0]
        out.append(blob[at:at + n]); at += n
    assert at == len(blob)
    return out


def golden_case(kind, tag):
    """(reads, fields, unit first_written or None, the reference CLI's records, ref_id) of one set of tests/golden/bam_records.npz: the reads
    and the fields are the first of sam_records_single.npz (names r<i>) / sam_fields_paired.npz (names p<i>/1, p<i>/2)."""
    z = golden()
    recs = split_records(z["%s_%s" % (kind, tag)].tobytes())
    if kind == "single":
        s = su.fixture(); n = int(z["single_n"])
        e = su.expected(s, tag)
        keep = e["rec_read"] < n
        f, fw, names = {k: e[k][keep] for k in e}, None, [b"r%d" % i for i in range(n)]
    else:
        s = np.load(os.path.join(util.GOLDEN, "sam_fields_paired.npz")); n = 2 * int(z["paired_n"])
        f = {k: s["%s_%s" % (tag, k)][:n] for k in PAIR_FIELDS}
        fw, names = s[tag + "_first_written"][:n // 2], [b"p%d/%d" % (i // 2, 1 + i % 2) for i in range(n)]
    offs = s["offsets"][:n + 1].astype(np.uint64); tot = int(offs[-1])
    reads = dict(bases=s["bases"][:tot], quals=s["quals"][:tot], offsets=offs)
    reads["names"], reads["name_off"] = pack(names)
    return reads, f, fw, recs, z[kind + "_ref_id"]


def check_restatement_against_reference(kind, tag):
    """No device: the restatement over the fields the reference CLI printed in SAM gives the bytes it wrote in BAM, record for record."""
    reads, f, fw, recs, ids = golden_case(kind, tag)
    exp = expected_single(ids, reads, f, rec_read=f["rec_read"]) if kind == "single" else expected_pairs(ids, reads, f, fw, None)
    first_difference(exp, recs)
    return len(recs)


def check_against_reference(index, kind, tag):
    """bamRecords / bamRecordsPaired over the fixture's fields: the reference CLI's bytes, record for record."""
    reads, f, fw, recs, ids = golden_case(kind, tag)
    a = make_aligner(index, ids=ids, paired=kind == "paired")
    try:
        if kind == "single":
            got = a.bamRecords(*[reads[k] for k in READS], *[f[k] for k in FIELDS], rec_read=f["rec_read"])
        else:
            got = a.bamRecordsPaired(*[reads[k] for k in READS], *[f[k] for k in PAIR_FIELDS], fw)
    finally:
        a.close()
    assert not got["truncated"] and got["bam_bytes"] == sum(map(len, recs))
    first_difference(records_of(got), recs)
    return len(recs)


def check_fused_single(index, tag="ea_om1", n=150):
    """alignSamBam == alignSamRecords followed by bamRecords, byte for byte; its two capacities (the records warning first); a cigar row that
    is too short; and, for the reads whose records do not depend on the batch's history, the reference CLI's bytes."""
    import pytest
    from snap_amd.aligner import SnapGpuError
    reads, f, _, recs, ids = golden_case("single", tag)
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
        rec = a.alignSamRecords(bases, quals, o, fc, dl, skip, **call)
        two = a.bamRecords(bases, quals, o, nb, noff, *[rec[k] for k in FIELDS], rec_read=rec["rec_read"])
        one = a.alignSamBam(bases, quals, o, fc, dl, skip, nb, noff, **call)
        assert one["n_records"] == rec["n_records"] and one["bam_bytes"] == two["bam_bytes"] and (one["block_begin"] == two["block_begin"]).all()
        assert one["bytes"][:one["bam_bytes"]].tobytes() == two["bytes"][:two["bam_bytes"]].tobytes() and (one["flag"] == rec["flag"]).all()
        few = a.alignSamBam(bases, quals, o, fc, dl, skip, nb, noff, capacity=n // 2, byte_capacity=16, grow=False, **call)
        assert few["records_truncated"] and few["n_records"] == rec["n_records"]
        tight = a.alignSamBam(bases, quals, o, fc, dl, skip, nb, noff, capacity=rec["n_records"], byte_capacity=two["bam_bytes"] - 1, grow=False, **call)
        assert tight["truncated"] and tight["bam_bytes"] == two["bam_bytes"] and (tight["block_begin"] == two["block_begin"]).all()
        assert records_of(tight, rec["n_records"] - 1) == records_of(two)[:-1]
        with pytest.raises(SnapGpuError, match=r"failed \(-1\).*ops_stride"):
            a.alignSamBam(bases, quals, o, fc, dl, skip, nb, noff, ops_stride=3, **call)
    finally:
        a.close()
    left_out = np.unique(rec["rec_read"][rec["stale"] != 0])
    assert left_out.size <= max(1, n // 100)
    keep = (f["rec_read"] < n) & ~np.isin(f["rec_read"], left_out)
    assert int((f["rec_read"] < n).sum()) == rec["n_records"]
    got = records_of(one)
    bad = [r for r in np.flatnonzero(keep) if got[r] != recs[r]]
    assert not bad, "%d records differ from the reference CLI's, record %d:\n%r\n%r" % (len(bad), bad[0], got[bad[0]], recs[bad[0]])
    return rec["n_records"]


def check_fused_paired(index, n_pairs=150):
    """alignSamBamPaired == alignSamPaired followed by bamRecordsPaired, byte for byte (the workload of the text twin); a capacity one byte
    short; a cigar row that is too short."""
    import pytest
    from snap_amd import abi
    from snap_amd.aligner import ChimericPairedEndAligner, SnapGpuError
    zp = np.load(os.path.join(util.GOLDEN, "paired_reads.npz"))
    o = zp["o150"][:2 * n_pairs + 1].astype(np.uint64)
    bases, quals = zp["b150"][:int(o[-1])], zp["q150"][:int(o[-1])]
    n = 2 * n_pairs
    fc = np.zeros(n, np.int32); dl = np.diff(o.astype(np.int64)).astype(np.int32); skip = np.zeros(n_pairs, np.uint8)
    skip[3] = 1                                                              # one pair that is not given to the aligner: two unmapped records
    nb, noff = pack([b"p%d/%d x" % (i // 2, 1 + i % 2) if i % 8 else b"p%d/%d" % (i // 2, 1 + i % 2) for i in range(n)])
    ids = ref_ids(len(index.contigs))
    a = ChimericPairedEndAligner(index, abi.default_params(max_k=8, max_read_len=160), abi.default_paired_params())
    try:
        a.setContigBamIds(ids)
        _, _, f = a.alignSamPaired(bases, quals, o, fc, dl, skip, want_results=False)
        two = a.bamRecordsPaired(bases, quals, o, nb, noff, *[f[k] for k in PAIR_FIELDS], f["first_written"])
        one = a.alignSamBamPaired(bases, quals, o, fc, dl, skip, nb, noff)
        assert int((f["flag"] & 4 == 0).sum()) > n_pairs                    # (the batch aligns)
        assert not one["truncated"] and one["bam_bytes"] == two["bam_bytes"] and (one["block_begin"] == two["block_begin"]).all()
        assert one["bytes"][:one["bam_bytes"]].tobytes() == two["bytes"][:two["bam_bytes"]].tobytes()
        assert (one["flag"] == f["flag"]).all() and (one["first_written"] == f["first_written"]).all()
        reads = dict(bases=bases, quals=quals, offsets=o, names=nb, name_off=noff)
        first_difference(records_of(two), expected_pairs(ids, reads, f, f["first_written"], None))
        tight = a.alignSamBamPaired(bases, quals, o, fc, dl, skip, nb, noff, byte_capacity=two["bam_bytes"] - 1, grow=False)
        assert tight["truncated"] and tight["bam_bytes"] == two["bam_bytes"] and (tight["block_begin"] == two["block_begin"]).all()
        assert records_of(tight, n - 1) == records_of(two)[:-1] and (tight["flag"] == f["flag"]).all()
        with pytest.raises(SnapGpuError, match=r"failed \(-1\).*ops_stride"):
            a.alignSamBamPaired(bases, quals, o, fc, dl, skip, nb, noff, ops_stride=3)
    finally:
        a.close()


def tool_env(env, switch):
    e = dict(os.environ if env is None else env)
    e.pop("SNAPGPU_SAM_DEVICE_BAM", None)
    if switch:
        e["SNAPGPU_SAM_DEVICE_BAM"] = "1"
    return e


def check_tool(tool, d, mode, index_dir, fqs, opts, env=None, expect_device=True, tool_opts=()):
    """`snapgpu-sam -o x.bam` with SNAPGPU_SAM_DEVICE_BAM=1: the reference CLI's header, reference table and records
    (test_zz_gpu_native_sam.run_and_compare_bam); the whole file the switch-off file's bytes, for the same -o path; the stderr line with as
    many records as the file holds (expect_device False: batches that fall back to the host path are not counted).  tool_opts: options of
    the tool alone (-b: its batch size), for the two runs that follow the comparison; their records are held against the reference's file
    too.  Returns the number of records."""
    import re
    import subprocess
    from tests.test_zz_gpu_native_sam import bam_parts, run_and_compare_bam
    n = run_and_compare_bam(tool, d, mode, index_dir, fqs, opts, env=tool_env(env, True))
    tag = mode + "_" + ("_".join(o.strip("-") or "eq" for o in opts) or "default")
    out = os.path.join(d, "new_%s.bam" % tag)                                # (the same output path every time: it is part of @PG)
    with open(out, "rb") as f:
        on = f.read()
    ref_parts = bam_parts(os.path.join(d, "ref_%s.bam" % tag))
    logs = []
    for switch in (True, False):
        r = subprocess.run([tool, mode, index_dir] + fqs + ["-o", out] + opts + list(tool_opts), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, stdin=subprocess.DEVNULL,
                           timeout=3000, env=tool_env(env, switch))
        assert r.returncode == 0, "snapgpu-sam failed:\n%s" % r.stdout.decode(errors="replace")[-3000:]
        logs.append(r.stdout.decode(errors="replace"))
        with open(out, "rb") as f:
            now = f.read()
        if switch:
            on = now
            assert bam_parts(out) == ref_parts
        assert now == on, "the switch-off file is not the switch-on file"
    m = re.search(r"BAM records from the device: (\d+) batches, (\d+) records", logs[0])
    assert "BAM records from the device" not in logs[1]
    if expect_device:
        assert m and int(m.group(2)) == n and int(m.group(1)) >= 1, logs[0][-500:]
    else:
        assert m is None or int(m.group(2)) < n
    return n
