"""Shared by the SAM-line tests (snapgpu_sam_text_single*, snapgpu_align_sam_single_text): a plain-Python restatement of the line a
single-end record gets in a SAM file (SAMFormat::createSAMLine / writeRead, SAM.cpp:1424-1572, 1898-2352: the name cut at its first
space, :2001-2004; the reverse complement of COMPLEMENT[], Tables.cpp), the handcrafted records that cover the layout's edges, and the
checks the emulator's and the device's test files both run.  The restatement knows nothing of the library."""
import numpy as np

from tests import samrec_util as su

RC = bytes(b"TGCA"[b"ACGT".index(c)] if c in b"ACGT" else ord("N") for c in range(256))
TAGS = [b"RG:Z:FASTQ", b"PL:Z:Illumina", b"PU:Z:pu", b"LB:Z:lb", b"SM:Z:sm"]
W_TEXT_TRUNCATED = 3
OPS_STRIDE = 7


def sam_line(name, flag, rname, pos, mapq, ops, n_ops, seq, qual, nm):
    """One record's line; name / rname / seq / qual are bytes, ops the record's row of BAM cigar operations, rname None for contig -1."""
    cigar = b"*" if n_ops < 0 else b"".join(b"%d%c" % (int(op) >> 4, b"MIDNSHP=X"[int(op) & 15]) for op in ops[:n_ops])
    if flag & 0x10:
        seq, qual = seq.translate(RC)[::-1], qual[::-1]
    fields = [name.split(b" ", 1)[0], b"%d" % flag, b"*" if rname is None else rname, b"%d" % pos, b"%d" % mapq, cigar, b"*", b"0", b"0",
              seq, qual, b"PG:Z:SNAP", b"NM:i:%d" % nm] + TAGS
    return b"\t".join(fields) + b"\n"


def expected_lines(contig_names, bases, quals, offsets, names, name_off, rec_read, flag, contig, pos, mapq, ops, n_ops, nm):
    out = []
    for r in range(len(flag)):
        rd = r if rec_read is None else int(rec_read[r])
        b, e = int(offsets[rd]), int(offsets[rd + 1])
        out.append(sam_line(names[int(name_off[rd]):int(name_off[rd + 1])].tobytes(), int(flag[r]), None if contig[r] < 0 else contig_names[int(contig[r])],
                            int(pos[r]), int(mapq[r]), ops[r], int(n_ops[r]), bases[b:e].tobytes(), quals[b:e].tobytes(), int(nm[r])))
    return out


def contig_names_of(index, long_last=False):
    """The index's contig names as bytes; long_last: a 1-character and a 60-character name in place of the first and the last."""
    names = [c.name.encode() for c in index.contigs]
    if long_last:
        names[0] = b"c"
        names[-1] = b"L" * 60
    return names


def pack(items):
    off = np.zeros(len(items) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in items])
    return np.frombuffer(b"".join(items) + b"\0", np.uint8)[:int(off[-1])].copy(), off


def handcrafted(n_contigs, seed=3):
    """About 200 records over 40 reads that cover every edge of the layout.  Returns dict(bases, quals, offsets, names, name_off, rec_read, flag, contig, pos,
    mapq, ops, n_ops, nm): the first items of every list meet in record 0, the last ones in the last record, and in between every value
    of every list turns up with both orientations of every read length."""
    rng = np.random.default_rng(seed)
    Us = [1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 400]
    flags = [0, 4, 16, 256, 272, 2064]
    poss = [0, 9, 10, 99_999_999, 2 ** 31, 4_294_967_294]
    mapqs = [0, 9, 10, 70, 255]
    nms = [-1, 0, 9, 10, 123]
    nopss = [-1, 0, 1, OPS_STRIDE]
    oplens = [1, 9, 10, 99, 100, 1000]
    contigs = [-1, 0, n_contigs - 1] + list(range(1, n_contigs - 1))
    name_kinds = [b"plainname", b"left right", b" spacefirst", b"x", b"n" * 255]
    alphabet = np.frombuffer(b"ACGTNacgtnRY.*", np.uint8)
    reads, quals, names = [], [], []
    for i in range(40):
        U = Us[i % len(Us)] if i < 33 else int(rng.integers(1, 300))
        reads.append(rng.choice(alphabet, size=U).tobytes())
        quals.append(rng.integers(33, 127, size=U).astype(np.uint8).tobytes())
        names.append(name_kinds[i % len(name_kinds)] if i < 35 else b"read%d some comment" % i)
    names[10] = name_kinds[-1]                                        # (read 10, the longest, is the last record's)
    # a read per record: every length with both orientations first, then repeats (several records on one read) and random ones
    rec_read = [i for i in range(11) for _ in (0, 1)] + [11, 11, 11, 12, 12] + [int(x) for x in rng.integers(0, 40, size=173)]
    rec_read[-1] = 10                                                 # the last record: the last item of every list
    n = len(rec_read)
    flag = np.array([flags[(r // 2) % len(flags)] ^ (0x10 if r % 2 else 0) if r < 22 else flags[int(rng.integers(len(flags)))] for r in range(n)], np.int32)
    def cyc(vals, dtype, stride): return np.array([vals[(r // stride) % len(vals)] for r in range(n)], dtype)
    contig = cyc(contigs, np.int32, 1); pos = cyc(poss, np.int64, 1); mapq = cyc(mapqs, np.int32, 1); nm = cyc(nms, np.int32, 1)
    n_ops = cyc(nopss, np.int32, 1)
    ops = np.zeros((n, OPS_STRIDE), np.uint32)
    for r in range(n):
        for j in range(OPS_STRIDE):
            ops[r, j] = (oplens[(r + j) % len(oplens)] << 4) | ((r + j) % 9)
    flag[0], contig[0], pos[0], mapq[0], nm[0], n_ops[0] = flags[0], contigs[0], poss[0], mapqs[0], nms[0], nopss[0]
    flag[-1], contig[-1], pos[-1], mapq[-1], nm[-1], n_ops[-1] = flags[-1], n_contigs - 1, poss[-1], mapqs[-1], nms[-1], nopss[-1]
    ops[-1, :] = [(oplens[-1] << 4) | 8] + [(oplens[j % len(oplens)] << 4) | j for j in range(1, OPS_STRIDE)]
    b, off = pack(reads); q, _ = pack(quals); nb, noff = pack(names)
    return dict(bases=b, quals=q, offsets=off, names=nb, name_off=noff, rec_read=np.array(rec_read, np.uint32), flag=flag, contig=contig, pos=pos, mapq=mapq,
                ops=ops, n_ops=n_ops, nm=nm)


FIELDS = ("flag", "contig", "pos", "mapq", "ops", "n_ops", "nm")


def run_text(a, h, rec=None, **kw):
    """samText over the records `rec` (indices; None: all) of a handcrafted set, with their reads as they are."""
    sel = slice(None) if rec is None else rec
    return a.samText(h["bases"], h["quals"], h["offsets"], h["names"], h["name_off"], *[h[f][sel] for f in FIELDS], rec_read=h["rec_read"][sel], **kw)


def lines_of(got, n=None):
    lb = got["line_begin"].astype(np.int64)
    n = lb.size - 1 if n is None else n
    return [got["text"][lb[i]:lb[i + 1]].tobytes() for i in range(n)]


def make_aligner(index, names=None, **kw):
    from snap_amd import abi
    from snap_amd.aligner import BaseAligner
    a = BaseAligner(index, abi.default_params(max_read_len=400, **kw))
    if names is not None:
        a.setContigNames(names)
    return a


def check_handcrafted(index):
    """Every handcrafted record through samText, all in one call and the first and the last on their own: the restatement's bytes."""
    cn = contig_names_of(index, long_last=True)
    h = handcrafted(len(cn))
    exp = expected_lines(cn, *[h[k] for k in ("bases", "quals", "offsets", "names", "name_off", "rec_read") + FIELDS])
    a = make_aligner(index, cn)
    try:
        got = run_text(a, h)
        assert not got["truncated"] and got["text_bytes"] == sum(map(len, exp))
        bad = [i for i, (x, y) in enumerate(zip(lines_of(got), exp)) if x != y]
        assert not bad, "record %d:\n%r\n%r" % (bad[0], lines_of(got)[bad[0]], exp[bad[0]])
        for r in (0, len(exp) - 1):
            one = run_text(a, h, rec=slice(r, r + 1))
            assert lines_of(one) == [exp[r]], r
        # rec_read = NULL: record i is read i
        n = h["offsets"].size - 1
        first = [int(np.flatnonzero(h["rec_read"] == i)[0]) if (h["rec_read"] == i).any() else 0 for i in range(n)]
        sub = {f: h[f][first] for f in FIELDS}
        plain = a.samText(h["bases"], h["quals"], h["offsets"], h["names"], h["name_off"], *[sub[f] for f in FIELDS])
        assert lines_of(plain) == expected_lines(cn, h["bases"], h["quals"], h["offsets"], h["names"], h["name_off"], None, *[sub[f] for f in FIELDS])
    finally:
        a.close()
    return h, exp, cn


def check_memory_discipline(index):
    """A text buffer pre-filled with 0xCD: an exact fit leaves every byte behind the text alone; a capacity one byte short, and none at
    all, warn, report the full size and the full line_begin, write the lines that fit as the full run did and nothing at or past the
    capacity; no records: line_begin[0] = 0."""
    cn = contig_names_of(index, long_last=True)
    h = handcrafted(len(cn))
    a = make_aligner(index, cn)
    try:
        full = run_text(a, h)
        tb = full["text_bytes"]
        ref_lines = lines_of(full)
        buf = np.full(tb + 64, 0xCD, np.uint8)
        exact = run_text(a, h, text=buf[:tb], grow=False)
        assert not exact["truncated"] and exact["text_bytes"] == tb and (buf[tb:] == 0xCD).all()
        assert buf[:tb].tobytes() == full["text"][:tb].tobytes()
        for cap in (tb - 1, 0):
            buf = np.full(tb + 64, 0xCD, np.uint8)
            short = run_text(a, h, text=buf[:cap], grow=False)
            assert short["truncated"] and short["text_bytes"] == tb and (short["line_begin"] == full["line_begin"]).all(), cap
            lb = full["line_begin"].astype(np.int64)
            fit = int(np.searchsorted(lb[1:], cap, side="right"))            # lines that end at or below the capacity
            assert fit == (len(ref_lines) - 1 if cap else 0)
            assert [buf[lb[i]:lb[i + 1]].tobytes() for i in range(fit)] == ref_lines[:fit]
            assert (buf[lb[fit]:] == 0xCD).all(), cap
        none = a.samText(h["bases"], h["quals"], h["offsets"], h["names"], h["name_off"], *[h[f][:0] for f in FIELDS], rec_read=h["rec_read"][:0],
                         text=np.full(16, 0xCD, np.uint8))
        assert none["text_bytes"] == 0 and int(none["line_begin"][0]) == 0 and (none["text"] == 0xCD).all()
    finally:
        a.close()


def scan_tile_sizes():
    """The tile of every level of the offsets' scan (sam_text.h: rounds of one wavefront inside tiles of SAMREC_CHUNK records; the tile
    sums themselves are scanned by one lane, which has no tile)."""
    return (64, 1024)


def check_scan_levels(index):
    """n_records one below, at and one above each tile size of the scan, 1-base reads: line_begin is the running sum of the restatement's
    line lengths, and the text is the lines."""
    cn = contig_names_of(index)
    a = make_aligner(index, cn)
    rng = np.random.default_rng(5)
    try:
        for tile in scan_tile_sizes():
            for n in (tile - 1, tile, tile + 1):
                bases = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=n); quals = rng.integers(33, 127, size=n).astype(np.uint8)
                offsets = np.arange(n + 1, dtype=np.uint64)
                nb, noff = pack([b"r%d" % i for i in range(n)])
                flag = (rng.integers(0, 2, size=n) * 16).astype(np.int32); contig = rng.integers(-1, len(cn), size=n).astype(np.int32)
                pos = rng.integers(0, 10 ** rng.integers(1, 10, size=n)).astype(np.int64); mapq = rng.integers(0, 71, size=n).astype(np.int32)
                n_ops = rng.integers(-1, 3, size=n).astype(np.int32); nm = rng.integers(-1, 30, size=n).astype(np.int32)
                ops = ((rng.integers(1, 2000, size=(n, 2)) << 4) | rng.integers(0, 9, size=(n, 2))).astype(np.uint32)
                got = a.samText(bases, quals, offsets, nb, noff, flag, contig, pos, mapq, ops, n_ops, nm)
                exp = expected_lines(cn, bases, quals, offsets, nb, noff, None, flag, contig, pos, mapq, ops, n_ops, nm)
                assert got["line_begin"].dtype == np.uint64
                assert (got["line_begin"].astype(np.int64) == np.concatenate([[0], np.cumsum([len(x) for x in exp])])).all(), n
                assert got["text"][:got["text_bytes"]].tobytes() == b"".join(exp), n
    finally:
        a.close()


def check_contig_names(index):
    """No names: the text calls fail with SNAPGPU_E_INVALID; a wrong count of names fails the same way; names given again replace the first."""
    import pytest
    from snap_amd.aligner import SnapGpuError
    cn = contig_names_of(index)
    h = handcrafted(len(cn))
    a = make_aligner(index)
    try:
        with pytest.raises(SnapGpuError, match=r"failed \(-1\).*snapgpu_set_contig_names"):
            run_text(a, h)
        for wrong in (cn[:-1], cn + [b"more"]):
            with pytest.raises(SnapGpuError, match=r"failed \(-1\)"):
                a.setContigNames(wrong)
        a.setContigNames([b"first%d" % i for i in range(len(cn))])
        a.setContigNames(cn)
        got = run_text(a, h, rec=slice(0, 30))
        assert lines_of(got) == expected_lines(cn, *[h[k] for k in ("bases", "quals", "offsets", "names", "name_off")], h["rec_read"][:30], *[h[f][:30] for f in FIELDS])
    finally:
        a.close()


def golden_names(n):
    """`r<i> x`: the cut at the space is exercised"""
    return pack([b"r%d x" % i for i in range(n)])


def check_against_reference(index, tag):
    """alignSamText over the golden reads of option set `tag`: the text equals the restatement applied to the reference CLI's fields.  The
    reads whose records the library flags reference_history_dependent are left out, as samrec_util.compare leaves them out; at most 1 %."""
    z = su.fixture()
    n = z["offsets"].size - 1
    cli, kw, sec, ae, use_m = su.SETS[tag]
    cn = contig_names_of(index)
    nb, noff = golden_names(n)
    exp_f = su.expected(z, tag)
    a = su.make_aligner(index, tag)
    try:
        a.setContigNames(cn)
        skip = su.skip_mask(z["bases"], z["offsets"], z["front_clip"], z["data_len"], int(a.params.max_k))
        rec = a.alignSamRecords(z["bases"], z["quals"], z["offsets"], z["front_clip"], z["data_len"], skip, use_m=bool(use_m), adjust_primary=bool(ae and sec is None))
        got = a.alignSamText(z["bases"], z["quals"], z["offsets"], z["front_clip"], z["data_len"], skip, nb, noff, use_m=bool(use_m),
                             adjust_primary=bool(ae and sec is None))
    finally:
        a.close()
    assert not got["truncated"] and not got["records_truncated"]
    assert got["n_records"] == exp_f["rec_read"].size == rec["n_records"] and (got["rec_begin"] == rec["rec_begin"]).all()
    exp = expected_lines(cn, z["bases"], z["quals"], z["offsets"], nb, noff, exp_f["rec_read"], exp_f["flag"], exp_f["contig"], exp_f["pos"], exp_f["mapq"],
                         exp_f["ops"], exp_f["n_ops"], exp_f["nm"])
    left_out = np.unique(rec["rec_read"][rec["stale"] != 0])
    assert left_out.size <= n // 100, "%d reads are reference_history_dependent" % left_out.size
    keep = ~np.isin(exp_f["rec_read"], left_out)
    lines = lines_of(got)
    bad = [r for r in np.flatnonzero(keep) if lines[r] != exp[r]]
    assert not bad, "%s: %d lines differ, record %d:\n%r\n%r" % (tag, len(bad), bad[0], lines[bad[0]], exp[bad[0]])
    assert (got["flag"] == rec["flag"]).all()
    return len(lines), int(left_out.size)


def check_fused_equals_two_calls(index, tag="ea_om1", n=150):
    """alignSamText == alignSamRecords followed by samText, byte for byte; and its two capacities: too few records, then too little text."""
    z = su.fixture()
    o = z["offsets"][:n + 1]
    bases, quals, fc, dl = z["bases"][:int(o[-1])], z["quals"][:int(o[-1])], z["front_clip"][:n], z["data_len"][:n]
    cli, kw, sec, ae, use_m = su.SETS[tag]
    cn = contig_names_of(index)
    nb, noff = golden_names(n)
    a = su.make_aligner(index, tag)
    try:
        a.setContigNames(cn)
        skip = su.skip_mask(bases, o, fc, dl, int(a.params.max_k))
        rec = a.alignSamRecords(bases, quals, o, fc, dl, skip, use_m=bool(use_m), adjust_primary=bool(ae and sec is None))
        two = a.samText(bases, quals, o, nb, noff, *[rec[f] for f in FIELDS], rec_read=rec["rec_read"])
        one = a.alignSamText(bases, quals, o, fc, dl, skip, nb, noff, use_m=bool(use_m), adjust_primary=bool(ae and sec is None))
        assert one["n_records"] == rec["n_records"] and one["text_bytes"] == two["text_bytes"]
        assert (one["line_begin"] == two["line_begin"]).all() and one["text"][:one["text_bytes"]].tobytes() == two["text"][:two["text_bytes"]].tobytes()
        few = a.alignSamText(bases, quals, o, fc, dl, skip, nb, noff, use_m=bool(use_m), adjust_primary=bool(ae and sec is None), capacity=n // 2, grow=False)
        assert few["records_truncated"] and few["n_records"] == rec["n_records"] and lines_of(few) == lines_of(two)[:n // 2]
        tight = a.alignSamText(bases, quals, o, fc, dl, skip, nb, noff, use_m=bool(use_m), adjust_primary=bool(ae and sec is None), capacity=rec["n_records"],
                               text_capacity=two["text_bytes"] - 1, grow=False)
        assert tight["truncated"] and tight["text_bytes"] == two["text_bytes"] and (tight["line_begin"] == two["line_begin"]).all()
        assert lines_of(tight, rec["n_records"] - 1) == lines_of(two)[:-1]
        import pytest
        from snap_amd.aligner import SnapGpuError
        with pytest.raises(SnapGpuError, match=r"failed \(-1\).*ops_stride"):                  # a cigar that does not fit its row is refused, not printed wrong
            a.alignSamText(bases, quals, o, fc, dl, skip, nb, noff, use_m=bool(use_m), adjust_primary=bool(ae and sec is None), ops_stride=3)
    finally:
        a.close()
    return rec, two


def check_device_form(index, hb):
    """samText_device == samText, with and without a record list, with a capacity that is too small, and with no records."""
    cn = contig_names_of(index, long_last=True)
    h = handcrafted(len(cn))
    a = make_aligner(index, cn)
    try:
        host = run_text(a, h)
        tb = host["text_bytes"]
        keys = ("bases", "quals", "offsets", "names", "name_off", "rec_read") + FIELDS
        d = {k: hb.upload(h[k]) for k in keys}
        n = h["flag"].size
        for cap in (tb, tb // 2):
            text0 = np.full(tb + 16, 0xCD, np.uint8); lb0 = np.zeros(n + 1, np.uint64)
            d_text, d_lb = hb.upload(text0), hb.upload(lb0)
            got_tb, truncated = a.samText_device(n, d["bases"], d["quals"], d["offsets"], d["names"], d["name_off"], d["rec_read"], d["flag"], d["contig"], d["pos"],
                                                 d["mapq"], d["ops"], OPS_STRIDE, d["n_ops"], d["nm"], cap, d_text, d_lb)
            assert got_tb == tb and truncated == (cap < tb)
            lb = hb.download(d_lb, lb0); text = hb.download(d_text, text0)
            assert (lb == host["line_begin"]).all()
            fit = int(np.searchsorted(lb[1:].astype(np.int64), cap, side="right"))
            assert text[:int(lb[fit])].tobytes() == host["text"][:int(lb[fit])].tobytes() and (text[int(lb[fit]):] == 0xCD).all(), cap
        d0 = hb.upload(np.full(1, 7, np.uint64))
        assert a.samText_device(0, *([0] * 11), OPS_STRIDE, 0, 0, 0, 0, d0) == (0, False)
        assert int(hb.download(d0, np.zeros(1, np.uint64))[0]) == 0
    finally:
        a.close()
        hb.free_all()
