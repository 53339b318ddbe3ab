"""Shared by the paired-end SAM-line tests (snapgpu_sam_text_paired*, snapgpu_align_sam_paired_text): a plain-Python restatement of the
two lines a pair's result gets in a SAM file (SAMFormat::writePairs, SAM.cpp:1575-1895, its snprintf at :1854-1875; QS :1826-1834; the
"/1" "/2" rule of ReadWriter.cpp:405-420 and the print order of :453-461), the handcrafted pair units that cover the layout's edges, and
the checks the emulator's and the device's test files both run.  The restatement knows nothing of the library."""
import os

import numpy as np

from tests import util
from tests.samtext_util import OPS_STRIDE, RC, TAGS, contig_names_of, lines_of, pack

SYMBOLS = ("snapgpu_sam_text_paired", "snapgpu_sam_text_paired_device", "snapgpu_align_sam_paired_text")
FIELDS = ("flag", "contig", "pos", "mapq", "ops", "n_ops", "nm", "rnext", "pnext", "tlen")          # per mate of a unit: [2 * n_units]
READS = ("bases", "quals", "offsets", "names", "name_off")


def strip_suffixes(n0, n1):
    """Both names lose two bytes when they have the same length L > 2, '/' at L - 2 and last bytes that are '1' and '2' either way round."""
    L = len(n0)
    if L == len(n1) and L > 2 and n0[L - 2] == 0x2F and n1[L - 2] == 0x2F and n0[L - 1] in b"12" and n1[L - 1] in b"12" and n0[L - 1] != n1[L - 1]:
        return n0[:L - 2], n1[:L - 2]
    return n0, n1


def qs_of(qual):
    """QS:i of the line of the OTHER mate: the sum of b - 33 over the bytes (unsigned) with b - 33 >= 15."""
    return sum(b - 33 for b in qual if b - 33 >= 15)


def pair_line(name, flag, rname, pos, mapq, ops, n_ops, rnext, pnext, tlen, seq, qual, nm, mate_qual):
    """One mate's line; name already without its suffix; rname / rnext bytes (rnext b"=" / b"*" / a contig's name), rname None for contig -1."""
    cigar = b"*" if n_ops < 0 else b"".join(b"%d%c" % (int(op) >> 4, b"MIDNSHP=X"[int(op) & 15]) for op in ops[:n_ops])
    if flag & 0x10:
        seq, qual = seq.translate(RC)[::-1], qual[::-1]
    tlen32 = (int(tlen) + 2 ** 31) % 2 ** 32 - 2 ** 31                                       # the 64-bit value cast to int32
    fields = [name.split(b" ", 1)[0], b"%d" % flag, b"*" if rname is None else rname, b"%d" % pos, b"%d" % mapq, cigar, rnext, b"%d" % pnext, b"%d" % tlen32,
              seq, qual, b"PG:Z:SNAP", b"NM:i:%d" % nm] + TAGS + [b"QS:i:%d" % qs_of(mate_qual)]
    return b"\t".join(fields) + b"\n"


def expected_lines(contig_names, bases, quals, offsets, names, name_off, unit_pair, f, first_written):
    """The 2 * n_units lines of a call: f maps each of FIELDS to its array."""
    out = []
    for u in range(len(first_written)):
        k = u if unit_pair is None else int(unit_pair[u])
        nm = [names[int(name_off[2 * k + v]):int(name_off[2 * k + v + 1])].tobytes() for v in (0, 1)]
        nm = strip_suffixes(*nm)
        sq = [(bases[int(offsets[2 * k + v]):int(offsets[2 * k + v + 1])].tobytes(), quals[int(offsets[2 * k + v]):int(offsets[2 * k + v + 1])].tobytes()) for v in (0, 1)]
        fw = int(first_written[u])
        for v in (fw, 1 - fw):
            i = 2 * u + v
            rn = int(f["rnext"][i])
            out.append(pair_line(nm[v], int(f["flag"][i]), None if f["contig"][i] < 0 else contig_names[int(f["contig"][i])], int(f["pos"][i]), int(f["mapq"][i]),
                                 f["ops"][i], int(f["n_ops"][i]), b"=" if rn == -2 else b"*" if rn == -1 else contig_names[rn], int(f["pnext"][i]), int(f["tlen"][i]),
                                 sq[v][0], sq[v][1], int(f["nm"][i]), sq[1 - v][1]))
    return out


QUAL_KINDS = 6
NAME_PAIRS = [(b"a/1", b"a/2"), (b"a/2", b"a/1"), (b"a/1", b"a/1"), (b"a/1", b"ab/2"), (b"/1", b"/2"), (b"a/3", b"a/1"), (b"x y/1", b"x y/2"), (b"x/1 c", b"x/2 c"),
              (b"n" * 253 + b"/1", b"n" * 253 + b"/2"), (b"m" * 255, b"m" * 255), (b"plainname", b"plainname"), (b"left right", b"left other"), (b"r/1", b"r/1x")]


def make_quals(kind, U, rng):
    if kind == 0: return b"/" * U                                                           # 14: QS 0
    if kind == 1: return b"0" * U                                                           # 15: counted
    if kind == 2: return bytes(b"/0"[int(x)] for x in rng.integers(0, 2, size=U))
    if kind == 3: return b"~" * U
    if kind == 4: return bytes([128, 255, 47, 48, 200][j % 5] for j in range(U))             # bytes that a signed reading would drop
    return rng.integers(33, 127, size=U).astype(np.uint8).tobytes()


def handcrafted(n_contigs, seed=3):
    """60 pairs and 150 pair units over them (a permutation of the pairs first, so every pair has a unit, then repeats) that cover every edge of
    the layout.  Returns dict(READS..., unit_pair, FIELDS..., first_written): the first items of every list meet in unit 0, the last ones in
    the last unit."""
    rng = np.random.default_rng(seed)
    Us = [1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 400]
    n_pairs = 60
    alphabet = np.frombuffer(b"ACGTNacgtnRY.*", np.uint8)
    reads, quals, names = [], [], []
    for i in range(n_pairs):
        for v in (0, 1):
            U = Us[(i + 4 * v * (1 + i // 11)) % len(Us)]                                   # mixed within a pair: QS comes from a mate of another length
            reads.append(rng.choice(alphabet, size=U).tobytes())
            quals.append(make_quals((2 * i + v + i // 3) % QUAL_KINDS, U, rng))
            names.append(NAME_PAIRS[i % len(NAME_PAIRS)][v] if i < 2 * len(NAME_PAIRS) else b"pair%d/%d some comment" % (i, v + 1))
    b, off = pack(reads); q, _ = pack(quals); nb, noff = pack(names)
    starts = {(k, a) for k in range(QUAL_KINDS) for a in range(4)}
    seen = {((2 * (m // 2) + m % 2 + (m // 2) // 3) % QUAL_KINDS, int(off[m]) % 4) for m in range(2 * n_pairs)}
    assert starts <= seen, "a kind of quality string does not start at every byte alignment: %r" % sorted(starts - seen)
    unit_pair = [0] + [int(x) for x in rng.permutation(n_pairs) if x != 0] + [7, 7, 7, 8, 8] + [int(x) for x in rng.integers(0, n_pairs, size=84)] + [n_pairs - 1]
    n_units = len(unit_pair); n = 2 * n_units
    flags = [0x41, 0x85, 0x51, 0xA1, 0x63, 0x93, 0x4D, 0x89, 0x871]
    poss = [0, 9, 10, 99_999_999, 2 ** 31, 4_294_967_294]
    mapqs = [0, 9, 10, 70, 255]
    nms = [-1, 0, 9, 10, 123]
    nopss = [-1, 0, 1, OPS_STRIDE]
    oplens = [1, 9, 10, 99, 100, 1000]
    contigs = [-1, 0, n_contigs - 1] + list(range(1, n_contigs - 1))
    rnexts = [-2, -1, 0, n_contigs - 1]
    pnexts = [0, 9, 10, 2 ** 31, 4_294_967_294]
    tlens = [0, -1, 9, -10, 2 ** 31 - 1, -2 ** 31, 2 ** 31 + 5]
    def cyc(vals, dtype): return np.array([vals[r % len(vals)] for r in range(n)], dtype)
    f = dict(flag=cyc(flags, np.int32), contig=cyc(contigs, np.int32), pos=cyc(poss, np.int64), mapq=cyc(mapqs, np.int32), nm=cyc(nms, np.int32),
             n_ops=cyc(nopss, np.int32), rnext=cyc(rnexts, np.int32), pnext=cyc(pnexts, np.int64), tlen=cyc(tlens, np.int64))
    f["flag"][1::4] ^= 0x10                                                                  # both orientations against every list
    ops = np.zeros((n, OPS_STRIDE), np.uint32)
    for r in range(n):
        for j in range(OPS_STRIDE):
            ops[r, j] = (oplens[(r + j) % len(oplens)] << 4) | ((r + j) % 9)
    f["ops"] = ops
    first_written = np.array([(u // 2 + u // 7) % 2 for u in range(n_units)], np.int32)
    first_written[0], first_written[-1] = 0, 1
    for k, vals in (("flag", flags), ("contig", [-1, n_contigs - 1]), ("pos", poss), ("mapq", mapqs), ("nm", nms), ("n_ops", nopss), ("rnext", rnexts),
                    ("pnext", pnexts), ("tlen", tlens)):
        f[k][0] = f[k][1] = vals[0]; f[k][-1] = f[k][-2] = vals[-1]
    h = dict(bases=b, quals=q, offsets=off, names=nb, name_off=noff, unit_pair=np.array(unit_pair, np.uint32), first_written=first_written)
    h.update(f)
    assert sorted(unit_pair[:n_pairs]) == list(range(n_pairs))
    return h


def make_aligner(index, names=None, **kw):
    from snap_amd import abi
    from snap_amd.aligner import ChimericPairedEndAligner
    a = ChimericPairedEndAligner(index, abi.default_params(max_read_len=400, **kw), abi.default_paired_params())
    if names is not None:
        a.setContigNames(names)
    return a


def run_text(a, h, units=None, unit_pair=True, **kw):
    """samTextPaired over the units `units` (a slice; None: all) of a handcrafted set, with the pairs as they are."""
    sel = slice(None) if units is None else units
    rows = np.arange(h["first_written"].size)[sel]
    rec = np.stack([2 * rows, 2 * rows + 1], axis=1).reshape(-1)
    return a.samTextPaired(*[h[k] for k in READS], *[h[k][rec] for k in FIELDS], h["first_written"][sel], unit_pair=h["unit_pair"][sel] if unit_pair else None, **kw)


def expected_of(cn, h, units=None):
    sel = slice(None) if units is None else units
    rows = np.arange(h["first_written"].size)[sel]
    rec = np.stack([2 * rows, 2 * rows + 1], axis=1).reshape(-1)
    return expected_lines(cn, *[h[k] for k in READS], h["unit_pair"][sel], {k: h[k][rec] for k in FIELDS}, h["first_written"][sel])


def first_difference(got, exp):
    bad = [i for i, (x, y) in enumerate(zip(got, exp)) if x != y]
    return "line %d:\n%r\n%r" % (bad[0], got[bad[0]], exp[bad[0]]) if bad else ("%d lines, %d expected" % (len(got), len(exp)) if len(got) != len(exp) else None)


def check_handcrafted(index):
    """Every handcrafted unit through samTextPaired, all in one call, the first and the last on their own, then unit_pair = NULL."""
    cn = contig_names_of(index, long_last=True)
    h = handcrafted(len(cn))
    exp = expected_of(cn, h)
    a = make_aligner(index, cn)
    try:
        got = run_text(a, h)
        assert not got["truncated"] and got["text_bytes"] == sum(map(len, exp))
        assert first_difference(lines_of(got), exp) is None, first_difference(lines_of(got), exp)
        n_units = h["first_written"].size
        for u in (0, n_units - 1):
            one = run_text(a, h, units=slice(u, u + 1))
            assert lines_of(one) == exp[2 * u:2 * u + 2], u
        # unit_pair = NULL: unit k is pair k -- the unit of the leading permutation that names pair k, in the pairs' order
        n_pairs = (h["offsets"].size - 1) // 2
        order = np.argsort(h["unit_pair"][:n_pairs], kind="stable")
        rec = np.stack([2 * order, 2 * order + 1], axis=1).reshape(-1)
        sub = {k: h[k][rec] for k in FIELDS}
        plain = a.samTextPaired(*[h[k] for k in READS], *[sub[k] for k in FIELDS], h["first_written"][order])
        exp_plain = expected_lines(cn, *[h[k] for k in READS], None, sub, h["first_written"][order])
        assert first_difference(lines_of(plain), exp_plain) is None, first_difference(lines_of(plain), exp_plain)
    finally:
        a.close()
    return h, exp, cn


def check_memory_discipline(index):
    """As samtext_util.check_memory_discipline: a text buffer pre-filled with 0xCD; an exact fit, a capacity one byte short, none at all, no units."""
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
        none = run_text(a, h, units=slice(0, 0), text=np.full(16, 0xCD, np.uint8))
        assert none["text_bytes"] == 0 and none["line_begin"].size == 1 and int(none["line_begin"][0]) == 0 and (none["text"] == 0xCD).all()
    finally:
        a.close()


def scan_unit_counts():
    """n_units with 2 * n_units lines one below, at and one above the tile of each level of the scan (64, 1024), as far as parity allows."""
    return (31, 32, 33, 511, 512, 513)


def check_scan_levels(index):
    """1-base mates: line_begin is the running sum of the restatement's line lengths, and the text is the lines."""
    cn = contig_names_of(index)
    a = make_aligner(index, cn)
    rng = np.random.default_rng(5)
    try:
        for nu in scan_unit_counts():
            n = 2 * nu
            bases = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=n); quals = rng.integers(33, 127, size=n).astype(np.uint8)
            offsets = np.arange(n + 1, dtype=np.uint64)
            nb, noff = pack([b"r%d/%d" % (i // 2, 1 + i % 2) for i in range(n)])
            f = dict(flag=(rng.integers(0, 2, size=n) * 16 + 1).astype(np.int32), contig=rng.integers(-1, len(cn), size=n).astype(np.int32),
                     pos=rng.integers(0, 10 ** rng.integers(1, 10, size=n)).astype(np.int64), mapq=rng.integers(0, 71, size=n).astype(np.int32),
                     n_ops=rng.integers(-1, 3, size=n).astype(np.int32), nm=rng.integers(-1, 30, size=n).astype(np.int32),
                     ops=((rng.integers(1, 2000, size=(n, 2)) << 4) | rng.integers(0, 9, size=(n, 2))).astype(np.uint32),
                     rnext=rng.integers(-2, len(cn), size=n).astype(np.int32), pnext=rng.integers(0, 10 ** rng.integers(1, 10, size=n)).astype(np.int64),
                     tlen=rng.integers(-10 ** 6, 10 ** 6, size=n).astype(np.int64))
            fw = rng.integers(0, 2, size=nu).astype(np.int32)
            got = a.samTextPaired(bases, quals, offsets, nb, noff, *[f[k] for k in FIELDS], fw)
            exp = expected_lines(cn, bases, quals, offsets, nb, noff, None, f, fw)
            assert got["line_begin"].dtype == np.uint64 and got["line_begin"].size == n + 1
            assert (got["line_begin"].astype(np.int64) == np.concatenate([[0], np.cumsum([len(x) for x in exp])])).all(), nu
            assert got["text"][:got["text_bytes"]].tobytes() == b"".join(exp), nu
    finally:
        a.close()


def check_argument_errors(index):
    """SNAPGPU_E_INVALID, and not a byte behind the text buffer: no contig names, first_written = 2, rnext = n_contigs, unit_pair out of range
    (host form), n_ops > ops_stride."""
    import pytest
    from snap_amd.aligner import SnapGpuError
    cn = contig_names_of(index, long_last=True)
    h = handcrafted(len(cn))
    n_pairs = (h["offsets"].size - 1) // 2
    a = make_aligner(index)
    try:
        with pytest.raises(SnapGpuError, match=r"failed \(-1\).*snapgpu_set_contig_names"):
            run_text(a, h)
        a.setContigNames(cn)
        good = run_text(a, h)
        tb = good["text_bytes"]
        for key, at, value in (("first_written", 5, 2), ("first_written", 6, -1), ("rnext", 11, len(cn)), ("rnext", 12, -3), ("unit_pair", 9, n_pairs),
                               ("n_ops", 13, OPS_STRIDE + 1)):
            bad = dict(h); bad[key] = h[key].copy(); bad[key][at] = value
            buf = np.full(tb + 64, 0xCD, np.uint8)
            with pytest.raises(SnapGpuError, match=r"failed \(-1\)"):
                run_text(a, bad, text=buf[:tb], grow=False)
            assert (buf[tb:] == 0xCD).all(), key
            if key == "unit_pair":
                assert (buf == 0xCD).all()                                   # refused on the host: nothing ran
        with pytest.raises(SnapGpuError, match=r"failed \(-1\).*n_units == n_pairs"):       # unit_pair NULL with more units than pairs
            run_text(a, h, unit_pair=False)
        assert lines_of(run_text(a, h)) == lines_of(good)                    # the context is as good as before
    finally:
        a.close()


FIXTURE_TAGS = ("default", "lvonly", "eqx")


def check_reference_fields(index, tag):
    """The reference CLI's own fields of option set `tag` (tests/golden/sam_fields_paired.npz) through samTextPaired, names p<i>/1 / p<i>/2: every
    line equals the restatement applied to the same fields."""
    z = np.load(os.path.join(util.GOLDEN, "sam_fields_paired.npz"))
    n_pairs = len(z[tag + "_first_written"]); n = 2 * n_pairs
    offs = z["offsets"][:n + 1].astype(np.uint64); tot = int(offs[-1])
    bases, quals = z["bases"][:tot], z["quals"][:tot]
    nb, noff = pack([b"p%d/%d" % (i // 2, 1 + i % 2) for i in range(n)])
    f = {k: z[tag + "_" + k][:n] for k in FIELDS}
    fw = z[tag + "_first_written"][:n_pairs]
    cn = contig_names_of(index)
    a = make_aligner(index, cn)
    try:
        got = a.samTextPaired(bases, quals, offs, nb, noff, *[f[k] for k in FIELDS], fw)
    finally:
        a.close()
    exp = expected_lines(cn, bases, quals, offs, nb, noff, None, f, fw)
    assert not got["truncated"] and got["text_bytes"] == sum(map(len, exp))
    assert first_difference(lines_of(got), exp) is None, (tag, first_difference(lines_of(got), exp))
    return len(exp)


def check_fused_equals_two_calls(index, n_pairs=150):
    """alignSamTextPaired == alignSamPaired followed by samTextPaired, byte for byte; a text capacity one byte short; a cigar row that is too short."""
    import pytest
    from snap_amd import abi
    from snap_amd.aligner import ChimericPairedEndAligner, SnapGpuError
    zp = np.load(os.path.join(util.GOLDEN, "paired_reads.npz"))
    o = zp["o150"][:2 * n_pairs + 1].astype(np.uint64)
    bases, quals = zp["b150"][:int(o[-1])], zp["q150"][:int(o[-1])]
    n = 2 * n_pairs
    fc = np.zeros(n, np.int32); dl = np.diff(o.astype(np.int64)).astype(np.int32); skip = np.zeros(n_pairs, np.uint8)
    skip[3] = 1                                                              # one pair that is not given to the aligner: two unmapped lines
    nb, noff = pack([b"p%d/%d x" % (i // 2, 1 + i % 2) if i % 8 else b"p%d/%d" % (i // 2, 1 + i % 2) for i in range(n)])
    cn = contig_names_of(index)
    a = ChimericPairedEndAligner(index, abi.default_params(max_k=8, max_read_len=160), abi.default_paired_params())
    try:
        a.setContigNames(cn)
        _, _, f = a.alignSamPaired(bases, quals, o, fc, dl, skip, want_results=False)
        two = a.samTextPaired(bases, quals, o, nb, noff, *[f[k] for k in FIELDS], f["first_written"])
        one = a.alignSamTextPaired(bases, quals, o, fc, dl, skip, nb, noff)
        assert int((f["flag"] & 4 == 0).sum()) > n_pairs                    # (the batch aligns)
        assert not one["truncated"] and one["text_bytes"] == two["text_bytes"] and (one["line_begin"] == two["line_begin"]).all()
        assert one["text"][:one["text_bytes"]].tobytes() == two["text"][:two["text_bytes"]].tobytes()
        assert (one["flag"] == f["flag"]).all() and (one["first_written"] == f["first_written"]).all()
        assert first_difference(lines_of(two), expected_lines(cn, bases, quals, o, nb, noff, None, f, f["first_written"])) is None
        tight = a.alignSamTextPaired(bases, quals, o, fc, dl, skip, nb, noff, text_capacity=two["text_bytes"] - 1, grow=False)
        assert tight["truncated"] and tight["text_bytes"] == two["text_bytes"] and (tight["line_begin"] == two["line_begin"]).all()
        assert lines_of(tight, n - 1) == lines_of(two)[:-1] and (tight["flag"] == f["flag"]).all()
        with pytest.raises(SnapGpuError, match=r"failed \(-1\).*ops_stride"):                  # a cigar that does not fit its row is refused, not printed wrong
            a.alignSamTextPaired(bases, quals, o, fc, dl, skip, nb, noff, ops_stride=3)
    finally:
        a.close()
    return f, two


def check_device_form(index, hb):
    """samTextPaired_device == samTextPaired at full and at half capacity, with and without unit_pair; no units."""
    cn = contig_names_of(index, long_last=True)
    h = handcrafted(len(cn))
    a = make_aligner(index, cn)
    try:
        host = run_text(a, h)
        tb = host["text_bytes"]
        d = {k: hb.upload(h[k]) for k in READS + ("unit_pair", "first_written") + FIELDS}
        nu = h["first_written"].size; n = 2 * nu
        for cap in (tb, tb // 2):
            text0 = np.full(tb + 16, 0xCD, np.uint8); lb0 = np.zeros(n + 1, np.uint64)
            d_text, d_lb = hb.upload(text0), hb.upload(lb0)
            got_tb, truncated = a.samTextPaired_device(nu, d["bases"], d["quals"], d["offsets"], d["names"], d["name_off"], d["unit_pair"], d["flag"], d["contig"],
                                                       d["pos"], d["mapq"], d["ops"], OPS_STRIDE, d["n_ops"], d["nm"], d["rnext"], d["pnext"], d["tlen"],
                                                       d["first_written"], cap, d_text, d_lb)
            assert got_tb == tb and truncated == (cap < tb)
            lb = hb.download(d_lb, lb0); text = hb.download(d_text, text0)
            assert (lb == host["line_begin"]).all()
            fit = int(np.searchsorted(lb[1:].astype(np.int64), cap, side="right"))
            assert text[:int(lb[fit])].tobytes() == host["text"][:int(lb[fit])].tobytes() and (text[int(lb[fit]):] == 0xCD).all(), cap
        d0 = hb.upload(np.full(1, 7, np.uint64))
        assert a.samTextPaired_device(0, *([0] * 11), OPS_STRIDE, *([0] * 6), 0, 0, d0) == (0, False)
        assert int(hb.download(d0, np.zeros(1, np.uint64))[0]) == 0
    finally:
        a.close()
        hb.free_all()
