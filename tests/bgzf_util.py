"""Checks of snapgpu_bgzf_compress / _device (snap_amd/csrc/bgzf.h), shared by tests/test_emu_bgzf.py (the wavefront emulator) and
tests/test_zz_gpu_bgzf.py (the GPU).  The yardstick is Python's zlib, gzip and struct, never the code under test: every member must carry
the BGZF header byte for byte, a BSIZE that agrees with member_begin, a raw DEFLATE payload that zlib consumes exactly up to the trailer,
and the CRC32 and ISIZE of its slice of the input; gzip.decompress of the whole output must return the input."""
import gzip
import hashlib
import os
import struct
import zlib

import numpy as np

from tests import deflate_util as du
from tests import util

SYMBOLS = ("snapgpu_bgzf_compress", "snapgpu_bgzf_compress_device", "snapgpu_align_sam_single_bgzf", "snapgpu_align_sam_paired_bgzf")
MAX_BLOCK = 0xff00
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
HEAD = bytes.fromhex("1f8b08040000000000ff060042430200")
GOLDEN = os.path.join(util.GOLDEN, "bam_records.npz")
# SHA-256 of the BGZF bytes of tests/golden/bam_records.npz["single_om1_omax4"] at block_input 0xff00, computed on the emulator: the GPU and
# the emulator run the same code, and the bytes depend on the input and block_input alone
SHA256_SINGLE_OM1_OMAX4 = "b51618296a5c0775646d075144aa7dea882d0c093099fd38980cb3974e89e416"
# device bytes / zlib level-1 bytes (raw deflate in members of 0xff00, what bgzf_append produces) on the ten fixture arrays: the worst measured
# ratio (DESIGN.md section 13 lists all ten) rounded up to the next 0.05
RATIO_CAP = 1.00                    # (measured: 0.934 .. 0.963)


def make_aligner(index):
    from snap_amd import abi
    from snap_amd.aligner import BaseAligner
    return BaseAligner(index, abi.default_params(max_k=8, max_read_len=160))


def as_bytes(x):
    return x if isinstance(x, (bytes, bytearray)) else np.ascontiguousarray(x, dtype=np.uint8).tobytes()


def check_output(data, block_input, bgzf, member_begin, n_members=None, bgzf_bytes=None, blocks=None):
    """every member of `bgzf` against zlib / gzip / struct; returns the members' sizes.  blocks: a list that receives every member's parsed
    block (check_coded_member)"""
    data = as_bytes(data); out = as_bytes(bgzf)
    mb = [int(x) for x in member_begin]
    nm = max(1, -(-len(data) // block_input))
    assert len(mb) == nm + 1 and mb[0] == 0, (len(mb), nm)
    if n_members is not None:
        assert n_members == nm
    if bgzf_bytes is not None:
        assert bgzf_bytes == mb[-1]
    sizes = []
    for m in range(nm):
        b, e = mb[m], mb[m + 1]
        src = data[m * block_input:(m + 1) * block_input]
        mem = out[b:e]
        assert e - b >= 28 and e - b <= len(src) + 31, (m, e - b, len(src))
        assert mem[:16] == HEAD, (m, mem[:18].hex())
        assert struct.unpack("<H", mem[16:18])[0] + 1 == e - b, m
        d = zlib.decompressobj(-15)
        got = d.decompress(mem[18:])                                        # (a wrong distance or an illegal code makes zlib raise)
        assert d.eof and got == src, m
        assert len(d.unused_data) == 8 and d.unused_data == mem[-8:], (m, len(d.unused_data))      # the payload ends exactly at the trailer
        crc, isize = struct.unpack("<II", mem[-8:])
        assert crc == zlib.crc32(src) and isize == len(src), m
        parsed = check_coded_member(src, mem)
        if blocks is not None:
            blocks.append(parsed)
        sizes.append(e - b)
    assert gzip.decompress(out[:mb[-1]]) == data
    return sizes


def check_coded_member(src, member):
    """what the DEFLATE payload of one member is made of, read by tests/deflate_util.py (the RFC, not zlib and not the code under test): one
    final block that replays to src and ends in the payload's last byte.  A stored block: LEN, NLEN and the bytes.  A dynamic block: matches
    of 4 .. 258 bytes within 32768, 258 as symbol 285 alone; the three codes complete, within 15 / 15 / 7 bits, coding exactly the used
    symbols and never giving a larger count a longer code (the exceptions are those bgzf.h names: one used distance symbol has one bit, no
    match at all sends one distance length of zero, a code-length code with one used symbol gets a second one-bit symbol); HLIT, HDIST and
    HCLEN minimal; the header's symbols those of a greedy run-length coder; and a payload below len + 5 bytes, what the stored block
    would take.  Returns the parsed block."""
    src = as_bytes(src); payload = as_bytes(member)[18:-8]
    blocks, out, end = du.read_stream(payload)
    assert len(blocks) == 1 and blocks[0].final == 1 and out == src
    assert (end + 7) // 8 == len(payload), (end, len(payload))
    b = blocks[0]
    if not src:
        assert payload == b"\x03\x00"
        return b
    if b.btype == 0:
        assert payload[0] == 1 and b.stored_len == len(src) and b.stored_nlen == len(src) ^ 0xffff and b.stored_at == 5
        assert payload[5:] == src and len(payload) == len(src) + 5
        return b
    assert b.btype == 2, b.btype
    for length, lsym, dist, dsym in b.matches():
        assert 4 <= length <= 258 and 1 <= dist <= 32768, (length, dist)
        assert (length == 258) == (lsym == 285), (length, lsym)
        assert du.LEN_BASE[lsym - 257] <= length and du.DIST_BASE[dsym] <= dist
    ll_counts = [0] * 286; d_counts = [0] * 30; cl_counts = [0] * 19
    ll_counts[256] = 1
    for t in b.tokens:
        if isinstance(t, int):
            ll_counts[t] += 1
        else:
            ll_counts[t[1]] += 1; d_counts[t[3]] += 1
    for s, _ in b.header_seq:
        cl_counts[s] += 1
    du.check_code_for_counts(ll_counts, b.ll_lengths, 15, "lit/len")
    if any(d_counts):
        du.check_code_for_counts(d_counts, b.d_lengths, 15, "distance", incomplete_single=True)
    else:
        assert b.d_lengths == [0], b.d_lengths
    du.check_code_for_counts(cl_counts, b.cl_lengths, 7, "code-length", filler_ok=True)
    assert du.kraft(b.cl_lengths, 7) == 128                                # (with the filler, complete in every case)
    assert b.hlit == 257 or b.ll_lengths[-1], b.hlit
    assert b.hdist == 1 or b.d_lengths[-1], b.hdist
    assert b.hclen == 4 or b.cl_lengths[du.CL_ORDER[b.hclen - 1]], b.hclen
    want = du.greedy_header_seq(b.ll_lengths + b.d_lengths)
    assert len(b.header_seq) == len(want), (len(b.header_seq), len(want))
    for i, (g, w) in enumerate(zip(b.header_seq, want)):
        assert g == w, (i, g, w)
    assert all(not (s == 16 and b.header_seq[i - 1][0] in (0, 17, 18)) for i, (s, _) in enumerate(b.header_seq) if i)
    assert len(payload) < len(src) + 5, (len(payload), len(src))
    return b


def compress(a, data, block_input=MAX_BLOCK, **kw):
    r = a.bgzfCompress(data, block_input, **kw)
    assert not r["truncated"]
    check_output(data, block_input, r["bgzf"][:r["bgzf_bytes"]], r["member_begin"], r["n_members"], r["bgzf_bytes"])
    return r["bgzf"][:r["bgzf_bytes"]].tobytes(), r


def rng_bytes(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def fibonacci_input(n_values, seed, times=1):
    """byte value v appears times * fib(v + 1) times, shuffled: an unrestricted Huffman code over these counts is n_values - 1 deep"""
    f = [1, 1]
    while len(f) < n_values:
        f.append(f[-1] + f[-2])
    x = np.concatenate([np.full(times * c, 65 + v, np.uint8) for v, c in enumerate(f[:n_values])])
    np.random.default_rng(seed).shuffle(x)                                # (24 values: 121 392 bytes, two members whose counts keep the proportions)
    return x.tobytes()


def btype(member):
    """BTYPE of a member's first DEFLATE block: 0 stored, 2 dynamic Huffman"""
    return (member[18] >> 1) & 3


def window_input(third_copy=True):
    """a 300-byte random string at 0, 33000 and 65000 of a member whose other bytes are all equal: the filler touches one entry of the hash table,
    so the candidate the second copy finds IS the first, 33000 back and beyond the 32768 window, and the third copy finds the second, 32000
    back.  third_copy False: other random bytes stand at 65000."""
    x = bytearray(b"a" * MAX_BLOCK)
    for at, seed in ((0, 12), (33000, 12), (65000, 12 if third_copy else 13)):
        x[at:at + 300] = rng_bytes(seed, 300)
    return bytes(x[:MAX_BLOCK])                                            # (the third copy is cut at the member's end: 280 bytes of it)


def small_cases():
    pat = b"ACGTTGCAAGGCTA" * 40
    return {
        "one_byte": b"x", "three_bytes": b"abc", "distinct_256": bytes(range(256)), "run_259": b"a" * 259, "run_600": b"a" * 600,
        "member_ends_in_pattern": pat[:517], "fib4": fibonacci_input(4, 5),
        "fib4_x300": fibonacci_input(4, 5, 300),                             # (long enough for the dynamic block to win)
    }


def check_empty_and_tiny(index):
    a = make_aligner(index)
    try:
        out, r = compress(a, b"")
        assert out == EOF_BLOCK and r["n_members"] == 1 and list(r["member_begin"]) == [0, 28]
        for name, data in small_cases().items():
            out, r = compress(a, data)
            if name in ("one_byte", "three_bytes", "distinct_256"):          # nothing to match: the stored block wins, len + 31
                assert len(out) <= len(data) + 31, name
            if name in ("run_259", "run_600"):
                assert len(out) < 100, (name, len(out))                      # matches were found
            if name in ("run_259", "run_600", "member_ends_in_pattern", "fib4_x300"):
                assert btype(out) == 2, name                                 # (these are here for LZ77 and the Huffman builder: a dynamic block)
        # a member that ends inside a repeated pattern: the second member starts in the middle of it as well
        data = (b"ACGTTGCAAGGCTA" * 40)
        out, r = compress(a, data, 257)
        assert r["n_members"] == 3
    finally:
        a.close()


def check_full_members(index, cases=("run", "exact", "plus_one", "random", "window", "fib24")):
    """members of 0xff00 bytes: equal bytes, the boundary and one byte beyond, incompressible data, the window limit, length limiting"""
    a = make_aligner(index)
    try:
        for c in cases:
            if c == "run":
                out, r = compress(a, b"\0" * MAX_BLOCK)
                assert len(out) < 1000
            elif c == "exact":
                out, r = compress(a, rng_bytes(3, MAX_BLOCK // 4) * 4)
                assert r["n_members"] == 1 and len(out) < MAX_BLOCK // 2
            elif c == "plus_one":
                data = rng_bytes(3, MAX_BLOCK // 4) * 4 + b"z"
                out, r = compress(a, data)
                assert r["n_members"] == 2 and int(r["member_begin"][2] - r["member_begin"][1]) == 1 + 31
            elif c == "random":
                data = rng_bytes(4, MAX_BLOCK)
                out, r = compress(a, data)
                assert len(out) == MAX_BLOCK + 31 and out[18] == 1 and out[23:23 + 64] == data[:64]      # one stored block
            elif c == "window":
                # a dynamic block, so distances are emitted and zlib raises on one beyond the window.  The first two copies cost 600 literals, the
                # 280 bytes of the third one match 32000 back (two tokens); other random bytes in their place cost 280 literals of about a byte each
                out, r = compress(a, window_input())
                other, _ = compress(a, window_input(third_copy=False))
                assert btype(out) == 2 and btype(other) == 2
                assert 600 <= len(out) < 1200, len(out)                          # (both early copies are literals: neither is matched at 33000)
                assert len(out) + 200 <= len(other), (len(out), len(other))
            elif c == "fib24":
                data = fibonacci_input(24, 6)
                out, r = compress(a, data)
                assert len(out) < len(data) // 2 and btype(out) == 2
    finally:
        a.close()


def check_many_members(index, shapes=((64, 300000), (1000, 70000))):
    a = make_aligner(index)
    try:
        for bi, n in shapes:
            data = (rng_bytes(20 + bi % 7, 997) * (n // 997 + 1))[:n]        # (repetitive, so that members of every kind occur)
            out, r = compress(a, data, bi)
            assert r["n_members"] == -(-n // bi)
    finally:
        a.close()


def fixture_arrays():
    z = np.load(GOLDEN)
    out = {k: z[k].tobytes() for k in z.files if (k.startswith("single_") or k.startswith("paired_")) and z[k].dtype == np.uint8 and z[k].size > 1000}
    assert len(out) == 10, sorted(out)
    return out


def zlib_members(data, block_input, level=1, strategy=zlib.Z_DEFAULT_STRATEGY):
    """the total size of the BGZF members bgzf_append makes with zlib: raw deflate per member, 26 bytes around each"""
    total = 0
    for at in range(0, max(len(data), 1), block_input):
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
        total += len(c.compress(data[at:at + block_input]) + c.flush()) + 26
    return total


def check_fixture(index, tag, block_inputs=(MAX_BLOCK, 4096), verbose=True):
    """a fixture array at both block sizes; the compressed-size conditions at 0xff00.  Returns the ratio to zlib level 1."""
    data = fixture_arrays()[tag]
    a = make_aligner(index)
    try:
        ratio = None
        for bi in block_inputs:
            out, r = compress(a, data, bi)
            if bi == MAX_BLOCK:
                l1, huff, fixed = zlib_members(data, bi), zlib_members(data, bi, 1, zlib.Z_HUFFMAN_ONLY), zlib_members(data, bi, 1, zlib.Z_FIXED)
                ratio = len(out) / l1
                if verbose:
                    print("bgzf %s: %d -> device %d, zlib level 1 %d (ratio %.3f), Z_HUFFMAN_ONLY %d, Z_FIXED %d%s"
                          % (tag, len(data), len(out), l1, ratio, huff, fixed, "  LARGER THAN Z_FIXED" if len(out) > fixed else ""))
                assert len(out) < huff, (tag, len(out), huff)
                assert ratio <= RATIO_CAP, (tag, ratio)
                if tag == "single_om1_omax4":
                    assert hashlib.sha256(out).hexdigest() == SHA256_SINGLE_OM1_OMAX4
        return ratio
    finally:
        a.close()


def check_determinism(index, make=make_aligner):
    """the same input twice on one context and on a second context gives equal bytes (the emulator: under another SNAPGPU_EMU_CUS)"""
    data = fixture_arrays()["paired_default"][:40000] + rng_bytes(9, 3000)
    a = make(index)
    try:
        o1, _ = compress(a, data, 4096)
        o2, _ = compress(a, data, 4096)
        assert o1 == o2
        # behind three more members the same members fall to other wavefronts of another grid: their bytes are the same
        o3, r3 = compress(a, rng_bytes(10, 3 * 4096) + data, 4096)
        assert o3[int(r3["member_begin"][3]):] == o1
    finally:
        a.close()
    return o1


def check_memory_discipline(index):
    data = fixture_arrays()["single_ea_om1"][:30000]
    a = make_aligner(index)
    try:
        full, r = compress(a, data, 4096)
        mb = r["member_begin"]
        nm = r["n_members"]
        # guard bytes around the output and member_begin
        buf = np.full(len(full) + 64, 0xA5, np.uint8); mbuf = np.full(nm + 1 + 8, 0x5A5A5A5A5A5A5A5A, np.uint64)
        f = a.lib.snapgpu_bgzf_compress
        import ctypes as C
        f.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint64] + [C.c_void_p] * 4
        src = np.frombuffer(data, np.uint8)
        n_mem = C.c_uint64(0); ob = C.c_uint64(0)
        rc = f(a.handle, src.size, src.ctypes.data, 4096, len(full), buf.ctypes.data + 32, mbuf.ctypes.data + 32, C.addressof(n_mem), C.addressof(ob))
        assert rc == 0 and ob.value == len(full) and n_mem.value == nm
        assert (buf[:32] == 0xA5).all() and (buf[32 + len(full):] == 0xA5).all() and buf[32:32 + len(full)].tobytes() == full
        assert (mbuf[:4] == 0x5A5A5A5A5A5A5A5A).all() and (mbuf[4 + nm + 1:] == 0x5A5A5A5A5A5A5A5A).all() and (mbuf[4:4 + nm + 1] == mb).all()
        # a capacity that cuts a member
        from snap_amd.aligner import W_TEXT_TRUNCATED
        cut = 3
        cap = int(mb[cut]) + 17
        buf = np.full(len(full) + 64, 0xA5, np.uint8); mb2 = np.zeros(nm + 1, np.uint64)
        rc = f(a.handle, src.size, src.ctypes.data, 4096, cap, buf.ctypes.data, mb2.ctypes.data, C.addressof(n_mem), C.addressof(ob))
        assert rc == W_TEXT_TRUNCATED and ob.value == len(full) and (mb2 == mb).all()
        assert buf[:int(mb[cut])].tobytes() == full[:int(mb[cut])] and (buf[int(mb[cut]):] == 0xA5).all()
        r2 = a.bgzfCompress(data, 4096, capacity=cap, grow=False)
        assert r2["truncated"] and r2["bgzf_bytes"] == len(full)
        # the argument errors
        for bi in (0, MAX_BLOCK + 1):
            assert f(a.handle, src.size, src.ctypes.data, bi, cap, buf.ctypes.data, mb2.ctypes.data, C.addressof(n_mem), C.addressof(ob)) == -1, bi
        assert f(a.handle, src.size, None, 4096, cap, buf.ctypes.data, mb2.ctypes.data, C.addressof(n_mem), C.addressof(ob)) == -1
        assert f(a.handle, src.size, src.ctypes.data, 4096, cap, None, mb2.ctypes.data, C.addressof(n_mem), C.addressof(ob)) == -1
        assert f(a.handle, src.size, src.ctypes.data, 4096, cap, buf.ctypes.data, None, C.addressof(n_mem), C.addressof(ob)) == -1
        assert f(a.handle, src.size, src.ctypes.data, 4096, cap, buf.ctypes.data, mb2.ctypes.data, None, C.addressof(ob)) == -1
        assert f(a.handle, 0, None, 4096, 28, buf.ctypes.data, mb2.ctypes.data, C.addressof(n_mem), C.addressof(ob)) == 0 and buf[:28].tobytes() == EOF_BLOCK
    finally:
        a.close()


def check_device_form(index, hb):
    """bgzfCompress_device == the host form, with d_in and d_out at odd addresses, guard bytes on both sides, and a capacity that is too small"""
    data = fixture_arrays()["single_ea_om1"][:20000]
    a = make_aligner(index)
    try:
        full, r = compress(a, data, 1000)
        nm = r["n_members"]
        for in_shift, out_shift in ((1, 3), (2, 1), (3, 2), (0, 0)):
            src0 = np.zeros(len(data) + 32, np.uint8); src0[16 + in_shift:16 + in_shift + len(data)] = np.frombuffer(data, np.uint8)
            buf0 = np.full(len(full) + 64, 0xA5, np.uint8); mb0 = np.full(nm + 1 + 4, 0x5A5A5A5A5A5A5A5A, np.uint64)
            d_src, d_buf, d_mb = hb.upload(src0), hb.upload(buf0), hb.upload(mb0)
            for cap in (int(r["member_begin"][5]) + 9, len(full)):               # (the cut call first: what it must not touch is still untouched)
                got = a.bgzfCompress_device(len(data), d_src + 16 + in_shift, 1000, cap, d_buf + 16 + out_shift, d_mb + 16)
                assert got == (nm, len(full), cap < len(full)), got
                buf, mb = hb.download(d_buf, buf0), hb.download(d_mb, mb0)
                fit = int(r["member_begin"][5]) if cap < len(full) else len(full)
                at = 16 + out_shift
                assert (buf[:at] == 0xA5).all() and buf[at:at + fit].tobytes() == full[:fit]
                assert (buf[at + fit:] == 0xA5).all()
                assert (mb[:2] == 0x5A5A5A5A5A5A5A5A).all() and (mb[2 + nm + 1:] == 0x5A5A5A5A5A5A5A5A).all() and (mb[2:2 + nm + 1] == r["member_begin"]).all()
    finally:
        a.close()
        hb.free_all()


def members_of(blob):
    """[(member bytes, ISIZE)] of concatenated BGZF members, walked by BSIZE"""
    out = []; at = 0
    while at < len(blob):
        assert blob[at:at + 16] == HEAD, at
        size = struct.unpack_from("<H", blob, at + 16)[0] + 1
        out.append((blob[at:at + size], struct.unpack_from("<I", blob, at + size - 4)[0])); at += size
    assert at == len(blob)
    return out


def check_fused(bam, z, block_input, cap_kw, call):
    """a fused _bgzf call (z) against its _bam form (bam) on the same input: the blocks hold the record bytes, every member is checked as
    check_output checks it; then a BGZF capacity and a member capacity that are too small (call: the _bgzf method with everything else bound)"""
    raw = bam["bytes"][:bam["bam_bytes"]].tobytes()
    assert int(bam["block_begin"][-1]) == len(raw) == z["bam_bytes"] and not z["truncated"]
    check_output(raw, block_input, z["bgzf"][:z["bgzf_bytes"]], z["member_begin"], z["n_members"], z["bgzf_bytes"])
    assert z["n_members"] >= 3                                               # (block_input is chosen so that there are several)
    full = z["bgzf"][:z["bgzf_bytes"]].tobytes(); mb = z["member_begin"]
    cut = int(mb[2]) + 5
    t = call(bgzf_capacity=cut, member_capacity=z["n_members"], grow=False, **cap_kw)
    assert t["truncated"] and t["bgzf_bytes"] == len(full) and t["bam_bytes"] == len(raw) and (t["member_begin"] == mb).all()
    assert t["bgzf"][:int(mb[2])].tobytes() == full[:int(mb[2])] and not t["bgzf"][int(mb[2]):].any()
    t = call(bgzf_capacity=len(full), member_capacity=2, grow=False, **cap_kw)
    assert t["truncated"] and t["n_members"] == z["n_members"] and (t["member_begin"] == mb[:3]).all() and t["bgzf"].tobytes() == full
    return t


def check_fused_single(index, tag="ea_om1", n=150, block_input=4096):
    """alignSamBgzf on the tiny index: decompressed, the block_begin-delimited bytes of alignSamBam; both warnings, the records' first"""
    from tests import bam_util as bu, samrec_util as su
    from tests.samtext_util import pack
    reads, f, _, recs, ids = bu.golden_case("single", tag)
    z0 = su.fixture()
    o = reads["offsets"][:n + 1]
    bases, quals, fc, dl = reads["bases"][:int(o[-1])], reads["quals"][:int(o[-1])], z0["front_clip"][:n], z0["data_len"][:n]
    nb, noff = pack([b"r%d" % i for i in range(n)])
    cli, kw, sec, ae, use_m = su.SETS[tag]
    a = su.make_aligner(index, tag)
    try:
        a.setContigBamIds(ids)
        skip = su.skip_mask(bases, o, fc, dl, int(a.params.max_k))
        args = (bases, quals, o, fc, dl, skip, nb, noff)
        kws = dict(use_m=bool(use_m), adjust_primary=bool(ae and sec is None), block_input=block_input)
        bam = a.alignSamBam(*args, use_m=kws["use_m"], adjust_primary=kws["adjust_primary"])
        z = a.alignSamBgzf(*args, **kws)
        assert z["n_records"] == bam["n_records"] and (z["flag"] == bam["flag"]).all() and (z["rec_begin"] == bam["rec_begin"]).all()
        check_fused(bam, z, block_input, dict(capacity=bam["n_records"]), lambda **k: a.alignSamBgzf(*args, **kws, **k))
        # the records' warning comes first: with both capacities too small it is the one returned, and the blocks are those of the records that fit
        few = a.alignSamBgzf(*args, capacity=n // 2, bgzf_capacity=16, member_capacity=1, grow=False, **kws)
        assert few["records_truncated"] and not few["truncated"] and few["n_records"] == bam["n_records"]
        assert few["bam_bytes"] == int(bam["block_begin"][n // 2])
        # then the text warning, once the records fit
        then = a.alignSamBgzf(*args, capacity=bam["n_records"], bgzf_capacity=16, member_capacity=1, grow=False, **kws)
        assert then["truncated"] and not then["records_truncated"] and then["bgzf_bytes"] == z["bgzf_bytes"]
        f2 = a.lib.snapgpu_align_sam_single_bgzf                            # (argtypes are set by now) block_input out of range
        import ctypes as C
        from snap_amd.aligner import ptr
        v = [C.c_uint64(0) for _ in range(4)]; flag = np.zeros(400, np.int32); rb = np.zeros(n + 1, np.uint64); mbuf = np.zeros(8, np.uint64); out = np.zeros(64, np.uint8)
        for bi in (0, MAX_BLOCK + 1):
            assert f2(a.handle, n, ptr(bases), ptr(quals), ptr(o), ptr(fc), ptr(dl), ptr(skip), 0, 0, ptr(nb), ptr(noff), 64, 400, C.addressof(v[0]), ptr(rb), ptr(flag),
                      bi, 64, ptr(out), ptr(mbuf), 7, C.addressof(v[1]), C.addressof(v[2]), C.addressof(v[3])) == -1, bi
    finally:
        a.close()


def check_fused_paired(index, n_pairs=60, block_input=4096):
    """alignSamBgzfPaired on the paired index with about 60 pairs, against alignSamBamPaired"""
    from snap_amd import abi
    from snap_amd.aligner import ChimericPairedEndAligner
    from tests import bam_util as bu
    from tests.samtext_util import pack
    zp = np.load(os.path.join(util.GOLDEN, "paired_reads.npz"))
    o = zp["o150"][:2 * n_pairs + 1].astype(np.uint64)
    bases, quals = zp["b150"][:int(o[-1])], zp["q150"][:int(o[-1])]
    n = 2 * n_pairs
    fc = np.zeros(n, np.int32); dl = np.diff(o.astype(np.int64)).astype(np.int32); skip = np.zeros(n_pairs, np.uint8)
    skip[3] = 1
    nb, noff = pack([b"p%d/%d x" % (i // 2, 1 + i % 2) if i % 8 else b"p%d/%d" % (i // 2, 1 + i % 2) for i in range(n)])
    a = ChimericPairedEndAligner(index, abi.default_params(max_k=8, max_read_len=160), abi.default_paired_params())
    try:
        a.setContigBamIds(bu.ref_ids(len(index.contigs)))
        args = (bases, quals, o, fc, dl, skip, nb, noff)
        bam = a.alignSamBamPaired(*args)
        z = a.alignSamBgzfPaired(*args, block_input=block_input)
        assert int((bam["flag"] & 4 == 0).sum()) > n_pairs                   # (the batch aligns)
        assert (z["flag"] == bam["flag"]).all() and (z["first_written"] == bam["first_written"]).all()
        check_fused(bam, z, block_input, {}, lambda **k: a.alignSamBgzfPaired(*args, block_input=block_input, **k))
    finally:
        a.close()


def check_tool(tool, d, mode, index_dir, fqs, opts, env=None, tool_opts=()):
    """`snapgpu-sam -o x.bam` with SNAPGPU_SAM_DEVICE_BGZF=1: the reference CLI's header, reference table and records, compared as
    bam_util.check_tool compares them (test_zz_gpu_native_sam.run_and_compare_bam, the switch on); with tool_opts, the switch-on file has the
    members of the switch-off file -- the same ISIZE sequence, the same decompressed bytes member by member -- and ends in the 28-byte
    block; the stderr line counts the batches, the blocks and the bytes.  bam_util.check_tool itself cannot be called here: it asserts that
    its switch-off run prints no "BAM records from the device" line, and with this switch in the environment both of its runs take the device's
    records; the comparison with the reference's file is the one it makes.  Returns (records, batches)."""
    import re
    import subprocess
    from tests.test_zz_gpu_native_sam import bam_parts, run_and_compare_bam
    base = dict(os.environ if env is None else env)
    for k in ("SNAPGPU_SAM_DEVICE_BAM", "SNAPGPU_SAM_DEVICE_BGZF"):
        base.pop(k, None)
    n = run_and_compare_bam(tool, d, mode, index_dir, fqs, opts, env=dict(base, SNAPGPU_SAM_DEVICE_BGZF="1"))
    tag = mode + "_" + ("_".join(o.strip("-") or "eq" for o in opts) or "default")
    out = os.path.join(d, "new_%s.bam" % tag)                                # (the same output path every time: it is part of @PG)
    ref_parts = bam_parts(os.path.join(d, "ref_%s.bam" % tag))
    files, logs = [], []
    for e in (dict(base, SNAPGPU_SAM_DEVICE_BGZF="1"), dict(base, SNAPGPU_SAM_DEVICE_BGZF="0"), base):
        r = subprocess.run([tool, mode, index_dir] + fqs + ["-o", out] + opts + list(tool_opts), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, stdin=subprocess.DEVNULL,
                           timeout=3000, env=e)
        assert r.returncode == 0, "snapgpu-sam failed:\n%s" % r.stdout.decode(errors="replace")[-3000:]
        logs.append(r.stdout.decode(errors="replace"))
        with open(out, "rb") as f:
            files.append(f.read())
        assert bam_parts(out) == ref_parts
    on, off = members_of(files[0]), members_of(files[1])
    assert files[1] == files[2]                                              # =0 is unset
    assert [i for _, i in on] == [i for _, i in off]
    assert [zlib.decompress(m[18:-8], -15) for m, _ in on] == [zlib.decompress(m[18:-8], -15) for m, _ in off]
    assert gzip.decompress(files[0]) == gzip.decompress(files[1])
    assert files[0][-28:] == EOF_BLOCK and on[-1][0] == EOF_BLOCK
    m = re.search(r"BGZF blocks from the device: (\d+) batches, (\d+) blocks, (\d+) -> (\d+) bytes", logs[0])
    assert m and "BGZF blocks from the device" not in logs[1] + logs[2], logs[0][-500:]
    batches, blocks, n_in, n_out = (int(x) for x in m.groups())
    header = len(on) - 1 - blocks                                            # the header's block(s) in front, the end-of-file block behind
    assert batches >= 1 and header >= 1 and n_in == sum(i for _, i in on[header:-1]) and n_out == sum(len(x) for x, _ in on[header:-1])
    assert files[0][:sum(len(x) for x, _ in on[:header])] == files[1][:sum(len(x) for x, _ in off[:header])]      # the header block stays host-made
    assert any(x != y for (x, _), (y, _) in zip(on[header:-1], off[header:-1]))      # (and the payloads are the device's, not zlib's)
    return n, batches


# ---- inputs that exist to reach one path of the coder each (tests/test_emu_bgzf_coder.py, tests/test_zz_gpu_bgzf_coder.py).  The lever is
# window_input's: an all-equal filler touches one entry of the hash table, so a planted word keeps its entry and its second copy is matched
# at exactly the gap it was planted at.  Every check asserts from the parsed stream that its path was reached, so a change to the matcher
# that steers an input elsewhere fails with a message that says so.  The seeds were found with scripts/bgzf_find_inputs.py on the emulator.
FILL, RUN, TERM = 0x61, 0x62, 0x7c


def planted_input(size, pairs, seed, plain=False):
    """`size` filler bytes and, for every (distance, length) of pairs, a word at a position q that is a multiple of 64 (lane 0 of its step)
    with its one earlier copy `distance` back; the byte behind the earlier copy differs from the one behind the later copy, so the match is
    `length` long.  A word is four random bytes and a run of one value (plain: random bytes throughout); a distance below the length
    makes it periodic.  Returns (bytes, [q])."""
    rng = np.random.default_rng(seed)
    x = bytearray([FILL]) * size
    busy = np.zeros(size + 8, bool)
    values = np.array([v for v in range(256) if v not in (FILL, RUN, TERM)], np.uint8)
    where = []
    for d, L in pairs:
        for _ in range(10000):
            q = 64 * int(rng.integers((d + 8) // 64 + 1, (size - L - 8) // 64 + 1))
            spans = [(q - d - 4, q + L + 4)] if d <= L + 8 else [(q - d - 4, q - d + L + 4), (q - 4, q + L + 4)]
            if q + L + 4 <= size and not any(busy[a:b].any() for a, b in spans):
                break
        else:
            raise AssertionError("no room for (%d, %d)" % (d, L))
        for a, b in spans:
            busy[a:b] = True
        word = bytes(rng.choice(values, L if plain else 4)) + bytes([RUN]) * (0 if plain else L - 4)
        n1 = min(d, L)
        x[q - d:q - d + n1] = word[:n1]
        if d > L:
            x[q - d + L] = TERM
        for i in range(L):
            x[q + i] = x[q - d + i]
        where.append(q)
    return bytes(x), where


def token_map(block):
    """{position in the member: token} of a parsed block"""
    out = {}; pos = 0
    for t in block.tokens:
        out[pos] = t
        pos += 1 if isinstance(t, int) else t[0]
    return out


def compress_members(a, data, block_input=MAX_BLOCK):
    """compress (every member through check_output) and the parsed block of every member"""
    r = a.bgzfCompress(data, block_input)
    assert not r["truncated"]
    blocks = []
    check_output(data, block_input, r["bgzf"][:r["bgzf_bytes"]], r["member_begin"], r["n_members"], r["bgzf_bytes"], blocks)
    return blocks


# (symbol 284 with extra value 31 would be 258 bytes, which is symbol 285's: its highest extra value is 30)
LENGTH_SYMBOLS_LOW_HIGH = sorted({(257 + i, min(e, 30) if i == 27 else e) for i in range(1, 29) for e in (0, (1 << du.LEN_EXTRA[i]) - 1)})
LENGTHS_LOW_HIGH = sorted(du.LEN_BASE[s - 257] + e for s, e in LENGTH_SYMBOLS_LOW_HIGH)                                  # 4 .. 258: 49 lengths
DISTANCES_LOW_HIGH = sorted({du.DIST_BASE[i] + e for i in range(30) for e in (0, (1 << du.DIST_EXTRA[i]) - 1)})          # 1 .. 32768: 56 distances
SYMBOL_SEEDS = (0, 0, 0, 1)                                                # one member each, 14 (distance, length) pairs a member


def symbol_pairs():
    """56 (distance, length): every distance once, and the 49 lengths taken in steps of five (5 and 49 have no common factor), so all occur"""
    return [(d, LENGTHS_LOW_HIGH[(5 * i) % len(LENGTHS_LOW_HIGH)]) for i, d in enumerate(DISTANCES_LOW_HIGH)]


def symbols_member(m, seed):
    pairs = symbol_pairs()
    per = -(-len(pairs) // len(SYMBOL_SEEDS))
    return planted_input(MAX_BLOCK, pairs[m * per:(m + 1) * per], seed)[0], pairs[m * per:(m + 1) * per]


def check_every_symbol(index, seeds=SYMBOL_SEEDS):
    """every length symbol that the matcher can emit (258 .. 285: 257 is a match of three bytes, below its minimum of four) and every
    distance symbol 0 .. 29, each with its lowest and its highest extra-bits value"""
    a = make_aligner(index)
    try:
        data = b"".join(symbols_member(m, s)[0] for m, s in enumerate(seeds))
        blocks = compress_members(a, data)
        assert all(b.btype == 2 for b in blocks)
        ms = [t for b in blocks for t in b.matches()]
        got_l = {(t[1], t[0] - du.LEN_BASE[t[1] - 257]) for t in ms}; got_d = {(t[3], t[2] - du.DIST_BASE[t[3]]) for t in ms}
        want_l = set(LENGTH_SYMBOLS_LOW_HIGH)
        want_d = {(i, e) for i in range(30) for e in (0, (1 << du.DIST_EXTRA[i]) - 1)}
        assert not want_l - got_l, ("length symbols / extra values not reached", sorted(want_l - got_l))
        assert not want_d - got_d, ("distance symbols / extra values not reached", sorted(want_d - got_d))
        assert not any(t[1] == 257 for t in ms)
        return blocks
    finally:
        a.close()


WINDOW_EDGE_SEED = 0


def window_edge_input(seed=WINDOW_EDGE_SEED):
    return planted_input(MAX_BLOCK, [(32768, 40), (32769, 40)], seed, plain=True)


def check_window_edge(index, seed=WINDOW_EDGE_SEED):
    """a word whose only earlier copy is 32768 back: one match, distance symbol 29 with extra value 8191.  32769 back: literals."""
    a = make_aligner(index)
    try:
        data, (q_in, q_out) = window_edge_input(seed)
        b, = compress_members(a, data)
        at = token_map(b)
        assert b.btype == 2 and at.get(q_in) == (40, 273, 32768, 29), ("the copy 32768 back was not matched", at.get(q_in))
        assert du.DIST_BASE[29] + 8191 == 32768 and du.LEN_BASE[273 - 257] + 5 == 40
        assert all(at.get(q_out + i) == data[q_out + i] for i in range(40)), "the copy 32769 back is not 40 literals"
        assert max(t[2] for t in b.matches()) == 32768
        return b
    finally:
        a.close()


CUT_REST = (1, 2, 3, 4, 5, 257, 258, 259)
CUT_BLOCK = 1024
CUT_SEED = 1


def cut_match_input(seed=CUT_SEED):
    """members of CUT_BLOCK bytes: 300 random bytes, filler, and the first `rest` of the same bytes again in front of the member's end"""
    out = b""
    for k, rest in enumerate(CUT_REST):
        w = rng_bytes(1000 * seed + k, 300).replace(bytes([FILL]), b"\x00")
        out += w + bytes([FILL]) * (CUT_BLOCK - 300 - rest) + w[:rest]
    return out


def check_cut_match(index, seed=CUT_SEED):
    """a match that the member's end cuts short, len - pos = 1 .. 5 and 257 .. 259 where it starts: below four bytes literals, then a match
    of exactly what is left, and at 259 a match of 258 with one literal behind it"""
    a = make_aligner(index)
    try:
        data = cut_match_input(seed)
        blocks = compress_members(a, data, CUT_BLOCK)
        assert len(blocks) == len(CUT_REST)
        for k, (b, rest) in enumerate(zip(blocks, CUT_REST)):
            q = CUT_BLOCK - rest; src = data[k * CUT_BLOCK:(k + 1) * CUT_BLOCK]
            at = token_map(b)
            assert b.btype == 2, rest
            if rest < 4:
                assert [at.get(q + i) for i in range(rest)] == list(src[q:]), (rest, "literals expected")
            else:
                t = at.get(q)
                assert t is not None and not isinstance(t, int) and t[0] == min(rest, 258) and t[2] == q, (rest, t)
                if rest == 259:
                    assert at.get(q + 258) == src[-1] and b.tokens[-1] == src[-1]
                else:
                    assert b.tokens[-1] == t
        return blocks
    finally:
        a.close()


def short_inputs(k):
    """the inputs of k bytes of check_short_members"""
    rng = np.random.default_rng(7000 + k)
    return {"run": b"a" * k, "alternating": (b"ab" * k)[:k], "two_values": bytes(rng.choice(np.array([0x30, 0x31], np.uint8), k, p=[0.8, 0.2]))}


def check_short_members(index):
    """one to two distinct bytes, 1 .. 130 of them: dynamic blocks of fewer than 64 tokens (lanes without a token in the emission), and of
    exactly 64 and 65 (the step from one token a lane to two).  Returns {token count with end-of-block: number of dynamic blocks}."""
    a = make_aligner(index)
    try:
        seen = {}
        for k in range(1, 131):
            for name, data in short_inputs(k).items():
                b, = compress_members(a, data)
                if b.btype == 2:
                    seen[len(b.tokens) + 1] = seen.get(len(b.tokens) + 1, 0) + 1
        assert any(n < 64 for n in seen) and 64 in seen and 65 in seen, ("token counts reached", sorted(seen))
        assert min(seen) <= 16, sorted(seen)                                  # (most lanes without a token)
        return seen
    finally:
        a.close()


def check_crc_slices(index, pairs=tuple(range(2, 201, 2)), singles=(4095, 4096, 4097, 65279, 65280)):
    """random bytes of every length 1 .. 200 (a call holds the members L and L - 1), around 4096 and at the largest member: the CRC's lane
    slices of (len + 63) / 64 bytes leave lanes empty at most of them.  Stored blocks: it is the CRC, which check_output compares with
    zlib's, that is under test."""
    a = make_aligner(index)
    try:
        lengths = set()
        for L in pairs:
            blocks = compress_members(a, rng_bytes(300 + L, 2 * L - 1), L)
            lengths |= {L, L - 1}
            assert len(blocks) == 2
        for L in singles:
            b, = compress_members(a, rng_bytes(300 + L, L), L)
            assert b.btype == 0
            lengths.add(L)
        return lengths
    finally:
        a.close()


def literal_input(groups, count, seed):
    """count bytes of every value of groups (a list of ranges), shuffled"""
    x = np.repeat(np.array([v for g in groups for v in g], np.uint8), count)
    np.random.default_rng(seed).shuffle(x)
    return x.tobytes()


# (what the case is for, the input); the run lengths are asserted from the parsed lengths
def header_run_cases():
    return {
        # 31 values of equal counts and end-of-block: 32 codes of five bits; the values stand in groups of 4, 7, 8 and 10 with zeros between
        "nonzero_4_7_8_10": literal_input([range(10, 14), range(20, 27), range(30, 38), range(40, 50), (60,), (70,)], 8, 1),
        # zeros between the used values: 3, 10, 11, 138; and 139 from the last used value to end-of-block
        "zero_3_10_11_138": literal_input([(0,), (4,), (15,), (27,), (166,)], 400, 2),
        "zero_139": literal_input([(5,), (116,)], 600, 3),
    }


HEADER_RUNS_WANTED = {"nonzero_4_7_8_10": [("nonzero", 4), ("nonzero", 7), ("nonzero", 8), ("nonzero", 10)],
                      "zero_3_10_11_138": [(0, 3), (0, 10), (0, 11), (0, 138)], "zero_139": [(0, 139)]}


def spans_boundary(block):
    """the header symbols (16, 17, 18) whose repeats cover lengths on both sides of the lit/len | distance boundary"""
    at = 0; out = []
    for s, n in block.header_seq:
        if n and at - (1 if s == 16 else 0) < block.hlit < at + n:
            out.append((s, n, at))
        at += n or 1
    return out


def check_header_runs(index):
    """the run-length coder of the block header at its edges: zero runs of exactly 3, 10 (one 17), 11, 138 (one 18) and 139 (an 18 and a plain
    zero), non-zero runs of exactly 4 (length, 16 x 3), 7 (length, 16 x 6), 8 (one more plain length) and 10 (16 x 6, 16 x 3); a run that
    goes on from the lit/len lengths into the distance lengths.  check_coded_member has compared each sequence with the greedy coder's."""
    a = make_aligner(index)
    try:
        reached = {}
        for name, data in header_run_cases().items():
            b, = compress_members(a, data)
            assert b.btype == 2, name
            runs = du.header_runs(b.ll_lengths + b.d_lengths)
            for v, n in HEADER_RUNS_WANTED[name]:
                assert any(rn == n and (rv == 0 if v == 0 else rv != 0) for rv, rn in runs), (name, "run not reached", (v, n), runs)
            reached[name] = runs
        # the first member of a fixture array: lit/len lengths that end in 9, 9, 9 and a first distance length of 9, one 16 over the boundary
        b, = compress_members(a, fixture_arrays()["single_ae_om1"][:MAX_BLOCK])
        assert b.btype == 2 and spans_boundary(b), ("no run crosses from the lit/len lengths into the distance lengths", b.header_seq[-40:])
        reached["crossing"] = spans_boundary(b)
        return reached
    finally:
        a.close()


def check_code_length_code_limited(index):
    """the code-length code limited at 7 bits by the fold-and-repair loop of bgzf_build_code: over the header of a fixture array's first member
    a plain Huffman code is 8 deep, and the code that was sent has a length of exactly 7 (and, by check_coded_member, is complete and ordered)"""
    a = make_aligner(index)
    try:
        b, = compress_members(a, fixture_arrays()["single_om1_omax4"][:MAX_BLOCK])
        counts = [0] * 19
        for s, _ in b.header_seq:
            counts[s] += 1
        deep = max(du.huffman_lengths(counts).values())
        assert deep > 7, ("the header's histogram no longer needs the limit: Huffman depth", deep, counts)
        assert max(b.cl_lengths) == 7, b.cl_lengths
        return deep, counts
    finally:
        a.close()


# ---- the distance code limited at 15: 4180 matches of four bytes over the 17 distance symbols 12 .. 28 in Fibonacci proportions, one member
DISTANCE_LIMIT_COUNTS = {12 + i: c for i, c in enumerate((1597, 987, 610, 377, 233, 144, 89, 55, 34, 21, 13, 8, 5, 3, 2, 1, 1))}
DISTANCE_LIMIT_SEED = 0


def distance_symbol(d):
    return max(s for s in range(30) if du.DIST_BASE[s] <= d)


def distance_limit_layout():
    """the member as a sequence of word numbers (a word is four bytes).  A section S(K, m): K new words, then the same K words again and
    again, adjacent words swapped in every other period, until m words have been repeated -- every repeat lies 4 K - 4 or 4 K + 4 bytes
    behind its word's last place.  A group G(n, inner): n new words, the inner sequence, the n words with adjacent ones swapped -- every
    repeat lies 4 (n + len(inner)) bytes, give or take four, behind.  Filler: new words that stand once.  The groups are nested so that
    every distance falls into the range of its symbol; every distance is 68 or more, so a word's earlier place belongs to an earlier
    64-byte step of the matcher."""
    n_words = [0]

    def new(k):
        n_words[0] += k
        return list(range(n_words[0] - k, n_words[0]))

    def swapped(w):
        out = list(w)
        for i in range(0, len(out) - 1, 2):
            out[i], out[i + 1] = out[i + 1], out[i]
        return out

    def S(K, m):
        w = new(K); out = list(w); t = 1
        while m:
            part = (swapped(w) if t & 1 else w)[:m]
            out += part; m -= len(part); t += 1
        return out

    def G(n, *inner):
        w = new(n)
        return w + [x for part in inner for x in part] + swapped(w)

    c = DISTANCE_LIMIT_COUNTS
    g25 = G(c[25], S(18, c[12]))
    g24 = G(c[24], G(c[21], S(50, c[15])), G(c[20], S(66, c[16])), S(98, c[17]))
    g26 = G(c[26], g25, G(c[18], new(50)), G(c[19], new(150)))
    g27 = G(c[27], g26, g24)
    return G(c[28], g27, G(c[23], S(26, c[13])), G(c[22], S(34, c[14])))


def distance_limit_input(seed=DISTANCE_LIMIT_SEED):
    """the bytes of distance_limit_layout() with random words, drawn again until, for every repeat of a word, (a) no four bytes between the
    word's last place and this one fall into the same one of 4096 hash classes -- otherwise the matcher's table no longer points at the last
    place, the word goes out as literals, the cursor leaves the word grid and 258-byte matches two periods back take over -- and (b) the
    byte behind the word differs from the byte behind its last place, so that the match is four bytes long.  (a) uses the matcher's hash,
    the top 12 bits of the little-endian word times 2654435761: should bgzf.h hash otherwise, check_distance_code_limited says that the
    input no longer reaches its path.  Returns (bytes, {distance symbol: planned matches})."""
    rng = np.random.default_rng(seed)
    layout = np.array(distance_limit_layout())
    n_words = int(layout.max()) + 1
    last = {}; plan = []                                                       # (slot, the word's last slot)
    for j, w in enumerate(layout.tolist()):
        if w in last:
            plan.append((j, last[w]))
        last[w] = j
    planned = {}
    for j, q in plan:
        s = distance_symbol(4 * (j - q)); planned[s] = planned.get(s, 0) + 1
    assert planned == DISTANCE_LIMIT_COUNTS and min(j - q for j, q in plan) >= 17, planned
    words = rng.integers(0, 256, (n_words, 4), dtype=np.uint8)
    p = np.array([4 * j for j, _ in plan]); q = np.array([4 * k for _, k in plan])
    for _ in range(5000):
        x = words[layout].reshape(-1)
        v = x[:-3].astype(np.uint64) | (x[1:-2].astype(np.uint64) << 8) | (x[2:-1].astype(np.uint64) << 16) | (x[3:].astype(np.uint64) << 24)
        h = ((v * 2654435761) & 0xffffffff) >> 20
        # the last place before every position where the position's hash class occurred
        order = np.lexsort((np.arange(h.size), h))
        prev = np.full(h.size, -1, np.int64)
        same = h[order][1:] == h[order][:-1]
        prev[order[1:][same]] = order[:-1][same]
        nxt = np.append(x, 0)[np.minimum(p + 4, x.size)]
        bad = (prev[p] != q) | ((p + 4 < x.size) & (nxt == np.append(x, 0)[q + 4]))
        if not bad.any():
            return x.tobytes(), planned
        again = np.unique(layout[p[bad] // 4])
        words[again] = rng.integers(0, 256, (again.size, 4), dtype=np.uint8)
    raise AssertionError("no clean set of words")


def check_distance_code_limited(index, seed=DISTANCE_LIMIT_SEED):
    """the distance code limited at 15 bits by the fold-and-repair loop of bgzf_build_code: the parsed distance histogram is the planned one
    (4180 matches, Fibonacci counts over 17 symbols), a plain Huffman code over it is 16 deep, and the code that was sent has a length of
    exactly 15 (and, by check_coded_member, is complete and ordered)"""
    a = make_aligner(index)
    try:
        data, planned = distance_limit_input(seed)
        b, = compress_members(a, data)
        counts = [0] * 30
        for t in b.matches():
            counts[t[3]] += 1
        got = {s: c for s, c in enumerate(counts) if c}
        deep = max(du.huffman_lengths(counts).values())
        assert b.btype == 2 and deep > 15, ("the input no longer reaches the limit of the distance code: Huffman depth, histogram", deep, got)
        assert max(b.d_lengths) == 15, b.d_lengths
        assert got == planned, ("the matcher no longer finds the planned matches", got)
        return deep, got
    finally:
        a.close()

