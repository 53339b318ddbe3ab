"""tests/deflate_util.py, the RFC 1951 reader the BGZF tests measure with, pinned to zlib: what zlib's deflate writes at levels 1, 6 and 9
and with Z_FIXED, the reader parses, its replay of the tokens is the input, and its end position is the end of the stream.  Then the reader's
refusals, on streams made by hand.  No emulator, no GPU."""
import zlib

import numpy as np
import pytest

from tests import bgzf_util as bz
from tests import deflate_util as du

Z_FIXED = 4
SETTINGS = [(1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_DEFAULT_STRATEGY), (6, Z_FIXED)]


def deflate(data, level, strategy):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return c.compress(data) + c.flush()


def expand(header_seq):
    """the lengths that a header's [(symbol, repeat)] stand for"""
    out = []
    for sym, n in header_seq:
        out += [sym] if sym < 16 else [out[-1] if sym == 16 else 0] * n
    return out


def check_against_zlib(data, level, strategy):
    z = deflate(data, level, strategy)
    blocks, out, end = du.read_stream(z)
    assert out == data
    assert (end + 7) // 8 == len(z), (end, len(z))                       # the final block ends in the stream's last byte
    produced = b""
    for b in blocks:
        if b.btype == 0:
            produced += z[b.stored_at:b.stored_at + b.stored_len]
        else:
            produced += du.replay(b.tokens, produced[-32768:])
            assert all(3 <= t[0] <= 258 and 1 <= t[2] <= 32768 for t in b.matches())
        if b.btype == 2:
            # zlib's header symbols expand to the lengths the reader returned, and so do the greedy coder's for the same lengths
            assert expand(b.header_seq) == b.ll_lengths + b.d_lengths
            assert expand(du.greedy_header_seq(b.ll_lengths + b.d_lengths)) == b.ll_lengths + b.d_lengths
        if strategy == Z_FIXED:
            assert b.btype in (0, 1)
    assert produced == data
    return blocks


def random_strings(n, seed):
    """byte strings of mixed compressibility: random bytes over alphabets of 1 .. 256 values, with copies of earlier pieces spliced in"""
    rng = np.random.default_rng(seed)
    for _ in range(n):
        size = int(rng.integers(0, 700)) if rng.random() < 0.97 else int(rng.integers(700, 9000))
        alpha = int(rng.choice([1, 2, 3, 4, 16, 64, 256]))
        x = bytearray(rng.integers(0, alpha, size, dtype=np.uint8).tobytes())
        for _ in range(int(rng.integers(0, 6))):
            if size < 8:
                break
            a, b = sorted(int(v) for v in rng.integers(0, size, 2))
            l = int(rng.integers(3, 300))
            x[b:b + l] = x[a:a + l][:max(0, size - b)]
        yield bytes(x[:size])


@pytest.mark.parametrize("tag", sorted(bz.fixture_arrays()))
def test_reader_equals_zlib_on_the_fixture_arrays(tag):
    data = bz.fixture_arrays()[tag]
    kinds = set()
    for level, strategy in SETTINGS:
        kinds |= {b.btype for b in check_against_zlib(data, level, strategy)}
    assert kinds >= {1, 2}


@pytest.mark.parametrize("seed", [101, 102, 103])
def test_reader_equals_zlib_on_random_strings(seed):
    kinds = set(); n_matches = 0
    for data in random_strings(1000, seed):
        for level, strategy in SETTINGS:
            blocks = check_against_zlib(data, level, strategy)
            kinds |= {b.btype for b in blocks}; n_matches += sum(len(b.matches()) for b in blocks)
    assert kinds == {0, 1, 2} and n_matches > 10000, (kinds, n_matches)


def test_reader_reads_stored_blocks_and_several_blocks():
    data = bz.rng_bytes(1, 70000)                                            # (incompressible: stored blocks, more than one of them)
    blocks = check_against_zlib(data, 1, zlib.Z_DEFAULT_STRATEGY)
    assert len(blocks) >= 2 and all(b.btype == 0 for b in blocks)
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    z = c.compress(b"abcabcabcabc" * 50) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(bytes(range(256)) * 3) + c.flush()
    blocks, out, end = du.read_stream(z)
    assert out == b"abcabcabcabc" * 50 + bytes(range(256)) * 3 and (end + 7) // 8 == len(z) and len(blocks) >= 3


class W:
    """a bit writer for the hand-made streams"""

    def __init__(self):
        self.bits = []

    def put(self, v, n):
        self.bits += [(v >> k) & 1 for k in range(n)]
        return self

    def code(self, c, n):                                                    # a Huffman code: most significant bit first
        self.bits += [(c >> (n - 1 - k)) & 1 for k in range(n)]
        return self

    def bytes(self):
        b = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(sum(b[i + k] << k for k in range(8)) for i in range(0, len(b), 8))


def dynamic_header(cl_lengths, hlit=257, hdist=1, hclen=19):
    w = W().put(1, 1).put(2, 2).put(hlit - 257, 5).put(hdist - 1, 5).put(hclen - 4, 4)
    for i in range(hclen):
        w.put(cl_lengths[du.CL_ORDER[i]], 3)
    return w


def test_reader_refuses_what_the_rfc_forbids():
    with pytest.raises(du.DeflateError, match="reserved"):
        du.read_stream(W().put(1, 1).put(3, 2).bytes())
    with pytest.raises(du.DeflateError, match="NLEN"):
        du.read_stream(bytes([1, 2, 0, 0xfd, 0xfe, 65, 66]))
    with pytest.raises(du.DeflateError, match="ends inside"):
        du.read_stream(bytes([1, 2, 0, 0xfd, 0xff, 65]))
    cl = [0] * 19
    cl[0] = cl[1] = cl[2] = 1                                                # three one-bit codes
    with pytest.raises(du.DeflateError, match="over-subscribed"):
        du.read_stream(dynamic_header(cl).bytes())
    cl = [0] * 19
    cl[0] = 1; cl[1] = 2                                                     # 1/2 + 1/4
    with pytest.raises(du.DeflateError, match="incomplete"):
        du.read_stream(dynamic_header(cl).bytes())
    cl = [0] * 19
    cl[16] = 1; cl[1] = 1                                                    # codes: 1 -> 0, 16 -> 1; the first symbol sent is 16
    with pytest.raises(du.DeflateError, match="no length before"):
        du.read_stream(dynamic_header(cl).code(1, 1).put(0, 2).bytes())
    cl = [0] * 19
    cl[18] = 1; cl[1] = 1                                                    # 1 -> 0, 18 -> 1: 138 + 138 zeros run past 257 + 1
    with pytest.raises(du.DeflateError, match="runs past"):
        du.read_stream(dynamic_header(cl).code(1, 1).put(127, 7).code(1, 1).put(127, 7).bytes())
    # fixed block: a match with nothing before it, and one that reaches one byte too far
    with pytest.raises(du.DeflateError, match="distance 1 with 0"):
        du.read_stream(W().put(1, 1).put(1, 2).code(1, 7).code(0, 5).bytes())              # 257 (length 3), distance symbol 0
    ok = W().put(1, 1).put(1, 2).code(0x30 + 65, 8).code(1, 7).code(0, 5).code(0, 7).bytes()
    assert du.read_stream(ok)[1] == b"AAAA"
    with pytest.raises(du.DeflateError, match="distance 2 with 1"):
        du.read_stream(W().put(1, 1).put(1, 2).code(0x30 + 65, 8).code(1, 7).code(1, 5).code(0, 7).bytes())
    # a dynamic block whose lit/len code lacks end-of-block, and one with an incomplete lit/len code
    cl = [0] * 19
    cl[18] = 1; cl[1] = 2; cl[0] = 2                                         # 18 -> 0, 0 -> 10, 1 -> 11
    w = dynamic_header(cl).code(0, 1).put(65 - 11, 7).code(3, 2).code(3, 2)  # zeros for 0..64, then 65 and 66 one bit each
    w.code(0, 1).put(138 - 11, 7).code(0, 1).put(51 - 11, 7).code(2, 2)      # zeros for 67..255, 256 and the distance length: zero
    with pytest.raises(du.DeflateError, match="end-of-block"):
        du.read_stream(w.code(2, 2).bytes())
    w = dynamic_header(cl).code(0, 1).put(65 - 11, 7).code(3, 2)             # 65: one bit
    w.code(0, 1).put(138 - 11, 7).code(0, 1).put(52 - 11, 7).code(3, 2)      # zeros for 66..255, 256: one bit
    blocks, out, _ = du.read_stream(w.code(2, 2).code(0, 1).code(0, 1).code(1, 1).bytes())      # no distance code; "AA", end
    assert out == b"AA" and blocks[0].d_lengths == [0] and blocks[0].header_seq[0] == (18, 65)


def test_huffman_and_package_merge_agree_where_the_limit_does_not_bind():
    rng = np.random.default_rng(7)
    for _ in range(300):
        n = int(rng.integers(2, 40))
        counts = [int(v) for v in rng.integers(0, 50, n)]
        if sum(1 for c in counts if c) < 2:
            continue
        h = du.huffman_lengths(counts)
        p = du.package_merge_lengths(counts, 15)
        assert max(h.values()) <= 15 and du.cost(counts, h) == du.cost(counts, p)
        du.check_code_for_counts(counts, [p.get(s, 0) for s in range(n)], 15, "package-merge")
    fib = [1, 1]
    while len(fib) < 12:
        fib.append(fib[-1] + fib[-2])
    assert max(du.huffman_lengths(fib).values()) == 11
    p = du.package_merge_lengths(fib, 7)
    assert max(p.values()) == 7 and du.kraft(p.values(), 7) == 128 and du.cost(fib, p) > du.cost(fib, du.huffman_lengths(fib))
