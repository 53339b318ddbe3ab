"""A plain, slow reader of raw DEFLATE (RFC 1951), written from the RFC: the yardstick of tests/bgzf_util.check_coded_member and of
tests/test_emu_bgzf_coder.py.  It does not look at the code under test and uses no zlib: tests/test_deflate_util.py pins it to zlib's output.
Where zlib's inflate only returns bytes, this reader returns what the stream is made of -- the block type, the three code tables of a dynamic
block, the run-length symbols its header was sent with, and the token list -- and it raises DeflateError on everything the RFC forbids: a
reserved block type, an over-subscribed or incomplete code (the RFC's one-distance-code case and "no distance code at all" aside), a repeat
with no length before it, lengths that run past HLIT + HDIST, a symbol without a code, a distance beyond the bytes produced so far, a stored
block whose NLEN is not ~LEN, and a stream that ends inside a block."""
import heapq

LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32                                                          # (30 and 31 have codes and never occur)


class DeflateError(ValueError):
    pass


def kraft(lengths, max_len):
    """the Kraft sum of the non-zero lengths, in units of 2^-max_len: a complete code gives exactly 1 << max_len"""
    return sum(1 << (max_len - l) for l in lengths if l)


def canonical_codes(lengths):
    """{symbol: (code, length)}, the code as the integer whose most significant bit is sent first (RFC 1951 section 3.2.2)"""
    max_len = max(lengths) if lengths else 0
    bl_count = [0] * (max_len + 2)
    for l in lengths:
        if l:
            bl_count[l] += 1
    next_code = [0] * (max_len + 2)
    code = 0
    for bits in range(1, max_len + 1):
        code = (code + bl_count[bits - 1]) << 1
        next_code[bits] = code
    out = {}
    for s, l in enumerate(lengths):
        if l:
            out[s] = (next_code[l], l); next_code[l] += 1
    return out


class Code:
    """a prefix code from its lengths.  what: the name in error messages; allow: "none" (no exception), "dist" (all lengths zero, or one
    code of one bit, may stand: RFC 1951 section 3.2.7)"""

    def __init__(self, lengths, max_len, what, allow="none"):
        if any(l > max_len for l in lengths):
            raise DeflateError("%s: a length above %d" % (what, max_len))
        used = [l for l in lengths if l]
        k = kraft(lengths, max_len)
        self.complete = k == 1 << max_len
        if k > 1 << max_len:
            raise DeflateError("%s: over-subscribed code (Kraft sum %d / %d)" % (what, k, 1 << max_len))
        if not self.complete and not (allow == "dist" and (not used or used == [1])):
            raise DeflateError("%s: incomplete code (Kraft sum %d / %d, %d symbols)" % (what, k, 1 << max_len, len(used)))
        self.what = what
        self.table = {(l << 16) | c: s for s, (c, l) in canonical_codes(list(lengths)).items()}
        self.max_len = max(used) if used else 0

    def decode(self, r):
        code = 0; l = 0
        bits = r.bits; pos = r.pos; table = self.table
        n = len(bits)
        while l < self.max_len:
            if pos >= n:
                raise DeflateError("%s: the stream ends inside a code" % self.what)
            code = (code << 1) | bits[pos]; pos += 1; l += 1
            s = table.get((l << 16) | code)
            if s is not None:
                r.pos = pos
                return s
        raise DeflateError("%s: a bit pattern that is no code" % self.what)


class Bits:
    def __init__(self, data):
        self.bits = [(b >> k) & 1 for b in bytes(data) for k in range(8)]
        self.pos = 0

    def take(self, n):
        """n bits as an integer, the first bit the least significant (every field that is not a Huffman code)"""
        if self.pos + n > len(self.bits):
            raise DeflateError("the stream ends inside a field")
        v = 0
        for k in range(n):
            v |= self.bits[self.pos + k] << k
        self.pos += n
        return v


class Block:
    """one block.  btype, final; end_bit: the bit position behind the block.
    stored: stored_len, stored_nlen, stored_at (byte offset of the copied bytes).
    dynamic: hlit, hdist, hclen (the counts, 257.., 1.., 4..), cl_lengths (19, by symbol), header_seq [(symbol, repeat)] -- repeat 0 for a
    plain length 0..15, the repeat count for 16, 17, 18 --, ll_lengths (hlit of them), d_lengths (hdist).
    dynamic and fixed: tokens -- an int 0..255 for a literal, (length, length symbol, distance, distance symbol) for a match; the end-of-block
    symbol is not in the list."""

    def __init__(self):
        self.btype = None; self.final = None; self.end_bit = None
        self.stored_len = self.stored_nlen = self.stored_at = None
        self.hlit = self.hdist = self.hclen = None
        self.cl_lengths = self.header_seq = self.ll_lengths = self.d_lengths = None
        self.tokens = []

    def matches(self):
        return [t for t in self.tokens if not isinstance(t, int)]


def read_block(r, out):
    """the block at r.pos; its bytes are appended to out (a bytearray that holds everything the stream produced so far)"""
    b = Block()
    b.final = r.take(1); b.btype = r.take(2)
    if b.btype == 3:
        raise DeflateError("reserved block type")
    if b.btype == 0:
        r.pos = (r.pos + 7) & ~7
        b.stored_len = r.take(16); b.stored_nlen = r.take(16)
        if b.stored_len ^ b.stored_nlen != 0xffff:
            raise DeflateError("stored block: NLEN is not the complement of LEN")
        b.stored_at = r.pos >> 3
        if r.pos + 8 * b.stored_len > len(r.bits):
            raise DeflateError("stored block: the stream ends inside it")
        for _ in range(b.stored_len):
            out.append(r.take(8))
        b.end_bit = r.pos
        return b
    if b.btype == 1:
        ll, d = Code(FIXED_LL, 9, "fixed lit/len"), Code(FIXED_D, 5, "fixed distance")
    else:
        b.hlit = r.take(5) + 257; b.hdist = r.take(5) + 1; b.hclen = r.take(4) + 4
        if b.hlit > 286 or b.hdist > 30:
            raise DeflateError("HLIT %d / HDIST %d beyond the alphabets" % (b.hlit, b.hdist))
        b.cl_lengths = [0] * 19
        for i in range(b.hclen):
            b.cl_lengths[CL_ORDER[i]] = r.take(3)
        cl = Code(b.cl_lengths, 7, "code-length code")
        lengths = []; b.header_seq = []
        total = b.hlit + b.hdist
        while len(lengths) < total:
            s = cl.decode(r)
            if s < 16:
                lengths.append(s); b.header_seq.append((s, 0))
                continue
            if s == 16:
                if not lengths:
                    raise DeflateError("repeat (16) with no length before it")
                n = 3 + r.take(2); v = lengths[-1]
            elif s == 17:
                n = 3 + r.take(3); v = 0
            else:
                n = 11 + r.take(7); v = 0
            if len(lengths) + n > total:
                raise DeflateError("a repeat runs past HLIT + HDIST")
            lengths += [v] * n; b.header_seq.append((s, n))
        b.ll_lengths = lengths[:b.hlit]; b.d_lengths = lengths[b.hlit:]
        if not b.ll_lengths[256]:
            raise DeflateError("no code for end-of-block")
        ll, d = Code(b.ll_lengths, 15, "lit/len code"), Code(b.d_lengths, 15, "distance code", allow="dist")
    while True:
        s = ll.decode(r)
        if s < 256:
            b.tokens.append(s); out.append(s)
            continue
        if s == 256:
            break
        if s > 285:
            raise DeflateError("lit/len symbol %d" % s)
        length = LEN_BASE[s - 257] + r.take(LEN_EXTRA[s - 257])
        if not d.max_len:
            raise DeflateError("a match in a block without a distance code")
        ds = d.decode(r)
        if ds > 29:
            raise DeflateError("distance symbol %d" % ds)
        dist = DIST_BASE[ds] + r.take(DIST_EXTRA[ds])
        if dist > len(out):
            raise DeflateError("distance %d with %d bytes produced" % (dist, len(out)))
        b.tokens.append((length, s, dist, ds))
        for _ in range(length):
            out.append(out[-dist])
    b.end_bit = r.pos
    return b


def read_stream(payload):
    """every block of a raw DEFLATE stream up to and including the final one: (blocks, the bytes they produce, the end bit position)"""
    r = Bits(payload); out = bytearray(); blocks = []
    while True:
        blocks.append(read_block(r, out))
        if blocks[-1].final:
            return blocks, bytes(out), r.pos


def replay(tokens, history=b""):
    """the bytes a token list stands for"""
    out = bytearray(history)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            for _ in range(t[0]):
                out.append(out[-t[2]])
    return bytes(out[len(history):])


# ---- what a Huffman code over a histogram has to look like

def huffman_lengths(counts):
    """{symbol: length} of an unrestricted Huffman code over the non-zero counts (heapq; ties by symbol).  One symbol: length 1."""
    used = [(c, s) for s, c in enumerate(counts) if c]
    if len(used) == 1:
        return {used[0][1]: 1}
    heap = [(c, s, (s,)) for c, s in used]
    heapq.heapify(heap)
    depth = {s: 0 for _, s in used}
    tie = len(counts)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for s in a[2] + b[2]:
            depth[s] += 1
        heapq.heappush(heap, (a[0] + b[0], tie, a[2] + b[2])); tie += 1
    return depth


def package_merge_lengths(counts, max_len):
    """{symbol: length} of an optimal code with no length above max_len (Larmore and Hirschberg's package-merge, the plain list form)"""
    used = sorted((c, s) for s, c in enumerate(counts) if c)
    n = len(used)
    if n == 1:
        return {used[0][1]: 1}
    assert n <= 1 << max_len
    leaves = [(c, (s,)) for c, s in used]
    prev = list(leaves)
    for _ in range(max_len - 1):
        packs = [(prev[i][0] + prev[i + 1][0], prev[i][1] + prev[i + 1][1]) for i in range(0, len(prev) - 1, 2)]
        prev = sorted(leaves + packs, key=lambda x: x[0])
    depth = {s: 0 for _, s in used}
    for _, syms in prev[:2 * n - 2]:
        for s in syms:
            depth[s] += 1
    return depth


def cost(counts, lengths):
    """sum of count * length; lengths: a list by symbol or a {symbol: length}"""
    get = lengths.get if isinstance(lengths, dict) else lambda s, d=0: lengths[s]
    return sum(c * get(s, 0) for s, c in enumerate(counts) if c)


def check_code_for_counts(counts, lengths, max_len, what, filler_ok=False, incomplete_single=False):
    """the properties a code (lengths by symbol) must have for a histogram: a code for every used symbol and for no other, no length above
    max_len, Kraft sum exactly 1, and never a longer code for a strictly larger count.  One used symbol: one bit -- with filler_ok the code
    may hold one more one-bit symbol of count zero (the code-length code, which must be complete); with incomplete_single it stands alone."""
    lengths = list(lengths) + [0] * (len(counts) - len(lengths))
    counts = list(counts) + [0] * (len(lengths) - len(counts))
    used = [s for s, c in enumerate(counts) if c]
    coded = [s for s, l in enumerate(lengths) if l]
    assert max(lengths, default=0) <= max_len, (what, max(lengths), max_len)
    if len(used) == 1:
        assert lengths[used[0]] == 1, (what, "one used symbol", lengths[used[0]])
        extra = [s for s in coded if s != used[0]]
        if filler_ok and extra:
            assert len(extra) == 1 and lengths[extra[0]] == 1, (what, "filler", extra)
        else:
            assert not extra and incomplete_single, (what, "one used symbol", coded)
        return
    assert coded == used, (what, "coded symbols are not the used ones", sorted(set(coded) ^ set(used)))
    if not used:
        return
    assert kraft(lengths, max_len) == 1 << max_len, (what, "Kraft sum", kraft(lengths, max_len), 1 << max_len)
    by_count = sorted(used, key=lambda s: counts[s])
    # the shortest code among the symbols of every strictly smaller count bounds the code of a larger count from above
    at = 0; shortest_so_far = None
    while at < len(by_count):
        c = counts[by_count[at]]; group = []
        while at < len(by_count) and counts[by_count[at]] == c:
            group.append(by_count[at]); at += 1
        if shortest_so_far is not None:
            bad = [s for s in group if lengths[s] > shortest_so_far]
            assert not bad, (what, "a larger count with a longer code", [(s, counts[s], lengths[s]) for s in bad], shortest_so_far)
        m = min(lengths[s] for s in group)
        shortest_so_far = m if shortest_so_far is None else min(shortest_so_far, m)


def greedy_header_seq(lengths):
    """the run-length coding of a dynamic block's lengths (lit/len followed by distance, as one list) that a greedy coder gives:
    zero runs: 18 for 11 and more in pieces of at most 138, 17 for what is left if 3..10, plain zeros below 3; a non-zero run: the length
    once, then 16 for 3..6 at a time, plain lengths for a rest below 3.  [(symbol, repeat)], repeat 0 for a plain length."""
    seq = []; i = 0
    while i < len(lengths):
        v = lengths[i]; run = 1
        while i + run < len(lengths) and lengths[i + run] == v:
            run += 1
        r = run
        if v == 0:
            while r >= 11:
                t = min(r, 138); seq.append((18, t)); r -= t
            if r >= 3:
                seq.append((17, r)); r = 0
        else:
            seq.append((v, 0)); r -= 1
            while r >= 3:
                t = min(r, 6); seq.append((16, t)); r -= t
        seq += [(v, 0)] * r
        i += run
    return seq


def header_runs(lengths):
    """[(value, run length)] of the maximal runs of equal values in a list of lengths"""
    runs = []
    for v in lengths:
        if runs and runs[-1][0] == v:
            runs[-1][1] += 1
        else:
            runs.append([v, 1])
    return [(v, n) for v, n in runs]
