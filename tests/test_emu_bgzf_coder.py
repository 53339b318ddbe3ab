"""The DEFLATE coder of snap_amd/csrc/bgzf.h held to the format path by path, on the wavefront emulator (tests/emu/).

Part one, the Huffman builder alone: bgzf_build_code has no entry of its own, so tests/emu/bgzf_coder_harness.cpp (a test kernel around it, in
a shared object of its own) runs it on histograms that no input of the compressor would produce, for the three alphabets it serves --
(286, 15), (30, 15), (19, 7).  Every code must be complete, within the limit, ordered by count and canonical; its cost is compared with the
package-merge optimum, and is Huffman's own where Huffman's depth is within the limit.

Part two, the whole coder: the cases of tests/bgzf_util.py that exist to reach one path each (every length and distance symbol, the window
edge, a match cut by the member's end, dynamic blocks of fewer than 64 tokens, CRC slices with empty lanes, the header's run-length edges,
the length limits), each asserting from the parsed stream (tests/deflate_util.py) that the path was reached.  tests/test_zz_gpu_bgzf_coder.py
runs the same functions on the GPU.

Test infrastructure only: see tests/test_emu_kernels.py for how the emulated library is swapped in."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

from tests import bgzf_util as bz
from tests import deflate_util as du

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ needed to build the wavefront emulator")

ALPHABETS = [(286, 15), (30, 15), (19, 7)]
# cost of the builder's code / cost of the package-merge optimum, the worst over the corpus below (DESIGN.md section 13 has the figures per
# alphabet), rounded up to the next 0.01
COST_CAP = {(286, 15): 1.01, (30, 15): 1.01, (19, 7): 1.12}
FIB = [1, 1]
while len(FIB) < 30:
    FIB.append(FIB[-1] + FIB[-2])                                            # (FIB[29] = 832 040: 286 of them stay far below 2^32, the routine's sums are 32-bit)


@pytest.fixture(scope="module")
def coder():
    from tests.emu.build import build_coder_harness
    lib = C.CDLL(build_coder_harness())
    lib.bgzf_coder_build.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32]
    lib.bgzf_coder_build.restype = C.c_int
    return lib


def build_codes(lib, hists, n_sym, max_len, blocks=4):
    f = np.ascontiguousarray(hists, dtype=np.uint32).reshape(-1, n_sym)
    out = np.full(f.shape, 0xdeadbeef, np.uint32)
    assert lib.bgzf_coder_build(f.ctypes.data, f.shape[0], n_sym, max_len, out.ctypes.data, blocks) == 0
    return out


def spread(values, n_sym, rng):
    """the values on randomly chosen symbols, the other counts zero"""
    h = np.zeros(n_sym, np.uint32)
    h[rng.permutation(n_sym)[:len(values)]] = values
    return h


def corpus(n_sym, max_len, n_random):
    """{name: [histograms]} for one alphabet"""
    rng = np.random.default_rng(1000 * n_sym + max_len)
    c = {}
    c["one_symbol"] = [spread([v], n_sym, rng) for v in (1, 7, 65281)] + [np.eye(n_sym, dtype=np.uint32)[s] for s in (0, n_sym - 1)]
    c["two_symbols"] = [spread(v, n_sym, rng) for v in ([1, 1], [1, 2], [1, 65280], [5, 5], [65280, 1])]
    c["equal"] = [np.full(n_sym, v, np.uint32) for v in (1, 3, 1000)]
    c["fibonacci"] = [spread([FIB[min(i, 29)] for i in range(n)], n_sym, rng) for n in range(max_len, n_sym + 1)]
    c["fibonacci_in_order"] = [np.array([FIB[min(i, 29)] if i < n else 0 for i in range(n_sym)], np.uint32) for n in range(max_len, n_sym + 1)]
    c["powers_of_two"] = [spread([1 << min(i, 20) for i in range(n)], n_sym, rng) for n in range(2, n_sym + 1, 1 if n_sym <= 30 else 7)] + \
                         [np.array([1 << min(i, 20) for i in range(n_sym)], np.uint32)[::-1].copy()]
    c["ones_and_one_huge"] = [spread([1 << 30] + [1] * (n - 1), n_sym, rng) for n in sorted({2, 3, max_len, max_len + 1, (1 << max_len) // 2 + 1, n_sym} & set(range(2, n_sym + 1)))]
    rnd = []
    for _ in range(n_random):
        n_used = int(rng.integers(2, n_sym + 1)) if rng.random() < 0.6 else int(rng.integers(2, min(n_sym, 24) + 1))
        kind = rng.integers(0, 4)
        if kind == 0:
            v = rng.integers(1, 100, n_used)                                   # flat
        elif kind == 1:
            v = np.ceil(rng.pareto(float(rng.uniform(0.3, 2.0)), n_used) * 3 + 1e-9).clip(1, 1 << 22)      # heavy tails
        elif kind == 2:
            ratio = float(rng.uniform(1.2, 2.2))                               # geometric around the golden ratio: where the limit binds
            v = np.ceil(ratio ** np.arange(n_used).clip(0, 40) * rng.uniform(0.7, 1.3, n_used)).clip(1, 1 << 22)
        else:
            v = rng.integers(1, 4, n_used) * (1 << rng.integers(0, 16, n_used))
        rnd.append(spread(np.asarray(v, np.uint64).astype(np.uint32), n_sym, rng))
    c["random"] = rnd
    return c


def check_code(counts, codes, n_sym, max_len):
    """one histogram's code table; returns (its cost, the package-merge cost), or None where fewer than two symbols are used"""
    counts = [int(v) for v in counts]; lengths = [int(v) & 255 for v in codes]; bits = [int(v) >> 8 for v in codes]
    used = [s for s, v in enumerate(counts) if v]
    if len(used) < 2:
        assert [int(v) for v in codes] == [1 if s in used else 0 for s in range(n_sym)]      # one bit, code 0
        return None
    du.check_code_for_counts(counts, lengths, max_len, "(%d, %d)" % (n_sym, max_len))
    for s, (c, l) in du.canonical_codes(lengths).items():
        assert bits[s] == int(format(c, "0%db" % l)[::-1], 2), (s, l, c, bits[s])      # sent from the most significant bit: stored reversed
    mine = du.cost(counts, lengths)
    best = du.cost(counts, du.package_merge_lengths(counts, max_len))
    assert mine >= best
    h = du.huffman_lengths(counts)
    if max(h.values()) <= max_len:
        assert mine == du.cost(counts, h) == best
    return mine, best


N_RANDOM = {(286, 15): 700, (30, 15): 2000, (19, 7): 3000}


@pytest.mark.parametrize("n_sym,max_len", ALPHABETS)
def test_builder_on_arbitrary_histograms(coder, n_sym, max_len):
    worst = 1.0; bound = 0; limited = 0
    for name, hists in corpus(n_sym, max_len, N_RANDOM[(n_sym, max_len)]).items():
        codes = build_codes(coder, np.stack(hists), n_sym, max_len)
        w = 1.0
        for h, c in zip(hists, codes):
            r = check_code(h, c, n_sym, max_len)
            if r:
                w = max(w, r[0] / r[1])
                limited += max(du.huffman_lengths([int(v) for v in h]).values()) > max_len
                bound += int((c & 255).max()) == max_len
        print("bgzf_build_code (%d, %d) %-20s %5d histograms, worst cost / package-merge %.6f" % (n_sym, max_len, name, len(hists), w))
        worst = max(worst, w)
    print("bgzf_build_code (%d, %d): worst %.6f; %d histograms deeper than the limit without it, %d codes reach it" % (n_sym, max_len, worst, limited, bound))
    assert limited >= 100 and bound >= limited                               # the fold-and-repair loop worked for its living
    assert worst <= COST_CAP[(n_sym, max_len)], worst


@pytest.fixture(scope="module")
def emu():
    import snap_amd.aligner as al
    from tests.emu.build import build
    path = build()
    saved = (al._lib, al.LIB_PATH)
    os.environ.setdefault("SNAPGPU_EMU_CUS", "4")
    al._lib, al.LIB_PATH = None, path
    try:
        yield al.load_library()
    finally:
        al._lib, al.LIB_PATH = saved


def test_emu_every_length_and_distance_symbol(emu, golden_index):
    bz.check_every_symbol(golden_index)


def test_emu_window_edge(emu, golden_index):
    bz.check_window_edge(golden_index)


def test_emu_match_cut_by_the_members_end(emu, golden_index):
    bz.check_cut_match(golden_index)


def test_emu_dynamic_blocks_of_fewer_than_64_tokens(emu, golden_index):
    bz.check_short_members(golden_index)


def test_emu_crc_slices(emu, golden_index):
    assert bz.check_crc_slices(golden_index) >= set(range(1, 201)) | {4095, 4096, 4097, 65279, 65280}


def test_emu_header_run_length_edges(emu, golden_index):
    bz.check_header_runs(golden_index)


def test_emu_code_length_code_limited_at_7(emu, golden_index):
    bz.check_code_length_code_limited(golden_index)


def test_emu_distance_code_limited_at_15(emu, golden_index):
    bz.check_distance_code_limited(golden_index)


def test_builder_is_the_same_on_every_wavefront(coder):
    """the same histograms on 1 and on 7 blocks: equal tables (the work area and the code table are per wave)"""
    hists = np.stack(corpus(30, 15, 50)["random"])
    assert (build_codes(coder, hists, 30, 15, 1) == build_codes(coder, hists, 30, 15, 7)).all()
    assert coder.bgzf_coder_build(None, 1, 30, 15, hists.ctypes.data, 1) == -1
