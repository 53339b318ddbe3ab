"""Search, on the wavefront emulator, for what tests/bgzf_util.py records for its path-reaching cases, and print it.  A seed or an input is
kept when the parsed stream (tests/deflate_util.py) shows that the case reached its path.

    python scripts/bgzf_find_inputs.py [symbols] [window] [cut] [distance] [crossing] [depths]

symbols, window, cut, distance: the first seed whose input reaches its path (SYMBOL_SEEDS, WINDOW_EDGE_SEED, CUT_SEED, DISTANCE_LIMIT_SEED).
crossing: the first fixture array whose first member has a repeat across the lit/len | distance boundary (check_header_runs names it).
depths: how deep a plain Huffman code over the parsed distance and code-length histograms of every case is -- a report, nothing to record.
The other inputs need no search: header_run_cases() and short_inputs() are written down from the format (which byte values are used decides
the zero runs, equal counts over a power of two of symbols the non-zero ones), and their checks assert the runs and token counts they reach.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import bgzf_util as bz                                        # noqa: E402
from tests import deflate_util as du                                     # noqa: E402
from tests import util                                                   # noqa: E402


def emulated():
    import snap_amd.aligner as al
    from tests.emu.build import build
    os.environ.setdefault("SNAPGPU_EMU_CUS", "4")
    al._lib, al.LIB_PATH = None, build()
    al.load_library()
    return bz.make_aligner(util.load_golden_index())


def find_symbols(a):
    seeds = []
    for m in range(len(bz.SYMBOL_SEEDS)):
        for seed in range(1000):
            data, pairs = bz.symbols_member(m, seed)
            b, = bz.compress_members(a, data)
            got = {(t[2], t[0]) for t in b.matches()}
            if all(p in got for p in pairs):
                seeds.append(seed)
                break
        else:
            raise SystemExit("member %d: no seed" % m)
    print("SYMBOL_SEEDS =", tuple(seeds))


def find_seed(name, check, index, tries=50):
    for seed in range(tries):
        try:
            check(index, seed)
        except AssertionError as e:
            print("%s: seed %d: %s" % (name, seed, str(e)[:200]))
            continue
        print("%s = %d" % (name, seed))
        return
    raise SystemExit(name + ": no seed")


def find_crossing(a):
    for tag, data in sorted(bz.fixture_arrays().items()):
        b, = bz.compress_members(a, data[:bz.MAX_BLOCK])
        if b.btype == 2 and bz.spans_boundary(b):
            print('crossing: fixture_arrays()["%s"][:MAX_BLOCK]: %s, lengths %s | %s' % (tag, bz.spans_boundary(b), b.ll_lengths[-3:], b.d_lengths[:3]))
            return
    raise SystemExit("crossing: no fixture array has one")


def depth(counts):
    return max(du.huffman_lengths(counts).values()) if sum(1 for c in counts if c) > 1 else 1


def report_depths(a):
    cases = dict(bz.header_run_cases())
    cases.update({"fib24": bz.fibonacci_input(24, 6)[:bz.MAX_BLOCK], "window": bz.window_input(), "distance_limit": bz.distance_limit_input()[0]})
    cases.update({"symbols%d" % m: bz.symbols_member(m, s)[0] for m, s in enumerate(bz.SYMBOL_SEEDS)})
    cases.update({"fixture_" + k: v[:bz.MAX_BLOCK] for k, v in bz.fixture_arrays().items()})
    for name, data in cases.items():
        b, = bz.compress_members(a, data)
        if b.btype != 2:
            continue
        d = [0] * 30; cl = [0] * 19
        for t in b.matches():
            d[t[3]] += 1
        for s, _ in b.header_seq:
            cl[s] += 1
        print("%-32s distance: %5d matches, %2d symbols, Huffman depth %2d, sent max %2d | code-length: %3d entries, %2d symbols, depth %2d, sent max %d"
              % (name, sum(d), sum(1 for c in d if c), depth(d), max(b.d_lengths), sum(cl), sum(1 for c in cl if c), depth(cl), max(b.cl_lengths)))


if __name__ == "__main__":
    what = sys.argv[1:] or ["symbols", "window", "cut", "distance", "crossing", "depths"]
    a = emulated()
    ix = util.load_golden_index()
    try:
        if "symbols" in what:
            find_symbols(a)
        if "window" in what:
            find_seed("WINDOW_EDGE_SEED", bz.check_window_edge, ix)
        if "cut" in what:
            find_seed("CUT_SEED", bz.check_cut_match, ix)
        if "distance" in what:
            find_seed("DISTANCE_LIMIT_SEED", bz.check_distance_code_limited, ix)
        if "crossing" in what:
            find_crossing(a)
        if "depths" in what:
            report_depths(a)
    finally:
        a.close()
