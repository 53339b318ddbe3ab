"""Generate tests/golden/ag_forms.npz with the compiled reference (oracle/_ref): affine-gap problems at the edges where the dispatcher of
snap_amd/csrc/ag_win.h decides which FUNCTION takes a call -- ag_hot_fn (the two forms of ag_banded_win) or ag_cold_fn (every other form):

  * band half-widths 12, 13, 15 | 16: segLen 32 (two segments fit one wavefront: hot) against segLen 40 (cold);
  * unbanded patterns of 64 | 65 positions (one segment of 64 lanes: hot) and shorter ones;
  * gap-open penalty 1 (the smallest the library accepts: 0, the v1 form, is refused at context creation) and the default 6;
  * patterns shorter than one segment; texts that end before the band has reached the pattern's end;
  * lazy-F walks that end in each of rounds 0 .. 6 of either segment: candidates with long gaps are run one by one through the wavefront
    emulator's counting build (-DSNAPGPU_AG_WIN_STATS: g_agwin_stats[16 + s * 8 + r] counts the rounds run) and kept, per segment and round,
    where walks ending in that round are the largest share; `walk_ends` [problem, segment, round] records the count for every problem.

Per gap-open value g and direction d the fixture holds the reference's answers twice: "alone" (every call on a newly constructed object:
what the ordinary batch entry must give wherever the traceback stays inside the band) and "seq" (the calls in order on ONE new object: what
the exact, image-keeping entry must give everywhere).  `stale` marks the calls whose traceback leaves the band (C restatement's count)."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np                                     # noqa: E402
import tests.emu.build as eb                           # noqa: E402
from oracle import ref                                 # noqa: E402
from tests import util                                 # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "ag_forms.npz")
# (A ZERO gap-open penalty -- the v1 form -- cannot be asked for: the library, like the reference (BaseAligner.cpp:141), requires
#  gapExtend < subPenalty <= gapOpen + gapExtend, which no subPenalty meets at gapOpen 0.  1 is the smallest penalty there is.)
GAP_OPENS = (1, 6)
SUB_PENALTY = {1: 2, 6: 4}
ACGT = np.frombuffer(b"ACGT", np.uint8)


def mutate(rng, pat, n_sub, gaps):
    """A text for `pat`: n_sub substitutions, then gaps = [(position, length)]: length > 0 inserts text bases, < 0 deletes them."""
    t = bytearray(pat)
    for _ in range(n_sub):
        i = int(rng.integers(0, len(t)))
        t[i] = int(ACGT[(b"ACGT".index(bytes([t[i]])) + 1 + int(rng.integers(0, 3))) % 4])
    for pos, ln in sorted(gaps, reverse=True):
        pos = min(pos, len(t))
        if ln > 0:
            t[pos:pos] = bytes(ACGT[rng.integers(0, 4, size=ln)])
        else:
            del t[pos:pos - ln]
    return bytes(t)


def problem(rng, plen, w, banded, n_sub=2, gaps=(), tail=None, tlen=None, n_frac=0.0):
    pat = bytes(ACGT[rng.integers(0, 4, size=plen)])
    text = mutate(rng, pat, n_sub, list(gaps))
    text += bytes(ACGT[rng.integers(0, 4, size=(w if tail is None else tail))])
    if tlen is not None:
        text = text[:tlen]
    if n_frac:
        tb = bytearray(text)
        for i in range(len(tb)):
            if rng.random() < n_frac: tb[i] = ord("N")
        text = bytes(tb)
    text = text[:160] or b"A"
    qual = bytes(rng.integers(35, 74, size=plen, dtype=np.uint8))
    # (a cut text: no soft clipping -- its extension step compares text bases beyond the best cell, past the text's end, i.e. whatever lies next in memory)
    return dict(text=text, pat=pat, qual=qual, w=w, si=int(rng.integers(20, 160)), rc=int(rng.integers(0, 2)), banded=int(banded),
                clip=int(rng.integers(0, 3)) if tlen is None else 0)


def edge_problems(rng):
    out = []
    for w in (12, 13, 15, 16):                                   # segLen 32, 32, 32 | 40
        for plen in (99, 100, 128, 150):
            out.append(problem(rng, plen, w, True))
            out.append(problem(rng, plen, w, True, n_sub=4, gaps=[(plen // 2, 3)]))
            out.append(problem(rng, plen, w, True, n_sub=1, gaps=[(plen // 3, -4)]))
        out.append(problem(rng, 150, w, True, n_sub=12, n_frac=0.03))
    for plen in (1, 5, 8, 9, 31, 33, 63, 64, 65, 72):            # unbanded: one segment of <= 64 lanes | more
        out.append(problem(rng, plen, 8, False, n_sub=min(2, plen // 8)))
        out.append(problem(rng, plen, 12, False, n_sub=1, gaps=[(plen // 2, 2)] if plen > 8 else ()))
        out.append(problem(rng, plen, 12, False, n_sub=1, gaps=[(plen // 2, -2)] if plen > 8 else ()))
    for plen in (7, 10, 20, 24, 25, 30):                         # banded, pattern shorter than one segment (band = min(2w + 1, pattern))
        for w in (8, 12):
            out.append(problem(rng, plen, w, True, n_sub=1))
    for plen, w in ((150, 8), (150, 12), (128, 15), (100, 4), (64, 12)):      # the text ends the band early
        for tlen in (1, w // 2 + 1, w + 3, plen // 3, plen - w - 2, plen - 1):
            out.append(problem(rng, plen, w, plen >= 3 * (2 * w + 1), tlen=tlen))
    for w in (0, 1, 3, 8):                                       # narrow bands: num_vec 1, 2
        out.append(problem(rng, 120, w, True, n_sub=3, gaps=[(50, min(w, 2))] if w else ()))
    return out


def gap_candidates(rng, n):
    """Long gaps on either side, high starting scores, gaps late in the band's second segment: what makes a lazy-F walk go on."""
    out = []
    for _ in range(n):
        w = int(rng.choice((8, 12, 15)))
        banded = rng.random() < 0.75
        plen = int(rng.integers(100, 151)) if banded else int(rng.integers(24, 65))
        ng = int(rng.integers(1, 4))
        gaps = [(int(rng.integers(2, plen - 2)), int(rng.integers(1, w + 1)) * (1 if rng.random() < 0.5 else -1)) for _ in range(ng)]
        p = problem(rng, plen, w, banded, n_sub=int(rng.integers(0, 6)), gaps=gaps)
        p["si"] = int(rng.integers(60, 200))
        out.append(p)
    return out


def walk_ends(probs):
    """int32 [len(probs), 2, 7]: how many rows of problem i end their lazy-F walk of segment s in round r on the emulated device (both directions,
    every gap-open value).  The counting build of the emulator goes to a temporary directory; tests.emu.build is left as it was found."""
    import tempfile
    saved = (eb.BDIR, eb.LIB, list(eb.FLAGS), eb.units)
    ends = np.zeros((len(probs), 2, 7), np.int32)
    import snap_amd.aligner as al
    saved_al = (al._lib, al.LIB_PATH)
    with tempfile.TemporaryDirectory(prefix="snapgpu_emu_agforms") as bdir:
        try:
            eb.BDIR, eb.LIB = bdir, os.path.join(bdir, os.path.basename(eb.LIB))
            stats_src = os.path.join(bdir, "stats.cpp")
            with open(stats_src, "w") as f:
                f.write("unsigned long long g_emu_stats[64]; unsigned long long g_agwin_stats[64]; unsigned long long g_agform_stats[64];\n")
            eb.FLAGS.append("-DSNAPGPU_AG_WIN_STATS")
            base_units = eb.units
            eb.units = lambda: base_units() + [("stats.o", stats_src, [])]
            lib_path = eb.build(verbose=True)
            al._lib, al.LIB_PATH = None, lib_path
            from snap_amd import abi
            from snap_amd.aligner import BaseAligner
            h = C.CDLL(lib_path)
            ag = (C.c_ulonglong * 64).in_dll(h, "g_agwin_stats")
            ix = util.load_golden_index()
            for g in GAP_OPENS:
                a = BaseAligner(ix, abi.default_params(max_k=8, max_read_len=160, gap_open_penalty=g, sub_penalty=SUB_PENALTY[g]))
                for i, c in enumerate(probs):
                    for d in (1, -1):
                        before = list(ag)
                        a.computeScoreAffine(d, [c["text"] if d == 1 else c["text"][::-1]], [c["pat"]], [c["qual"]], [c["w"]], [c["si"]], [c["rc"]], [c["banded"]], [c["clip"]])
                        for s in (0, 1):
                            ran = [ag[16 + s * 8 + r] - before[16 + s * 8 + r] for r in range(7)] + [0]      # rows that ran round r: a walk ends in r where fewer ran r + 1
                            for r in range(7):
                                ends[i, s, r] += max(0, ran[r] - ran[r + 1])
                a.close()
        finally:
            eb.BDIR, eb.LIB, eb.units = saved[0], saved[1], saved[3]
            eb.FLAGS[:] = saved[2]
            al._lib, al.LIB_PATH = saved_al
    return ends


def main():
    rng = np.random.default_rng(20261019)
    probs = edge_problems(rng)
    cands = gap_candidates(rng, 600)
    ends = walk_ends(probs + cands)
    n_edge = len(probs)
    cend = ends[n_edge:]
    # per (segment, round): the candidates in which walks ending in THAT round are the largest share of the segment's walks -- problems that differ by round
    picked = []
    for s in (0, 1):
        tot = np.maximum(cend[:, s, :].sum(axis=1), 1)
        for r in range(7):
            share = cend[:, s, r] / tot
            order = [int(i) for i in np.argsort(-share, kind="stable") if cend[i, s, r] > 0 and int(i) not in picked]
            assert order, "no walk of segment %d ends in round %d: widen gap_candidates" % (s, r)
            picked += order[:6]
    print("rows of the picked problems whose walk ends in round r (segment 0 | segment 1):", cend[picked, 0, :].sum(axis=0).tolist(), cend[picked, 1, :].sum(axis=0).tolist())
    probs += [cands[i] for i in picked]
    n = len(probs)
    out = {"n_edge": np.int32(n_edge), "gap_opens": np.array(GAP_OPENS, np.int32), "sub_penalties": np.array([SUB_PENALTY[g] for g in GAP_OPENS], np.int32),
           "walk_ends": np.concatenate([ends[:n_edge], cend[picked]]).astype(np.int32)}
    for k, key in (("text", "texts"), ("pat", "pats"), ("qual", "quals")):
        out[key] = np.array([p[k] for p in probs], dtype=object)
    for k, key, dt in (("w", "w", np.int32), ("si", "si", np.int32), ("rc", "rc", np.uint8), ("banded", "banded", np.uint8), ("clip", "clip", np.uint8)):
        out[key] = np.array([p[k] for p in probs], dt)
    for g in GAP_OPENS:
        agp = (1, SUB_PENALTY[g], g, 1, 10, 7)
        for d in (1, -1):
            tt = [t if d == 1 else t[::-1] for t in out["texts"]]
            with ref.fresh_objects():
                seq = ref.affine_gap(d, tt, list(out["pats"]), list(out["quals"]), out["w"], out["si"], out["rc"], out["banded"], out["clip"], agparams=agp)
            alone = {k: np.zeros_like(v) for k, v in seq.items()}
            stale = np.zeros(n, bool)
            for i in range(n):
                with ref.fresh_objects():
                    r = ref.affine_gap(d, [tt[i]], [out["pats"][i]], [out["quals"][i]], [out["w"][i]], [out["si"][i]], [out["rc"][i]], [out["banded"][i]],
                                       [out["clip"][i]], agparams=agp)
                for k in alone: alone[k][i] = r[k][0]
                stale[i] = util.oracle_ag(d, out["banded"][i], tt[i], out["pats"][i], out["quals"][i], out["w"][i], out["si"][i], out["rc"][i],
                                          out["clip"][i], params=agp)["stale_reads"] != 0
            for k in seq:
                out["g%d%+d_seq_%s" % (g, d, k)] = seq[k]
                out["g%d%+d_alone_%s" % (g, d, k)] = alone[k]
            out["g%d%+d_stale" % (g, d)] = stale
            print("gap open", g, "direction", d, "problems", n, "leave the band:", int(stale.sum()), "aligned:", int((alone["ag_score"] != -1).sum()))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
