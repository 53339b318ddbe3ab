"""Generate tests/golden/lv_forms.npz with the compiled reference (oracle/_ref: LandauVishkin<1> and <-1>): Landau-Vishkin problems at the
edges of snap_amd/csrc/lv.h that tests/golden/primitives.npz does not reach --

  * pattern lengths on both sides of every mask-word count up to 16 words, limits on both sides of level 32 (the second pass of the
    diagonal loop) up to the clamp at 126;
  * answers of 32 and 64 edits and more, a limit equal to the answer and one below it, net indels beyond 33 in either sign (a winning
    diagonal of rank 64 and more), an 'X' cell that wins over an indel cell of lower rank, several indel cells that reach the end;
  * texts shorter than the pattern, the all-match prefix with its trailing deletions; alignments that begin with indels at offset 0;
  * runs of equal actions, adjacent unlike actions, edits at the first and the last pattern position; mismatches at mask-word boundaries,
    matching runs over whole words; N in either sequence; the whole range of quality bytes; k = 126 on 1000 bases.

tests/lv_forms_util.py: fixture_covers_the_edges() states each class as a condition on the fixture and LENGTHS / LIMITS / group_of.

Reference determinism: the reference compares *p == *t before it looks at the end of either sequence (LandauVishkin.h:200, 211, 226), so
what lies beside a sequence is read.  Every sequence is laid out with GUARD bytes on both sides, texts and patterns with different guard
values that occur in no sequence, and the offsets go to snapref_landau_vishkin as they are; the reference runs twice with two pairs of
guard values and a problem is kept only where both runs agree in every field and direction."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np                                     # noqa: E402
from oracle import ref                                 # noqa: E402
from tests import lv_forms_util as fu                  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "lv_forms.npz")
GUARDS = ((0x6e, 0x4f), (0x23, 0x2a))                  # (text guard, pattern guard): 'n' / 'O', '#' / '*'
ACGT = b"ACGT"


class Gen:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.genome = bytes(np.frombuffer(ACGT, np.uint8)[self.rng.integers(0, 4, size=60000)])
        self.probs = []

    def other(self, c):
        return ACGT[(ACGT.index(c) + 1 + int(self.rng.integers(0, 3))) % 4] if c in ACGT else ACGT[0]

    def bases(self, n, alphabet=ACGT):
        return bytes(np.frombuffer(alphabet, np.uint8)[self.rng.integers(0, len(alphabet), size=n)])

    def window(self, n):
        s = int(self.rng.integers(0, len(self.genome) - n))
        return self.genome[s:s + n]

    def add(self, cls, plen, k, edits=(), extra=127, tlen=None, src=None, n_pat=(), n_text=(), alphabet=None):
        """A pattern of plen bases read off a text with planted edits [(text position, 'X' | 'I' | 'D', length)] ('I': bases the pattern has
        and the text has not; 'D': text bases the pattern skips), and the text cut to plen + extra (or tlen) bases."""
        src = src if src is not None else (self.window(plen + 400) if alphabet is None else self.bases(plen + 400, alphabet))
        out, ti = bytearray(), 0
        for pos, kind, ln in sorted(edits, key=lambda e: e[0]):           # (edits at one position in the caller's order)
            if pos < ti: continue
            out += src[ti:pos]; ti = pos
            if kind == "X":
                for _ in range(ln): out.append(self.other(src[ti])); ti += 1
            elif kind == "I":
                ins = bytearray(self.bases(ln))
                ins[-1] = self.other(src[ti])              # (an inserted base equal to the next text base would shift the insertion)
                out += ins
            else:
                ti += ln
        out += src[ti:]
        pat = bytearray(out[:plen])
        assert len(pat) == plen
        text = bytearray(src[:plen + extra if tlen is None else tlen])
        for j in n_pat: pat[j] = ord("N")
        for j in n_text: text[j] = ord("N")
        qual = bytes(self.rng.integers(33, 127, size=plen, dtype=np.uint8))
        self.probs.append(dict(cls=cls, text=bytes(text), pat=bytes(pat), qual=qual, k=int(k)))
        return self.probs[-1]

    def spread(self, plen, n, lo=0, hi=None):
        """n distinct text positions in [lo, hi), at least two apart."""
        hi = plen if hi is None else hi
        pos = self.rng.choice(np.arange(lo, hi, 2), size=n, replace=False)
        return sorted(int(p) for p in pos)


def reference(probs, guards):
    texts, pats, quals, k = [p["text"] for p in probs], [p["pat"] for p in probs], [p["qual"] for p in probs], [p["k"] for p in probs]
    out = {}
    for d in (1, -1):
        rc, out[d] = fu.lv_call(ref.lib().snapref_landau_vishkin, None, d, texts, pats, quals, k, text_guard=guards[0], pat_guard=guards[1])
        assert rc == 0
    return out


def score_of(g, p):
    return int(reference([dict(p, k=126)], GUARDS[0])[1]["score"][0])


def twins(g, cls, p, deltas=(-1, 0)):
    """The problem again with limits around its answer: one edit too many (answer - 1), exactly enough, ..."""
    s = score_of(g, p)
    assert s > 0, (cls, s)
    g.probs.pop()
    for dk in deltas:
        g.probs.append(dict(p, cls=cls, k=s + dk))
    return s


def build(g):
    rng = g.rng
    # ---- lengths x limits: a few edits, every limit at several lengths and every length below and above its answer
    lim = list(fu.LIMITS)
    for li, plen in enumerate(fu.LENGTHS):
        for j in range(7):
            k = lim[(li * 5 + j * 3) % len(lim)]
            if plen >= 959 and k > 100: k = 60                                   # (k above 100 on 15 and 16 words is the largest working set, below)
            n_e = 0 if plen <= 2 and j % 2 else int(rng.integers(1, 5))
            n_e = min(n_e, plen)
            edits = [(p, "X", 1) for p in g.spread(plen, n_e)] if plen > 8 else [(p, "X", 1) for p in range(n_e)]
            if plen > 8 and j % 3 == 2:
                p0 = int(rng.integers(1, plen - 2))
                edits = [e for e in edits if abs(e[0] - p0) > 3] + [(p0, "ID"[j % 2], int(rng.integers(1, 3)))]
            g.add("grid", plen, k, edits, extra=int(rng.choice((0, 1, 40, 127))) if j % 3 != 2 else 127)
        if plen > 2:
            p = g.add("grid", plen, 126, [(q, "X", 1) for q in g.spread(plen, 3 if plen < 100 else 5)])
            twins(g, "grid_twin", p)
    for k in (64, 100, 126, 127, 200):                                           # the high limits on one, two and eight mask words, answered early
        for plen in (40, 150, 512):
            g.add("grid_high_k", plen, k, [(p, "X", 1) for p in g.spread(plen, 3)] + ([(plen // 2, "D", 2)] if k % 2 else []))
    # ---- depth
    for plen, n_sub in ((150, 31), (150, 32), (150, 33), (250, 34), (250, 40), (250, 47), (250, 63), (250, 64), (250, 65), (400, 70), (250, 100), (512, 125)):
        p = g.add("deep_subs", plen, 126, [(q, "X", 1) for q in g.spread(plen, n_sub)])
        twins(g, "deep_subs", p, deltas=(-1, 0, 1) if n_sub in (32, 33, 64) else (-1, 0))
    for n_sub in (3, 8):
        p = g.add("deep_subs", 100, 126, [(q, "X", 1) for q in g.spread(100, n_sub)])
        twins(g, "deep_subs", p)
    for plen in (150, 250):
        for kind in "ID":
            for ln, k in ((33, 33), (34, 48), (40, 60), (45, 63), (50, 64)):
                g.add("deep_indel", plen, k, [(plen // 3, kind, ln)])
                g.add("deep_indel", plen, k + 3, [(plen // 3, kind, ln), (plen // 3 + ln + 20, "X", 1), (plen - 9, "X", 2)])
            g.add("deep_indel", plen, 60, [(20, kind, 12), (60, kind, 11), (100, kind, 12)])      # several indels adding up to 35
            g.add("deep_indel", plen, 126, [(20, kind, 30), (80, kind, 25), (120, "X", 3)])
    # an 'X' cell at a higher rank than an indel cell of the same level: a deletion, then a substitution at the last base (the insertion from
    # the next diagonal reaches the end as well, at a lower rank) -- one base deleted (rank 1 over rank 0) up to 33 (rank 65, the second pass, over rank 63)
    for plen in (30, 100, 150):
        for ln in (1, 2, 5, 33, 34):
            g.add("x_over_indel", plen, ln + 1 if plen == 30 else 60, [(plen // 2, "D", ln), (plen // 2 + ln + (plen - 1 - plen // 2), "X", 1)])
            g.add("x_over_indel", plen, ln + 8, [(plen // 2, "I", ln), (plen - 1 - ln, "X", 1)])
    for ln in (33,):
        g.add("x_over_indel", 250, 60, [(125, "D", ln), (249 + ln, "X", 1)])
    # several indel cells of one level reach the end and the smallest |d| wins: the text ends in a repeat of period two and the pattern skips one
    # base of it, so the deletion (d + 1) and the insertion (d - 1) both run to the end -- after no other edit (ranks 1 and 2), after 31 and 32
    # substitutions (levels 32 and 33), after 32 deleted or inserted bases (ranks 61 and 65: one cell in either pass of the diagonal loop)
    for plen, pre, shift in ((20, [], 0), (70, [], 0), (70, [(5, "X", 1)], 0), (150, None, 0), (150, None, 0), (150, [(10, "D", 32)], 32), (150, [(10, "I", 32)], -32),
                             (250, [(10, "D", 40), (90, "X", 1)], 40)):
        start = plen - 14 + shift
        if pre is None: pre = [(q, "X", 1) for q in g.spread(plen, 31 + len(g.probs) % 2, hi=start - 2)]
        g.add("indel_cells", plen, 60, pre + [(start + 4, "D", 1)], src=g.window(start) + b"AC" * 300)
        g.add("indel_cells", plen, 60, pre + [(start + 5, "I", 1)], src=g.window(start) + b"AC" * 300)
    # ---- low-complexity sequences, many edits: ties between cells of a level (several indel cells reach the end; 'X' over indel)
    for _ in range(70):
        plen = int(rng.integers(8, 60))
        src = g.bases(plen + 400, alphabet=(b"AC", b"A", b"ACG", b"AAC")[int(rng.integers(0, 4))])
        n_e = int(rng.integers(1, 6))
        edits = [(int(rng.integers(0, plen)), "XID"[int(rng.integers(0, 3))], int(rng.integers(1, 4))) for _ in range(n_e)]
        g.add("ties", plen, int(rng.choice((3, 8, 31, 32, 33))), edits, src=src, extra=int(rng.choice((0, 1, 5, 127))))
    # ---- short texts, limits on both sides of the missing tail; the all-match prefix
    for plen in (20, 150, 401):
        for delta in (-5, -1, 0, 1):
            for variant in range(3):
                edits = [] if variant == 0 else [(plen // 2, "X", 1)] if variant == 1 else [(plen // 3, "X", 1), (2 * plen // 3, "ID"[plen % 2], 2)]
                need = max(0, -delta) + (0, 1, 3)[variant]
                for k in sorted({max(need - 1, 0) if need else 0, need, need + 3}):
                    g.add("short_text", plen, k, edits, tlen=plen + delta)
            g.add("short_text", plen, 8, [(plen - 3, "X", 1)], tlen=plen + delta)          # an edit inside the tail region
            g.add("short_text", plen, 4, [(q, "X", 1) for q in g.spread(plen, 6)], tlen=plen + delta)
    for plen, cut in ((65, 1), (129, 5), (513, 64), (1000, 60), (2, 1), (150, 40)):      # the all-match prefix alone, longer missing tails
        for k in (cut - 1, cut, 126):
            g.add("prefix", plen, k, [], tlen=plen - cut)
    # ---- alignments that begin with indels at offset 0 (text before its start); edits at the first and the last position
    for plen in (30, 100, 150):
        for ln in (1, 2, 3, 5):
            g.add("lead", plen, 8, [(0, "I", ln)])
            g.add("lead", plen, 8, [(0, "D", ln)])
            g.add("lead", plen, 8, [(0, "D", ln), (ln, "X", 1)])
            g.add("lead", plen, 8, [(0, "I", ln), (1, "X", 1)])
        g.add("ends", plen, 3, [(0, "X", 1)])
        g.add("ends", plen, 3, [(plen - 1, "X", 1)])
        g.add("ends", plen, 8, [(0, "X", 3), (plen - 3, "X", 3)])
        g.add("ends", plen, 8, [(0, "X", 1), (plen // 2, "D", 2), (plen + 1, "X", 1)])
        g.add("ends", plen, 8, [(3, "D", 3), (8, "X", 1)])                                 # offset below zero at a substitution: the qi clamp
        g.add("ends", plen, 8, [(0, "D", 4), (4, "X", 2)])
    # ---- runs of equal actions, unlike actions side by side
    for plen in (40, 130):
        for at in (5, plen // 2, plen - 12):
            for ln in (3, 4, 7):
                for kind in "XID":
                    g.add("runs", plen, 31 if kind == "X" else 32, [(at, kind, ln)])
            g.add("runs", plen, 33, [(at, "X", 2), (at + 2, "I", 2)])
            g.add("runs", plen, 33, [(at, "I", 2), (at, "X", 2)])
            g.add("runs", plen, 33, [(at, "X", 2), (at + 2, "D", 3)])
            g.add("runs", plen, 33, [(at, "D", 2), (at + 2, "X", 2)])
            g.add("runs", plen, 33, [(at, "I", 3), (at, "D", 2)])
    for _ in range(40):                                                                    # clustered random edits
        plen = int(rng.integers(30, 200))
        c = int(rng.integers(0, plen - 10))
        edits = [(c + int(rng.integers(0, 10)), "XID"[int(rng.integers(0, 3))], int(rng.integers(1, 4))) for _ in range(int(rng.integers(3, 9)))]
        edits += [(int(rng.integers(0, plen)), "X", 1) for _ in range(int(rng.integers(0, 12)))]
        g.add("dense", plen, int(rng.choice((31, 32, 33, 48, 60))), edits)
    # ---- mask-word boundaries
    for pos in fu.WORD_EDGES:
        for plen in ((200, 1000) if pos < 200 else (960, 1000)):
            g.add("words", plen, 3, [(pos, "X", 1)])
            g.add("words", plen, 8, [(5, "X", 1), (pos, "X", 1)])
            g.add("words", plen, 8, [(pos - 1, "X", 1), (pos, "X", 1), (pos + 1, "X", 1)] if pos + 1 < plen else [(pos - 1, "X", 2)])
            g.add("words", plen, 8, [(7, "D", 1), (pos, "X", 1)])
            g.add("words", plen, 8, [(7, "I", 1), (pos, "X", 1)])
    for plen in (400, 1000):
        g.add("words", plen, 3, [(10, "X", 1), (plen - 40, "X", 1)])                      # matching runs over whole words
        g.add("words", plen, 3, [(10, "X", 1)])
        g.add("words", plen, 8, [(3, "I", 2), (plen - 70, "D", 3)])
    # ---- N
    for plen in (50, 151):
        for j in (0, 7, plen - 1):
            g.add("alphabet", plen, 3, [(20, "X", 1)], n_pat=[j])
            g.add("alphabet", plen, 3, [(20, "X", 1)], n_text=[j])
            g.add("alphabet", plen, 3, [(20, "X", 1)], n_pat=[j], n_text=[j])
        g.add("alphabet", plen, 8, [(15, "D", 2)], n_pat=[30, 31], n_text=[31, 32, 33])
    # ---- the largest working set: k = 126 on 1000 bases
    p = g.add("largest", 1000, 126, [(q, "X", 1) for q in g.spread(1000, 70)])
    g.add("largest", 1000, 126, [(q, "X", 1) for q in g.spread(1000, 90, lo=100)] + [(30, "D", 10), (60, "I", 6)])
    g.add("largest", 1000, 126, [(q, "X", 1) for q in g.spread(1000, 135)])               # not found within 126
    g.add("largest", 1000, 126, [(500, "X", 1)])
    g.add("largest", 960, 126, [(q, "X", 1) for q in g.spread(960, 20)])
    g.add("largest", 959, 127, [(q, "X", 1) for q in g.spread(959, 4)])
    g.add("largest", 1000, 200, [(q, "X", 1) for q in g.spread(1000, 4)] + [(700, "I", 35)])


def main():
    g = Gen(20261020)
    build(g)
    probs = g.probs
    a, b = reference(probs, GUARDS[0]), reference(probs, GUARDS[1])
    keep = np.ones(len(probs), bool)
    for d in (1, -1):
        for f in fu.FIELDS:
            x, y = a[d][f], b[d][f]
            if f == "match_probability": x, y = x.view(np.uint64), y.view(np.uint64)
            keep &= x == y
    classes = sorted(set(p["cls"] for p in probs))
    dropped = int((~keep).sum())
    print("problems generated:", len(probs), "dropped because the reference's answer depends on the guard bytes:", dropped)
    assert dropped <= 0.02 * len(probs), dropped
    for c in classes:
        assert any(k for p, k in zip(probs, keep) if p["cls"] == c), "class %s lost all its members" % c
    probs = [p for p, k in zip(probs, keep) if k]
    n = len(probs)
    out = {"cls": np.array([p["cls"] for p in probs]), "k": np.array([p["k"] for p in probs], np.int32),
           "group": np.array([fu.group_of(len(p["pat"]), p["k"]) for p in probs], np.int32)}
    for key, name in (("text", "texts"), ("pat", "pats"), ("qual", "quals")):
        arr = np.empty(n, dtype=object)
        arr[:] = [p[key] for p in probs]
        out[name] = arr
    for d in (1, -1):
        for f in fu.FIELDS:
            out["lv%+d_%s" % (d, f)] = a[d][f][keep]
    assert all((out["lv+1_" + f] == out["lv-1_" + f]).all() for f in fu.FIELDS)           # one problem, walked in either direction
    sc = out["lv+1_score"]
    print("classes:", {c: int((out["cls"] == c).sum()) for c in classes})
    print("n", n, "k >= 64:", int((out["k"] >= 64).sum()), "score >= 32:", int((sc >= 32).sum()), "score >= 64:", int((sc >= 64).sum()),
          "not found:", int((sc == -1).sum()), "groups:", len(set(out["group"].tolist())))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
