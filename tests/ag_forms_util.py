"""Shared by tests/test_emu_ag_forms.py and tests/test_zz_gpu_ag_forms.py: tests/golden/ag_forms.npz (scripts/make_golden_ag_forms.py, answers of
the compiled reference) through the batch entries of the affine-gap primitive -- the problems sit at the edges where ag_win.h's dispatcher
decides between ag_hot_fn and ag_cold_fn, and at lazy-F walks ending in each round."""
import os

import numpy as np

from snap_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("ag_score", "text_offset", "pattern_offset", "n_edits", "match_probability")
_fixture = None


def fixture():
    global _fixture
    if _fixture is None:
        _fixture = np.load(os.path.join(ROOT, "tests", "golden", "ag_forms.npz"), allow_pickle=True)
    return _fixture


def check_gap_open(index, g, **aligner_kw):
    """Both text directions, the ordinary entry (every call on an object of its own) and the exact one (the calls in order on one object): every
    field of every aligned problem against the reference's.  Returns (compared ordinary, compared exact)."""
    from snap_amd.aligner import BaseAligner
    z = fixture()
    assert g in z["gap_opens"].tolist()
    texts, pats, quals = list(z["texts"]), list(z["pats"]), list(z["quals"])
    sub = int(z["sub_penalties"][z["gap_opens"].tolist().index(g)])          # (the aligner requires subPenalty <= gapOpen + gapExtend)
    a = BaseAligner(index, abi.default_params(max_k=8, max_read_len=160, gap_open_penalty=g, sub_penalty=sub), **aligner_kw)
    n_plain = n_exact = 0
    try:
        for d in (1, -1):
            tt = [t if d == 1 else t[::-1] for t in texts]
            pre = "g%d%+d_" % (g, d)
            for exact in (False, True):
                got = a.computeScoreAffine(d, tt, pats, quals, z["w"], z["si"], z["rc"], z["banded"], z["clip"], sequence=exact)
                exp = {k: z[pre + ("seq_" if exact else "alone_") + k] for k in FIELDS}
                # (ordinary entry: where the traceback leaves the band the reference reads what its object's history left there -- not defined for a call alone)
                use = np.ones(len(tt), bool) if exact else ~z[pre + "stale"]
                bad = [i for i in np.nonzero(use)[0] if got["ag_score"][i] != exp["ag_score"][i]]
                assert not bad, ("ag_score", g, d, exact, bad[:8])
                ok = use & (exp["ag_score"] != -1)
                for k in FIELDS[1:]:
                    bad = [int(i) for i in np.nonzero(ok)[0] if got[k][i] != exp[k][i]]
                    assert not bad, (k, g, d, exact, bad[:8], [(got[k][i], exp[k][i]) for i in bad[:4]])
                if exact:
                    # (the result's remaining field, stale_reads, is this library's own count of traceback steps outside the band: the reference's result has no
                    #  such field.  What the reference pins of it: an answer that differs from the call's answer alone came about through such steps.)
                    dep = np.zeros(len(tt), bool)
                    for k in FIELDS: dep |= (z[pre + "seq_" + k] != z[pre + "alone_" + k]) & (exp["ag_score"] != -1)
                    assert ((got["stale_steps"][dep] & 0xffff) > 0).all(), (g, d, np.nonzero(dep)[0][:8])
                    assert ((got["stale_steps"][~z[pre + "stale"] & ok] & 0xffff) == 0).all(), (g, d)       # ... and none where the restatement's walk stays inside the band
                if exact: n_exact += int(ok.sum())
                else: n_plain += int(ok.sum())
    finally:
        a.close()
    return n_plain, n_exact


def fixture_covers_the_edges():
    """The fixture itself: both sides of every edge of the selection are present, and every lazy-F round of the first segment ends some walk."""
    z = fixture()
    w, banded = z["w"], z["banded"] != 0
    plen = np.array([len(p) for p in z["pats"]])
    tlen = np.array([len(t) for t in z["texts"]])
    bw = np.minimum(2 * w + 1, plen)
    seg = np.where(banded, (bw + 7) // 8 * 8, (plen + 7) // 8 * 8)
    assert (banded & (seg == 32)).any() and (banded & (seg == 40)).any()
    for lim in (12, 13): assert (banded & (w == lim)).any()
    for pl in (64, 65): assert (~banded & (plen == pl)).any()
    assert (banded & (plen < seg)).any() or (banded & (plen < 2 * w + 1)).any()
    assert (banded & (tlen + w < plen)).any()
    assert 1 in z["gap_opens"].tolist()          # (0 is refused by snapgpu_create: gapExtend < subPenalty <= gapOpen + gapExtend has no solution there)
    ends = z["walk_ends"]                                   # [problem, segment, round]: rows whose lazy-F walk of that segment ends in that round
    assert ends.shape == (len(plen), 2, 7) and (ends.sum(axis=0) > 0).all(), ends.sum(axis=0)
    for s in (0, 1):                                        # ... and the problems differ by round: every round is where MOST walks of some problem end
        has = ends[:, s, :].sum(axis=1) > 0
        assert set(np.argmax(ends[has, s, :], axis=1).tolist()) == set(range(7)), (s, np.bincount(np.argmax(ends[has, s, :], axis=1), minlength=7))
    assert max(plen.max(), tlen.max()) <= 160 and 200 <= len(plen) <= 600
