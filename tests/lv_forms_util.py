"""Shared by tests/test_emu_lv_forms.py and tests/test_zz_gpu_lv_forms.py: tests/golden/lv_forms.npz (scripts/make_golden_lv_forms.py, answers of
the compiled reference's LandauVishkin<1> and <-1>) through snapgpu_landau_vishkin in each of its forms (SNAPGPU_LV_FORM: unset, lds, hbm) -- pattern
lengths on both sides of every mask-word count, limits on both sides of the second pass of the diagonal loop (level 32), texts shorter than
the pattern, deep backtraces, and the largest working set the entry takes.

`texts` holds every text in the order Landau-Vishkin walks it; direction -1 is given the same bytes reversed in memory, so both directions
answer the same problem."""
import ctypes as C
import os

import numpy as np

from snap_amd.abi import ptr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("score", "match_probability", "net_indel", "total_indels", "text_span")
FORMS = (None, "lds", "hbm")
LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 150, 151, 250, 400, 401, 511, 512, 513, 959, 960, 1000)
LIMITS = (-1, 0, 1, 2, 3, 8, 31, 32, 33, 48, 60, 63, 64, 100, 126, 127, 200)
WORD_EDGES = (63, 64, 127, 128, 959)
K_BUCKETS = (8, 33, 63, 100, 126)
GUARD = 144                      # bytes around every sequence of a guarded layout: the reference looks up to 127 + 8 bytes outside a text
E_INVALID, E_UNSUPPORTED = -1, -3
_fixture = None


def fixture():
    global _fixture
    if _fixture is None:
        _fixture = np.load(os.path.join(ROOT, "tests", "golden", "lv_forms.npz"), allow_pickle=True)
    return _fixture


def group_of(plen, k):
    """Problems that share a batch: the entry sizes LDS by the batch's longest pattern (in mask words) and largest limit."""
    kk = min(max(int(k), 0), 126)
    return ((max(int(plen), 1) + 63) // 64) * 8 + next(i for i, b in enumerate(K_BUCKETS) if kk <= b)


def layout(seqs, guard_byte, guard=GUARD):
    """The sequences in one buffer with `guard` bytes of guard_byte before, between and after them (guard None: back to back, 16 zero bytes
    behind the last, as BaseAligner.computeEditDistance packs them).  Returns (uint8 buffer, uint32 start of each, int32 length of each)."""
    lens = np.array([len(s) for s in seqs], np.int32)
    if guard_byte is None:
        offs = np.zeros(len(seqs), np.uint32)
        offs[1:] = np.cumsum(lens[:-1])
        return np.frombuffer(b"".join(seqs) + b"\0" * 16, np.uint8).copy(), offs, lens
    g = bytes([guard_byte]) * guard
    offs = (guard + np.concatenate([[0], np.cumsum(lens[:-1] + guard)])).astype(np.uint32)
    return np.frombuffer(g + g.join(seqs) + g, np.uint8).copy(), offs, lens


def lv_call(fn, handle, direction, texts, pats, quals, k, text_guard=None, pat_guard=None):
    """One call of an entry with the signature of snapgpu_landau_vishkin (handle given) or snapref_landau_vishkin (handle None); direction -1:
    the text in memory is the reverse of texts[i] and the entry gets the address one past its end.  Returns (return code, answers)."""
    n = len(texts)
    tbuf, toff, tlen = layout([t if direction == 1 else t[::-1] for t in texts], text_guard)
    if direction == -1:
        toff = (toff + tlen.astype(np.uint32)).astype(np.uint32)
    pbuf, poff, plen = layout(pats, pat_guard)
    qbuf, _, _ = layout(quals, None if pat_guard is None else 33)
    k = np.ascontiguousarray(k, np.int32)
    out = dict(score=np.zeros(n, np.int32), match_probability=np.zeros(n, np.float64), net_indel=np.zeros(n, np.int32),
               total_indels=np.zeros(n, np.int32), text_span=np.zeros(n, np.int32))
    res = [ptr(out[f]) for f in FIELDS]
    if handle is None:
        rc = fn(C.c_int(direction), C.c_uint32(n), ptr(tbuf), ptr(toff), ptr(tlen), ptr(pbuf), ptr(qbuf), ptr(poff), ptr(plen), ptr(k), *res)
    else:
        rc = fn(handle, C.c_int(direction), C.c_uint32(n), ptr(tbuf), C.c_uint64(tbuf.size), ptr(toff), ptr(tlen),
                ptr(pbuf), ptr(qbuf), C.c_uint64(pbuf.size), ptr(poff), ptr(plen), ptr(k), *res)
    return rc, out


def lv_lds_bytes(kmax, pcap):
    """lv.h: lv_lds_bytes."""
    tri = ((kmax + 1) * (kmax + 1) * 2 + 3) & ~3
    tri = (tri + (kmax + 1) * 4 + 7) & ~7
    return tri + (2 * kmax + 1) * ((pcap + 63) >> 6) * 8


def lds_form_fits(pats, texts, k):
    """Whether SNAPGPU_LV_FORM=lds takes this batch: the triangle and the staged pattern, qualities and text of one wave within 64 KB."""
    kmax = max(0, min(126, max(int(x) for x in k)))
    pcap = (max(64, max(len(p) for p in pats)) + 63) & ~63
    tcap = (max(16, max(min(len(t), len(p) + 127) for p, t in zip(pats, texts))) + 15) & ~15
    return ((lv_lds_bytes(kmax, pcap) + 15) & ~15) + 2 * pcap + tcap <= 64 * 1024


def _same(got, exp, idx, what):
    for f in FIELDS:
        g, e = got[f], exp[f][idx]
        if f == "match_probability":               # bit for bit, on ScoreAboveLimit answers too (1.0, or perfect[pattern_len] from the all-match prefix)
            g, e = g.view(np.uint64), np.ascontiguousarray(e).view(np.uint64)
        bad = np.nonzero(g != e)[0]
        assert bad.size == 0, (f, what, [int(idx[i]) for i in bad[:8]], [(got[f][i], exp[f][idx[i]]) for i in bad[:4]])


def check_form(index, form):
    """Every problem of the fixture through BaseAligner.computeEditDistance under SNAPGPU_LV_FORM = form, both directions, one batch per group:
    all five fields equal to the reference's.  Then every batch once more from a layout with guard bytes of a value the generator did not use
    (the answers may not depend on what lies beside a sequence), one batch holding the shortest and the largest problem, and the refusals.
    Returns the number of problems compared.  (The environment variable is left as it was found.)"""
    from snap_amd import abi
    from snap_amd.aligner import BaseAligner, SnapGpuError
    z = fixture()
    texts, pats, quals, k, group = list(z["texts"]), list(z["pats"]), list(z["quals"]), z["k"], z["group"]
    exp = {d: {f: z["lv%+d_%s" % (d, f)] for f in FIELDS} for d in (1, -1)}
    saved = os.environ.get("SNAPGPU_LV_FORM")
    a = BaseAligner(index, abi.default_params(max_k=8, max_read_len=160))
    n_done, refused = 0, []
    try:
        if form is None: os.environ.pop("SNAPGPU_LV_FORM", None)
        else: os.environ["SNAPGPU_LV_FORM"] = form
        small = [b"ACGTACGTAC"], [b"ACGTTCGTAC"], [b"5" * 10], [3]

        def normal_call():
            r = a.computeEditDistance(1, *small)
            assert (int(r["score"][0]), int(r["net_indel"][0]), int(r["text_span"][0])) == (1, 0, 10), r

        for g in sorted(set(group.tolist())):
            idx = np.nonzero(group == g)[0]
            sel = lambda xs: [xs[i] for i in idx]
            fits = form != "lds" or lds_form_fits(sel(pats), sel(texts), k[idx])
            for d in (1, -1):
                tt = [t if d == 1 else t[::-1] for t in sel(texts)]
                if not fits:
                    try:
                        a.computeEditDistance(d, tt, sel(pats), sel(quals), k[idx])
                    except SnapGpuError as e:
                        assert "(%d)" % E_UNSUPPORTED in str(e), e
                    else:
                        raise AssertionError("SNAPGPU_LV_FORM=lds took group %d, which does not fit its LDS" % g)
                    normal_call()                                  # the context answers after a refusal
                    continue
                got = a.computeEditDistance(d, tt, sel(pats), sel(quals), k[idx])
                _same(got, exp[d], idx, (form, d, "group", g))
                rc, got = lv_call(a.lib.snapgpu_landau_vishkin, a.handle, d, sel(texts), sel(pats), sel(quals), k[idx], text_guard=0x7e, pat_guard=0x7c)
                assert rc == 0, (rc, form, d, g)
                _same(got, exp[d], idx, (form, d, "guarded group", g))
                n_done += len(idx)
            if not fits: refused.append(g)
        plen = np.array([len(p) for p in pats])
        big = int(np.nonzero((plen == 1000) & (k == 126) & (z["lv+1_score"] >= 64))[0][0])
        tiny = int(np.nonzero((plen == 1) & (k >= 0))[0][0])
        if form == "lds":
            # what does not fit is the largest working set and nothing much smaller: every refused group has 15 or 16 mask words and a limit above 100
            assert refused and all(g // 8 >= 15 and g % 8 == len(K_BUCKETS) - 1 for g in refused), refused
            assert group[big] in refused
            big = int(np.nonzero((plen == 512) & (k == 126))[0][0])         # the largest it takes
        else:
            assert not refused
        idx = np.array([tiny, big, tiny])
        for d in (1, -1):
            got = a.computeEditDistance(d, [texts[i] if d == 1 else texts[i][::-1] for i in idx], [pats[i] for i in idx], [quals[i] for i in idx], k[idx])
            _same(got, exp[d], idx, (form, d, "mixed batch"))
        os.environ["SNAPGPU_LV_FORM"] = "neither"                  # the switch is read by every call: a value that names no form is an error
        try:
            a.computeEditDistance(1, *small)
        except SnapGpuError as e:
            assert "(%d)" % E_INVALID in str(e), e
        else:
            raise AssertionError("SNAPGPU_LV_FORM=neither was accepted")
        os.environ.pop("SNAPGPU_LV_FORM")
        normal_call()
    finally:
        if saved is None: os.environ.pop("SNAPGPU_LV_FORM", None)
        else: os.environ["SNAPGPU_LV_FORM"] = saved
        a.close()
    return n_done


def check_restatement():
    """tests.util.oracle_lv (the C restatement of the reference) on the same problems: a third opinion, every field, both directions."""
    from tests import util
    z = fixture()
    n = len(z["k"])
    for d in (1, -1):
        for i in range(n):
            t = z["texts"][i]
            r = util.oracle_lv(d, t if d == 1 else t[::-1], z["pats"][i], z["quals"][i], int(z["k"][i]))
            for f in FIELDS:
                e = z["lv%+d_%s" % (d, f)][i]
                assert r[f] == e, (f, d, i, r[f], e)
    return 2 * n


def py_lv(text, pat, k):
    """LandauVishkin<1>::computeEditDistance restated for what the fixture's classes are about (LandauVishkin.h:165-342, bytes outside either
    sequence equal to nothing): score, net_indel, total_indels, text_span, run0, `steps` -- the forward pass's merged actions as (action,
    count, offset before it) -- `cells` -- the cells of the last level that reach the pattern's end as (rank, d, action), in visiting order
    up to and including the winner -- and `winner` (rank, d, action)."""
    n, tl = len(pat), len(text)
    out = dict(score=-1, net_indel=0, total_indels=0, text_span=0, steps=[], cells=[], winner=None, run0=0)
    if k < 0: return out
    k = min(k, 126)

    def run(x, d):
        if x < 0: return x
        end = min(n, tl - d)
        while x < end and d + x >= 0 and pat[x] == text[d + x]: x += 1
        return x
    end0 = min(n, tl)
    run0 = run(0, 0) if end0 > 0 else 0
    out["run0"] = run0
    if run0 == end0:
        res = n - end0 if n > end0 else 0
        if res <= k: out["score"], out["text_span"] = res, n
        return out
    L, A = [{0: run0}], [{}]
    best_d, e = None, 0
    for e in range(1, k + 1):
        L.append({}); A.append({})
        prev = L[e - 1]
        for r in range(2 * e + 1):
            d = (r + 1) // 2 if r & 1 else -(r // 2)
            best, act = run(prev.get(d, -2) + 1, d), "X"
            left = run(prev.get(d - 1, -2), d)
            if left > best: best, act = left, "D"
            right = run(prev.get(d + 1, -2) + 1, d)
            if right > best: best, act = right, "I"
            L[e][d], A[e][d] = best, act
            if best == n:
                out["cells"].append((r, d, act))
                if act == "X":
                    best_d = d
                    break
                if best_d is None or abs(d) < abs(best_d): best_d = d
        if best_d is not None: break
    if best_d is None: return out
    out["winner"] = (2 * best_d - 1 if best_d > 0 else -2 * best_d, best_d, A[e][best_d])
    out["cells"] = [c for c in out["cells"] if c[0] <= out["winner"][0] or out["winner"][2] != "X"]
    bt, cur = [None] * (e + 1), best_d
    for ce in range(e, 0, -1):
        act = A[ce][cur]
        pd = cur + 1 if act == "I" else cur - 1 if act == "D" else cur
        bt[ce] = (act, L[ce][cur] - L[ce - 1].get(pd, -2) - (0 if act == "D" else 1))
        cur = pd
    ce, offset = 1, run0
    while ce <= e:
        act, count = bt[ce][0], 1
        while ce + 1 <= e and bt[ce][1] == 0 and bt[ce + 1][0] == act:
            count += 1; ce += 1
        out["steps"].append((act, count, offset))
        if act == "I": offset += count; out["net_indel"] += count; out["total_indels"] += count
        elif act == "D": offset -= count; out["net_indel"] -= count; out["total_indels"] += count; out["text_span"] += count
        else: offset += count
        offset += bt[ce][1]
        ce += 1
    out["text_span"] += n
    out["score"] = e
    return out


def fixture_covers_the_edges():
    """The fixture itself: every class its generator is asked for is present, read from the problems and the reference's answers.  What the
    answers alone do not show (which cells of the last level reached the end, where the actions lie) comes from py_lv on the problems small
    enough for it, after py_lv has been held against the reference's four integer fields on them."""
    z = fixture()
    texts, pats, quals, k = list(z["texts"]), list(z["pats"]), list(z["quals"]), z["k"]
    n = len(k)
    assert 400 <= n <= 800, n
    plen = np.array([len(p) for p in pats]); tlen = np.array([len(t) for t in texts])
    sc, net, tot = z["lv+1_score"], z["lv+1_net_indel"], z["lv+1_total_indels"]
    for d in (1, -1):
        for f in FIELDS: assert z["lv%+d_%s" % (d, f)].shape == (n,)
    assert all(len(q) == len(p) for p, q in zip(pats, quals))
    assert (z["group"] == np.array([group_of(p, kk) for p, kk in zip(plen, k)])).all()
    # lengths and limits; every limit at a length of one, two, three and more mask words, every length below and from the second pass on
    assert set(LENGTHS) <= set(plen.tolist()), sorted(set(LENGTHS) - set(plen.tolist()))
    assert set(LIMITS) <= set(k.tolist()), sorted(set(LIMITS) - set(k.tolist()))
    for L in LENGTHS:
        if L > 2: assert ((plen == L) & (sc >= 1)).any() and ((plen == L) & (sc == -1)).any(), L
    for lim in (127, 200): assert ((k == lim) & (sc > 0)).any(), lim
    # depth
    assert (sc >= 32).sum() >= 8 and (sc >= 64).sum() >= 4 and ((sc == k) & (sc >= 32)).any() and ((sc == k) & (sc > 0) & (sc < 32)).any()
    key = {(texts[i], pats[i], int(k[i])): i for i in range(n)}
    twins = [i for i in range(n) if sc[i] == -1 and k[i] >= 0 and sc[key.get((texts[i], pats[i], int(k[i]) + 1), i)] == k[i] + 1]
    assert len(twins) >= 6 and any(k[i] + 1 in (32, 33) for i in twins) and any(k[i] + 1 >= 64 for i in twins), twins      # one edit too many
    assert (net >= 33).any() and (net <= -33).any()
    assert ((sc == -1) & (z["lv+1_match_probability"] != 1.0)).any() and ((sc == -1) & (z["lv+1_match_probability"] == 1.0)).any()
    # short texts: each length difference with a limit on both sides of the missing tail, and the all-match prefix among them
    for delta in (-5, -1, 0, 1):
        at = tlen - plen == delta
        assert (at & (sc == -1)).any() and (at & (sc >= max(0, -delta))).any(), delta
    prefix = np.array([t == p[:len(t)] and len(t) < len(p) for t, p in zip(texts, pats)])
    assert (prefix & (sc == -1)).any() and (prefix & (sc == plen - tlen)).any() and (prefix & (k == plen - tlen)).any() and (prefix & (k == plen - tlen - 1)).any()
    # word boundaries: the first mismatch exactly there (the level-0 loop), and a later one there (extend)
    def mism(i):
        m = min(len(pats[i]), len(texts[i]))
        return np.nonzero(np.frombuffer(pats[i][:m], np.uint8) != np.frombuffer(texts[i][:m], np.uint8))[0]
    subs_only = [i for i in range(n) if tlen[i] >= plen[i] and sc[i] > 0 and tot[i] == 0 and len(mism(i)) == sc[i]]
    for pos in WORD_EDGES:
        assert any(mism(i)[0] == pos for i in subs_only), pos
        assert any(pos in mism(i)[1:] for i in subs_only), pos
    assert any(((mism(i)[1:] >> 6) - (mism(i)[:-1] >> 6)).max(initial=0) >= 3 for i in subs_only)        # a matching run over two or more whole words
    assert any((plen[i] - 1 >> 6) - (mism(i)[-1] >> 6) >= 3 for i in subs_only)                              # ... and one that runs to the pattern's end
    # alphabet
    N = ord("N")
    assert any(any(p[j] == N and t[j] != N for j in range(min(len(p), len(t)))) for p, t in zip(pats, texts))
    assert any(any(p[j] != N and t[j] == N for j in range(min(len(p), len(t)))) for p, t in zip(pats, texts))
    assert any(any(p[j] == N and t[j] == N for j in range(min(len(p), len(t)))) for p, t in zip(pats, texts))
    qall = np.frombuffer(b"".join(quals), np.uint8)
    assert qall.min() == 33 and qall.max() == 126 and len(set(qall.tolist())) == 94
    # the largest working set
    assert ((plen == 1000) & (k == 126) & (sc >= 64)).any() and ((plen == 1000) & (k == 126) & (sc == -1)).any()
    assert lv_lds_bytes(126, 1024) == 65152
    assert ((k >= 64).sum()) <= 90, int((k >= 64).sum())
    # what needs the cells and the actions
    small = [i for i in range(n) if plen[i] <= 260 and 0 <= k[i] <= 63]
    have = dict(x_over_indel=0, x_over_indel_second_pass=0, indel_cells=0, lead_I=0, lead_D=0, run_X=0, run_I=0, run_D=0, adjacent=0, at_0=0, at_last=0,
                low_clamp=0, winner_rank_64=0, indel_cells_both_passes=0)
    for i in small:
        r = py_lv(texts[i], pats[i], int(k[i]))
        assert (r["score"], r["net_indel"], r["total_indels"], r["text_span"]) == (sc[i], net[i], tot[i], z["lv+1_text_span"][i]), (i, r)
        if r["winner"] is None: continue
        w, cells, steps = r["winner"], r["cells"], r["steps"]
        if w[2] == "X" and any(c[2] != "X" and c[0] < w[0] for c in cells):
            have["x_over_indel"] += 1
            if w[0] >= 64 and any(c[2] != "X" and c[0] < 64 for c in cells): have["x_over_indel_second_pass"] += 1
        if w[2] != "X" and len(cells) >= 2 and w[0] == min(c[0] for c in cells): have["indel_cells"] += 1
        if w[2] != "X" and w[0] < 64 and any(c[0] >= 64 for c in cells): have["indel_cells_both_passes"] += 1
        if w[0] >= 64: have["winner_rank_64"] += 1
        if steps[0][2] == 0 and steps[0][0] != "X": have["lead_" + steps[0][0]] += 1
        for a, c, o in steps:
            if c >= 3: have["run_" + a] += 1
            if a == "X" and o == 0: have["at_0"] += 1
            if a == "X" and o + c - 1 == plen[i] - 1: have["at_last"] += 1
            if a == "X" and o < 0: have["low_clamp"] += 1
        for (a1, c1, o1), (a2, c2, o2) in zip(steps, steps[1:]):
            if a1 != a2 and (o2 == o1 + (c1 if a1 != "D" else -c1)): have["adjacent"] += 1
    assert all(v >= 2 for v in have.values()), have
    return have
