"""Paired-end reads to SAM fields in one call: snapgpu_align_sam_paired (the paired align kernels over Read::clip's windows, the
row-loop pre-pass for the mates, k_sam_fields_paired, device-resident in between) against the calls it replaces, and
snapgpu_sam_fields_paired_device / snapgpu_sam_fields_paired with and without the pre-pass against the reference CLI's records
(tests/golden/sam_fields_paired.npz).  The helpers are shared with the emulator twins (tests/test_emu_paired_sam_onecall.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from snap_amd import abi
from tests import util
from tests.pairs_util import hard_pairs

NOT_FOUND_LOCATION = 0xFFFFFFFF                             # SNAPGPU_InvalidGenomeLocation32
FIELD_KEYS = ("flag", "contig", "pos", "mapq", "n_ops", "nm", "rnext", "pnext", "tlen", "first_written", "stale", "ops")
FIXTURE_KEYS = ("flag", "contig", "pos", "mapq", "nm", "n_ops", "rnext", "pnext", "tlen")
FIXTURE_TAGS = ("default", "lvonly", "eqx")

# name: (read length, -d, clip '#' in front, clip '#' at the back, pairs on the GPU, hard_pairs / paired-parameter keywords)
BATCHES = {
    "150_d8":  (150, 8, False, True, 2000, dict(insert_mean=380), {}),                                                  # -C-+ (the CLI's default)
    "250_d20": (250, 20, True, True, 1000, dict(insert_mean=600, insert_max=1000), {}),                                 # -C++
    "420_d27": (420, 27, True, True, 300, dict(insert_mean=900, insert_max=1400), dict(max_spacing=1500)),             # beyond 400 bp: no pre-pass
}


def golden_contigs(ix):
    """(name, bases) of every contig of a golden index, without the padding between them."""
    from snap_amd.index import GENOME_PAD
    genome = ix.genome_padded[GENOME_PAD:GENOME_PAD + ix.n_bases]
    begins = [c.begin for c in ix.contigs] + [ix.n_bases]
    out = []
    for i, c in enumerate(ix.contigs):
        seq = np.ascontiguousarray(genome[begins[i]:begins[i + 1] - ix.chromosome_padding])
        out.append((c.name, np.char.upper(seq.view("S1")).view(np.uint8).copy()))
    return out


def make_batch(ix, name, n_pairs, seed=41):
    """Hard pairs (tests/pairs_util.py) of the batch's shape plus what Read::clip and the useless-read filter react to: '#'-quality tails and
    heads, mates shorter than -mrl, mates with more Ns than -d, pairs with both mates useless."""
    L, max_k, _, _, _, pkw, _ = BATCHES[name]
    pr = hard_pairs(seed + L, golden_contigs(ix), n_pairs, L, **pkw)
    o = pr["offsets"].astype(np.int64)
    rng = np.random.default_rng(seed)
    bs, qs = [], []
    for i in range(n_pairs):
        for w in (0, 1):
            r = 2 * i + w
            b = pr["bases"][o[r]:o[r + 1]].copy(); q = pr["quals"][o[r]:o[r + 1]].copy()
            if r % 19 == 3: q[len(q) - int(rng.integers(1, 30)):] = ord("#")
            if r % 23 == 5: q[:int(rng.integers(1, 20))] = ord("#")
            if i % 53 == 7: b, q = b[:40], q[:40]                                           # both mates below -mrl: the pair is skipped
            if i % 59 == 11 and w == 1: b, q = b[:35], q[:35]                               # exactly one useless mate: the pair is still aligned
            if i % 61 == 13 and w == 0: b[rng.integers(0, len(b), size=min(3 * max_k + 12, len(b)))] = ord("N")
            if i % 67 == 17: b[rng.integers(0, len(b), size=min(4 * max_k + 20, len(b)))] = ord("N")      # both mates: too many Ns (skipped, as a rule)
            bs.append(b); qs.append(q)
    offs = np.concatenate([[0], np.cumsum([len(b) for b in bs])]).astype(np.uint64)
    return dict(bases=np.concatenate(bs), quals=np.concatenate(qs), offsets=offs)


def read_clip(batch, clip_front, clip_back, max_k, min_read_len=50):
    """Read::clip (Read.h:586-608: back first, then front) and the useless-read test (PairedAligner.cpp:680-682) per mate."""
    o = batch["offsets"].astype(np.int64)
    n = o.size - 1
    fc = np.zeros(n, np.int32); dl = np.zeros(n, np.int32); useful = np.zeros(n, bool)
    for i in range(n):
        q = batch["quals"][o[i]:o[i + 1]]; b = batch["bases"][o[i]:o[i + 1]]
        m, f = len(q), 0
        if clip_back:
            while m > 0 and q[m - 1] == ord("#"): m -= 1
        if clip_front:
            while f < m and q[f] == ord("#"): f += 1
        m -= f
        fc[i], dl[i] = f, m
        useful[i] = m >= min_read_len and int((b[f:f + m] == ord("N")).sum()) <= max_k
    skip = (~useful[0::2] & ~useful[1::2]).astype(np.uint8)
    return fc, dl, skip


def paired_aligner(ix, name, max_read_len=None):
    from snap_amd.aligner import ChimericPairedEndAligner
    L, max_k, _, _, _, _, ppkw = BATCHES[name]
    return ChimericPairedEndAligner(ix, abi.default_params(max_k=max_k, max_read_len=max_read_len or L + 10), abi.default_paired_params(**ppkw))


def not_found_results(n):
    """What a pair that is not given to the aligner is written from: NotFound, no location, score -1, every other field 0."""
    r = np.zeros(n, dtype=abi.PAIRED_RESULT_DTYPE)
    r["status"] = 0; r["location"] = NOT_FOUND_LOCATION; r["score"] = -1
    return r


def two_calls(a, batch, fc, dl, skip, use_m=False):
    """The calls the fused one replaces: ChimericPairedEndAligner::align on a clipped copy of the pairs with a useful mate, the results scattered
    over the batch, then the paired writer on the unclipped batch."""
    o = batch["offsets"].astype(np.int64)
    n_pairs = skip.size
    keep = np.nonzero(skip == 0)[0]
    cb, cq, co = [], [], [0]
    for k in keep:
        for r in (2 * k, 2 * k + 1):
            s = o[r] + fc[r]
            cb.append(batch["bases"][s:s + dl[r]]); cq.append(batch["quals"][s:s + dl[r]]); co.append(co[-1] + int(dl[r]))
    results, first_alt = not_found_results(n_pairs), not_found_results(n_pairs)
    if keep.size:
        prim, alt = a.align(np.concatenate(cb), np.concatenate(cq), np.array(co, dtype=np.uint64))
        results[keep] = prim; first_alt[keep] = alt
    fields = a.samFieldsPaired(batch["bases"], batch["quals"], batch["offsets"], fc, dl, results, use_m)
    return results, first_alt, fields


def check_fused_equals_two_calls(a, ix, name, n_pairs, use_m=False):
    """alignSamPaired on the unclipped batch == align on the clipped copy, scattered, + samFieldsPaired: every output, bit for bit.
    Returns (pairs skipped, SamfPre records the fused call's pre-pass left valid)."""
    _, max_k, clip_front, clip_back, _, _, _ = BATCHES[name]
    batch = make_batch(ix, name, n_pairs)
    fc, dl, skip = read_clip(batch, clip_front, clip_back, max_k)
    assert int(skip.sum()) >= 2 and int((fc > 0).sum()) >= (2 if clip_front else 0) and int((dl < np.diff(batch["offsets"].astype(np.int64)) - fc).sum()) >= 2
    res, alt, got = a.alignSamPaired(batch["bases"], batch["quals"], batch["offsets"], fc, dl, skip, use_m)
    n_valid = a.samf_pre_valid()
    exp_res, exp_alt, exp = two_calls(a, batch, fc, dl, skip, use_m)
    assert int((exp_res["status"] != 0).sum()) > n_pairs                                  # (the batch aligns: most mates have a location)
    for f in exp_res.dtype.names:
        bad = np.nonzero((res[f] != exp_res[f]).reshape(n_pairs, -1).any(axis=1))[0]
        assert bad.size == 0, (name, "results", f, bad[:5], res[f][bad[:5]], exp_res[f][bad[:5]])
        bad = np.nonzero((alt[f] != exp_alt[f]).reshape(n_pairs, -1).any(axis=1))[0]
        assert bad.size == 0, (name, "first_alt", f, bad[:5], alt[f][bad[:5]], exp_alt[f][bad[:5]])
    assert res.tobytes() == exp_res.tobytes() and alt.tobytes() == exp_alt.tobytes()
    for k in FIELD_KEYS:
        bad = np.nonzero((got[k] != exp[k]).reshape(got[k].shape[0], -1).any(axis=1))[0]
        assert bad.size == 0, (name, k, bad[:5], got[k][bad[:5]], exp[k][bad[:5]])
    # the skipped pairs: both records unmapped
    sk = np.nonzero(skip)[0]
    assert (got["flag"][2 * sk] & 4 != 0).all() and (got["flag"][2 * sk + 1] & 4 != 0).all()
    # without the results the call computes the same fields
    r0, a0, g0 = a.alignSamPaired(batch["bases"], batch["quals"], batch["offsets"], fc, dl, skip, use_m, want_results=False)
    assert r0 is None and a0 is None
    for k in FIELD_KEYS:
        assert (g0[k] == got[k]).all(), (name, "results == NULL", k)
    return int(skip.sum()), n_valid


def check_fixture(z, tag, got, n_pairs):
    """All nine computed fields of both records of each pair and the order of the two records against the reference CLI's
    (tests/golden/sam_fields_paired.npz; keys as tests/test_zz_gpu_cigar.py: check_sam_fields_paired_against_reference_cli)."""
    n = 2 * n_pairs
    for k in FIXTURE_KEYS:
        bad = np.nonzero(got[k] != z[tag + "_" + k][:n])[0]
        assert bad.size == 0, (tag, k, bad[:5], got[k][bad[:5]], z[tag + "_" + k][:n][bad[:5]])
    for i in range(n):
        assert util.cigar_text(got["ops"][i], got["n_ops"][i]) == util.cigar_text(z[tag + "_ops"][i], z[tag + "_n_ops"][i]), (tag, i)
    assert (got["first_written"] == z[tag + "_first_written"][:n_pairs]).all()


def fixture_aligner(tag):
    from snap_amd.aligner import BaseAligner
    kw = dict(use_affine_gap=0) if tag.startswith("lvonly") else {}
    return BaseAligner(util.load_golden_index("paired_index.npz"), abi.default_params(max_read_len=400, **kw))


def fixture_through_device_form(z, tag, n_pairs, hip):
    """snapgpu_sam_fields_paired_device over the fixture's reads, clipping and results, everything in device memory.  Returns (fields, valid SamfPre records)."""
    n = 2 * n_pairs
    offs = z["offsets"][:n + 1].astype(np.uint64)
    tot = int(offs[-1])
    stride = 64
    ins = [z["bases"][:tot], z["quals"][:tot], offs, z["front_clip"][:n].astype(np.int32), z["data_len"][:n].astype(np.int32),
           np.ascontiguousarray(z[tag + "_results"][:n_pairs])]
    outs = dict(flag=np.zeros(n, np.int32), contig=np.zeros(n, np.int32), pos=np.zeros(n, np.int64), mapq=np.zeros(n, np.int32),
                ops=np.zeros((n, stride), np.uint32), n_ops=np.zeros(n, np.int32), nm=np.zeros(n, np.int32), rnext=np.zeros(n, np.int32),
                pnext=np.zeros(n, np.int64), tlen=np.zeros(n, np.int64), first_written=np.zeros(n_pairs, np.int32), stale=np.zeros(n, np.int32))
    a = fixture_aligner(tag)
    try:
        d_in = [hip.upload(x) for x in ins]
        d = {k: hip.upload(v) for k, v in outs.items()}
        a.samFieldsPaired_device(n_pairs, int(np.diff(offs.astype(np.int64)).max()), *d_in, d["flag"], d["contig"], d["pos"], d["mapq"], d["ops"], stride, d["n_ops"], d["nm"], d["rnext"],
                                 d["pnext"], d["tlen"], d["first_written"], d["stale"], use_m=bool(z[tag + "_use_m"]))
        n_valid = a.samf_pre_valid()
        got = {k: hip.download(d[k], v) for k, v in outs.items()}
    finally:
        hip.free_all()
        a.close()
    check_fixture(z, tag, got, n_pairs)
    return got, n_valid


def fixture_through_host_call(n_pairs=None, lib_path=None):
    """snapgpu_sam_fields_paired over the fixture, the three option sets.  Run in a process of its own per value of SNAPGPU_SAMF_DP8 (the switch is
    read once per process): with the pre-pass off no SamfPre record may be valid, with it on the affine-gap sets must have some."""
    if lib_path:
        import snap_amd.aligner as al
        al.LIB_PATH, al._lib = lib_path, None
    z = np.load(os.path.join(util.GOLDEN, "sam_fields_paired.npz"))
    pre_on = os.environ.get("SNAPGPU_SAMF_DP8", "1") != "0"
    for tag in FIXTURE_TAGS:
        npairs = len(z[tag + "_first_written"]) if n_pairs is None else n_pairs
        n = 2 * npairs
        offs = z["offsets"][:n + 1]
        a = fixture_aligner(tag)
        try:
            got = a.samFieldsPaired(z["bases"][:int(offs[-1])], z["quals"][:int(offs[-1])], offs, z["front_clip"][:n], z["data_len"][:n],
                                    z[tag + "_results"][:npairs], bool(z[tag + "_use_m"]))
            n_valid = a.samf_pre_valid()
        finally:
            a.close()
        check_fixture(z, tag, got, npairs)
        if n_pairs is None:
            assert int((got["flag"] & 2 != 0).sum()) > 1500 and int((got["first_written"] == 1).sum()) > 300
        if pre_on and not tag.startswith("lvonly"):
            assert n_valid > npairs // 2, (tag, n_valid)
        else:
            assert n_valid == 0, (tag, n_valid)
        print("fixture", tag, "pairs", npairs, "pre-pass", "on" if pre_on else "off", "valid SamfPre records", n_valid)


def run_fixture_child(dp8, n_pairs=None, lib_path=None, timeout=3000):
    code = "from tests.test_zz_gpu_paired_sam_onecall import fixture_through_host_call as f; f(%r, %r)" % (n_pairs, lib_path)
    r = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code], cwd=util.ROOT, env=dict(os.environ, SNAPGPU_SAMF_DP8=dp8),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, stdin=subprocess.DEVNULL, timeout=timeout)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-4000:]
    assert r.stdout.decode().count("fixture ") == len(FIXTURE_TAGS)


def check_argument_errors(ix):
    from snap_amd.aligner import BaseAligner, ChimericPairedEndAligner, SnapGpuError
    name = "150_d8"
    batch = make_batch(ix, name, 64)
    fc, dl, skip = read_clip(batch, False, True, 8)
    a = paired_aligner(ix, name)
    try:
        # n_pairs == 0: a call like any other
        r0, _, g0 = a.alignSamPaired(batch["bases"][:0], batch["quals"][:0], np.zeros(1, np.uint64), fc[:0], dl[:0], skip[:0])
        assert r0.size == 0 and g0["flag"].size == 0 and g0["first_written"].size == 0
        with pytest.raises(SnapGpuError, match="ops_stride"):
            a.alignSamPaired(batch["bases"], batch["quals"], batch["offsets"], fc, dl, skip, ops_stride=2)
        n = 2 * skip.size
        outs = [np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int64), np.zeros(n, np.int32), np.zeros((n, 8), np.uint32), np.zeros(n, np.int32),
                np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(skip.size, np.int32), np.zeros(n, np.int32)]
        ins = [batch["bases"], batch["quals"], batch["offsets"], fc, dl, skip]
        p = lambda x: C.c_void_p(x.ctypes.data)
        def call(ins_, outs_):
            return a.lib.snapgpu_align_sam_paired(a.handle, C.c_uint32(skip.size), *ins_, C.c_int(0), None, None, *outs_[:5], C.c_uint32(8), *outs_[5:])
        for j in range(len(ins)):                                              # NULL inputs
            assert call([None if k == j else p(x) for k, x in enumerate(ins)], [p(x) for x in outs]) == -1, j
        for j in range(len(outs)):                                             # NULL outputs
            assert call([p(x) for x in ins], [None if k == j else p(x) for k, x in enumerate(outs)]) == -1, j
        assert a.lib.snapgpu_align_sam_paired(None, C.c_uint32(skip.size), *[p(x) for x in ins], C.c_int(0), None, None, *[p(x) for x in outs[:5]], C.c_uint32(8),
                                              *[p(x) for x in outs[5:]]) == -1
        assert call([p(x) for x in ins], [p(x) for x in outs]) == 0              # (and the same call with nothing missing)
        # the device-pointer form: NULL arguments, ops_stride, max_read_len
        with pytest.raises(SnapGpuError, match="null argument"):
            a.samFieldsPaired_device(4, 160, *([0] * 6), *([0] * 5), 64, *([0] * 7))
        d = [x.ctypes.data for x in ins[:5]] + [not_found_results(skip.size).ctypes.data]
        do = [x.ctypes.data for x in outs]
        with pytest.raises(SnapGpuError, match="ops_stride"):
            a.samFieldsPaired_device(skip.size, 160, *d, *do[:5], 2, *do[5:])
        with pytest.raises(SnapGpuError, match="max_read_len"):
            a.samFieldsPaired_device(skip.size, 0, *d, *do[:5], 8, *do[5:])
    finally:
        a.close()
    # a mate the aligner is given that is longer than the context's max_read_len
    a = paired_aligner(ix, name, max_read_len=120)
    try:
        with pytest.raises(SnapGpuError, match="max_read_len"):
            a.alignSamPaired(batch["bases"], batch["quals"], batch["offsets"], fc, dl, skip)
    finally:
        a.close()
    # a context without snapgpu_enable_paired; one with snapgpu_enable_secondary
    s = BaseAligner(ix, abi.default_params(max_k=8, max_read_len=160))
    try:
        with pytest.raises(SnapGpuError, match="snapgpu_enable_paired"):
            ChimericPairedEndAligner.alignSamPaired(s, batch["bases"], batch["quals"], batch["offsets"], fc, dl, skip)
    finally:
        s.close()
    a = paired_aligner(ix, name)
    try:
        a.enable_secondary(1)
        with pytest.raises(SnapGpuError, match="snapgpu_enable_secondary"):
            a.alignSamPaired(batch["bases"], batch["quals"], batch["offsets"], fc, dl, skip)
    finally:
        a.close()


# ------------------------------------------------------------------------------------------------------------------------ the GPU tests
@pytest.fixture(scope="module")
def pindex():
    return util.load_golden_index("paired_index.npz")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["150_d8", "250_d20"])
def test_fused_call_equals_the_two_calls_it_replaces(pindex, name):
    a = paired_aligner(pindex, name)
    try:
        n_skipped, n_valid = check_fused_equals_two_calls(a, pindex, name, BATCHES[name][4])
    finally:
        a.close()
    assert n_skipped >= 10 and (n_valid > 0 or name != "150_d8")     # (2 x 250: the pre-pass's LDS rows for four waves go beyond 64 KiB, none runs)


@pytest.mark.gpu
def test_fused_call_on_mates_beyond_400_bp_runs_without_the_pre_pass(pindex):
    name = "420_d27"
    a = paired_aligner(pindex, name)
    try:
        n_skipped, n_valid = check_fused_equals_two_calls(a, pindex, name, BATCHES[name][4])
    finally:
        a.close()
    assert n_skipped >= 2 and n_valid == 0


@pytest.mark.gpu
def test_fused_call_through_a_replica_context(pindex):
    name = "150_d8"
    owner = paired_aligner(pindex, name)
    a = owner.replica()
    try:
        n_skipped, n_valid = check_fused_equals_two_calls(a, pindex, name, 800, use_m=True)
    finally:
        a.close()
        owner.close()
    assert n_skipped >= 5 and n_valid > 0


@pytest.mark.gpu
def test_pre_pass_takes_part_in_the_paired_launches(pindex):
    """A paired launch that passed pre == NULL would leave the count at 0: the 2 x 150 batch must have valid SamfPre records after the fused call and
    after the two-call path's snapgpu_sam_fields_paired, the batch beyond 400 bp none."""
    for name, n_pairs in (("150_d8", 600), ("420_d27", 120)):
        _, max_k, clip_front, clip_back, _, _, _ = BATCHES[name]
        batch = make_batch(pindex, name, n_pairs)
        fc, dl, skip = read_clip(batch, clip_front, clip_back, max_k)
        a = paired_aligner(pindex, name)
        try:
            res, _, _ = a.alignSamPaired(batch["bases"], batch["quals"], batch["offsets"], fc, dl, skip)
            fused_valid = a.samf_pre_valid()
            a.samFieldsPaired(batch["bases"], batch["quals"], batch["offsets"], fc, dl, res)
            fields_valid = a.samf_pre_valid()
        finally:
            a.close()
        assert fused_valid == fields_valid
        if name == "150_d8":
            assert 0 < fused_valid <= 2 * n_pairs
        else:
            assert fused_valid == 0


@pytest.mark.gpu
@pytest.mark.parametrize("tag", FIXTURE_TAGS)
def test_sam_fields_paired_device_form_vs_reference_cli_fixture(tag):
    z = np.load(os.path.join(util.GOLDEN, "sam_fields_paired.npz"))
    got, n_valid = fixture_through_device_form(z, tag, len(z[tag + "_first_written"]), util.HipBuffers())
    assert int((got["flag"] & 2 != 0).sum()) > 1500 and int((got["first_written"] == 1).sum()) > 300
    assert (n_valid == 0) if tag.startswith("lvonly") else (n_valid > 1300)


@pytest.mark.gpu
@pytest.mark.parametrize("dp8", ["0", "1"])
def test_sam_fields_paired_host_call_vs_reference_cli_fixture_with_and_without_the_pre_pass(dp8):
    import snap_amd.aligner as al
    run_fixture_child(dp8, lib_path=al.LIB_PATH)


@pytest.mark.gpu
def test_paired_sam_onecall_argument_errors(pindex):
    check_argument_errors(pindex)
