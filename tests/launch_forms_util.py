"""The launch forms and overflow passes that the context picks from its geometry and from what a first pass reports, reached with the
switches the product already has: the LDS affine-gap form on short reads (SNAPGPU_AG_LDS), many work items per wave (SNAPGPU_WAVES_PER_CU,
SNAPGPU_PAIRED_WAVES_PER_CU, SNAPGPU_PAIRED_GRID_SHARE), the two help protocols published eagerly, and the second pass of launch_paired
over pairs that overflowed the first one's affine-gap candidate buffers (SNAPGPU_PAIRED_AGC_CAP, SNAPGPU_PAIRED_POOL).

Every switch is read by getenv when a context is created (snapgpu_create, snapgpu_enable_paired) or per launch, none is cached in a
static: `form` sets them before the aligner is constructed, every aligner is closed before the next form is built, no child process
is needed.  Expectations, in this order: the committed reference fixtures (util.with_fresh_overrides), the compiled reference with fresh
aligner objects where oracle/_ref is present, and the same call in the default form, byte for byte.

Shared by tests/test_zz_gpu_launch_forms.py (GPU) and tests/test_emu_launch_forms.py (wavefront emulator)."""
import ctypes as C
import os

import numpy as np

from snap_amd import abi, synth
from tests import util
from tests.pairs_util import compare_paired, compare_paired_secondary, load_paired_secondary_sets

E_UNSUPPORTED = -3                                   # SNAPGPU_E_UNSUPPORTED (include/snapgpu.h)
POOL_OVERFLOW = 1                                    # SNAPGPU_PAIR_POOL_OVERFLOW
POOL_OVERFLOW_TEXT = b"more candidate entries than the per-wave pools hold"
INFO_MASK = np.uint32(0x3fffffff)                    # `reserved` of a single-end result: the two top bits say who scored it (help, replay)
WORK_COUNTERS = ("n_hash_table_lookups", "n_lv_locations", "n_ag_locations")
SWITCHES = ("SNAPGPU_AG_LDS", "SNAPGPU_WAVES_PER_CU", "SNAPGPU_PAIRED_WAVES_PER_CU", "SNAPGPU_PAIRED_GRID_SHARE", "SNAPGPU_PAIRED_GRID_OVER",
            "SNAPGPU_SINGLE_HEAVY_FIRST", "SNAPGPU_SINGLE_HELP", "SNAPGPU_SINGLE_HELP_EAGER", "SNAPGPU_SINGLE_HELP_KEEP", "SNAPGPU_PAIRED_HELP_MIN",
            "SNAPGPU_PAIRED_HELP_EAGER", "SNAPGPU_PAIRED_AGC_CAP", "SNAPGPU_PAIRED_POOL", "SNAPGPU_PHASE_TIMERS", "SNAPGPU_LV_PLANES", "SNAPGPU_DEBUG_PAIRED_FLAG_EVERY")


def form(mp, **env):
    """The environment of one launch form: every switch of this module unset, then the given ones (FOO="1" sets SNAPGPU_FOO)."""
    for k in SWITCHES:
        mp.delenv(k, raising=False)
    for k, v in env.items():
        assert "SNAPGPU_" + k in SWITCHES, k
        mp.setenv("SNAPGPU_" + k, str(v))


def same_bytes_masked(a, b, what):
    """Two RESULT_DTYPE arrays: every field the same bytes, `reserved` under INFO_MASK."""
    for f in a.dtype.names:
        if f == "reserved":
            assert ((a[f] & INFO_MASK) == (b[f] & INFO_MASK)).all(), (what, f)
        else:
            assert a[f].tobytes() == b[f].tobytes(), (what, f, np.flatnonzero((a[f] != b[f]).reshape(a.size, -1).any(axis=1))[:5])


def same_pairs(a, b, what, sel=None, info=0):
    """Two PAIRED_RESULT_DTYPE arrays: every field the same bytes (for the pairs of `sel`), `flags` included -- as the paired-end tests
    compare two forms (tests/test_emu_kernels.py: grid share, help on demand): who scored a candidate leaves no trace in a pair's record.
    `info`: bits of `flags` that only say which pass wrote the record (EXACT_REPLAY, where a form forces pairs through that pass)."""
    if sel is not None:
        a, b = a[sel], b[sel]
    for f in a.dtype.names:
        if f == "flags" and info:
            assert ((a[f] & ~np.uint32(info)) == (b[f] & ~np.uint32(info))).all(), (what, f)
            continue
        assert a[f].tobytes() == b[f].tobytes(), (what, f, np.flatnonzero((a[f] != b[f]).reshape(a.size, -1).any(axis=1))[:5])


def work(c):
    return [c[k] for k in WORK_COUNTERS]


# ------------------------------------------------------------------------------------------------ A. the LDS affine-gap form on short reads
def replay_sample(reads, tag, n):
    """n reads of the golden batch (None: all of it): the first ones and, so that a reduced sample still holds reads that go through the
    replay, every read whose reference answer moves with the aligner object's history -- the fixture's `unstable` reads and the ones
    tests/golden/fresh_overrides.npz patches; their banded affine-gap traceback leaves the band."""
    total = reads["b" + tag].shape[0]
    if n is None or n >= total:
        return np.arange(total)
    key = "default_d8_%s_" % tag
    moved = reads[key + "unstable"].copy()
    moved[util.with_fresh_overrides(reads[key + "primary"], key + "primary")[1]] = True
    return np.union1d(np.arange(n), np.flatnonzero(moved))


def single_fixture(reads, name, tag, sel):
    key = "%s_%s_" % (name, tag)
    exp, patched = util.with_fresh_overrides(reads[key + "primary"], key + "primary")
    ea, _ = util.with_fresh_overrides(reads[key + "alt"], key + "alt")
    return exp[sel], ea[sel], reads[key + "counters"].tolist()


def run_single(ix, reads, tag, sel, kw=None):
    from snap_amd.aligner import BaseAligner
    L = int(tag)
    b, q = reads["b" + tag][sel], reads["q" + tag][sel]
    offs = np.arange(b.shape[0] + 1, dtype=np.uint64) * L
    a = BaseAligner(ix, abi.default_params(max_read_len=160, **(kw or dict(max_k=8))))
    try:
        a.counters(reset=True)
        prim, alt = a.AlignRead(b, q, offs)
        return prim, alt, a.counters()
    finally:
        a.close()


def check_single_against_fixture(reads, tag, sel, prim, alt, counters, what):
    exp, ea, ec = single_fixture(reads, "default_d8", tag, sel)
    problems = util.compare_results(exp, prim)
    assert (ea["status"] == alt["status"]).all(), what
    found = ea["status"] != 0
    problems += util.compare_results(ea[found], alt[found], "firstALT")
    assert not problems, (what, problems)
    if len(sel) == reads["b" + tag].shape[0]:               # (the fixture's counters are the whole batch's)
        assert work(counters) == ec, what


def check_ag_lds_single(ix, reads, mp, n=None, tags=("100", "150"), lds_forms=("lds", "lds_nohelp")):
    """SNAPGPU_AG_LDS=1 on the 100 and 150 bp golden reads, default_d8: launch_align's `exact` branch at variant 0 -- k_align_single<0>
    with a flag list, then snapgpu_launch_single_exact_0 over 64 waves with `persist` -- with and without the help for heavy reads.  The
    fixture's records and counters, and variant 3's bytes.  The flag count itself stays on the device; a read that went through the
    replay carries bit 31 of `reserved` ("this record is the exact pass's answer", single_kernel.h; in this form only the replay is an exact
    pass), which is asserted to occur.  Returns the number of such reads."""
    replayed = 0
    envs = dict(default={}, lds=dict(AG_LDS=1), lds_nohelp=dict(AG_LDS=1, SINGLE_HELP=0))
    for tag in tags:
        sel = replay_sample(reads, tag, n)
        out = {}
        for name in ("default",) + tuple(lds_forms):
            form(mp, **envs[name])
            out[name] = run_single(ix, reads, tag, sel)
            check_single_against_fixture(reads, tag, sel, *out[name], what=(name, tag))
        for name in lds_forms:
            same_bytes_masked(out["default"][0], out[name][0], (name, tag))
            assert out["default"][1].tobytes() == out[name][1].tobytes(), (name, tag, "firstALT")
            assert work(out["default"][2]) == work(out[name][2]), (name, tag)
            replayed += int(((out[name][0]["reserved"] >> 31) != 0).sum())
    assert replayed > 0, "no read of the batch went through the replay of the flagged reads"
    return replayed


def secondary_replay_sample(z, name, tag, n):
    """n reads of the -om fixture's (None: all of them): the first ones and the reads whose reference answer moves with the aligner object's
    history (see replay_sample), which are the ones the replay redoes."""
    key = "%s_%s_" % (name, tag)
    total = z[key + "primary"].shape[0]
    if n is None or n >= total:
        return np.arange(total)
    moved = z[key + "unstable"].copy()
    for k in ("primary", "secondary", "nsec"):
        moved[util.with_fresh_overrides(z[key + k], "sec_" + key + k)[1]] = True
    return np.union1d(np.arange(n), np.flatnonzero(moved))


def check_ag_lds_single_secondary(ix, reads, mp, n=None, sets=None, tags=("100", "150")):
    """-om single end under SNAPGPU_AG_LDS=1 (snapgpu_launch_single_sec_0, snapgpu_launch_single_exact_0 with secondary results): the option
    sets `sets` (None: all seven) of tests/golden/secondary_reads.npz at the read lengths `tags`, every read of the fixture (or a sample that
    keeps the replayed ones), record order included, and the default form's bytes.  Over the sets that use affine gap, some read must carry
    bit 31 of `reserved`: it went through the replay (see check_ag_lds_single).  Returns (secondary records, replayed reads)."""
    import tests.test_gpu_secondary as gs
    z = np.load(os.path.join(util.GOLDEN, "secondary_reads.npz"))
    all_sets = gs._sets(z)
    total = replayed = 0
    uses_ag = False
    for tag in tags:
        for i in (range(len(all_sets)) if sets is None else sets):
            uses_ag |= bool(all_sets[i][1].get("use_affine_gap", 1))
            t, r = _ag_lds_single_secondary_set(ix, reads, mp, z, all_sets[i], tag, n)
            total += t; replayed += r
    assert total > 0
    assert replayed > 0 or not uses_ag, "no read went through the replay of the flagged reads"
    return total, replayed


def _ag_lds_single_secondary_set(ix, reads, mp, z, the_set, tag, n):
    from snap_amd.aligner import BaseAligner
    total = 0
    for name, kw, om, omax, mpc in (the_set,):
        sel = secondary_replay_sample(z, name, tag, n)
        b, q = reads["b" + tag][sel], reads["q" + tag][sel]
        m = sel.size
        offs = np.arange(m + 1, dtype=np.uint64) * b.shape[1]
        got = {}
        for f, env in (("default", {}), ("lds", dict(AG_LDS=1))):
            form(mp, **env)
            a = BaseAligner(ix, abi.default_params(max_read_len=160, **kw))
            try:
                a.enable_secondary(om, max_results=omax, max_per_contig=mpc)
                got[f] = a.AlignReadSecondary(b, q, offs, stride=4)
            finally:
                a.close()
            key = "%s_%s_" % (name, tag)
            e_prim, _ = util.with_fresh_overrides(z[key + "primary"], "sec_" + key + "primary")
            e_sec, _ = util.with_fresh_overrides(z[key + "secondary"], "sec_" + key + "secondary")
            e_nsec, _ = util.with_fresh_overrides(z[key + "nsec"], "sec_" + key + "nsec")
            problems = util.compare_results(e_prim[sel], got[f][0], "primary")
            problems += util.compare_secondary(e_sec[sel], e_nsec[sel], got[f][2], got[f][3], np.zeros(m, bool))
            assert not problems, (name, f, problems)
        same_bytes_masked(got["default"][0], got["lds"][0], name)
        assert (got["default"][3] == got["lds"][3]).all(), name
        w = min(got["default"][2].shape[1], got["lds"][2].shape[1])
        live = np.arange(w)[None, :] < got["lds"][3][:, None]
        assert got["default"][2][:, :w][live].tobytes() == got["lds"][2][:, :w][live].tobytes(), name
        total += int(got["lds"][3].sum())
    return total, int(((got["lds"][0]["reserved"] >> 31) != 0).sum())


EXACT_REPLAY = 4                                     # SNAPGPU_PAIR_EXACT_REPLAY: the record is the exact pass's answer


def take_pairs(b, q, o, idx):
    """The pairs `idx` of a batch as a batch of their own: (bases, quals, offsets)."""
    o = o.astype(np.int64)
    b, q = b.reshape(-1), q.reshape(-1)
    take = np.concatenate([np.arange(o[2 * i], o[2 * i + 2]) for i in idx])
    lens = np.concatenate([[o[2 * i + 1] - o[2 * i], o[2 * i + 2] - o[2 * i + 1]] for i in idx])
    return b[take], q[take], np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)


def run_paired(pix, z, tag, n, kw=None, pkw=None):
    """n: the first n pairs, or an index array."""
    from snap_amd.aligner import ChimericPairedEndAligner
    if np.ndim(n):
        b, q, o = take_pairs(z["b" + tag], z["q" + tag], z["o" + tag], n)
    else:
        o = z["o" + tag][:2 * n + 1]
        b, q = z["b" + tag].reshape(-1)[:int(o[-1])], z["q" + tag].reshape(-1)[:int(o[-1])]
    a = ChimericPairedEndAligner(pix, abi.default_params(max_read_len=160, **(kw or dict(max_k=8))), abi.default_paired_params(**(pkw or {})))
    try:
        a.counters(reset=True)
        prim, alt = a.align(b, q, o)
        return prim, alt, a.counters()
    finally:
        a.close()


def check_paired_against_fixture(z, tag, n, prim, alt, counters, what):
    key = "default_d8_%s_s0" % tag
    sel = n if np.ndim(n) else np.arange(n)
    exp, _ = util.with_fresh_overrides(z[key + "_primary"], "pe_" + key + "_primary")
    assert not compare_paired(exp[sel], prim, verbose=3).any(), what
    e_alt, _ = util.with_fresh_overrides(z[key + "_alt"], "pe_" + key + "_alt")
    assert (alt["status"] == e_alt["status"][sel]).all(), what
    assert not (prim["flags"] & POOL_OVERFLOW).any(), what
    if len(sel) == (z["o" + tag].size - 1) // 2:
        assert [counters["n_lv_locations"], counters["n_ag_locations"]] == z[key + "_counters"].tolist(), what


def check_ag_lds_paired(pix, z, mp, n=None, tags=("150", "100")):
    """SNAPGPU_AG_LDS=1 through snapgpu_align_paired: snapgpu_launch_paired_0 and snapgpu_launch_paired_exact_0 on the 150 and 100 bp golden
    pairs, default_d8: the fixture's records and counters, and the register form's bytes.  A pair the exact pass redid carries
    SNAPGPU_PAIR_EXACT_REPLAY in `flags`; no golden pair is known to (none of the first 300, none of those fresh_overrides.npz patches), so
    without more the exact kernel would be launched over an empty list.  A third form therefore adds the hook of
    test_exact_replay_of_flagged_pairs, SNAPGPU_DEBUG_PAIRED_FLAG_EVERY=5: every fifth pair is flagged by the main pass and redone by
    snapgpu_launch_paired_exact_0 (asserted: at least that many carry the bit), to the same records.  Returns how many were redone."""
    replayed = 0
    for tag in tags:
        m = n or (z["o" + tag].size - 1) // 2
        out = {}
        for name, env in (("default", {}), ("lds", dict(AG_LDS=1)), ("lds_every5", dict(AG_LDS=1, DEBUG_PAIRED_FLAG_EVERY=5))):
            form(mp, **env)
            out[name] = run_paired(pix, z, tag, m)
            check_paired_against_fixture(z, tag, m, *out[name], what=(name, tag))
        same_pairs(out["default"][0], out["lds"][0], tag)
        same_pairs(out["default"][0], out["lds_every5"][0], (tag, "every fifth pair through the exact pass"), info=EXACT_REPLAY)
        for name in ("lds", "lds_every5"):
            assert out["default"][1].tobytes() == out[name][1].tobytes(), (name, tag)
            assert work(out["default"][2]) == work(out[name][2]), (name, tag)
        r = int(((out["lds_every5"][0]["flags"] & EXACT_REPLAY) != 0).sum())
        assert r >= (m + 4) // 5, (tag, r)
        replayed += r
    return replayed


def check_ag_lds_paired_secondary(pix, mp, n=None, sets=(0, 1)):
    """Paired -om under SNAPGPU_AG_LDS=1 (snapgpu_launch_paired_sec_0, snapgpu_launch_paired_sec_exact_0) against tests/golden/paired_secondary.npz,
    150 bp, option sets `sets` of the fixture's five; excluded are the pairs test_paired_secondary_results_vs_reference_fixture excludes
    (SNAPGPU_PAIR_REF_BUFFER_DEPENDENT).  The two forms' secondary records are the same bytes.  Returns (secondary records, pairs that
    carry SNAPGPU_PAIR_EXACT_REPLAY in the LDS form, which also flags every fifth pair for snapgpu_launch_paired_sec_exact_0 as
    check_ag_lds_paired does; the caller asserts the latter where the option set uses affine gap, without which there is no exact pass)."""
    from snap_amd.aligner import ChimericPairedEndAligner
    z = np.load(os.path.join(util.GOLDEN, "paired_secondary.npz"))
    gp = np.load(os.path.join(util.GOLDEN, "paired_reads.npz"))
    tag = "150"
    m = n or 600
    o = gp["o" + tag][:2 * m + 1]
    b, q = gp["b" + tag][:int(o[-1])], gp["q" + tag][:int(o[-1])]
    total = replayed = 0
    for name, kw, pkw, om, omax, mpc in [load_paired_secondary_sets(z)[i] for i in sets]:
        key = "%s_%s_" % (name, tag)
        ref_t = tuple(util.with_fresh_overrides(z[key + k], "pesec_" + key + k)[0][:m] for k in ("primary", "alt", "secondary", "nsec", "single_secondary", "nssec"))
        got = {}
        # (two forms, not three: creating a context with secondary results costs seconds.  In the second, four pairs of five are scored by
        # snapgpu_launch_paired_sec_0 alone, as under SNAPGPU_AG_LDS=1 by itself.)
        for f, env in (("default", {}), ("lds_every5", dict(AG_LDS=1, DEBUG_PAIRED_FLAG_EVERY=5))):
            form(mp, **env)
            a = ChimericPairedEndAligner(pix, abi.default_params(max_read_len=160, **kw), abi.default_paired_params(**pkw))
            try:
                a.enable_secondary(om, max_results=omax, max_per_contig=mpc)
                got[f] = a.align_secondary(b, q, o, stride=2, single_stride=4)
            finally:
                a.close()
            exclude = (got[f][0]["flags"] & 2) != 0
            assert int(exclude.sum()) <= 2 + m // 100, (name, f)
            assert not compare_paired(ref_t[0], got[f][0], verbose=3, exclude=exclude).any(), (name, f)
            problems = compare_paired_secondary(ref_t, got[f], exclude)
            assert not problems, (name, f, problems)
        lds = got["lds_every5"]
        same_pairs(got["default"][0], lds[0], name, info=EXACT_REPLAY)
        assert (got["default"][3] == lds[3]).all() and (got["default"][5] == lds[5]).all(), name
        assert not compare_paired_secondary(got["default"], lds, np.zeros(m, bool)), name
        total += int(lds[3].sum()) + int(lds[5].sum())
        replayed += int(((got["lds_every5"][0]["flags"] & EXACT_REPLAY) != 0).sum())
    assert total > 0
    return total, replayed


def check_ag_lds_sam_calls(ix, mp, n_single=None, n_pairs=None, n_records=None, pix=None):
    """The one-call SAM paths under SNAPGPU_AG_LDS=1, one option set each, against the reference CLI's records: snapgpu_align_sam_single
    (tests/golden/sam_fields.npz, `default`), snapgpu_align_sam_paired (sam_fields_paired.npz, `default`: snapgpu_launch_paired_clip_0 and
    snapgpu_launch_paired_clip_exact_0) and snapgpu_align_sam_single_records (sam_records_single.npz, `om1_omax4`)."""
    import tests.test_zz_gpu_cigar as gc
    import tests.test_zz_gpu_paired_sam_onecall as oc
    from tests import samrec_util as su
    form(mp, AG_LDS=1)
    z = np.load(os.path.join(util.GOLDEN, "sam_fields.npz"))
    gc.check_align_sam_single_against_reference_cli(ix, z, "default", n=n_single)
    # paired: the fixture's unclipped mates and Read::clip's outcome through the fused call, the fields against the CLI's
    z = np.load(os.path.join(util.GOLDEN, "sam_fields_paired.npz"))
    from snap_amd.aligner import ChimericPairedEndAligner
    m = n_pairs or len(z["default_first_written"])
    offs = z["offsets"][:2 * m + 1]
    bases, quals = z["bases"][:int(offs[-1])], z["quals"][:int(offs[-1])]
    fc, dl = z["front_clip"][:2 * m].astype(np.int32), z["data_len"][:2 * m].astype(np.int32)
    prm = abi.default_params(max_read_len=400)
    batch = dict(bases=bases, quals=quals, offsets=offs)
    _, _, skip = oc.read_clip(batch, False, True, int(prm.max_k))
    out = {}
    pix = pix if pix is not None else util.load_golden_index("paired_index.npz")
    for f, env in (("default", {}), ("lds", dict(AG_LDS=1)), ("lds_every5", dict(AG_LDS=1, DEBUG_PAIRED_FLAG_EVERY=5))):
        form(mp, **env)
        a = ChimericPairedEndAligner(pix, prm, abi.default_paired_params())
        try:
            out[f] = a.alignSamPaired(bases, quals, offs, fc, dl, skip, bool(z["default_use_m"]))
        finally:
            a.close()
    same_pairs(out["default"][0], out["lds"][0], "alignSamPaired results")
    same_pairs(out["default"][0], out["lds_every5"][0], "alignSamPaired results, every fifth pair through the exact pass", info=EXACT_REPLAY)
    for k in oc.FIELD_KEYS:
        assert (out["default"][2][k] == out["lds"][2][k]).all(), k
        assert (out["default"][2][k] == out["lds_every5"][2][k]).all(), (k, "every fifth pair through the exact pass")
    assert ((out["lds_every5"][0]["flags"] & EXACT_REPLAY) != 0).any(), "snapgpu_launch_paired_clip_exact_0 had no pair to redo"
    exp = z["default_results"][:m]
    stable = (out["lds"][2]["stale"].reshape(m, 2) == 0).all(axis=1)
    assert stable.sum() > m * 0.9
    assert not compare_paired(exp, out["lds"][0], verbose=3, exclude=~stable | (skip != 0)).any()
    got = out["lds"][2]
    for k in oc.FIXTURE_KEYS:
        bad = np.flatnonzero((got[k] != z["default_" + k][:2 * m]) & np.repeat(stable, 2))
        assert bad.size == 0, (k, bad[:5])
    # records
    form(mp, AG_LDS=1)
    z = su.fixture()
    tag = "om1_omax4"
    r = min(n_records or (1 << 30), z["offsets"].size - 1)
    offs = z["offsets"][:r + 1]
    got = su.run_set(ix, tag, z["bases"][:int(offs[-1])], z["quals"][:int(offs[-1])], offs, z["front_clip"][:r], z["data_len"][:r])
    exp = su.expected(z, tag)
    keep = exp["rec_read"] < r
    problems, left_out = su.compare({k: v[keep] for k, v in exp.items()}, got, r)
    assert not problems, problems[:5]
    assert left_out <= 2 + r // 100


# ------------------------------------------------------------------------------------------------ B. many work items per wave
def single_wave_slots(ix, mp, **env):
    """n_wave_slots of a single-end context created under `env`: what snapgpu_debug_launch_profile reports for a context that carries the
    phase timers (the slots are num_cus x waves per CU whether or not the timers are on)."""
    from snap_amd.aligner import BaseAligner
    form(mp, PHASE_TIMERS=1, **env)
    a = BaseAligner(ix, abi.default_params(max_k=8, max_read_len=160))
    try:
        b = np.frombuffer(b"ACGT" * 25, dtype=np.uint8)
        a.AlignRead(b, b, np.array([0, 100], np.uint64))
        return int(a.launch_profile()["wave_start"].size)
    finally:
        a.close()


def paired_waves_launched(num_cus, waves_per_cu=4, share=16, over=1.5):
    """snapgpu_enable_paired's wave slots and paired_grid_share's part of them, in waves.  A COPY of the product's arithmetic (snapgpu.hip:
    snapgpu_enable_paired, paired_grid_share) -- a paired launch reports its grid nowhere, and the issue rules out a product hook -- so the
    `n > 2 * waves` assertion of check_many_pairs_per_wave is only as good as this copy: whoever changes that arithmetic changes it here."""
    all_blocks = (num_cus * waves_per_cu & ~3) // 4
    blocks = int(all_blocks * min(1.0, over / share) + 0.999)
    return 4 * max(1, min(blocks, all_blocks))


MANY_SINGLE = dict(WAVES_PER_CU=1)
MANY_PAIRED = dict(PAIRED_WAVES_PER_CU=4, PAIRED_GRID_SHARE=16)


def permuted_half(n, seed=3):
    return np.random.default_rng(seed).permutation(n)[: n // 2]


def check_many_reads_per_wave(ix, reads, mp, n, forms=((1, 0), (0, 0), (1, 1), (0, 1)), tag="100"):
    """SNAPGPU_WAVES_PER_CU=1: n golden reads over num_cus wave slots, so that every wave dequeues several (asserted: n > n_wave_slots, the
    condition under which launch_unit_order runs at all), heavy-first on / off x help off / on: the fixture, each other after masking, the
    same bytes when the batch runs again through the same context, and the same records for a permuted half of it."""
    from snap_amd.aligner import BaseAligner
    slots = single_wave_slots(ix, mp, **MANY_SINGLE)
    assert n > 2 * slots, (n, slots)
    L = int(tag)
    b, q = reads["b" + tag][:n], reads["q" + tag][:n]
    assert b.shape[0] == n
    offs = np.arange(n + 1, dtype=np.uint64) * L
    order = permuted_half(n)
    out = {}
    for heavy, help_on in forms:
        form(mp, SINGLE_HEAVY_FIRST=heavy, SINGLE_HELP=help_on, **MANY_SINGLE)
        a = BaseAligner(ix, abi.default_params(max_k=8, max_read_len=160))
        try:
            a.counters(reset=True)
            prim, alt = a.AlignRead(b, q, offs)
            c = a.counters(reset=True)
            again, alt2 = a.AlignRead(b, q, offs)
            sub, _ = a.AlignRead(b[order], q[order], offs[:order.size + 1])
        finally:
            a.close()
        what = ("heavy_first", heavy, "help", help_on)
        check_single_against_fixture(reads, tag, np.arange(n), prim, alt, c, what)
        assert prim.tobytes() == again.tobytes() and alt.tobytes() == alt2.tobytes(), what
        same_bytes_masked(prim[order], sub, what + ("permuted half",))
        out[(heavy, help_on)] = (prim, alt, c)
    first = out[forms[0]]
    for k, v in out.items():
        same_bytes_masked(first[0], v[0], k)
        assert first[1].tobytes() == v[1].tobytes(), k
        assert work(first[2]) == work(v[2]), k
    form(mp)
    base = run_single(ix, reads, tag, np.arange(n))
    same_bytes_masked(base[0], first[0], "default geometry")
    assert work(base[2]) == work(first[2])
    return slots


def check_many_pairs_per_wave(pix, z, ix, mp, n, tag="150"):
    """SNAPGPU_PAIRED_WAVES_PER_CU=4 with SNAPGPU_PAIRED_GRID_SHARE=16: n golden pairs over the few waves such a launch asks for (asserted:
    n is more than twice that; the wave count is paired_waves_launched's copy of the product's formula over the CU count a single-end
    context reports, not something the paired launch reports), against the fixture, the default geometry's bytes, a second run through the same context and a permuted half."""
    from snap_amd.aligner import ChimericPairedEndAligner
    num_cus = single_wave_slots(ix, mp, **MANY_SINGLE)          # (one wave per CU, rounded up to a workgroup)
    waves = paired_waves_launched(num_cus)
    assert n > 2 * waves, (n, waves)
    form(mp)
    base = run_paired(pix, z, tag, n)
    o = z["o" + tag][:2 * n + 1].astype(np.int64)
    b, q = z["b" + tag].reshape(-1)[:int(o[-1])], z["q" + tag].reshape(-1)[:int(o[-1])]
    order = permuted_half(n)
    bb, qq, oo = take_pairs(b, q, o, order)
    form(mp, **MANY_PAIRED)
    a = ChimericPairedEndAligner(pix, abi.default_params(max_k=8, max_read_len=160), abi.default_paired_params())
    try:
        a.counters(reset=True)
        prim, alt = a.align(b, q, o.astype(np.uint64))
        c = a.counters(reset=True)
        again, alt2 = a.align(b, q, o.astype(np.uint64))
        sub, _ = a.align(bb, qq, oo)
    finally:
        a.close()
    check_paired_against_fixture(z, tag, n, prim, alt, c, "many pairs per wave")
    assert prim.tobytes() == base[0].tobytes() and alt.tobytes() == base[1].tobytes()
    assert work(c) == work(base[2])
    assert prim.tobytes() == again.tobytes() and alt.tobytes() == alt2.tobytes()
    assert sub.tobytes() == prim[order].tobytes()
    return waves


# ------------------------------------------------------------------------------------------------ repeat-built genomes (C, D)
def repeat_bed(d, seed, n_bases, **kw):
    """A genome of high-copy repeats, its index in d/idx (built by the reference's indexer where oracle/_ref is present, by the library's own
    otherwise: the same directory), the loaded index and -- where the compiled reference is present -- a RefIndex over it (else None)."""
    from oracle import ref
    from snap_amd.index import GenomeIndex, build_index
    g = synth.make_genome(seed, n_bases, n_contigs=2, **kw)
    synth.write_fasta(d + "/g.fa", g)
    have_ref = ref.available() and os.path.exists(ref.CLI_PATH)
    if have_ref:
        ref.build_index(d + "/g.fa", d + "/idx", 20, threads=8)
    else:
        os.makedirs(d + "/idx", exist_ok=True)
        build_index(d + "/g.fa", d + "/idx", seed_len=20)
    return g, GenomeIndex.load_from_directory(d + "/idx"), (ref.RefIndex(d + "/idx") if have_ref else None)


# ------------------------------------------------------------------------------------------------ C. the help protocols, forced
HELP_PAIRED_GENOME = dict(seed=11, n_bases=1_200_000, repeat_frac=0.8, max_copies=1200, repeat_len=(400, 1200), max_divergence=0.012)
HELP_SINGLE_GENOME = dict(seed=13, n_bases=1_500_000, repeat_frac=0.85, max_copies=280, repeat_len=(400, 1500), max_divergence=0.03)


def check_paired_help(d, mp, n_pairs=40, help_min=16):
    """The Phase-4 help slots (paired_dev.h) published eagerly, on pairs with long candidate lists: every pair equals the reference with fresh
    aligner objects (where it is present), every byte equals a context created with SNAPGPU_PAIRED_HELP_MIN=0, lists were published, answers
    were used, and no wait ended by the watchdog."""
    from oracle import ref
    from snap_amd.aligner import ChimericPairedEndAligner
    g, gi, rix = repeat_bed(d, **HELP_PAIRED_GENOME)
    pairs = synth.make_pairs(5, g, n_pairs, 150)
    params, pparams = abi.default_params(max_k=8, max_read_len=160), abi.default_paired_params()
    out = {}
    for name, env in (("eager", dict(PAIRED_HELP_MIN=help_min, PAIRED_HELP_EAGER=1)), ("alone", dict(PAIRED_HELP_MIN=0))):
        form(mp, **env)
        a = ChimericPairedEndAligner(gi, params, pparams)
        try:
            a.counters(reset=True)
            got, alt = a.align(pairs["bases"], pairs["quals"], pairs["offsets"])
            out[name] = (got, alt, a.counters())
        finally:
            a.close()
    ce, ca = out["eager"][2], out["alone"][2]
    assert ce["help_watchdog_events"] == 0 and ca["help_watchdog_events"] == 0
    assert ce["help_lists_published"] > 0 and ce["help_answers_used"] > 0, ce
    assert ca["help_lists_published"] == 0 and ca["help_answers_used"] == 0, ca
    assert out["eager"][0].tobytes() == out["alone"][0].tobytes() and out["eager"][1].tobytes() == out["alone"][1].tobytes()
    assert work(ce) == work(ca)
    if rix is not None:
        with ref.fresh_objects():
            exp, _, rcnt, _ = rix.align_paired(params, pparams, pairs["bases"], pairs["quals"], pairs["offsets"], threads=8, stage=0)
        assert not compare_paired(exp, out["eager"][0], verbose=3).any()
        assert (ce["n_lv_locations"], ce["n_ag_locations"]) == (rcnt["lv"], rcnt["ag"])
    return ce


def check_single_help(d, mp, n_reads=160):
    """se_help.h: a forced walk's remaining candidates published eagerly for idle waves, on reads out of diverged high-copy repeats, against
    SNAPGPU_SINGLE_HELP=0: the same records (`reserved` under INFO_MASK), the same work counters -- the reference's where it is present --,
    lists published, answers used, no watchdog event."""
    from oracle import ref
    from snap_amd.aligner import BaseAligner
    g, ix, rix = repeat_bed(d, **HELP_SINGLE_GENOME)
    reads = synth.make_reads(7, g, n_reads, 150)
    params = abi.default_params(max_k=8, max_read_len=160)
    out = {}
    for name, env in (("eager", dict(SINGLE_HELP=1, SINGLE_HELP_EAGER=1)), ("off", dict(SINGLE_HELP=0))):
        form(mp, **env)
        a = BaseAligner(ix, params)
        try:
            a.counters(reset=True)
            got, alt = a.AlignRead(reads["bases"], reads["quals"], reads["offsets"])
            out[name] = (got, alt, a.counters())
        finally:
            a.close()
    ce, co = out["eager"][2], out["off"][2]
    assert ce["help_lists_published"] > 0 and ce["help_answers_used"] > 0 and ce["help_watchdog_events"] == 0, ce
    assert co["help_lists_published"] == 0 and co["help_watchdog_events"] == 0, co
    for k in ("n_hash_table_lookups", "n_hits_consumed", "n_lv_locations", "n_ag_locations", "n_lv_ref_bytes"):
        assert ce[k] == co[k], k
    same_bytes_masked(out["off"][0], out["eager"][0], "help eager against help off")
    assert out["off"][1].tobytes() == out["eager"][1].tobytes()
    if rix is not None:
        with ref.fresh_objects():
            exp, _, rc, _ = rix.align_single(params, reads["bases"], reads["quals"], reads["offsets"], threads=8)
        for name in out:
            assert not util.compare_results(exp, out[name][0]), name
        assert work(ce) == [rc["lookups"], rc["lv"], rc["ag"]]
    return ce


# ------------------------------------------------------------------------------------------------ D. the overflow passes of launch_paired
# EXACT copies of up to 1 200 per family: a mate out of a large family has more than 512 Phase-4 candidates, none of which needs affine-gap
# scoring, so the pair is cheap and still outgrows a first pass of 64 and a second of 512 entries.  Of the 32 pairs of seed 5, pair 6 is such a
# pair (more than 512, at most 1 024 candidates); pairs 4 .. 11 are the batch, the smallest that meets the conditions.
OVERFLOW_GENOME = dict(seed=29, n_bases=1_200_000, repeat_frac=0.8, max_copies=1200, repeat_len=(400, 1200), max_divergence=0.0)
# The emulator twin runs the same eight pairs (not 24 - 40): they meet every condition, and a larger batch only adds pairs no pass flags.
OVERFLOW_PAIRS, OVERFLOW_KEEP = 32, (4, 12)


def raw_align_paired(a, b, q, o):
    """snapgpu_align_paired without the mirror's exception: (return code, last error, results, first-ALT results)."""
    b = np.ascontiguousarray(b, dtype=np.uint8).reshape(-1); q = np.ascontiguousarray(q, dtype=np.uint8).reshape(-1)
    o = np.ascontiguousarray(o, dtype=np.uint64)
    n = (o.size - 1) // 2
    prim = np.zeros(n, dtype=abi.PAIRED_RESULT_DTYPE); alt = np.zeros(n, dtype=abi.PAIRED_RESULT_DTYPE)
    rc = a.lib.snapgpu_align_paired(a.handle, C.c_uint32(n), abi.ptr(b), abi.ptr(q), abi.ptr(o), abi.ptr(prim), abi.ptr(alt))
    return rc, (a.lib.snapgpu_last_error(a.handle) if rc else b""), prim, alt


def raw_align_paired_secondary(a, b, q, o, stride=16, single_stride=64):
    b = np.ascontiguousarray(b, dtype=np.uint8).reshape(-1); q = np.ascontiguousarray(q, dtype=np.uint8).reshape(-1)
    o = np.ascontiguousarray(o, dtype=np.uint64)
    n = (o.size - 1) // 2
    prim = np.zeros(n, dtype=abi.PAIRED_RESULT_DTYPE); alt = np.zeros(n, dtype=abi.PAIRED_RESULT_DTYPE)
    sec = np.zeros((n, stride), dtype=abi.PAIRED_RESULT_DTYPE); nsec = np.zeros(n, dtype=np.uint32)
    ssec = np.zeros((n, single_stride), dtype=abi.RESULT_DTYPE); nssec = np.zeros((n, 2), dtype=np.uint32)
    rc = a.lib.snapgpu_align_paired_secondary(a.handle, C.c_uint32(n), abi.ptr(b), abi.ptr(q), abi.ptr(o), abi.ptr(prim), abi.ptr(alt), abi.ptr(sec),
                                              C.c_uint32(stride), abi.ptr(nsec), abi.ptr(ssec), C.c_uint32(single_stride), abi.ptr(nssec))
    return rc, (a.lib.snapgpu_last_error(a.handle) if rc else b""), prim, alt, nsec, nssec, sec, ssec


def raw_align_sam_paired(a, b, q, o, use_m=True, ops_stride=64):
    """snapgpu_align_sam_paired on reads nothing is clipped from, without the mirror's exception: (return code, last error, results, fields)."""
    b = np.ascontiguousarray(b, dtype=np.uint8).reshape(-1); q = np.ascontiguousarray(q, dtype=np.uint8).reshape(-1)
    o = np.ascontiguousarray(o, dtype=np.uint64)
    n = o.size - 1; npairs = n // 2
    fc = np.zeros(n, np.int32); dl = np.diff(o.astype(np.int64)).astype(np.int32); skip = np.zeros(npairs, np.uint8)
    res = np.zeros(npairs, dtype=abi.PAIRED_RESULT_DTYPE); alt = np.zeros(npairs, dtype=abi.PAIRED_RESULT_DTYPE)
    f = dict(flag=np.zeros(n, np.int32), contig=np.zeros(n, np.int32), pos=np.zeros(n, np.int64), mapq=np.zeros(n, np.int32),
             ops=np.zeros((n, ops_stride), np.uint32), n_ops=np.zeros(n, np.int32), nm=np.zeros(n, np.int32), rnext=np.zeros(n, np.int32),
             pnext=np.zeros(n, np.int64), tlen=np.zeros(n, np.int64), first_written=np.zeros(npairs, np.int32), stale=np.zeros(n, np.int32))
    p = abi.ptr
    rc = a.lib.snapgpu_align_sam_paired(a.handle, C.c_uint32(npairs), p(b), p(q), p(o), p(fc), p(dl), p(skip), C.c_int(1 if use_m else 0), p(res), p(alt),
                                        p(f["flag"]), p(f["contig"]), p(f["pos"]), p(f["mapq"]), p(f["ops"]), C.c_uint32(ops_stride), p(f["n_ops"]), p(f["nm"]),
                                        p(f["rnext"]), p(f["pnext"]), p(f["tlen"]), p(f["first_written"]), p(f["stale"]))
    return rc, (a.lib.snapgpu_last_error(a.handle) if rc else b""), res, f


def flagged(prim):
    return (prim["flags"] & POOL_OVERFLOW) != 0


class OverflowBed:
    """The workload of the overflow tests: pairs out of a genome of high-copy repeats, their answers at the default capacities (no pair
    flagged) and -- where the compiled reference is present -- the reference's."""
    def __init__(self, d, mp, keep=OVERFLOW_KEEP, seed=5):
        from oracle import ref
        self.g, self.gi, self.rix = repeat_bed(d, **OVERFLOW_GENOME)
        pr = synth.make_pairs(seed, self.g, OVERFLOW_PAIRS, 150)
        o = pr["offsets"][2 * keep[0]:2 * keep[1] + 1].astype(np.int64)
        self.pairs = dict(bases=pr["bases"].reshape(-1)[o[0]:o[-1]].copy(), quals=pr["quals"].reshape(-1)[o[0]:o[-1]].copy(), offsets=(o - o[0]).astype(np.uint64))
        self.params, self.pparams = abi.default_params(max_k=8, max_read_len=160), abi.default_paired_params()
        self.n = keep[1] - keep[0]
        self.mp = mp
        self.at_cap = {}
        rc, _, self.base, self.base_alt = self.run()
        assert rc == 0 and not flagged(self.base).any()
        self.exp = None
        if self.rix is not None:
            with ref.fresh_objects():
                self.exp = self.rix.align_paired(self.params, self.pparams, self.pairs["bases"], self.pairs["quals"], self.pairs["offsets"], threads=8, stage=0)[0]
            assert not compare_paired(self.exp, self.base, verbose=3).any()

    def aligner(self, **env):
        from snap_amd.aligner import ChimericPairedEndAligner
        form(self.mp, **env)
        try:
            return ChimericPairedEndAligner(self.gi, self.params, self.pparams)
        finally:
            form(self.mp)                                  # (read at snapgpu_enable_paired; nothing stays set between tests)

    def run(self, **env):
        a = self.aligner(**env)
        try:
            return raw_align_paired(a, self.pairs["bases"], self.pairs["quals"], self.pairs["offsets"])
        finally:
            a.close()

    def paired_at(self, cap):
        """snapgpu_align_paired under SNAPGPU_PAIRED_AGC_CAP=cap, run once and kept: (return code, last error, results, first-ALT results).
        F(cap) of the tests is flagged(paired_at(cap)[2])."""
        if cap not in self.at_cap:
            self.at_cap[cap] = self.run(PAIRED_AGC_CAP=cap)
        return self.at_cap[cap]

    def run_only(self, idx, **env):
        """The pairs `idx` as a batch of their own: (return code, results, n_lv_locations of the call)."""
        b, q, o = take_pairs(self.pairs["bases"], self.pairs["quals"], self.pairs["offsets"], idx)
        a = self.aligner(**env)
        try:
            a.counters(reset=True)
            rc, _, prim, _ = raw_align_paired(a, b, q, o)
            return rc, prim, a.counters()["n_lv_locations"]
        finally:
            a.close()

    def check_unflagged(self, prim, alt, what):
        """every pair that is not flagged: the default capacities' bytes (and so the reference's records)"""
        ok = ~flagged(prim)
        same_pairs(self.base, prim, what, sel=ok)
        same_pairs(self.base_alt, alt, what, sel=ok)
        if self.exp is not None:
            assert not compare_paired(self.exp, prim, verbose=3, exclude=~ok).any(), what

    def check_report(self, rc, msg, prim, what):
        if flagged(prim).any():
            assert rc == E_UNSUPPORTED and POOL_OVERFLOW_TEXT in msg, (what, rc, msg)
        else:
            assert rc == 0, (what, rc, msg)


def check_agc_overflow_passes(bed, caps=(64, 128, 512)):
    """SNAPGPU_PAIRED_AGC_CAP=C: the first pass holds C affine-gap candidates per pair, the second (pargs_big, 256 waves, reached through
    `remap`) 8 C.  F(C): the pairs still flagged when the call returns.  Required of the workload, so that the test cannot pass vacuously:
    F(64) is not empty and F(512) is a strict subset of it -- some pair overflowed a first pass of 512 <= 8 * 64 entries (it is in F(64)) and
    is not flagged at C = 512: the second pass completed it."""
    F = {}
    for cap in caps:
        rc, msg, prim, alt = bed.paired_at(cap)
        F[cap] = flagged(prim)
        bed.check_report(rc, msg, prim, cap)
        bed.check_unflagged(prim, alt, cap)
    lo, hi = caps[0], caps[-1]
    assert F[lo].any(), "no pair overflows %d candidates twice" % (8 * lo)
    for a_, b_ in zip(caps, caps[1:]):
        assert not (F[b_] & ~F[a_]).any(), (a_, b_)                  # F(64) >= F(128) >= F(512)
    rescued = F[lo] & ~F[hi]
    assert rescued.any(), "no pair that overflowed the first pass was completed by the second"
    # ... and that is what happened to them, whatever the capacities of the two passes are: as a batch of their own at C = 512 they all end
    # unflagged with the default capacities' bytes, and the call scored more locations than it does at the default capacity -- a pair was
    # begun in the first pass, given up there and done again by the second.
    idx = np.flatnonzero(rescued)
    rc0, base, lv0 = bed.run_only(idx)
    rc1, prim, lv1 = bed.run_only(idx, PAIRED_AGC_CAP=hi)
    assert rc0 == 0 and rc1 == 0 and not flagged(prim).any()
    assert prim.tobytes() == base.tobytes() == bed.base[idx].tobytes()
    assert lv1 > lv0, (lv0, lv1)
    return {c: int(f.sum()) for c, f in F.items()}, int(rescued.sum())


def check_agc_overflow_secondary(bed, cap=512, lo=64):
    """The same rescue through snapgpu_align_paired_secondary (pargs_sec_big: setup_paired_secondary copies the first pass's ag_cand_cap and
    multiplies it by 8, as snapgpu_enable_paired does, so C means the same).  Whether a pair fits a candidate buffer does not depend on
    secondary results being kept, so the pairs this call leaves flagged at C are exactly snapgpu_align_paired's F(C), which
    check_agc_overflow_passes shows to be what a first pass of C and a second of 8 C entries leave: with a second pass that did nothing, or
    one no larger than the first, the pairs of F(64) - F(512) that hold more than 512 candidates would stay flagged here at C = 512.  Every
    unflagged pair: the default capacity's records, secondary records included, byte for byte."""
    assert (flagged(bed.paired_at(lo)[2]) & ~flagged(bed.paired_at(cap)[2])).any()          # the workload's condition, whichever test runs first
    out, lv = {}, {}
    for c in (None, cap):                                    # (a context with secondary results costs seconds: C = 64 is left to the other two calls)
        a = bed.aligner(**({} if c is None else dict(PAIRED_AGC_CAP=c)))
        try:
            a.enable_secondary(1)
            a.counters(reset=True)
            out[c] = raw_align_paired_secondary(a, bed.pairs["bases"], bed.pairs["quals"], bed.pairs["offsets"])
            lv[c] = a.counters()["n_lv_locations"]
        finally:
            a.close()
    rc0, _, base, base_alt, nsec0, nssec0, sec0, ssec0 = out[None]
    assert rc0 in (0, 1) and not flagged(base).any()
    assert int(nsec0.sum()) + int(nssec0.sum()) > 0
    if bed.exp is not None:
        assert not compare_paired(bed.exp, base, verbose=3, exclude=(base["flags"] & 2) != 0).any()
    for c in (cap,):
        rc, msg, prim, alt, nsec, nssec, sec, ssec = out[c]
        assert (flagged(prim) == flagged(bed.paired_at(c)[2])).all(), ("-om", c, np.flatnonzero(flagged(prim)), np.flatnonzero(flagged(bed.paired_at(c)[2])))
        ok = ~flagged(prim)
        if ok.all():
            assert rc in (0, 1), (c, rc, msg)
        else:
            assert rc == E_UNSUPPORTED and POOL_OVERFLOW_TEXT in msg, (c, rc, msg)
        same_pairs(base, prim, ("-om", c), sel=ok)
        same_pairs(base_alt, alt, ("-om firstALT", c), sel=ok)
        assert (nsec0[ok] == nsec[ok]).all() and (nssec0[ok] == nssec[ok]).all(), c
        live = (np.arange(sec.shape[1])[None, :] < nsec[:, None]) & ok[:, None]
        assert sec0[live].tobytes() == sec[live].tobytes(), ("-om secondary records", c)
        nss = nssec.sum(axis=1)                              # (a pair's single-end secondary records: mate 0's, then mate 1's)
        live = (np.arange(ssec.shape[1])[None, :] < nss[:, None]) & ok[:, None]
        assert ssec0[live].tobytes() == ssec[live].tobytes(), ("-om single-end secondary records", c)
    rescued = flagged(bed.paired_at(lo)[2]) & ~flagged(out[cap][2])         # (in F(64), and this call leaves them unflagged at C = 512)
    assert rescued.any()
    # ... by this call's own second pass: no pair is left flagged at C = 512, and yet the call scored more locations than at the default
    # capacity -- a pair was begun in the first pass, given up at 512 candidates and done again in pargs_sec_big's larger buffers.
    assert not flagged(out[cap][2]).any() and lv[cap] > lv[None], (lv, np.flatnonzero(flagged(out[cap][2])))
    return int(rescued.sum())


def check_agc_overflow_sam_call(bed, cap=512, lo=64):
    """The same rescue through snapgpu_align_sam_paired, whose report is the COUNT of the pairs still flagged after the second pass: a batch
    whose overflowing pairs were all rescued returns SNAPGPU_OK and the default capacities' fields; one with a pair left returns
    SNAPGPU_E_UNSUPPORTED with the pool-overflow text.  The pairs left flagged at C are exactly snapgpu_align_paired's F(C) (see
    check_agc_overflow_secondary: a dead or unenlarged second pass behind snapgpu_launch_paired_clip_N leaves more of them at C = 512)."""
    assert (flagged(bed.paired_at(lo)[2]) & ~flagged(bed.paired_at(cap)[2])).any()          # the workload's condition, whichever test runs first
    out, lv = {}, {}
    for c in (None, lo, cap):
        a = bed.aligner(**({} if c is None else dict(PAIRED_AGC_CAP=c)))
        try:
            a.counters(reset=True)
            out[c] = raw_align_sam_paired(a, bed.pairs["bases"], bed.pairs["quals"], bed.pairs["offsets"])
            lv[c] = a.counters()["n_lv_locations"]
        finally:
            a.close()
    rc0, _, base, f0 = out[None]
    assert rc0 == 0 and base.tobytes() == bed.base.tobytes()
    for c in (lo, cap):
        rc, msg, res, f = out[c]
        assert (flagged(res) == flagged(bed.paired_at(c)[2])).all(), ("sam", c, np.flatnonzero(flagged(res)), np.flatnonzero(flagged(bed.paired_at(c)[2])))
        bed.check_report(rc, msg, res, ("sam", c))
        ok = ~flagged(res)
        same_pairs(base, res, ("sam", c), sel=ok)
        for k, v in f.items():
            m = ok if v.shape[0] == ok.size else np.repeat(ok, 2)
            assert (v[m] == f0[k][m]).all(), (c, k)
    assert out[lo][0] == E_UNSUPPORTED
    rescued = flagged(out[lo][2]) & ~flagged(out[cap][2])
    assert rescued.any()
    # ... by this call's own second pass (see check_agc_overflow_secondary): nothing left flagged at C = 512, more locations scored
    assert out[cap][0] == 0 and not flagged(out[cap][2]).any() and lv[cap] > lv[None], (lv, np.flatnonzero(flagged(out[cap][2])))
    return int(rescued.sum())


def check_pool_overflow_is_reported(bed, pool=64):
    """SNAPGPU_PAIRED_POOL=64: pargs_big keeps the first pass's pool_size (only the affine-gap candidate buffers grow), so a pair whose
    candidate POOL overflows is flagged again by the second pass and reported -- the documented limit (the reference
    refuses such a read and asks for -mcp): error code, text, flagged pairs, and every unflagged pair equal to the default bytes."""
    rc, msg, prim, alt = bed.run(PAIRED_POOL=pool)
    assert flagged(prim).any()
    assert rc == E_UNSUPPORTED and POOL_OVERFLOW_TEXT in msg, (rc, msg)
    assert (~flagged(prim)).any()
    bed.check_unflagged(prim, alt, "pool")
    return int(flagged(prim).sum())
