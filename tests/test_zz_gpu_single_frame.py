"""The single-end kernel's Aligner lives in a per-wave LDS frame (kernel_common.h: SE_FRAME_BYTES; single_kernel.h).  The shapes at which
such a frame can go wrong, each against the committed reference fixtures (tests/golden/tiny_reads.npz, secondary_reads.npz), bit for bit:

1. carve-outs of neighbouring waves: four waves of a block holding different reads, at max_read_len 160 and at the largest max_read_len the
   192-position affine-gap variant takes with -d 8 (212: every block of the carve-out at its maximum, the frame behind them);
2. every instantiation that includes single_kernel.h: default (fast form + replay, and the exact form as the one pass), -om, the phase
   timers, the plane Landau-Vishkin, and one long-read context each for the affine-gap variants 4, 6 and 0;
3. state carried from read to read in one wave: one batch, the reversed batch and batches of one read on a context with one wave per CU,
   with a read shorter than a seed and a read of all 'N' among them;
4. the help for heavy reads on one context, published eagerly, whose helper branch uses the frame after the wave's last read.
"""
import ast
import os

import numpy as np
import pytest

from snap_amd import abi, synth
from tests import launch_forms_util as lf
from tests import util

pytestmark = pytest.mark.gpu

N = 512                     # the reads smoke() aligns: 128 blocks of four waves, every wave of a block on a read of its own
AGC3_MAX_READ_LEN_D8 = 212  # ag_max_positions(max_read_len - 20, 9) <= 192 up to here (ag_reg.h); RL = 224


@pytest.fixture(scope="module")
def expected(golden_reads):
    """The fixture's answers, computed once: {tag: (primary, first ALT)} of the default -d 8 set with the fresh-object patches."""
    out = {}
    for tag in ("100", "150"):
        key = "default_d8_%s_" % tag
        out[tag] = (util.with_fresh_overrides(golden_reads[key + "primary"], key + "primary")[0],
                    util.with_fresh_overrides(golden_reads[key + "alt"], key + "alt")[0])
    return out


def _align(ix, reads, tag, n, max_read_len=160, secondary=None):
    from snap_amd.aligner import BaseAligner
    L = int(tag)
    b, q = reads["b" + tag][:n], reads["q" + tag][:n]
    offs = np.arange(n + 1, dtype=np.uint64) * L
    a = BaseAligner(ix, abi.default_params(max_k=8, max_read_len=max_read_len))
    try:
        if secondary is None:
            return a.AlignRead(b, q, offs)
        a.enable_secondary(secondary[0], max_results=secondary[1], max_per_contig=secondary[2])
        return a.AlignReadSecondary(b, q, offs, stride=4)
    finally:
        a.close()


def _check(expected, tag, n, prim, alt, what):
    exp, ea = expected[tag][0][:n], expected[tag][1][:n]
    problems = util.compare_results(exp, prim)
    assert (ea["status"] == alt["status"]).all(), what
    found = ea["status"] != 0
    problems += util.compare_results(ea[found], alt[found], "firstALT")
    assert not problems, (what, problems)


@pytest.mark.parametrize("max_read_len", [160, AGC3_MAX_READ_LEN_D8])
@pytest.mark.parametrize("help_on", ["1", "0"])
def test_carve_outs_of_block_mates(golden_index, golden_reads, expected, monkeypatch, max_read_len, help_on):
    """help on: k_align_single<3> + the replay <3, false, true> on 64 waves; off: the exact form as the one pass (the kernel the benchmark
    times)."""
    lf.form(monkeypatch, SINGLE_HELP=help_on)
    prim, alt = _align(golden_index, golden_reads, "100", N, max_read_len)
    _check(expected, "100", N, prim, alt, (max_read_len, help_on))


def test_secondary_instantiations(golden_index, golden_reads, monkeypatch):
    """-om: k_align_single<3, true> and its exact twin, the first set of the secondary fixture on the same 512 reads."""
    lf.form(monkeypatch)
    z = np.load(os.path.join(util.GOLDEN, "secondary_reads.npz"))
    name, kw, om, omax, mpc = [(str(r[0]), ast.literal_eval(str(r[1])), int(r[2]), int(r[3]), int(r[4])) for r in z["sets"]][0]
    assert kw == dict(max_k=8), kw
    prim, alt, sec, nsec = _align(golden_index, golden_reads, "100", N, secondary=(om, omax, mpc))
    key = "%s_100_" % name
    e_prim = util.with_fresh_overrides(z[key + "primary"], "sec_" + key + "primary")[0][:N]
    e_sec = util.with_fresh_overrides(z[key + "secondary"], "sec_" + key + "secondary")[0][:N]
    e_nsec = util.with_fresh_overrides(z[key + "nsec"], "sec_" + key + "nsec")[0][:N]
    problems = util.compare_results(e_prim, prim, "primary") + util.compare_secondary(e_sec, e_nsec, sec, nsec, np.zeros(N, bool))
    assert not problems, problems
    assert int(nsec.sum()) > 0


@pytest.mark.parametrize("switch", ["PHASE_TIMERS", "LV_PLANES"])
@pytest.mark.parametrize("help_on", ["1", "0"])
def test_timed_and_plane_instantiations(golden_index, golden_reads, expected, monkeypatch, switch, help_on):
    lf.form(monkeypatch, SINGLE_HELP=help_on, **{switch: 1})
    prim, alt = _align(golden_index, golden_reads, "100", N)
    _check(expected, "100", N, prim, alt, (switch, help_on))


@pytest.mark.parametrize("max_read_len", [256, 400, 512])
def test_long_read_contexts(golden_index, golden_reads, expected, monkeypatch, max_read_len):
    """k_align_single<4>, <6> and <0> with their replays (max_read_len 256 / 400 / 512 at -d 8: ag_max_positions > 192 / 256 / 384): the
    150 bp fixture reads, whose answers do not depend on the context's max_read_len."""
    lf.form(monkeypatch)
    n = 256
    prim, alt = _align(golden_index, golden_reads, "150", n, max_read_len)
    _check(expected, "150", n, prim, alt, max_read_len)


@pytest.mark.parametrize("help_on", ["0", "1"])
def test_state_carried_from_read_to_read(golden_index, golden_reads, expected, monkeypatch, help_on):
    """One wave per CU (256 wave slots or fewer: every wave takes several of the 512 reads): the batch, the reversed batch and 512 batches of
    one read.  Reads 100 and 300 are replaced by a read shorter than a seed and by a read of all 'N' -- the reads after which a per-read
    field that nobody reset would show.  Help off: the exact form is the only pass and the three runs are the same bytes; help on: who
    scored a read shows in the two top bits of `reserved` (launch_forms_util.INFO_MASK), everything else is the same bytes."""
    from snap_amd.aligner import BaseAligner
    slots = lf.single_wave_slots(golden_index, monkeypatch, WAVES_PER_CU=1)
    assert N > slots, (N, slots)
    lf.form(monkeypatch, WAVES_PER_CU=1, SINGLE_HELP=help_on)
    b, q = golden_reads["b100"][:N], golden_reads["q100"][:N]
    lens = np.full(N, 100, dtype=np.int64); lens[100] = 12
    rows_b = [b[i, :lens[i]].copy() for i in range(N)]
    rows_q = [q[i, :lens[i]].copy() for i in range(N)]
    rows_b[300][:] = ord("N")

    def batch(order):
        offs = np.concatenate([[0], np.cumsum(lens[order])]).astype(np.uint64)
        return np.concatenate([rows_b[i] for i in order]), np.concatenate([rows_q[i] for i in order]), offs

    a = BaseAligner(golden_index, abi.default_params(max_k=8, max_read_len=160))
    try:
        fwd = np.arange(N); rev = fwd[::-1]
        p_f, a_f = a.AlignRead(*batch(fwd))
        p_r, a_r = a.AlignRead(*batch(rev))
        one = [a.AlignRead(*batch(np.array([i]))) for i in range(N)]
    finally:
        a.close()
    p_1 = np.concatenate([o[0] for o in one]); a_1 = np.concatenate([o[1] for o in one])
    if help_on == "0":
        assert p_f.tobytes() == p_r[::-1].tobytes() and p_f.tobytes() == p_1.tobytes()
    else:
        lf.same_bytes_masked(p_f, p_r[::-1], "reversed"); lf.same_bytes_masked(p_f, p_1, "one read per batch")
    assert a_f.tobytes() == a_r[::-1].tobytes() and a_f.tobytes() == a_1.tobytes()
    for i in (100, 300):
        assert p_f["status"][i] == abi.NOT_FOUND and p_f["location"][i] == abi.INVALID_GENOME_LOCATION_32, i
    keep = np.ones(N, bool); keep[[100, 300]] = False
    assert not util.compare_results(expected["100"][0][:N][keep], p_f[keep])


# tests/test_gpu_repeats.py's genome of diverged high-copy repeats and its single-end reads (seed 11), cut to HELP_READS = 2: the one read of
# a batch of one has no forced walk long enough for a list (SE_HELP_MIN_ITEMS), of a batch of two one has -- the smallest count that publishes.
HELP_GENOME = dict(seed=23, n_bases=1_500_000, repeat_frac=0.75, max_copies=900, repeat_len=(300, 1500), max_divergence=0.02)
HELP_READS = 2


def test_help_on_one_context(tmp_path, monkeypatch):
    """se_help.h with one context (one feeder), the fast form, lists published eagerly: the same records (`reserved` under INFO_MASK) and
    work counters as with the help off.  After its last read every wave goes through the helper branch, which loads reads into its LDS and
    evaluates candidates through the frame."""
    from snap_amd.aligner import BaseAligner
    g, ix, _ = lf.repeat_bed(str(tmp_path), **HELP_GENOME)
    rd = synth.make_reads(11, g, HELP_READS, 150)
    offs = np.arange(HELP_READS + 1, dtype=np.uint64) * 150
    params = abi.default_params(max_k=8, max_read_len=160)
    out = {}
    for name, env in (("eager", dict(SINGLE_HELP=1, SINGLE_HELP_EAGER=1)), ("off", dict(SINGLE_HELP=0))):
        lf.form(monkeypatch, **env)
        a = BaseAligner(ix, params)
        try:
            a.counters(reset=True)
            got, alt = a.AlignRead(rd["bases"].reshape(-1), rd["quals"].reshape(-1), offs)
            out[name] = (got, alt, a.counters())
        finally:
            a.close()
    ce, co = out["eager"][2], out["off"][2]
    print("help lists published with %d reads: %d, answers used %d" % (HELP_READS, ce["help_lists_published"], ce["help_answers_used"]))
    assert ce["help_lists_published"] > 0 and ce["help_watchdog_events"] == 0, ce
    assert co["help_lists_published"] == 0 and co["help_watchdog_events"] == 0, co
    for k in ("n_hash_table_lookups", "n_hits_consumed", "n_lv_locations", "n_ag_locations", "n_lv_ref_bytes"):
        assert ce[k] == co[k], k
    lf.same_bytes_masked(out["off"][0], out["eager"][0], "help eager against help off")
    assert out["off"][1].tobytes() == out["eager"][1].tobytes()
