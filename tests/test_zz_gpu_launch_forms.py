"""The launch forms and overflow passes no other GPU test selects (tests/launch_forms_util.py): the LDS affine-gap form (variant 0) on the
short-read fixtures, several work items per wave, the two help protocols forced, and the second pass of launch_paired over pairs that
overflowed the first.  Each test asserts itself that the form did run: reads went through the replay, n > n_wave_slots, help lists were
published and answers used without a watchdog event, a pair overflowed the first pass and was completed by the second.
Emulator twin: tests/test_emu_launch_forms.py."""
import os

import numpy as np
import pytest

from tests import launch_forms_util as lf
from tests import util

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pindex():
    return util.load_golden_index("paired_index.npz")


@pytest.fixture(scope="module")
def golden_pairs():
    return np.load(os.path.join(util.GOLDEN, "paired_reads.npz"))


# ---- A. SNAPGPU_AG_LDS=1
def test_lds_affine_gap_form_single_end(golden_index, golden_reads, monkeypatch):
    assert lf.check_ag_lds_single(golden_index, golden_reads, monkeypatch) > 0


@pytest.mark.parametrize("option_set", range(7))
def test_lds_affine_gap_form_single_end_secondary(golden_index, golden_reads, monkeypatch, option_set):
    """Every read of tests/golden/secondary_reads.npz, 100 and 150 bp, one of its seven option sets per case."""
    lf.check_ag_lds_single_secondary(golden_index, golden_reads, monkeypatch, sets=(option_set,))


@pytest.mark.parametrize("tag", ["150", "100"])
def test_lds_affine_gap_form_paired(pindex, golden_pairs, monkeypatch, tag):
    assert lf.check_ag_lds_paired(pindex, golden_pairs, monkeypatch, tags=(tag,)) > 0


@pytest.mark.parametrize("option_set", range(5))
def test_lds_affine_gap_form_paired_secondary(pindex, monkeypatch, option_set):
    """All 600 pairs of tests/golden/paired_secondary.npz, one of its five option sets per case (set 3 scores without affine gap: it has no
    exact pass, and only shows that the switch changes nothing there)."""
    total, replayed = lf.check_ag_lds_paired_secondary(pindex, monkeypatch, sets=(option_set,))
    assert total > 0 and (replayed > 0 or option_set == 3)


def test_lds_affine_gap_form_one_call_sam_paths(golden_index, pindex, monkeypatch):
    lf.check_ag_lds_sam_calls(golden_index, monkeypatch, n_single=1500, n_pairs=600, n_records=975, pix=pindex)


# ---- B. many items per wave
def test_many_reads_per_wave(golden_index, golden_reads, monkeypatch):
    """1 500 golden reads over one wave per CU (256 slots on an MI355X: about six reads per wave, n > n_wave_slots)."""
    lf.check_many_reads_per_wave(golden_index, golden_reads, monkeypatch, n=1500)


def test_many_pairs_per_wave(pindex, golden_pairs, golden_index, monkeypatch):
    """600 golden pairs over the 96 waves a launch asks for with four waves per CU and a sixteenth of the chip."""
    lf.check_many_pairs_per_wave(pindex, golden_pairs, golden_index, monkeypatch, n=600)


# ---- C. the help protocols, published eagerly
def test_paired_help_forced(tmp_path, monkeypatch):
    lf.check_paired_help(str(tmp_path), monkeypatch, n_pairs=40, help_min=16)


def test_single_end_help_forced(tmp_path, monkeypatch):
    lf.check_single_help(str(tmp_path), monkeypatch, n_reads=160)


# ---- D. the overflow passes of launch_paired
@pytest.fixture(scope="module")
def overflow_bed(tmp_path_factory):
    mp = pytest.MonkeyPatch()
    try:
        yield lf.OverflowBed(str(tmp_path_factory.mktemp("overflow")), mp)
    finally:
        mp.undo()


def test_second_pass_completes_pairs_that_overflowed_the_first(overflow_bed):
    counts, rescued = lf.check_agc_overflow_passes(overflow_bed)
    assert rescued > 0 and counts[64] > counts[512]


def test_second_pass_with_secondary_results(overflow_bed):
    assert lf.check_agc_overflow_secondary(overflow_bed) > 0


def test_second_pass_through_the_one_call_sam_path(overflow_bed):
    assert lf.check_agc_overflow_sam_call(overflow_bed) > 0


def test_candidate_pool_overflow_is_reported_not_rescued(overflow_bed):
    assert lf.check_pool_overflow_is_reported(overflow_bed) > 0
