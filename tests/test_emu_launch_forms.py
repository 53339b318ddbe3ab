"""Emulator twin of tests/test_zz_gpu_launch_forms.py: the same check_* functions (tests/launch_forms_util.py) on the wavefront emulator
(tests/emu/) at reduced counts.  The emulator runs many items per wave already (4 "compute units"), so of B only the heavy-first on / off
pair is kept; its fibers run in sequence, so it cannot see a missing wait or fence between two waves -- that is what the GPU module is for.
Pattern and fixture as tests/test_emu_kernels.py."""
import os
import shutil

import numpy as np
import pytest

from tests import launch_forms_util as lf
from tests import util

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ needed to build the wavefront emulator")


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


@pytest.fixture(scope="module")
def pindex():
    return util.load_golden_index("paired_index.npz")


@pytest.fixture(scope="module")
def golden_pairs():
    return np.load(os.path.join(util.GOLDEN, "paired_reads.npz"))


def test_emu_lds_affine_gap_form_single_end(emu, golden_index, golden_reads, monkeypatch):
    """One read length and the form with the help only: the emulator cannot tell the two apart (the help's hand-offs are sequential there)."""
    assert lf.check_ag_lds_single(golden_index, golden_reads, monkeypatch, n=24, tags=("100",), lds_forms=("lds",)) > 0


def test_emu_lds_affine_gap_form_single_end_secondary(emu, golden_index, golden_reads, monkeypatch):
    total, replayed = lf.check_ag_lds_single_secondary(golden_index, golden_reads, monkeypatch, n=24, sets=(0,), tags=("100",))
    assert total > 0 and replayed > 0


def test_emu_lds_affine_gap_form_paired(emu, pindex, golden_pairs, monkeypatch):
    assert lf.check_ag_lds_paired(pindex, golden_pairs, monkeypatch, n=16, tags=("150",)) > 0


def test_emu_lds_affine_gap_form_paired_secondary(emu, pindex, monkeypatch):
    total, replayed = lf.check_ag_lds_paired_secondary(pindex, monkeypatch, n=12, sets=(0,))
    assert total > 0 and replayed > 0


def test_emu_lds_affine_gap_form_one_call_sam_paths(emu, golden_index, pindex, monkeypatch):
    lf.check_ag_lds_sam_calls(golden_index, monkeypatch, n_single=60, n_pairs=24, n_records=60, pix=pindex)


def test_emu_heavy_first_order_on_and_off(emu, golden_index, golden_reads, monkeypatch):
    assert lf.check_many_reads_per_wave(golden_index, golden_reads, monkeypatch, n=40, forms=((1, 0), (0, 0))) == 4


def test_emu_paired_help_forced(emu, tmp_path, monkeypatch):
    lf.check_paired_help(str(tmp_path), monkeypatch, n_pairs=24, help_min=16)


def test_emu_single_end_help_forced(emu, tmp_path, monkeypatch):
    lf.check_single_help(str(tmp_path), monkeypatch, n_reads=64)


@pytest.fixture(scope="module")
def overflow_bed(emu, tmp_path_factory):
    mp = pytest.MonkeyPatch()
    try:
        yield lf.OverflowBed(str(tmp_path_factory.mktemp("overflow")), mp)
    finally:
        mp.undo()


def test_emu_second_pass_completes_pairs_that_overflowed_the_first(overflow_bed):
    counts, rescued = lf.check_agc_overflow_passes(overflow_bed)
    assert rescued > 0 and counts[64] > counts[512]


def test_emu_second_pass_with_secondary_results(overflow_bed):
    assert lf.check_agc_overflow_secondary(overflow_bed) > 0


def test_emu_second_pass_through_the_one_call_sam_path(overflow_bed):
    assert lf.check_agc_overflow_sam_call(overflow_bed) > 0


def test_emu_candidate_pool_overflow_is_reported_not_rescued(overflow_bed):
    assert lf.check_pool_overflow_is_reported(overflow_bed) > 0
