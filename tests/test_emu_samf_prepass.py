"""Emulator twin of tests/test_zz_gpu_samf_prepass.py: the row-loop pre-pass (k_samf_dp8, k_samf_dp8_rec, k_samf_dp8_paired) on the wavefront
emulator (tests/emu/), the same check_* functions with the class list intact -- every class at RL = 64, the row-cap class also at 145 (= 9 * 16 + 1:
a read of RL bases whose last rows the cap RL + 16 cuts off) and 400 (where the pre-pass is not launched) -- and the random-order batch cut to 64 items.  Pattern and fixture as
tests/test_emu_kernels.py."""
import os
import shutil

import pytest

import tests.test_zz_gpu_samf_prepass as sp

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ needed to build the wavefront emulator")

EMU_SPEC = dict(rls=[64], rowcap_rls=[145, 400], n_random=64, n_reads=40, rec_rls=[64])


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
def single_on(emu, golden_index):
    return sp.run_single(golden_index, EMU_SPEC)


@pytest.fixture(scope="module")
def all_off(emu, tmp_path_factory):
    import snap_amd.aligner as al
    return sp.run_child("all", EMU_SPEC, tmp_path_factory.mktemp("samf") / "off.npz", al.LIB_PATH)


def test_emu_valid_count_is_the_predicates(emu, golden_index, single_on):
    table = sp.check_who_took_the_prepass(golden_index, EMU_SPEC, single_on)
    assert all(table[(64, c)][0] > 0 for c in sp.ELIGIBLE_CLASSES) and table[(145, "rowcap")][0] > 0
    sp.check_no_prepass_without_affine_gap(golden_index)


def test_emu_single_end_with_the_prepass_equals_without(emu, golden_index, single_on, all_off):
    sp.check_on_equals_off(single_on, all_off)


def test_emu_records_satisfy_the_cigar_properties(emu, golden_index, single_on):
    sp.check_single_properties(golden_index, EMU_SPEC, single_on)


def test_emu_eligible_records_equal_the_reference(emu, golden_index, single_on, tmp_path):
    ri = sp.reference_index(golden_index, tmp_path)
    if ri is None:
        pytest.skip("oracle/_ref not built here")
    assert sp.check_against_reference(golden_index, EMU_SPEC, single_on, ri) > 300


def test_emu_paired_mates_with_the_prepass(emu, golden_index, single_on, all_off):
    on = sp.run_paired(golden_index, EMU_SPEC)
    sp.check_paired_against_single(golden_index, EMU_SPEC, single_on, on)
    sp.check_on_equals_off(on, all_off)


def test_emu_record_list_with_the_prepass(emu, golden_index, all_off):
    on = sp.run_records(golden_index, EMU_SPEC)
    sp.check_records_valid(golden_index, EMU_SPEC, on)
    sp.check_on_equals_off(on, all_off)
