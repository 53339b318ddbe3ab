"""Landau-Vishkin (snap_amd/csrc/lv.h) on the emulated device against the compiled reference at every level, length and form:
tests/golden/lv_forms.npz (scripts/make_golden_lv_forms.py) through snapgpu_landau_vishkin as it is (ByteSeq, LDS triangle) and in the two
forms the kernels run, SNAPGPU_LV_FORM=lds (LdsSeq: every call of the aligners) and =hbm (lv_compute<false>: the paired-end kernel's calls
with a limit above AlignCfg::kmax).  All five fields, both directions; tests.util.oracle_lv on the same problems as a third opinion.

What these tests cannot see, because no input can: lv.h without the upper `qi` clamp of the forward pass, or without `d + i < 0` in build_mask,
answers every problem alike (DESIGN.md section 12 has the argument; both were tried, 0 of 795 problems changed in any form)."""
import os
import shutil

import pytest

from tests import lv_forms_util as fu

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


def test_fixture_covers_the_edges_of_landau_vishkin():
    fu.fixture_covers_the_edges()


def test_c_restatement_agrees_with_the_reference_on_the_fixture():
    assert fu.check_restatement() >= 800


@pytest.mark.parametrize("form", fu.FORMS)
def test_emu_lv_forms_vs_reference(emu, golden_index, form):
    assert fu.check_form(golden_index, form) >= (1400 if form == "lds" else 1500)
