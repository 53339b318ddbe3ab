"""The hot / cold split of the affine-gap functions (snap_amd/csrc/ag_win.h: ag_hot_fn, ag_cold_fn) on the emulated device: the fixture of
handcrafted problems at the edges of the selection (tests/golden/ag_forms.npz, answers of the compiled reference) through both batch entries
of the primitive, every field."""
import os
import shutil

import pytest

from tests import ag_forms_util as fu

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


def test_fixture_covers_the_edges_of_the_selection():
    fu.fixture_covers_the_edges()


@pytest.mark.parametrize("gap_open", [1, 6])
def test_emu_ag_forms_vs_reference(emu, golden_index, gap_open):
    n_plain, n_exact = fu.check_gap_open(golden_index, gap_open)
    assert n_plain > 150 and n_exact > 150
