"""Landau-Vishkin (snap_amd/csrc/lv.h) on the GPU against the compiled reference at every level, length and form: tests/golden/lv_forms.npz
(scripts/make_golden_lv_forms.py) through k_lv_batch as it is (ByteSeq, LDS triangle) and in the two forms the kernels run,
SNAPGPU_LV_FORM=lds (LdsSeq: every call of the aligners) and =hbm (lv_compute<false>: the paired-end kernel's calls with a limit above
AlignCfg::kmax).  All five fields, both directions, every batch also from a guarded layout."""
import pytest

from tests import lv_forms_util as fu

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("form", fu.FORMS)
def test_gpu_lv_forms_vs_reference(golden_index, form):
    assert fu.check_form(golden_index, form) >= (1400 if form == "lds" else 1500)
