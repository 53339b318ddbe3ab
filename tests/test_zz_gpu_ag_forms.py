"""The hot / cold split of the affine-gap functions (snap_amd/csrc/ag_win.h: ag_hot_fn, ag_cold_fn) on the GPU: the fixture of handcrafted
problems at the edges of the selection (tests/golden/ag_forms.npz, answers of the compiled reference) through both batch entries of the
primitive (k_ag_batch), every field, both text directions."""
import pytest

from tests import ag_forms_util as fu

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("gap_open", [1, 6])
def test_gpu_ag_forms_vs_reference(golden_index, gap_open):
    n_plain, n_exact = fu.check_gap_open(golden_index, gap_open)
    assert n_plain > 150 and n_exact > 150
