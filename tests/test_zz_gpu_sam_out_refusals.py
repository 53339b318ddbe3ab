"""The 17 SAM / BAM / BGZF output calls of the C ABI on the GPU: what each answers to a call it refuses -- the return code, the text of
snapgpu_last_error, every output word -- and to the smallest calls it accepts, row by row of the table in tests/sam_out_refusals_util.py.
The same rows as tests/test_emu_sam_out_refusals.py; a refused call launches nothing."""
import pytest

from tests import sam_out_refusals_util as ru

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def contexts():
    c = ru.Contexts()
    try:
        yield c
    finally:
        c.close()


@pytest.mark.parametrize("call", ru.CALLS)
def test_gpu_rows(contexts, call):
    from tests import util
    assert ru.check_call(contexts, util.HipBuffers(), call, ru.ROWS) >= 9
