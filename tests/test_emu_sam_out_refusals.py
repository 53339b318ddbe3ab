"""The 17 SAM / BAM / BGZF output calls of the C ABI on the wavefront emulator (tests/emu/): what each answers to a call it refuses -- the
return code, the text of snapgpu_last_error, every output word -- and to the smallest calls it accepts, row by row of the table in
tests/sam_out_refusals_util.py.  The same rows as tests/test_zz_gpu_sam_out_refusals.py.

Test infrastructure only: see tests/test_emu_kernels.py for how the emulated library is swapped in."""
import os
import shutil

import pytest

from tests import sam_out_refusals_util as ru

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
def contexts(emu):
    c = ru.Contexts()
    try:
        yield c
    finally:
        c.close()


def test_the_table_has_every_call_and_every_defect():
    assert sorted({r[0] for r in ru.ROWS}) == ru.CALLS
    assert [(r[0], r[1]) for r in ru.ROWS] == [(c, d) for c in ru.CALLS for d in ru.defects_of(c)]
    assert all((r[2] < 0) == bool(r[3]) for r in ru.ROWS)                    # a refusal has a message, and nothing else has


@pytest.mark.parametrize("call", ru.CALLS)
def test_emu_rows(emu, contexts, call):
    from tests import util
    assert ru.check_call(contexts, util.HipBuffers(emu=True), call, ru.ROWS) >= 9
