"""snapgpu_sam_text_single / _device and snapgpu_align_sam_single_text on the wavefront emulator (tests/emu/): records to the bytes of
their SAM lines.  The device code that runs here is the code the GPU runs (sam_text.h: the length pass, the 64-bit scan of the line
offsets, the write pass with its byte-wise head and tail and dword middle of SEQ and QUAL).  What a line must be is restated in plain
Python in tests/samtext_util.py.

Not tested: text beyond 2^32 bytes, which would need a 4 GB buffer; line_begin, text_bytes and every sum on the way to them are 64-bit
by construction (uint64 arrays in the ABI, samtext_incl_scan64 and unsigned long long carries in the kernels).

Test infrastructure only: see tests/test_emu_kernels.py for how the emulated library is swapped in."""
import os
import shutil

import pytest

from tests import samrec_util as su
from tests import samtext_util as tu

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


def test_emulated_library_exports_the_text_calls(emu):
    for name in ("snapgpu_set_contig_names", "snapgpu_sam_text_single", "snapgpu_sam_text_single_device", "snapgpu_align_sam_single_text"):
        assert hasattr(emu, name), name


def test_emu_handcrafted_records_equal_the_restatement(emu, golden_index):
    h, exp, cn = tu.check_handcrafted(golden_index)
    assert len(exp) >= 200


def test_emu_memory_discipline(emu, golden_index):
    tu.check_memory_discipline(golden_index)


def test_emu_scan_levels(emu, golden_index):
    assert all(t < 300_000 for t in tu.scan_tile_sizes())
    tu.check_scan_levels(golden_index)


def test_emu_contig_names_are_required_and_counted(emu, golden_index):
    tu.check_contig_names(golden_index)


@pytest.mark.parametrize("tag", list(su.SETS))
def test_emu_text_equals_the_reference_cli(emu, golden_index, tag):
    n_lines, left_out = tu.check_against_reference(golden_index, tag)
    print("%s: %d lines, %d reads left out (reference_history_dependent)" % (tag, n_lines, left_out))


def test_emu_fused_call_equals_records_then_text(emu, golden_index):
    tu.check_fused_equals_two_calls(golden_index)


def test_emu_device_form_equals_the_host_form(emu, golden_index):
    from tests import util
    tu.check_device_form(golden_index, util.HipBuffers(emu=True))
