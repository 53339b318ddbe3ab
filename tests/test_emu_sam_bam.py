"""snapgpu_bam_records_single / _paired (and _device), snapgpu_align_sam_single_bam / _paired_bam on the wavefront emulator (tests/emu/):
records to the bytes of their BAM records.  The device code that runs here is the code the GPU runs (sam_bam.h: the length pass, sam_text.h's
64-bit scan, the write pass with its byte-wise fixed head, the packed SEQ and the shifted QUAL with their byte-wise ends and dword middle).
What a record must be is restated in plain Python in tests/bam_util.py, which is held against the reference CLI's own BAM bytes
(tests/golden/bam_records.npz) before the device code is held against it.  The same checks as tests/test_zz_gpu_sam_bam.py, at reduced
counts where a count is the test's to choose.

Test infrastructure only: see tests/test_emu_kernels.py for how the emulated library is swapped in."""
import os
import shutil

import pytest

from tests import bam_util as bu
from tests import samrec_util as su

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


@pytest.mark.parametrize("tag", list(su.SETS))
def test_restatement_equals_the_reference_cli_single(tag):
    assert bu.check_restatement_against_reference("single", tag) >= 200


@pytest.mark.parametrize("tag", bu.PAIRED_TAGS)
def test_restatement_equals_the_reference_cli_paired(tag):
    assert bu.check_restatement_against_reference("paired", tag) >= 200


def test_emulated_library_exports_the_bam_calls(emu):
    from snap_amd.aligner import EXPORTED_SYMBOLS
    for name in bu.SYMBOLS:
        assert name in EXPORTED_SYMBOLS and hasattr(emu, name), name


def test_emu_handcrafted_records_equal_the_restatement(emu, golden_index):
    h, exp = bu.check_handcrafted(golden_index)
    assert len(exp) >= 150


def test_emu_handcrafted_pair_units_equal_the_restatement(emu, golden_index):
    h, exp = bu.check_handcrafted_pairs(golden_index)
    assert len(exp) >= 200


def test_emu_memory_discipline(emu, golden_index):
    bu.check_memory_discipline(golden_index)


def test_emu_scan_levels(emu, golden_index):
    bu.check_scan_levels(golden_index)


def test_emu_argument_errors(emu, golden_index):
    bu.check_errors(golden_index)


def test_emu_device_form_equals_the_host_form(emu, golden_index):
    from tests import util
    bu.check_device_form(golden_index, util.HipBuffers(emu=True))


@pytest.mark.parametrize("tag", list(su.SETS))
def test_emu_records_equal_the_reference_cli_single(emu, golden_index, tag):
    bu.check_against_reference(golden_index, "single", tag)


@pytest.mark.parametrize("tag", bu.PAIRED_TAGS)
def test_emu_records_equal_the_reference_cli_paired(emu, tag):
    from tests import util
    bu.check_against_reference(util.load_golden_index("paired_index.npz"), "paired", tag)


def test_emu_fused_single_call_equals_records_then_bam(emu, golden_index):
    bu.check_fused_single(golden_index)


def test_emu_fused_paired_call_equals_fields_then_bam(emu):
    from tests import util
    bu.check_fused_paired(util.load_golden_index("paired_index.npz"), n_pairs=60)


def test_emu_tool_with_device_bam(emu, tmp_path):
    """`snapgpu-sam -o x.bam` with SNAPGPU_SAM_DEVICE_BAM=1 on the emulated library: the reference CLI's BAM, the switch-off file byte for
    byte, and the stderr line; as test_emu_native_fastq_to_bam."""
    from oracle import ref
    if not ref.available() or not os.path.exists(ref.CLI_PATH):
        pytest.skip("oracle/_ref not built here")
    from tests.emu.build import TOOL
    from tests.test_zz_gpu_native_sam import make_paired_workload, make_workload
    env = dict(os.environ, SNAPGPU_EMU_CUS="4")
    ds, dp = str(tmp_path / "s"), str(tmp_path / "p")
    os.makedirs(ds); os.makedirs(dp)
    index_dir, fastq = make_workload(ds, 400, genome_bases=300_000)
    assert bu.check_tool(TOOL, ds, "single", index_dir, [fastq], ["-om", "1", "-omax", "3"], env, tool_opts=["-b", "128"]) > 400
    index_dir, fq = make_paired_workload(dp, 150, genome_bases=300_000)
    assert bu.check_tool(TOOL, dp, "paired", index_dir, fq, [], env) == 300
