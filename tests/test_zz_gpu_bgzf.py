"""snapgpu_bgzf_compress / _device on the device: the checks of tests/test_emu_bgzf.py through the same utility (tests/bgzf_util.py), against
Python's zlib / gzip / struct.  The SHA-256 constant of bgzf_util was computed on the emulator: asserting it here states that the GPU and the
emulator produce the same bytes."""
import pytest

from tests import bgzf_util as bz
from tests import util

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden_ix():
    return util.load_golden_index()


def test_library_exports_the_bgzf_calls():
    from snap_amd.aligner import EXPORTED_SYMBOLS, load_library
    lib = load_library()
    for name in bz.SYMBOLS:
        assert name in EXPORTED_SYMBOLS and hasattr(lib, name), name


def test_empty_and_tiny_inputs(golden_ix):
    bz.check_empty_and_tiny(golden_ix)


def test_full_members(golden_ix):
    bz.check_full_members(golden_ix)


def test_many_members(golden_ix):
    bz.check_many_members(golden_ix)


@pytest.mark.parametrize("tag", sorted(bz.fixture_arrays()))
def test_reference_bytes(golden_ix, tag):
    bz.check_fixture(golden_ix, tag)


def test_determinism(golden_ix):
    bz.check_determinism(golden_ix)


def test_memory_discipline_and_argument_errors(golden_ix):
    bz.check_memory_discipline(golden_ix)


def test_device_form_equals_the_host_form(golden_ix):
    bz.check_device_form(golden_ix, util.HipBuffers())


def test_fused_single_call_equals_the_bam_call(golden_ix):
    bz.check_fused_single(golden_ix)


def test_fused_paired_call_equals_the_bam_call():
    bz.check_fused_paired(util.load_golden_index("paired_index.npz"), n_pairs=60)


def _needs_ref():
    import os
    from oracle import ref
    if not ref.available() or not os.path.exists(ref.CLI_PATH):
        pytest.skip("oracle/_ref not on this box")


def test_tool_single_with_device_bgzf(tmp_path):
    """-b 128 over 400 reads with -om 1 -omax 3: several batches"""
    _needs_ref()
    from tests.test_zz_gpu_native_sam import TOOL, make_workload
    d = str(tmp_path)
    index_dir, fastq = make_workload(d, 400, genome_bases=300_000)
    n, batches = bz.check_tool(TOOL, d, "single", index_dir, [fastq], ["-om", "1", "-omax", "3"], tool_opts=["-b", "128"])
    assert n > 400 and batches == 4


def test_tool_paired_with_device_bgzf(tmp_path):
    _needs_ref()
    from tests.test_zz_gpu_native_sam import TOOL, make_paired_workload
    d = str(tmp_path)
    index_dir, fq = make_paired_workload(d, 150, genome_bases=300_000)
    n, batches = bz.check_tool(TOOL, d, "paired", index_dir, fq, [])
    assert n == 300 and batches >= 1
