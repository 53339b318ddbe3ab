"""snapgpu_bgzf_compress / _device on the wavefront emulator (tests/emu/): bytes to BGZF blocks.  The device code that runs here is the code
the GPU runs (bgzf.h: LZ77 over an LDS hash table, length-limited Huffman codes, the bit emission with its shared dwords, the CRC32 combine,
sam_text.h's 64-bit scan, the copy into place).  The checks are those of tests/test_zz_gpu_bgzf.py (tests/bgzf_util.py, held against
Python's zlib / gzip / struct); the SHA-256 constant there states that the emulator and the GPU produce the same bytes.

Test infrastructure only: see tests/test_emu_kernels.py for how the emulated library is swapped in."""
import os
import shutil

import pytest

from tests import bgzf_util as bz

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


def test_emulated_library_exports_the_bgzf_calls(emu):
    from snap_amd.aligner import EXPORTED_SYMBOLS
    for name in bz.SYMBOLS:
        assert name in EXPORTED_SYMBOLS and hasattr(emu, name), name


def test_emu_empty_and_tiny_inputs(emu, golden_index):
    bz.check_empty_and_tiny(golden_index)


@pytest.mark.parametrize("case", ["run", "exact", "plus_one", "random", "window", "fib24"])
def test_emu_full_members(emu, golden_index, case):
    bz.check_full_members(golden_index, (case,))


@pytest.mark.parametrize("shape", [(64, 300000), (1000, 70000)])
def test_emu_many_members(emu, golden_index, shape):
    bz.check_many_members(golden_index, (shape,))


@pytest.mark.parametrize("tag", sorted(bz.fixture_arrays()))
def test_emu_reference_bytes(emu, golden_index, tag):
    bz.check_fixture(golden_index, tag)


def test_emu_determinism_across_grids(emu, golden_index):
    """the same input twice, and under 1 and 4 emulated CUs (the grid follows the CU count), gives equal bytes"""
    saved = os.environ.get("SNAPGPU_EMU_CUS")
    try:
        outs = []
        for cus in ("1", "4"):
            os.environ["SNAPGPU_EMU_CUS"] = cus
            outs.append(bz.check_determinism(golden_index))
        assert outs[0] == outs[1]
    finally:
        if saved is None:
            os.environ.pop("SNAPGPU_EMU_CUS", None)
        else:
            os.environ["SNAPGPU_EMU_CUS"] = saved


def test_emu_memory_discipline_and_argument_errors(emu, golden_index):
    bz.check_memory_discipline(golden_index)


def test_emu_device_form_equals_the_host_form(emu, golden_index):
    from tests import util
    bz.check_device_form(golden_index, util.HipBuffers(emu=True))


def test_emu_fused_single_call_equals_the_bam_call(emu, golden_index):
    bz.check_fused_single(golden_index, n=60)


def test_emu_fused_paired_call_equals_the_bam_call(emu):
    from tests import util
    bz.check_fused_paired(util.load_golden_index("paired_index.npz"), n_pairs=60)


def test_emu_tool_with_device_bgzf(emu, tmp_path):
    """`snapgpu-sam -o x.bam` with SNAPGPU_SAM_DEVICE_BGZF=1 on the emulated library, the workloads of test_emu_tool_with_device_bam: the
    reference CLI's records, the members of the switch-off file, the end-of-file block and the stderr line"""
    from oracle import ref
    if not ref.available() or not os.path.exists(ref.CLI_PATH):
        pytest.skip("oracle/_ref not built here")
    from tests.emu.build import TOOL
    from tests.test_zz_gpu_native_sam import make_paired_workload, make_workload
    env = dict(os.environ, SNAPGPU_EMU_CUS="4")
    ds, dp = str(tmp_path / "s"), str(tmp_path / "p")
    os.makedirs(ds); os.makedirs(dp)
    index_dir, fastq = make_workload(ds, 400, genome_bases=300_000)
    n, batches = bz.check_tool(TOOL, ds, "single", index_dir, [fastq], ["-om", "1", "-omax", "3"], env, tool_opts=["-b", "128"])
    assert n > 400 and batches == 4
    index_dir, fq = make_paired_workload(dp, 150, genome_bases=300_000)
    n, batches = bz.check_tool(TOOL, dp, "paired", index_dir, fq, [], env)
    assert n == 300 and batches >= 1
