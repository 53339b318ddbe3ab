"""snapgpu_bam_sort / _device and snapgpu_align_sam_single_bam_sorted / _paired_bam_sorted on the wavefront emulator (tests/emu/): the BAM records
of a batch into coordinate order.  The device code that runs here is the code the GPU runs (bam_sort.h: the key pass, radix_pass.h's stable LSD
pass -- the index builder's --, sam_text.h's 64-bit scan, the gather between two byte addresses of any alignment).  What the output must be is
restated in plain Python in tests/bam_sort_util.py.  The same cases as tests/test_zz_gpu_bam_sort.py, with fewer reads in the fused calls.

Test infrastructure only: see tests/test_emu_kernels.py for how the emulated library is swapped in."""
import os
import shutil

import pytest

from tests import bam_sort_util as bs
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


@pytest.fixture(scope="module")
def sorter(emu, golden_index):
    a = bs.make_aligner(golden_index)
    yield a
    a.close()


def test_restatement_on_a_case_worked_by_hand():
    recs = bs.make_records([1, -1, 0, 1, 0], [7, -1, 9, -1, 9], [12, 13, 14, 15, 16])
    _, begin, key, perm = bs.restate(recs)
    assert perm.tolist() == [2, 4, 3, 0, 1] and begin.tolist() == [0, 14, 30, 45, 57, 70]
    assert key.tolist() == [10, 10, 1 << 32, (1 << 32) | 8, 0xFFFFFFFF << 32]


def test_emulated_library_exports_the_sort_calls(emu):
    from snap_amd.aligner import EXPORTED_SYMBOLS
    for name in bs.SYMBOLS:
        assert name in EXPORTED_SYMBOLS and hasattr(emu, name), name


@pytest.mark.parametrize("name", list(bs.all_cases()))
def test_emu_sort_equals_the_restatement(sorter, name):
    bs.check_case(sorter, bs.all_cases()[name], name)


def test_emu_key_and_perm_are_optional(sorter):
    bs.check_optional_outputs(sorter)


def test_emu_every_source_and_destination_residue(sorter):
    bs.check_host_residues(sorter)


def test_emu_device_form(emu, sorter):
    from tests import util
    bs.check_device_form(sorter, util.HipBuffers(emu=True))


def test_emu_refusals(emu, sorter):
    from tests import util
    bs.check_refusals(sorter, util.HipBuffers(emu=True))


@pytest.mark.parametrize("tag", list(su.SETS))
def test_emu_fused_single_call(emu, golden_index, tag):
    assert bs.check_fused_single(golden_index, tag, n=40) >= 40


def test_emu_fused_single_call_tiny_reads(emu, golden_index):
    bs.check_fused_tiny_reads(golden_index, n=48)


def test_emu_fused_paired_call(emu):
    from tests import util
    bs.check_fused_paired(util.load_golden_index("paired_index.npz"), n_pairs=24)


def _needs_ref():
    from oracle import ref
    if not ref.available() or not os.path.exists(ref.CLI_PATH):
        pytest.skip("oracle/_ref not built here (it builds the test index)")


@pytest.fixture(scope="module")
def tool_workloads(tmp_path_factory):
    _needs_ref()
    out = {}
    for mode in ("single", "paired"):
        d = str(tmp_path_factory.mktemp("so_" + mode))
        out[mode] = (d, bs.make_tool_workload(d, mode))
    return out


@pytest.mark.parametrize("mode,opts", bs.TOOL_CASES, ids=["%s%s" % (m, "".join(o).replace("-", "_")) for m, o in bs.TOOL_CASES])
def test_emu_tool_sorted_bam(emu, tool_workloads, mode, opts):
    from tests.emu.build import TOOL
    d, workload = tool_workloads[mode]
    n, runs = bs.check_tool(TOOL, d, mode, opts, env=dict(SNAPGPU_EMU_CUS="4"), workload=workload)
    assert n >= (160 if mode == "single" else 112) and runs >= 5


def test_emu_tool_refuses_sorted_sam(emu, tool_workloads):
    from tests.emu.build import TOOL
    d, workload = tool_workloads["single"]
    bs.check_tool_refuses_sorted_sam(TOOL, d, workload)
