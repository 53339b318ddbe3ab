"""snapgpu_bam_sort / _device and snapgpu_align_sam_single_bam_sorted / _paired_bam_sorted on the device: the BAM records of a batch into
coordinate order.  The cases of tests/test_emu_bam_sort.py through the same utility (tests/bam_sort_util.py), whose plain-Python restatement
-- keys from the record bytes, the stable sort, the records concatenated in that order -- is the whole definition of the output."""
import pytest

from tests import bam_sort_util as bs
from tests import samrec_util as su
from tests import util

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden_ix():
    return util.load_golden_index()


@pytest.fixture(scope="module")
def sorter(golden_ix):
    a = bs.make_aligner(golden_ix)
    yield a
    a.close()


def test_library_exports_the_sort_calls():
    from snap_amd.aligner import EXPORTED_SYMBOLS, load_library
    lib = load_library()
    for name in bs.SYMBOLS:
        assert name in EXPORTED_SYMBOLS and hasattr(lib, name), name


@pytest.mark.parametrize("name", list(bs.all_cases()))
def test_sort_equals_the_restatement(sorter, name):
    bs.check_case(sorter, bs.all_cases()[name], name)


def test_key_and_perm_are_optional(sorter):
    bs.check_optional_outputs(sorter)


def test_every_source_and_destination_residue(sorter):
    bs.check_host_residues(sorter)


def test_device_form(sorter):
    bs.check_device_form(sorter, util.HipBuffers())


def test_refusals(sorter):
    bs.check_refusals(sorter, util.HipBuffers())


@pytest.mark.parametrize("tag", list(su.SETS))
def test_fused_single_call(golden_ix, tag):
    assert bs.check_fused_single(golden_ix, tag, n=150) >= 150


def test_fused_single_call_tiny_reads(golden_ix):
    bs.check_fused_tiny_reads(golden_ix, n=120)


def test_fused_paired_call():
    bs.check_fused_paired(util.load_golden_index("paired_index.npz"), n_pairs=150)


# ---------------------------------------------------------------------------------------- the tool
import os  # noqa: E402

from oracle import ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.environ.get("SNAPGPU_TEST_TOOL") or os.path.join(ROOT, "snap_amd", "snapgpu-sam")
needs_ref = pytest.mark.skipif(not ref.available() or not os.path.exists(ref.CLI_PATH), reason="oracle/_ref not on this box (it builds the test index)")
CASE_IDS = ["%s%s" % (m, "".join(o).replace("-", "_")) for m, o in bs.TOOL_CASES]


@pytest.fixture(scope="module")
def tool_workloads(tmp_path_factory):
    out = {}
    for mode in ("single", "paired"):
        d = str(tmp_path_factory.mktemp("so_" + mode))
        out[mode] = (d, bs.make_tool_workload(d, mode))
    return out


@needs_ref
@pytest.mark.parametrize("mode,opts", bs.TOOL_CASES, ids=CASE_IDS)
def test_tool_sorted_bam(tool_workloads, mode, opts):
    d, workload = tool_workloads[mode]
    n, runs = bs.check_tool(TOOL, d, mode, opts, workload=workload)
    assert n >= (160 if mode == "single" else 112) and runs >= 5


@needs_ref
def test_tool_refuses_sorted_sam(tool_workloads):
    d, workload = tool_workloads["single"]
    bs.check_tool_refuses_sorted_sam(TOOL, d, workload)


@needs_ref
@pytest.mark.parametrize("mode,opts", bs.TOOL_CASES, ids=CASE_IDS)
def test_tool_sorted_bam_against_the_reference_cli(tool_workloads, mode, opts):
    d, workload = tool_workloads[mode]
    where = bs.check_tool_against_reference(TOOL, d, mode, opts, workload)
    print("the reference's -so file has its refID -1 records:", where)
