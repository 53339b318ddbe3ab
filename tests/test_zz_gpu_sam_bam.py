"""snapgpu_bam_records_single / _paired (and _device), snapgpu_align_sam_single_bam / _paired_bam on the device: the checks of
tests/test_emu_sam_bam.py through the same utility (tests/bam_util.py), and `snapgpu-sam -o x.bam` with SNAPGPU_SAM_DEVICE_BAM=1 -- the
records written by the device -- against the reference CLI's BAM and against the tool's own host formatter."""
import os
import subprocess

import pytest

from oracle import ref
from tests import bam_util as bu
from tests import samrec_util as su
from tests import util
from tests.test_zz_gpu_native_sam import (make_paired_alt_workload, make_paired_workload, make_workload,  # noqa: F401
                                          run_and_compare_paired, sam_lines)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.environ.get("SNAPGPU_TEST_TOOL") or os.path.join(ROOT, "snap_amd", "snapgpu-sam")
needs_ref = pytest.mark.skipif(not ref.available() or not os.path.exists(ref.CLI_PATH), reason="oracle/_ref not on this box")


@pytest.fixture(scope="module")
def golden_ix():
    return util.load_golden_index()


@pytest.fixture(scope="module")
def paired_ix():
    return util.load_golden_index("paired_index.npz")


def test_library_exports_the_bam_calls():
    from snap_amd.aligner import EXPORTED_SYMBOLS, load_library
    lib = load_library()
    for name in bu.SYMBOLS:
        assert name in EXPORTED_SYMBOLS and hasattr(lib, name), name


def test_handcrafted_records_equal_the_restatement(golden_ix):
    bu.check_handcrafted(golden_ix)


def test_handcrafted_pair_units_equal_the_restatement(golden_ix):
    bu.check_handcrafted_pairs(golden_ix)


def test_memory_discipline(golden_ix):
    bu.check_memory_discipline(golden_ix)


def test_scan_levels(golden_ix):
    bu.check_scan_levels(golden_ix)


def test_argument_errors(golden_ix):
    bu.check_errors(golden_ix)


def test_device_form_equals_the_host_form(golden_ix):
    bu.check_device_form(golden_ix, util.HipBuffers())


@pytest.mark.parametrize("tag", list(su.SETS))
def test_records_equal_the_reference_cli_single(golden_ix, tag):
    bu.check_against_reference(golden_ix, "single", tag)


@pytest.mark.parametrize("tag", bu.PAIRED_TAGS)
def test_records_equal_the_reference_cli_paired(paired_ix, tag):
    bu.check_against_reference(paired_ix, "paired", tag)


def test_fused_single_call_equals_records_then_bam(golden_ix):
    bu.check_fused_single(golden_ix)


def test_fused_paired_call_equals_fields_then_bam(paired_ix):
    bu.check_fused_paired(paired_ix)


# ---------------------------------------------------------------------------------------- snapgpu-sam, SNAPGPU_SAM_DEVICE_BAM=1
@pytest.fixture(scope="module")
def single_workload(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("devbam_s"))
    return (d,) + make_workload(d, 3000)


@pytest.fixture(scope="module")
def paired_workload(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("devbam_p"))
    return (d,) + make_paired_workload(d, 1500)


@needs_ref
@pytest.mark.parametrize("opts", [[], ["-om", "1", "-omax", "4"], ["-ae"]])
def test_tool_single_with_device_bam(single_workload, opts):
    """-b 512: several batches, whose feeders interleave"""
    assert os.path.exists(TOOL), "snap_amd/snapgpu-sam not built: run __graft_entry__.build()"
    d, index_dir, fastq = single_workload
    assert bu.check_tool(TOOL, d, "single", index_dir, [fastq], opts, tool_opts=["-b", "512"]) > 3000


@needs_ref
@pytest.mark.parametrize("opts", [[], ["-G-"]])
def test_tool_paired_with_device_bam(paired_workload, opts):
    d, index_dir, fq = paired_workload
    assert bu.check_tool(TOOL, d, "paired", index_dir, fq, opts) == 3000


@needs_ref
def test_tool_paired_ea_falls_back_and_equals_the_reference(tmp_path):
    """-ea over the ALT workload: the batches in which a first-ALT pair turns up go through the host path; the file is the reference's."""
    d = str(tmp_path)
    index_dir, fq = make_paired_alt_workload(d, 400)
    assert bu.check_tool(TOOL, d, "paired", index_dir, fq, ["-ea"], expect_device=False) >= 800


@needs_ref
def test_switch_changes_nothing_for_sam_output(single_workload):
    d, index_dir, fastq = single_workload
    out = os.path.join(d, "plain.sam")
    got = []
    for switch in (True, False):
        r = subprocess.run([TOOL, "single", index_dir, fastq, "-o", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, stdin=subprocess.DEVNULL,
                           timeout=600, env=bu.tool_env(None, switch))
        assert r.returncode == 0 and b"BAM records from the device" not in r.stdout, r.stdout.decode(errors="replace")[-2000:]
        with open(out, "rb") as f:
            got.append(f.read())
    assert got[0] == got[1]
