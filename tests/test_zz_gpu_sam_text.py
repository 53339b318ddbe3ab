"""snapgpu_sam_text_single / _device and snapgpu_align_sam_single_text on the device: the checks of tests/test_emu_sam_text.py through
the same utility (tests/samtext_util.py), and `snapgpu-sam single` with SNAPGPU_SAM_DEVICE_TEXT=1 -- the lines written by the device --
against the reference CLI and against the tool's own host formatter."""
import os
import subprocess

import pytest

from oracle import ref
from tests import samrec_util as su
from tests import samtext_util as tu
from tests import util
from tests.test_zz_gpu_native_sam import make_workload, run_and_compare, sam_lines  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.environ.get("SNAPGPU_TEST_TOOL") or os.path.join(ROOT, "snap_amd", "snapgpu-sam")
needs_ref = pytest.mark.skipif(not ref.available() or not os.path.exists(ref.CLI_PATH), reason="oracle/_ref not on this box")


@pytest.fixture(scope="module")
def golden_ix():
    return util.load_golden_index()


def test_library_exports_the_text_calls():
    from snap_amd.aligner import EXPORTED_SYMBOLS, load_library
    lib = load_library()
    for name in ("snapgpu_set_contig_names", "snapgpu_sam_text_single", "snapgpu_sam_text_single_device", "snapgpu_align_sam_single_text"):
        assert name in EXPORTED_SYMBOLS and hasattr(lib, name), name


def test_handcrafted_records_equal_the_restatement(golden_ix):
    tu.check_handcrafted(golden_ix)


def test_memory_discipline(golden_ix):
    tu.check_memory_discipline(golden_ix)


def test_scan_levels(golden_ix):
    tu.check_scan_levels(golden_ix)


def test_contig_names_are_required_and_counted(golden_ix):
    tu.check_contig_names(golden_ix)


@pytest.mark.parametrize("tag", list(su.SETS))
def test_text_equals_the_reference_cli(golden_ix, tag):
    tu.check_against_reference(golden_ix, tag)


def test_fused_call_equals_records_then_text(golden_ix):
    tu.check_fused_equals_two_calls(golden_ix)


def test_device_form_equals_the_host_form(golden_ix):
    tu.check_device_form(golden_ix, util.HipBuffers())


# ---------------------------------------------------------------------------------------- snapgpu-sam single, SNAPGPU_SAM_DEVICE_TEXT=1
@pytest.fixture(scope="module")
def workload(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("devtext"))
    return (d,) + make_workload(d, 20000)


def _env(switch):
    e = dict(os.environ)
    e.pop("SNAPGPU_SAM_DEVICE_TEXT", None)
    if switch:
        e["SNAPGPU_SAM_DEVICE_TEXT"] = "1"
    return e


def _run_tool(index_dir, fastq, out, opts, switch):
    r = subprocess.run([TOOL, "single", index_dir, fastq, "-o", out] + opts, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, stdin=subprocess.DEVNULL,
                       timeout=600, env=_env(switch))
    assert r.returncode == 0, "snapgpu-sam failed:\n%s" % r.stdout.decode(errors="replace")[-3000:]
    with open(out, "rb") as f:
        return f.read()


@needs_ref
@pytest.mark.parametrize("opts", [[], ["-om", "1", "-omax", "4"], ["-ae"]])
def test_tool_with_device_text_equals_the_reference_cli_and_its_own_host_path(workload, opts):
    assert os.path.exists(TOOL), "snap_amd/snapgpu-sam not built: run __graft_entry__.build()"
    d, index_dir, fastq = workload
    assert run_and_compare(TOOL, d, index_dir, fastq, opts, env=_env(True)) > 20000
    tag = "_".join(o.strip("-") or "eq" for o in opts) or "default"
    new = os.path.join(d, "new_%s.sam" % tag)                               # (the same output path both times: it is part of @PG)
    with open(new, "rb") as f:
        on = f.read()
    assert _run_tool(index_dir, fastq, new, opts, False) == on


@needs_ref                                                                  # (the workload's index comes from the reference's builder)
def test_tool_ignores_the_switch_for_bam(workload):
    d, index_dir, fastq = workload
    out = os.path.join(d, "out.bam")
    assert _run_tool(index_dir, fastq, out, [], True) == _run_tool(index_dir, fastq, out, [], False)
