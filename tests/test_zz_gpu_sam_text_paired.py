"""snapgpu_sam_text_paired / _device and snapgpu_align_sam_paired_text on the device: the checks of tests/test_emu_sam_text_paired.py through
the same utility (tests/samtext_paired_util.py), and `snapgpu-sam paired` with SNAPGPU_SAM_DEVICE_TEXT=1 -- the lines written by the
device -- against the reference CLI and against the tool's own host formatter."""
import os
import subprocess

import pytest

from oracle import ref
from tests import samtext_paired_util as pu
from tests import util
from tests.test_zz_gpu_native_sam import make_paired_alt_workload, make_paired_workload, run_and_compare_paired

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.environ.get("SNAPGPU_TEST_TOOL") or os.path.join(ROOT, "snap_amd", "snapgpu-sam")
needs_ref = pytest.mark.skipif(not ref.available() or not os.path.exists(ref.CLI_PATH), reason="oracle/_ref not on this box")


@pytest.fixture(scope="module")
def pindex():
    return util.load_golden_index("paired_index.npz")


def test_library_exports_the_paired_text_calls():
    from snap_amd.aligner import EXPORTED_SYMBOLS, load_library
    lib = load_library()
    for name in pu.SYMBOLS:
        assert name in EXPORTED_SYMBOLS and hasattr(lib, name), name


def test_handcrafted_units_equal_the_restatement(pindex):
    pu.check_handcrafted(pindex)


def test_memory_discipline(pindex):
    pu.check_memory_discipline(pindex)


def test_scan_levels(pindex):
    pu.check_scan_levels(pindex)


def test_argument_errors(pindex):
    pu.check_argument_errors(pindex)


@pytest.mark.parametrize("tag", pu.FIXTURE_TAGS)
def test_text_of_the_reference_cli_fields(pindex, tag):
    assert pu.check_reference_fields(pindex, tag) == 2600


def test_fused_call_equals_fields_then_text(pindex):
    pu.check_fused_equals_two_calls(pindex)


def test_device_form_equals_the_host_form(pindex):
    pu.check_device_form(pindex, util.HipBuffers())


# ---------------------------------------------------------------------------------------- snapgpu-sam paired, SNAPGPU_SAM_DEVICE_TEXT=1
@pytest.fixture(scope="module")
def workload(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("devtextp"))
    return (d,) + make_paired_workload(d, 2500, genome_bases=2_000_000)


def _env(switch):
    e = dict(os.environ)
    e.pop("SNAPGPU_SAM_DEVICE_TEXT", None)
    if switch:
        e["SNAPGPU_SAM_DEVICE_TEXT"] = "1"
    return e


def _run_tool(index_dir, fq, out, opts, switch):
    r = subprocess.run([TOOL, "paired", index_dir, fq[0], fq[1], "-o", out] + opts, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, stdin=subprocess.DEVNULL,
                       timeout=600, env=_env(switch))
    assert r.returncode == 0, "snapgpu-sam failed:\n%s" % r.stdout.decode(errors="replace")[-3000:]
    with open(out, "rb") as f:
        return f.read()


def _but_pg(data):
    return [x for x in data.split(b"\n") if not x.startswith(b"@PG")]


@needs_ref
@pytest.mark.parametrize("opts", [[], ["-G-"], ["-="]])
def test_tool_with_device_text_equals_the_reference_cli_and_its_own_host_path(workload, opts):
    assert os.path.exists(TOOL), "snap_amd/snapgpu-sam not built: run __graft_entry__.build()"
    d, index_dir, fq = workload
    assert run_and_compare_paired(TOOL, d, index_dir, fq, opts, env=_env(True)) > 5000
    tag = "_".join(o.strip("-") or "eq" for o in opts) or "default"
    new = os.path.join(d, "pnew_%s.sam" % tag)                              # (the same output path both times: it is part of @PG)
    with open(new, "rb") as f:
        on = f.read()
    assert _but_pg(_run_tool(index_dir, fq, new, opts, False)) == _but_pg(on)


@needs_ref
def test_tool_first_alt_pairs_fall_back_to_the_host_path(tmp_path):
    """-ea over an index with an ALT contig: batches with a first-ALT pair leave the device-text path, and the file is still the reference's."""
    d = str(tmp_path)
    index_dir, fq = make_paired_alt_workload(d, 1500)
    assert run_and_compare_paired(TOOL, d, index_dir, fq, ["-ea"], env=_env(True)) > 3000


@needs_ref                                                                  # (the workload's index comes from the reference's builder)
def test_tool_ignores_the_switch_for_bam(workload):
    d, index_dir, fq = workload
    out = os.path.join(d, "out.bam")
    assert _run_tool(index_dir, fq, out, [], True) == _run_tool(index_dir, fq, out, [], False)
