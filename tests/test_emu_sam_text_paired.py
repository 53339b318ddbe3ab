"""snapgpu_sam_text_paired / _device and snapgpu_align_sam_paired_text on the wavefront emulator (tests/emu/): pair units to the bytes of
their two SAM lines.  The device code that runs here is the code the GPU runs (sam_text.h: k_samtext_qs with its byte-wise head and tail and
dword middle, the pair instantiations of the length pass and the write pass, the scan kernels as they are).  What the lines must be is
restated in plain Python in tests/samtext_paired_util.py.

Test infrastructure only: see tests/test_emu_kernels.py for how the emulated library is swapped in."""
import os
import shutil

import pytest

from tests import samtext_paired_util as pu
from tests import util

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
def pindex():
    return util.load_golden_index("paired_index.npz")


def test_emulated_library_exports_the_paired_text_calls(emu):
    for name in pu.SYMBOLS:
        assert hasattr(emu, name), name


def test_emu_handcrafted_units_equal_the_restatement(emu, pindex):
    h, exp, cn = pu.check_handcrafted(pindex)
    assert len(exp) == 300 and h["offsets"].size == 121


def test_emu_memory_discipline(emu, pindex):
    pu.check_memory_discipline(pindex)


def test_emu_scan_levels(emu, pindex):
    pu.check_scan_levels(pindex)


def test_emu_argument_errors(emu, pindex):
    pu.check_argument_errors(pindex)


@pytest.mark.parametrize("tag", pu.FIXTURE_TAGS)
def test_emu_text_of_the_reference_cli_fields(emu, pindex, tag):
    assert pu.check_reference_fields(pindex, tag) == 2600


def test_emu_fused_call_equals_fields_then_text(emu, pindex):
    pu.check_fused_equals_two_calls(pindex)


def test_emu_device_form_equals_the_host_form(emu, pindex):
    pu.check_device_form(pindex, util.HipBuffers(emu=True))


def test_emu_tool_with_device_text_equals_the_reference_cli_and_its_own_host_path(emu, tmp_path):
    """`snapgpu-sam paired` with SNAPGPU_SAM_DEVICE_TEXT=1 on the small FASTQ pair of test_emu_paired_sam_onecall.py: the reference CLI's file line
    for line, and the tool's own switch-off file byte for byte but for @PG."""
    from oracle import ref
    if not ref.available() or not os.path.exists(ref.CLI_PATH):
        pytest.skip("oracle/_ref not built here")
    import subprocess
    from tests.emu.build import TOOL
    from tests.test_zz_gpu_native_sam import make_paired_workload, run_and_compare_paired
    d = str(tmp_path)
    env = dict(os.environ, SNAPGPU_EMU_CUS="4")
    env.pop("SNAPGPU_SAM_DEVICE_TEXT", None)
    index_dir, fq = make_paired_workload(d, 200, genome_bases=300_000)
    assert run_and_compare_paired(TOOL, d, index_dir, fq, [], env=dict(env, SNAPGPU_SAM_DEVICE_TEXT="1")) > 400
    on = os.path.join(d, "pnew_default.sam")
    off = os.path.join(d, "off.sam")
    r = subprocess.run([TOOL, "paired", index_dir, fq[0], fq[1], "-o", off], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, stdin=subprocess.DEVNULL,
                       timeout=3000, env=env)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    lines = lambda path: [x for x in open(path, "rb") if not x.startswith(b"@PG")]          # (@PG holds the command line, with the output's name)
    assert lines(off) == lines(on)
