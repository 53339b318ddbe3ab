"""Host side of the single-end wave's LDS frame (kernel_common.h: SE_FRAME_BYTES, lds_layout): what a context launches its kernels with
(AlignCfg::lds_per_wave, printed under SNAPGPU_VERBOSE) is lds_layout()'s total for the same geometry -- the function the kernel finds its
blocks with -- and that total is the carve-out of before plus the frame, for max_read_len 160 / 256 / 400 and -d 8 / -d 20.  Contexts are
created on the wavefront emulator's build of the library; lds_layout is called from a small host program compiled here."""
import os
import re
import shutil
import subprocess

import pytest

from snap_amd import abi

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ needed to build the wavefront emulator")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "kernel_common.h"
#include <cstdio>
#include <cstdlib>
int main(int argc, char **argv) {
    const uint32_t RL = atoi(argv[1]), nwl = atoi(argv[2]), kmax = atoi(argv[3]), ag = atoi(argv[4]);
    const LdsLayout a = lds_layout(RL, nwl, kmax, ag), b = lds_layout(RL, nwl, kmax, ag, SE_FRAME_BYTES);
    printf("%u %u %u %u\n", a.total, b.total, b.frame, (unsigned)SE_FRAME_BYTES);
    return 0;
}
"""


@pytest.fixture(scope="module")
def layout_tool(tmp_path_factory, emu_lib):
    from tests.emu.build import BDIR
    d = tmp_path_factory.mktemp("layout")
    src, exe = str(d / "layout.cpp"), str(d / "layout")
    open(src, "w").write(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-O0", "-w", "-I", os.path.join(ROOT, "tests", "emu", "include"), "-I", os.path.join(ROOT, "snap_amd", "csrc"),
                    "-o", exe, src, "-L" + BDIR, "-lsnapgpu_emu", "-Wl,-rpath," + BDIR, "-lpthread"], check=True)      # (the device headers' emulator hooks)
    return lambda *a: [int(x) for x in subprocess.run([exe] + [str(v) for v in a], check=True, capture_output=True, text=True).stdout.split()]


@pytest.fixture(scope="module")
def emu_lib():
    import snap_amd.aligner as al
    from tests.emu.build import build
    path = build()
    saved = (al._lib, al.LIB_PATH)
    al._lib, al.LIB_PATH = None, path
    try:
        al.load_library()
        yield
    finally:
        al._lib, al.LIB_PATH = saved


@pytest.mark.parametrize("max_k", [8, 20])
@pytest.mark.parametrize("max_read_len", [160, 256, 400])
def test_launched_lds_is_the_layouts_total(emu_lib, layout_tool, golden_index, monkeypatch, capfd, max_read_len, max_k):
    from snap_amd.aligner import BaseAligner
    monkeypatch.setenv("SNAPGPU_VERBOSE", "1")
    capfd.readouterr()
    a = BaseAligner(golden_index, abi.default_params(max_k=max_k, max_read_len=max_read_len))
    a.close()
    m = re.search(r"single-end context: AGC (\d+) RL (\d+) weight_lists (\d+) kmax (\d+) ag_lds (\d+): lds_per_wave (\d+) \((\d+) without", capfd.readouterr().err)
    assert m, "no SNAPGPU_VERBOSE line"
    agc, RL, nwl, kmax, ag_lds, launched, unframed = [int(x) for x in m.groups()]
    assert RL == max_read_len and kmax == max_k + 1
    before, total, frame_at, frame_bytes = layout_tool(RL, nwl, kmax, ag_lds)
    assert launched == total and unframed == before == frame_at
    assert total == before + frame_bytes and frame_bytes % 16 == 0
    assert 4 * total <= 160 * 1024                     # one workgroup of four waves fits a CU
    if (max_read_len, max_k) == (160, 8):              # the benchmark's geometry keeps its 24 waves per CU
        assert agc == 3 and 24 * total <= 160 * 1024
