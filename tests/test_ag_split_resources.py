"""The affine-gap code of the single-end kernel is two out-of-line functions (snap_amd/csrc/ag_win.h): ag_hot_fn -- the two forms of
ag_banded_win, every call of a 150-bp read at -d 8 -- and ag_cold_fn, every other form.

Both must exist in the cross-compiled single_timed_k.o (the code object's symbol table), and the hot function's OWN resources must stay
what profiles/r07b/kernel_resources.txt records.  A device function that is no kernel has no entry in the object's metadata note (a
kernel's entry folds its callees in: private_segment_fixed_size = own frame + the deepest callee's, which the cold function's 72 bytes
decide), so the function's own figures are read from the `; Function info:` block of the unit's listing, compiled with the build's flags
(scripts/kernel_resources.py: listing, function_info).  Resource figures only; no instruction is looked at.

Budgets = the measured figure plus a margin for compiler noise:
  * scratch of ag_hot_fn<EXACT = true> 20 bytes per lane, of <false> 16: callee-saved VGPRs stored on entry (among them the two whose lanes
    hold the saved and the spilled SGPRs) -- i.e. NO spilled VGPR and no SGPR spilled to memory; budget 20 + 8;
  * VGPRs 72 (the kernels' 80 decide the occupancy: six waves per SIMD);
  * code 14 780 / 14 100 bytes; budget 16 384, a quarter of the instruction cache.
SGPRs parked in VGPR LANES (7 slots in the exact form, all read on the slide and (nk0, nk1)-change paths) are not a resource figure the
compiler states for a function -- only for kernels -- and counting them means naming the lane instructions: that count is recorded in
profiles/r07b/ from scripts/asm_loops.py and not asserted here.  What the scratch budget does catch is the step after that: a spilled VGPR,
or SGPRs that no longer find a lane and go to memory."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "snap_amd", "build", "single_timed_k.o")
SRC = os.path.join(ROOT, "snap_amd", "csrc", "single_timed_k.hip")

HOT_SCRATCH_MAX = 20 + 8           # bytes per lane, the function's own frame (measured 20 exact / 16 fast)
HOT_VGPRS_MAX = 72 + 8             # measured 72; 80 is where the kernel's occupancy would change
HOT_CODE_BYTES_MAX = 16384         # measured 14 780 / 14 100; the one function it replaces was 61 136 / 58 056

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf") or shutil.which("c++filt") is None
                                or not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), reason="needs hipcc and the ROCm LLVM tools")


def _kr():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def info(tmp_path_factory):
    kr = _kr()
    return kr.function_info(kr.listing(SRC, str(tmp_path_factory.mktemp("listing") / "single_timed_k.s")))


def test_hot_and_cold_functions_exist_in_the_object():
    if not os.path.exists(OBJ):
        import __graft_entry__ as g
        g.build_library()
    sizes = _kr().function_sizes(OBJ)
    hot = sorted(n for n in sizes if "ag_hot_fn" in n)
    cold = sorted(n for n in sizes if "ag_cold_fn" in n)
    assert len(hot) == 2 and len(cold) == 2, (hot, cold)                            # the exact and the fast instantiation of each
    assert not [n for n in sizes if "ag_dispatch_fn" in n]


def test_hot_function_own_resources(info):
    hot = {n: v for n, v in info.items() if "ag_hot_fn" in n}
    cold = {n: v for n, v in info.items() if "ag_cold_fn" in n}
    assert len(hot) == 2 and len(cold) == 2, sorted(info)
    for n, v in sorted(hot.items()) + sorted(cold.items()):
        print(n, v)
    for n, v in hot.items():
        assert v["ScratchSize"] <= HOT_SCRATCH_MAX, (n, v)
        assert v["NumVgprs"] <= HOT_VGPRS_MAX, (n, v)
        assert v["codeLenInByte"] <= HOT_CODE_BYTES_MAX, (n, v)
    assert min(v["codeLenInByte"] for v in cold.values()) > max(v["codeLenInByte"] for v in hot.values())     # (the forms that never run on the headline workload are the bulk)
