"""Emulator twins of tests/test_zz_gpu_paired_sam_onecall.py: the paired align kernels over Read::clip's windows
(k_align_paired<.., CLIP>), the row-loop pre-pass for mates (k_samf_dp8_paired) and k_sam_fields_paired with its SamfPre records, executed
on the host by the wavefront emulator (tests/emu/), with the same test bodies at a few hundred pairs; and `snapgpu-sam paired` through the
one-call path against the reference CLI's file.  Pattern and fixture as tests/test_emu_kernels.py."""
import os
import shutil

import numpy as np
import pytest

from tests import util
import tests.test_zz_gpu_paired_sam_onecall as oc

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


def test_emulated_library_exports_the_new_entry_points(emu):
    for s in ("snapgpu_align_sam_paired", "snapgpu_sam_fields_paired_device", "snapgpu_debug_samf_pre_valid"):
        assert hasattr(emu, s), s


@pytest.mark.parametrize("name,n_pairs", [("150_d8", 240), ("250_d20", 120)])
def test_emu_fused_call_equals_the_two_calls_it_replaces(emu, pindex, name, n_pairs):
    a = oc.paired_aligner(pindex, name)
    try:
        n_skipped, n_valid = oc.check_fused_equals_two_calls(a, pindex, name, n_pairs)
    finally:
        a.close()
    assert n_skipped >= 2 and (n_valid > 0 or name != "150_d8")      # (2 x 250: the pre-pass's LDS rows for four waves go beyond 64 KiB, none runs)


def test_emu_fused_call_beyond_400_bp_and_through_a_replica(emu, pindex):
    a = oc.paired_aligner(pindex, "420_d27")
    try:
        _, n_valid = oc.check_fused_equals_two_calls(a, pindex, "420_d27", 110)
    finally:
        a.close()
    assert n_valid == 0                                       # no pre-pass beyond 400 bp
    owner = oc.paired_aligner(pindex, "150_d8")
    a = owner.replica()
    try:
        _, n_valid = oc.check_fused_equals_two_calls(a, pindex, "150_d8", 110, use_m=True)
    finally:
        a.close()
        owner.close()
    assert n_valid > 0


@pytest.mark.parametrize("tag", oc.FIXTURE_TAGS)
def test_emu_sam_fields_paired_device_form_vs_reference_cli_fixture(emu, tag):
    z = np.load(os.path.join(util.GOLDEN, "sam_fields_paired.npz"))
    n_pairs = 300
    _, n_valid = oc.fixture_through_device_form(z, tag, n_pairs, util.HipBuffers(emu=True))
    assert (n_valid == 0) if tag.startswith("lvonly") else (n_valid > n_pairs)


@pytest.mark.parametrize("dp8", ["0", "1"])
def test_emu_sam_fields_paired_host_call_with_and_without_the_pre_pass(emu, dp8):
    import snap_amd.aligner as al
    oc.run_fixture_child(dp8, n_pairs=300, lib_path=al.LIB_PATH)


def test_emu_paired_sam_onecall_argument_errors(emu, pindex):
    oc.check_argument_errors(pindex)


def test_emu_native_paired_fastq_to_sam_through_the_one_call_path(emu, tmp_path):
    """`snapgpu-sam paired` on the small FASTQ pair of test_emu_native_paired_fastq_to_sam: the file written through snapgpu_align_sam_paired (the
    default) equals the reference CLI's line for line, and equals, byte for byte but for @PG, the file the calls it replaces write (SNAPGPU_SAM_PAIRED_FUSED=0);
    with -C++ as well, where mates lose '#' heads."""
    from oracle import ref
    if not ref.available() or not os.path.exists(ref.CLI_PATH):
        pytest.skip("oracle/_ref not built here")
    import subprocess
    from tests.emu.build import TOOL
    from tests.test_zz_gpu_native_sam import make_paired_workload, run_and_compare_paired
    d = str(tmp_path)
    env = dict(os.environ, SNAPGPU_EMU_CUS="4")
    index_dir, fq = make_paired_workload(d, 200, genome_bases=300_000)
    for opts in ([], ["-C++"]):
        assert run_and_compare_paired(TOOL, d, index_dir, fq, opts, env=env) > 400
        tag = "_".join(o.strip("-") or "eq" for o in opts) or "default"
        two = os.path.join(d, "two_%s.sam" % tag)
        r = subprocess.run([TOOL, "paired", index_dir, fq[0], fq[1], "-o", two] + opts, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, stdin=subprocess.DEVNULL,
                           timeout=3000, env=dict(env, SNAPGPU_SAM_PAIRED_FUSED="0"))
        assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
        lines = lambda path: [x for x in open(path, "rb") if not x.startswith(b"@PG")]          # (@PG holds the command line, with the output's name)
        assert lines(two) == lines(os.path.join(d, "pnew_%s.sam" % tag))
