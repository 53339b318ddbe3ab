"""snapgpu_align_sam_single_records on the wavefront emulator (tests/emu/): for every option set of
tests/golden/sam_records_single.npz -- -om / -omax / -mpc, -ea, -ae and their combinations -- the call's record list, order included,
equals what the reference CLI wrote, field for field.  The device code that runs here is the code the GPU runs: the align kernels with
secondary results, the adjuster, the record-list kernels (sam_records.h), k_samf_dp8_rec and k_sam_fields_rec.  And `snapgpu-sam single`
linked against the emulated library: the records call against the calls it replaces, the grouped call against batch by batch.

Test infrastructure only: see tests/test_emu_kernels.py for how the emulated library is swapped in."""
import os
import shutil

import numpy as np
import pytest

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


def test_emulated_library_exports_the_records_call(emu):
    assert hasattr(emu, "snapgpu_align_sam_single_records") and hasattr(emu, "snapgpu_align_sam_single_records_device")


@pytest.mark.parametrize("tag", list(su.SETS))
def test_emu_records_equal_the_reference_cli(emu, golden_index, tag):
    z = su.fixture()
    n = z["offsets"].size - 1
    got = su.run_set(golden_index, tag, z["bases"], z["quals"], z["offsets"], z["front_clip"], z["data_len"])
    problems, left_out = su.compare(su.expected(z, tag), got, n)
    print("%s: %d records of %d reads, %d reads left out (reference_history_dependent)" % (tag, got["n_records"], n, left_out))
    assert not problems, problems[:5]
    assert left_out <= 1 + n // 2000


def test_emu_capacity_too_small_then_retry(emu, golden_index):
    """A record capacity below what the batch has: the warning, the needed count, the records that fit exactly as a large enough call
    writes them; a read with more secondary results than the library's first launch has room for (8) is rerun inside the call."""
    z = su.fixture()
    n = 300
    o = z["offsets"][:n + 1]
    args = (golden_index, "ea_om1", z["bases"][:int(o[-1])], z["quals"][:int(o[-1])], o, z["front_clip"][:n], z["data_len"][:n])
    full = su.run_set(*args)
    assert not full["truncated"] and full["n_records"] > n
    assert int(full["n_secondary"].max()) > 8, "the read set no longer has a read whose secondary results outgrow the first stride"
    small = su.run_set(*args, capacity=n // 2, grow=False)
    assert small["truncated"] and small["n_records"] == full["n_records"] and small["rec_read"].size == n // 2
    assert (small["rec_begin"] == full["rec_begin"]).all()
    for f in ("rec_read", "rec_kind", "flag", "contig", "pos", "mapq", "n_ops", "nm", "ops"):
        assert (small[f] == full[f][:n // 2]).all(), f
    again = su.run_set(*args, capacity=n // 2, grow=True)
    for f in ("rec_read", "rec_kind", "flag", "contig", "pos", "mapq", "n_ops", "nm", "ops"):
        assert (again[f] == full[f]).all(), f


def test_emu_ae_refuses_a_clipped_read_at_a_contig_end(emu, golden_index):
    su.check_ae_refusal(golden_index)


def test_emu_device_form_equals_the_host_form(emu, golden_index):
    from tests import util
    su.check_device_form(golden_index, util.HipBuffers(emu=True), n=120)


# ---------------------------------------------------------------------------------------- snapgpu-sam single on the emulated library: one path against another
@pytest.fixture(scope="module")
def tool_workload(emu, tmp_path_factory):
    """The small FASTQ of test_emu_kernels.py::test_emu_native_fastq_to_sam (ragged, '#'-clipped, N-rich and unalignable reads, three read
    lengths) over an index with an ALT contig: 336 reads."""
    from oracle import ref
    if not ref.available() or not os.path.exists(ref.CLI_PATH):
        pytest.skip("oracle/_ref not built here")
    from tests.test_zz_gpu_native_sam import make_workload
    d = str(tmp_path_factory.mktemp("samrec_tool"))
    return (d,) + make_workload(d, 300, genome_bases=300_000)


def _run_tool(d, sub, index_dir, fastq, ext, opts, env):
    """One run in its own directory with a relative `-o`, so that two runs with the same options write the same @PG line.  Returns the
    file and what the program printed."""
    import subprocess
    from tests.emu.build import TOOL
    sub = os.path.join(d, sub)
    os.makedirs(sub, exist_ok=True)
    r = subprocess.run([TOOL, "single", index_dir, fastq, "-o", "out." + ext] + opts, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, stdin=subprocess.DEVNULL,
                       timeout=1800, cwd=sub, env=dict(os.environ, SNAPGPU_EMU_CUS="4", **env))
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    return open(os.path.join(sub, "out." + ext), "rb").read(), r.stdout.decode(errors="replace")


@pytest.mark.parametrize("tag", list(su.SETS))
def test_emu_tool_writes_the_same_bytes_with_and_without_the_records_call(tool_workload, tag):
    """SNAPGPU_SAM_SINGLE_FUSED=1 (every record from snapgpu_align_sam_single_records) against =0 (the calls it replaces): the same file,
    SAM and BAM, for every option set; three batches of at most 128 reads (the GPU twin: tests/test_zz_gpu_sam_single_records.py).
    Not asserted: that the record-capacity retry fires.  The first capacity of a 128-read batch is 128 * 24 / 16 + 16 = 208 records, the
    tool does not say when it calls again, and whether a set writes more than 1.6 records per read depends on the genome; the retry itself
    is pinned at the library by test_emu_capacity_too_small_then_retry above."""
    d, index_dir, fastq = tool_workload
    for ext in ("sam", "bam"):
        outs = [_run_tool(d, "%s_fused%s" % (tag, knob), index_dir, fastq, ext, ["-b", "128"] + su.SETS[tag][0], {"SNAPGPU_SAM_SINGLE_FUSED": knob})[0] for knob in ("1", "0")]
        assert len(outs[0]) > 10_000 and outs[0] == outs[1], (tag, ext, len(outs[0]), len(outs[1]))


@pytest.mark.parametrize("opts", [[], ["-ea"]])
def test_emu_tool_writes_the_same_bytes_grouped_and_batch_by_batch(tool_workload, opts):
    """`-b 32 -g 4` (four batches per snapgpu_align_sam_single call, scattered back) against `-g 1`: the same bytes but for the command line
    in @PG, SAM and decompressed BAM (32-read batches, not 64: eleven batches leave whole groups of four between a short first and last one).
    That grouped calls happen is read off the emulated runtime's report: the tool page-locks buffers only
    for a call over more than one batch (SNAPGPU_SAM_PIN_MIN=1: however small), and never with -g 1.  With -ea the index's ALT contig gives
    first-ALT records, and a group that holds one is redone batch by batch.  One feeder (-q 1) takes the eleven batches in order, and all
    are parsed long before its first emulated call returns, so only its first and its last group can be a single batch: first-ALT records
    in three different batches put one in a group of several.  tests/test_emu_kernels.py's page-locking test runs groups without that fallback."""
    import gzip
    import re
    d, index_dir, fastq = tool_workload
    env = {"SNAPGPU_SAM_PIN_MIN": "1", "SNAPGPU_EMU_PIN_REPORT": "1", "SNAPGPU_LOAD_PIN": "0"}      # (the index loader registers nothing)
    for ext in ("sam", "bam"):
        runs = [_run_tool(d, "group%s_%s" % (g, "_".join(opts)), index_dir, fastq, ext, ["-b", "32", "-g", g, "-q", "1"] + opts, env) for g in ("4", "1")]
        pinned = [sum(int(line.split("calls")[1].split(",")[0]) for line in r[1].splitlines() if line.startswith("emu: hipHostRegister calls")) for r in runs]
        assert pinned[0] > 0 and pinned[1] == 0, pinned                     # (the report is printed only when something was registered)
        outs = [gzip.decompress(r[0]) if ext == "bam" else r[0] for r in runs]
        outs = [re.sub(rb"@PG[^\n]*\n", b"", x, count=1) for x in outs]
        assert len(outs[0]) > 10_000 and outs[0] == outs[1], (opts, ext, len(outs[0]), len(outs[1]))
        if ext == "sam":
            names = [line.split(b"\t")[0] for line in open(fastq, "rb").read().split(b"\n")[0::4] if line]
            batch_of = {nm[1:].split(b" ")[0]: i // 32 for i, nm in enumerate(names)}
            alt_batches = {batch_of[line.split(b"\t")[0]] for line in outs[0].split(b"\n") if line and not line.startswith(b"@") and int(line.split(b"\t")[1]) & 0x100}
            assert (len(alt_batches) >= 3) if opts else not alt_batches, (opts, sorted(alt_batches))
