"""Single-end reads to all their SAM records in one call (snapgpu_align_sam_single_records: -om / -omax / -mpc, -ea, -ae) on the GPU:
the committed fixture (tests/golden/sam_records_single.npz, what the reference CLI wrote), the live reference CLI on a fresh genome,
the growth paths inside the call (record capacity, the per-read secondary stride), argument errors, and `snapgpu-sam single` with the
new call against the calls it replaces (SNAPGPU_SAM_SINGLE_FUSED=0): the same bytes, SAM and BAM."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from snap_amd import synth
from snap_amd.index import GenomeIndex
from oracle import ref
from tests import samrec_util as su
from tests import util

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.environ.get("SNAPGPU_TEST_TOOL") or os.path.join(ROOT, "snap_amd", "snapgpu-sam")
PER_RECORD = ("rec_read", "rec_kind", "flag", "contig", "pos", "mapq", "n_ops", "nm", "ops", "stale")
needs_ref = pytest.mark.skipif(not ref.available() or not os.path.exists(ref.CLI_PATH), reason="oracle/_ref not on this box")


@pytest.fixture(scope="module")
def golden_ix():
    return util.load_golden_index()


@pytest.mark.parametrize("tag", list(su.SETS))
def test_records_equal_the_reference_fixture(golden_ix, tag):
    z = su.fixture()
    n = z["offsets"].size - 1
    got = su.run_set(golden_ix, tag, z["bases"], z["quals"], z["offsets"], z["front_clip"], z["data_len"])
    problems, left_out = su.compare(su.expected(z, tag), got, n)
    print("%s: %d records of %d reads, %d reads left out" % (tag, got["n_records"], n, left_out))
    assert not problems, problems[:5]
    assert left_out <= 1 + n // 2000


# ---------------------------------------------------------------------------------------- the live reference CLI on a fresh genome
N_LIVE = 20000


@pytest.fixture(scope="module")
def live(tmp_path_factory):
    """20 000 reads of a fresh 2 Mb genome with repeats and an ALT contig (tests/test_zz_gpu_native_sam.py: ragged lengths, '#' tails,
    N-rich and unalignable reads, 250 / 380 / 60 bp reads) plus reads over the two ends of every contig."""
    from tests.test_zz_gpu_native_sam import make_workload
    d = str(tmp_path_factory.mktemp("samrec"))
    genome_bases = 2_000_000
    index_dir, fastq = make_workload(d, N_LIVE, genome_bases=genome_bases)
    contigs = synth.make_genome(177, genome_bases, n_contigs=3, repeat_frac=0.1)          # (the genome make_workload indexed, before its ALT contig)
    rng = np.random.default_rng(23)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    k0 = sum(1 for line in open(fastq, "rb")) // 4
    with open(fastq, "ab") as f:
        for _, seq in contigs:
            for L in (100, 150):
                for k in (1, 3, 9):
                    for b in (np.concatenate([rng.choice(acgt, size=k), seq[:L - k]]), np.concatenate([seq[seq.size - (L - k):], rng.choice(acgt, size=k)])):
                        f.write(b"@read%d\n" % k0 + b.tobytes() + b"\n+\n" + rng.integers(45, 74, size=L).astype(np.uint8).tobytes() + b"\n"); k0 += 1
    bs, qs = [], []
    lines = open(fastq, "rb").read().split(b"\n")
    for i in range(0, len(lines) - 1, 4):
        bs.append(np.frombuffer(lines[i + 1], dtype=np.uint8)); qs.append(np.frombuffer(lines[i + 3], dtype=np.uint8))
    n = len(bs)
    assert n >= N_LIVE
    offsets = np.concatenate([[0], np.cumsum([b.size for b in bs])]).astype(np.uint64)
    fc = np.zeros(n, np.int32); dl = np.zeros(n, np.int32)
    for i, q in enumerate(qs):                                        # Read::clip, ClipBack (the CLI's default)
        m = q.size
        while m > 0 and q[m - 1] == ord("#"):
            m -= 1
        dl[i] = m
    idx = GenomeIndex.load_from_directory(index_dir)
    return dict(dir=d, index_dir=index_dir, fastq=fastq, idx=idx, n=n, bases=np.concatenate(bs), quals=np.concatenate(qs), offsets=offsets, front_clip=fc, data_len=dl)


def reference_records(live, tag):
    cli = su.SETS[tag][0]
    sam = os.path.join(live["dir"], "ref_%s.sam" % tag)
    r = subprocess.run([ref.CLI_PATH, "single", live["index_dir"], live["fastq"], "-o", sam, "-t", "1"] + cli, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       stdin=subprocess.DEVNULL, timeout=1800)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    contig_of = {c.name: i for i, c in enumerate(live["idx"].contigs)}
    cig = {c: i for i, c in enumerate("MIDNSHP=X")}
    rows = []
    for line in open(sam):
        if line.startswith("@"):
            continue
        t = line.rstrip("\n").split("\t")
        ops = []
        if t[5] != "*":
            num = ""
            for ch in t[5]:
                if ch.isdigit():
                    num += ch
                else:
                    ops.append((int(num) << 4) | cig[ch]); num = ""
        flag = int(t[1])            # (under -ea the reference prints an uninitialised `supplementary` in a first-ALT record -- tests/test_zz_gpu_native_sam.py,
                                    #  sam_lines -- : the caller clears 0x800 on the records the library calls first-ALT, on both sides)
        rows.append((int(t[0][4:]), flag, contig_of.get(t[2], -1), int(t[3]), int(t[4]), int([x for x in t[11:] if x.startswith("NM:i:")][0][5:]), ops))
    width = max(3, max(len(x[6]) for x in rows))
    ops = np.zeros((len(rows), width), np.uint32)
    for k, x in enumerate(rows):
        ops[k, :len(x[6])] = x[6]
    return dict(rec_read=np.array([x[0] for x in rows], np.uint32), flag=np.array([x[1] for x in rows], np.int32), contig=np.array([x[2] for x in rows], np.int32),
                pos=np.array([x[3] for x in rows], np.int64), mapq=np.array([x[4] for x in rows], np.int32), nm=np.array([x[5] for x in rows], np.int32),
                n_ops=np.array([len(x[6]) if x[6] else -1 for x in rows], np.int32), ops=ops)


@needs_ref
@pytest.mark.parametrize("tag", ["om1_omax4", "ea_om1", "ae_om1"])
def test_records_equal_the_live_reference_cli(live, tag):
    exp = reference_records(live, tag)
    got = su.run_set(live["idx"], tag, live["bases"], live["quals"], live["offsets"], live["front_clip"], live["data_len"], ops_stride=128)
    if "-ea" in su.SETS[tag][0] and got["rec_kind"].size == exp["flag"].size:      # 0x800 of a first-ALT record: see reference_records
        alt = got["rec_kind"] == 2
        got["flag"] = np.where(alt, got["flag"] & ~0x800, got["flag"]); exp["flag"] = np.where(alt, exp["flag"] & ~0x800, exp["flag"])
    problems, left_out = su.compare(exp, got, live["n"])
    print("%s: %d records of %d reads, %d reads left out" % (tag, got["n_records"], live["n"], left_out))
    assert not problems, problems[:5]
    assert left_out <= 1 + live["n"] // 2000
    assert got["n_records"] > live["n"]


# ---------------------------------------------------------------------------------------- growth inside the call
def _golden_batch(n):
    z = su.fixture()
    o = z["offsets"][:n + 1]
    return z["bases"][:int(o[-1])], z["quals"][:int(o[-1])], o, z["front_clip"][:n], z["data_len"][:n]


def test_capacity_too_small_returns_the_count_and_the_retry_matches(golden_ix):
    n = 600
    args = (golden_ix, "ea_om1") + _golden_batch(n)
    full = su.run_set(*args)
    assert not full["truncated"] and full["n_records"] > n
    small = su.run_set(*args, capacity=n // 2, grow=False)
    assert small["truncated"] and small["n_records"] == full["n_records"] and small["rec_read"].size == n // 2
    assert (small["rec_begin"] == full["rec_begin"]).all() and (small["n_secondary"] == full["n_secondary"]).all()
    for f in PER_RECORD:
        assert (small[f] == full[f][:n // 2]).all(), f
    again = su.run_set(*args, capacity=n // 2, grow=True)
    for f in PER_RECORD:
        assert (again[f] == full[f]).all(), f


def test_a_read_with_more_secondaries_than_the_first_stride(golden_ix):
    """The library's first launch has room for 8 secondary results per read (or the caller's stride); reads with more are rerun inside
    the call.  Whatever the first stride, the records are the same -- and equal to those of a call whose stride holds everything."""
    n = 300
    args = (golden_ix, "ea_om1") + _golden_batch(n)
    default = su.run_set(*args)
    most = int(default["n_secondary"].max())
    assert most > 8, "the read set no longer has a read whose secondary results outgrow the first stride"
    assert int((default["n_secondary"] > 8).sum()) < n // 2
    wide = su.run_set(*args, secondary_stride=most)
    narrow = su.run_set(*args, secondary_stride=1)
    for f in PER_RECORD:
        assert (wide[f] == default[f]).all() and (narrow[f] == default[f]).all(), f
    assert (wide["n_secondary"] == default["n_secondary"]).all() and (narrow["n_secondary"] == default["n_secondary"]).all()
    # the strided result array of the wide call holds what the records were written from: the same locations, in the records' order
    i = int(np.argmax(default["n_secondary"]))
    b = int(default["rec_begin"][i])
    sec = wide["secondary"][i, :most]
    assert (default["rec_kind"][b + 1:b + 1 + most] == 1).all() and (sec["status"] != 0).all()


def test_ae_refuses_a_clipped_read_at_a_contig_end(golden_ix):
    su.check_ae_refusal(golden_ix)


def test_device_form_equals_the_host_form(golden_ix):
    su.check_device_form(golden_ix, util.HipBuffers())


def test_no_reads(golden_ix):
    a = su.make_aligner(golden_ix, "om1_omax4")
    try:
        out = a.alignSamRecords(np.zeros(0, np.uint8), np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.uint8))
        assert out["n_records"] == 0 and out["rec_read"].size == 0 and out["rec_begin"][0] == 0 and not out["truncated"]
    finally:
        a.close()


def test_argument_errors(golden_ix):
    from snap_amd.aligner import BaseAligner, ChimericPairedEndAligner, SnapGpuError
    from snap_amd import abi
    n = 64
    bases, quals, offsets, fc, dl = _golden_batch(n)
    a = su.make_aligner(golden_ix, "om1_omax4", max_read_len=160)
    try:
        skip = su.skip_mask(bases, offsets, fc, dl, int(a.params.max_k))
        with pytest.raises(SnapGpuError, match="ops_stride"):
            a.alignSamRecords(bases, quals, offsets, fc, dl, skip, ops_stride=2)
        cap = 4 * n
        n_rec = C.c_uint64(0)
        ins = [bases, quals, offsets, fc, dl, skip]
        outs = [np.zeros(n + 1, np.uint64), np.zeros(cap, np.uint32), np.zeros(cap, np.uint8), np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int64),
                np.zeros(cap, np.int32), np.zeros((cap, 8), np.uint32), np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int32)]
        p = lambda x: C.c_void_p(np.ascontiguousarray(x).ctypes.data)
        f = a.lib.snapgpu_align_sam_single_records

        def call(handle, ins_, outs_, n_rec_=C.addressof(n_rec), ops_stride=8, adjust=0):
            return f(handle, n, *ins_, 0, adjust, None, None, None, 0, None, cap, n_rec_, *outs_[:8], ops_stride, *outs_[8:])
        ins = [np.ascontiguousarray(x) for x in ins]
        for j in range(len(ins)):                                              # NULL inputs
            assert call(a.handle, [None if k == j else p(x) for k, x in enumerate(ins)], [p(x) for x in outs]) == -1, j
        for j in range(len(outs)):                                             # NULL outputs
            assert call(a.handle, [p(x) for x in ins], [None if k == j else p(x) for k, x in enumerate(outs)]) == -1, j
        assert call(a.handle, [p(x) for x in ins], [p(x) for x in outs], n_rec_=None) == -1
        assert call(None, [p(x) for x in ins], [p(x) for x in outs]) == -1
        assert call(a.handle, [p(x) for x in ins], [p(x) for x in outs], ops_stride=2) == -1
        assert call(a.handle, [p(x) for x in ins], [p(x) for x in outs], adjust=1) == -1          # -ae belongs to snapgpu_enable_secondary on this context
        assert call(a.handle, [p(x) for x in ins], [p(x) for x in outs]) == 0 and n_rec.value >= n  # (and the same call with nothing missing)
        # the device-pointer form: NULL arguments, ops_stride, max_read_len
        g = a.lib.snapgpu_align_sam_single_records_device
        g.argtypes = ([C.c_void_p, C.c_uint32, C.c_uint32] + [C.c_void_p] * 6 + [C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_uint32, C.c_void_p, C.c_uint64] +
                      [C.c_void_p] * 9 + [C.c_uint32] + [C.c_void_p] * 4)
        d_in = [p(x) for x in ins]; d_out = [p(x) for x in outs]               # (never dereferenced: every call below is refused before anything is launched)
        dev = lambda mrl, ins_, outs_, stride: g(a.handle, n, mrl, *ins_, 0, 0, None, None, None, 0, None, cap, C.addressof(n_rec), *outs_[:8], stride, *outs_[8:], None)
        assert dev(160, [None] + d_in[1:], d_out, 8) == -1 and b"null argument" in a.lib.snapgpu_last_error(a.handle)
        assert dev(160, d_in, d_out[:3] + [None] + d_out[4:], 8) == -1
        assert dev(160, d_in, d_out, 2) == -1 and b"ops_stride" in a.lib.snapgpu_last_error(a.handle)
        assert dev(0, d_in, d_out, 8) == -1 and b"max_read_len" in a.lib.snapgpu_last_error(a.handle)
        # a read the aligner is given that is longer than the context's max_read_len
        long_o = np.array([0, 200], np.uint64)
        with pytest.raises(SnapGpuError, match="max_read_len"):
            a.alignSamRecords(np.full(200, ord("A"), np.uint8), np.full(200, ord("I"), np.uint8), long_o, np.zeros(1, np.int32), np.array([200], np.int32), np.zeros(1, np.uint8))
        with pytest.raises(SnapGpuError, match="clipping"):
            a.alignSamRecords(bases, quals, offsets, fc, dl + 1000, skip)
    finally:
        a.close()
    # a paired-end context is refused; the primary-only call's own refusal of a context with secondary results stays
    pa = ChimericPairedEndAligner(util.load_golden_index("paired_index.npz"), abi.default_params(max_k=8, max_read_len=160), abi.default_paired_params())
    try:
        with pytest.raises(SnapGpuError, match="single-end context"):
            BaseAligner.alignSamRecords(pa, bases, quals, offsets, fc, dl, skip)
    finally:
        pa.close()
    a = su.make_aligner(golden_ix, "om1_omax4", max_read_len=160)
    try:
        with pytest.raises(SnapGpuError, match="plain single-end context"):
            a.alignSam(bases, quals, offsets, fc, dl, skip)
    finally:
        a.close()


# ---------------------------------------------------------------------------------------- snapgpu-sam single: the new call against the calls it replaces
@pytest.fixture(scope="module")
def tool_workload(tmp_path_factory):
    from tests.test_zz_gpu_native_sam import make_workload
    d = str(tmp_path_factory.mktemp("samrec_tool"))
    return (d,) + make_workload(d, 6000, genome_bases=1_000_000)


@needs_ref
@pytest.mark.parametrize("tag", list(su.SETS))
def test_tool_writes_the_same_bytes_with_and_without_the_one_call_path(tool_workload, tag):
    assert os.path.exists(TOOL), "snap_amd/snapgpu-sam not built: run __graft_entry__.build()"
    d, index_dir, fastq = tool_workload
    opts = su.SETS[tag][0]
    for ext in ("sam", "bam"):
        outs = []
        for knob in ("1", "0"):
            sub = os.path.join(d, "%s_fused%s" % (tag, knob))              # (the @PG line carries the command line: the same `-o` for both runs)
            os.makedirs(sub, exist_ok=True)
            r = subprocess.run([TOOL, "single", index_dir, fastq, "-o", "out." + ext, "-b", "2000"] + opts, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                               stdin=subprocess.DEVNULL, timeout=1800, cwd=sub, env=dict(os.environ, SNAPGPU_SAM_SINGLE_FUSED=knob))
            assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
            outs.append(open(os.path.join(sub, "out." + ext), "rb").read())
        assert len(outs[0]) > 100_000 and outs[0] == outs[1], (tag, ext, len(outs[0]), len(outs[1]))
