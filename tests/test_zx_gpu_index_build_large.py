"""The GPU index builder's other two index shapes on the hardware (include/snapgpu.h: snapgpu_index_build_shape): `-large` hash tables
(a seed and its reverse complement share one slot of two values) and `-locationSize 5..8` files.  Against the reference's own
`snap-aligner index -exact` with the same flags on the same FASTA (tests/index_build_util.py), then the aligners over a built -large
index against the reference over its own -large index, then the command line end to end."""
import os
import subprocess

import pytest

from snap_amd import abi, synth
from tests import util

pytestmark = pytest.mark.gpu


def _need_ref():
    from oracle import ref
    if not ref.available() or not os.path.exists(ref.CLI_PATH):
        pytest.skip("oracle/_ref not built")
    return ref


@pytest.mark.parametrize("seed_len,kw,extra", [(17, dict(large=True), ["-large", "-locationSize", "4"]), (20, dict(large=True), ["-large"]),
                                               (22, dict(large=True), ["-large"]), (24, dict(large=True), ["-large"]),
                                               (31, dict(large=True), ["-large"]),
                                               (20, dict(location_size=5), ["-locationSize", "5"]), (20, dict(location_size=6), ["-locationSize", "6"]),
                                               # the reference's own default shape for -s 18: it picks 5-byte locations by itself (GenomeIndex.cpp:446-453)
                                               (18, dict(large=True, location_size=5), ["-large"])])
def test_built_shape_equals_the_reference_indexer(tmp_path, seed_len, kw, extra):
    _need_ref()
    from tests.index_build_util import compare_with_reference
    from tests.index_shape_util import both_strand_slots, rc_fasta
    from snap_amd.index import GenomeIndex
    fasta = os.path.join(str(tmp_path), "g.fa")
    rc_fasta(fasta)
    stats, _, d_gpu = compare_with_reference(tmp_path, seed_len=seed_len, fasta=fasta, extra_ref=extra, **kw)
    assert stats["n_repeated_seeds"] > 0
    hdr = open(os.path.join(d_gpu, "GenomeIndex")).read().split()
    assert (hdr[8], hdr[9]) == ("0" if kw.get("large") else "1", str(kw.get("location_size", 4)))
    if kw.get("large"):
        assert both_strand_slots(GenomeIndex.load_from_directory(d_gpu)) > 1000


def test_large_index_on_a_larger_genome_and_the_aligners_over_it(tmp_path):
    """16 Mb with planted repeats and a reverse-complemented stretch, built with -large: the directory test, then BaseAligner over the built
    index (files, and the HBM-resident view) and ChimericPairedEndAligner over the files must equal the reference over the REFERENCE-built
    -large directory, work counters included."""
    ref = _need_ref()
    from tests.index_build_util import compare_with_reference
    from tests.index_shape_util import revcomp
    from tests.pairs_util import compare_paired, hard_pairs
    from snap_amd.aligner import BaseAligner, ChimericPairedEndAligner
    from snap_amd.index import GenomeIndex, build_index
    g = synth.make_genome(31, 16_000_000, n_contigs=5, repeat_frac=0.3, max_copies=800, repeat_len=(200, 3000), max_divergence=0.05, n_run_frac=0.001)
    g.append(("chrRC", revcomp(g[0][1][1_000_000:1_600_000])))
    fasta = os.path.join(str(tmp_path), "g.fa")
    synth.write_fasta(fasta, g)
    stats, d_ref, d_gpu = compare_with_reference(tmp_path, fasta=fasta, n_reads=4000, large=True, extra_ref=["-large"])
    reads = synth.make_reads(5, g, 20000, 150)
    params = abi.default_params(max_k=8, max_read_len=160)
    with ref.fresh_objects():
        exp, _, cnt, _ = ref.RefIndex(d_ref).align_single(params, reads["bases"], reads["quals"], reads["offsets"], threads=16)
    want = [cnt["lookups"], cnt["lv"], cnt["ag"]]

    def check(a):
        try:
            got, _ = a.AlignRead(reads["bases"], reads["quals"], reads["offsets"])
            c = a.counters()
        finally:
            a.close()
        assert not util.compare_results(exp, got), util.compare_results(exp, got)
        assert [c["n_hash_table_lookups"], c["n_lv_locations"], c["n_ag_locations"]] == want

    ix = GenomeIndex.load_from_directory(d_gpu)
    assert ix.large
    check(BaseAligner(ix, params))
    st2, built = build_index(fasta, None, large=True, keep=True)
    try:
        assert st2["n_distinct_seeds"] == stats["n_distinct_seeds"] and st2["overflow_table_size"] == stats["overflow_table_size"]
        assert built.view().large_hash_table == 1
        check(BaseAligner.from_built_index(built, None, params))
    finally:
        built.close()

    pr = hard_pairs(13, g, 2000, 150, insert_mean=400, insert_max=1000)
    pp = abi.default_paired_params(max_spacing=1000)
    with ref.fresh_objects():
        rp, _, rcnt, _ = ref.RefIndex(d_ref).align_paired(params, pp, pr["bases"], pr["quals"], pr["offsets"], threads=16, stage=0)
    a = ChimericPairedEndAligner(ix, params, pp)
    try:
        gp, _ = a.align(pr["bases"], pr["quals"], pr["offsets"])
        c = a.counters()
    finally:
        a.close()
    assert not compare_paired(rp, gp, verbose=3).any()
    assert (c["n_lv_locations"], c["n_ag_locations"]) == (rcnt["lv"], rcnt["ag"])


def test_snapgpu_index_large_command_line(tmp_path):
    """`snapgpu-index <fasta> <dir> -s 20 -large`: the reference CLI's SAM over that directory equals its SAM over its own -large index, and
    `snapgpu-sam single` over the GPU-built directory writes the same records."""
    ref = _need_ref()
    from tests.index_shape_util import rc_fasta
    tool = os.path.join(util.ROOT, "snap_amd", "snapgpu-index")
    sam_tool = os.path.join(util.ROOT, "snap_amd", "snapgpu-sam")
    assert os.path.exists(tool) and os.path.exists(sam_tool), "run __graft_entry__.build()"
    fasta = os.path.join(str(tmp_path), "g.fa")
    contigs = rc_fasta(fasta)
    d_ref, d_gpu = os.path.join(str(tmp_path), "r"), os.path.join(str(tmp_path), "g")
    ref.build_index(fasta, d_ref, 20, threads=8, large=True)
    r = subprocess.run([tool, fasta, d_gpu, "-s", "20", "-large"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()
    assert open(os.path.join(d_gpu, "GenomeIndex")).read().split()[8] == "0"
    reads = synth.make_reads(9, contigs, 3000, 100)
    fq = os.path.join(str(tmp_path), "r.fq")
    synth.write_fastq(fq, reads)

    def sam(cmd, out):
        r = subprocess.run(cmd + ["-o", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, stdin=subprocess.DEVNULL, timeout=900)
        assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
        return [l for l in open(out) if not l.startswith("@PG")]
    a = sam([ref.CLI_PATH, "single", d_ref, fq, "-t", "1", "-d", "8"], os.path.join(str(tmp_path), "ref_ref.sam"))
    b = sam([ref.CLI_PATH, "single", d_gpu, fq, "-t", "1", "-d", "8"], os.path.join(str(tmp_path), "ref_gpu.sam"))
    c = sam([sam_tool, "single", d_gpu, fq, "-d", "8"], os.path.join(str(tmp_path), "gpu_gpu.sam"))
    assert len(a) > 3000
    assert a == b
    assert sorted(c) == sorted(a)
