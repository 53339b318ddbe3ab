"""The GPU index builder's -large tables and -locationSize 5..8 files (include/snapgpu.h: snapgpu_index_build_shape), executed on the host
by the wavefront emulator (tests/emu/) against the reference's own `snap-aligner index -exact` with the same flags: same Genome file, same
GenomeIndex fields and table sizes, same answers to every probed seed on both strands, same alignments (tests/index_build_util.py)."""
import ctypes as C
import os
import shutil

import pytest

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
        lib = al.load_library()
        for f in ("emu_total_ops", "emu_partial_ops", "emu_inactive_reads"):
            getattr(lib, f).restype = C.c_ulonglong
        yield lib
    finally:
        al._lib, al.LIB_PATH = saved


def _need_ref():
    from oracle import ref
    if not ref.available() or not os.path.exists(ref.CLI_PATH):
        pytest.skip("oracle/_ref not built")


def _header(d):
    return [int(x) for x in open(os.path.join(d, "GenomeIndex")).read().split()]


@pytest.mark.parametrize("seed_len", [20, 22])
def test_emu_large_index_vs_reference(emu, tmp_path, seed_len):
    """-s 20: 12-byte entries [value0][value1][key32]; -s 22: 5-byte keys (13-byte entries)."""
    _need_ref()
    from tests.index_build_util import compare_with_reference
    from tests.index_shape_util import both_strand_slots, rc_fasta
    from snap_amd.index import GenomeIndex, build_index
    fasta = os.path.join(str(tmp_path), "g.fa")
    rc_fasta(fasta)
    stats, d_ref, d_gpu = compare_with_reference(tmp_path, lib=emu, seed_len=seed_len, fasta=fasta, n_reads=600, large=True,
                                                 extra_ref=["-large"])
    h = _header(d_gpu)
    assert h[8] == 0 and h[9] == 4
    assert stats["n_repeated_seeds"] > 0
    assert both_strand_slots(GenomeIndex.load_from_directory(d_gpu)) > 1000
    # a seed and its reverse complement are one slot: fewer slots than a small build of the same genome has
    small = build_index(fasta, None, seed_len=seed_len, lib=emu)
    assert stats["n_seed_locations"] == small["n_seed_locations"]
    assert stats["n_distinct_seeds"] < small["n_distinct_seeds"]


def test_emu_wide_locations_vs_reference(emu, tmp_path):
    """-locationSize 5 at -s 20: 5-byte values in the hash tables, 8-byte overflow entries."""
    _need_ref()
    from tests.index_build_util import compare_with_reference
    from tests.index_shape_util import rc_fasta
    fasta = os.path.join(str(tmp_path), "g.fa")
    rc_fasta(fasta)
    stats, d_ref, d_gpu = compare_with_reference(tmp_path, lib=emu, seed_len=20, fasta=fasta, n_reads=600, location_size=5,
                                                 extra_ref=["-locationSize", "5"])
    h = _header(d_gpu)
    assert h[8] == 1 and h[9] == 5
    assert os.path.getsize(os.path.join(d_gpu, "OverflowTable")) == 8 * stats["overflow_table_size"] > 0


def test_emu_large_wide_and_the_view(emu, tmp_path):
    """-large with -locationSize 6 (-s 18); then the index straight from HBM (its view says -large) aligns like the saved directory."""
    _need_ref()
    from tests.index_build_util import compare_with_reference
    from tests import util
    from snap_amd import abi, synth
    from snap_amd.aligner import BaseAligner
    from snap_amd.index import GenomeIndex, build_index
    from tests.index_shape_util import rc_fasta
    rc_fasta(os.path.join(str(tmp_path), "g.fa"))
    stats, _, d_gpu = compare_with_reference(tmp_path, lib=emu, seed_len=18, n_reads=400, large=True, location_size=6,
                                             extra_ref=["-large", "-locationSize", "6"])
    assert _header(d_gpu)[8:] == [0, 6]
    st2, built = build_index(os.path.join(str(tmp_path), "g.fa"), None, seed_len=18, large=True, location_size=6, lib=emu, keep=True)
    assert st2["n_distinct_seeds"] == stats["n_distinct_seeds"]
    assert built.view().large_hash_table == 1
    ix = GenomeIndex.load_from_directory(d_gpu)
    params = abi.default_params(max_k=8, max_read_len=112)
    a_files = BaseAligner(ix, params)
    a_view = BaseAligner.from_built_index(built, ix, params)
    contigs = [(c.name, ix.genome[c.begin:c.begin + 20000]) for c in ix.contigs[:3]]
    reads = synth.make_reads(3, contigs, 300, 100)
    p1, _ = a_files.AlignRead(reads["bases"], reads["quals"], reads["offsets"])
    p2, _ = a_view.AlignRead(reads["bases"], reads["quals"], reads["offsets"])
    a_files.close(); a_view.close(); built.close()
    assert not util.compare_results(p1, p2)


def test_emu_shape_is_checked(emu, tmp_path):
    from tests.index_build_util import hard_fasta
    from snap_amd.index import build_index
    fasta = os.path.join(str(tmp_path), "g.fa")
    hard_fasta(fasta, size=20_000)
    for ls in (3, 9):
        with pytest.raises(RuntimeError, match="location size"):
            build_index(fasta, None, location_size=ls, lib=emu)
