"""Test infrastructure for the index builder's -large shape: a FASTA in which seeds meet their reverse complements, so that -large slots
hold both strands (GenomeIndex.cpp:1596-1599, "both complements used"), both strands carry overflow lists, and seeds that are their own
reverse complement occur (GenomeIndex.cpp:1515: they are filed under the forward strand)."""
import numpy as np

from snap_amd import synth
from tests.index_build_util import hard_fasta

_COMP = np.full(256, ord("N"), dtype=np.uint8)
for _a, _b in zip(b"ACGTN", b"TGCAN"):
    _COMP[_a] = _b


def revcomp(g):
    return _COMP[np.asarray(g, dtype=np.uint8)][::-1].copy()


def rc_fasta(path, seed=7, size=120_000):
    """hard_fasta (tests/index_build_util.py), then one more contig made of reverse complements of pieces of the first contig (one of them
    three times: repeated seeds on the reverse strand of seeds that also occur forward) and palindromic runs."""
    contigs = hard_fasta(path, seed=seed, size=size)
    g0 = contigs[0][1]
    rng = np.random.default_rng(seed + 1)
    pal = np.frombuffer(b"ACGT" * 12 + b"GAATTC" * 6 + b"AATT" * 10, dtype=np.uint8)
    parts = [revcomp(g0[10_000:16_000]), pal]
    rep = revcomp(g0[20_000:20_800])
    for _ in range(3):
        parts += [synth._ACGT[rng.integers(0, 4, size=300)], rep]
    parts += [pal, revcomp(g0[30_000:31_000])]
    extra = np.concatenate(parts)
    with open(path, "ab") as f:
        f.write(b">chrRC\n")
        for i in range(0, len(extra), 70):
            f.write(bytes(extra[i:i + 70]) + b"\n")
    return contigs + [("chrRC", extra)]


def both_strand_slots(ix):
    """Occupied slots of a loaded -large index (snap_amd.index.GenomeIndex, values narrowed to 4 bytes) whose two values are both in use."""
    e = np.asarray(ix.hash_blob[:len(ix.hash_blob) - 16]).reshape(-1, ix.entry_bytes)
    v = e[:, :8].copy().view(np.uint32)
    return int(np.count_nonzero((v[:, 0] != 0xffffffff) & (v[:, 0] != 0xfffffffe) & (v[:, 1] != 0xfffffffe)))
