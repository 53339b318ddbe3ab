"""MI355X: the SAM-field kernels for pairs on their own.  Aligns N pairs (2 x 150 bp, the bench's paired generator) over the bench's
seeded genome, then times snapgpu_sam_fields_paired over their results: one warm-up call, then `--calls` calls, each timed with
snapgpu_kernel_time (the hipEvent time of the pre-pass + field kernels).  Prints one JSON line with every call's reads/s, their median
and their spread.  SNAPGPU_SAMF_DP8=0 in the environment: without the row-loop pre-pass (the switch is read once per process).
SNAPGPU_AB_LIB=<libsnapgpu.so of another build>: the same measurement on that build.  --fastq DIR also writes the pairs as r1.fq / r2.fq
(input for `snapgpu-sam paired -passes N`).

    python scripts/gpu_paired_sam_perf.py [N=500000] [--genome-mb 64] [--calls 6] [--fastq DIR]
"""
import argparse, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from snap_amd import abi, synth
import snap_amd.aligner as al
if os.environ.get("SNAPGPU_AB_LIB"):
    al.LIB_PATH = os.path.abspath(os.environ["SNAPGPU_AB_LIB"]); al._lib = None
from snap_amd.index import GenomeIndex
import bench

ap = argparse.ArgumentParser()
ap.add_argument("n", nargs="?", type=int, default=500_000)
ap.add_argument("--genome-mb", type=int, default=64)
ap.add_argument("--calls", type=int, default=6)
ap.add_argument("--fastq", default="")
a = ap.parse_args()

bargs = bench.parse_args(["--genome-mb", str(a.genome_mb)])
genome, idx, built, info = bench.ensure_index(bargs, 0, 0)
if built is not None:
    built.close()
pr = synth.make_pairs(bargs.seed + 1000, genome, a.n, 150, insert_mean=400.0, insert_sd=50.0)
if a.fastq:
    os.makedirs(a.fastq, exist_ok=True)
    b = pr["bases"].reshape(2 * a.n, 150); q = pr["quals"].reshape(2 * a.n, 150)
    for w in (0, 1):
        names = np.array([b"@p%09d/%d\n" % (i, w + 1) for i in range(a.n)], dtype="S14").view(np.uint8).reshape(a.n, 14)
        rec = np.concatenate([names, b[w::2], np.full((a.n, 3), np.frombuffer(b"\n+\n", np.uint8)), q[w::2], np.full((a.n, 1), 10, np.uint8)], axis=1)
        rec.tofile(os.path.join(a.fastq, "r%d.fq" % (w + 1)))
    print(json.dumps({"fastq": a.fastq, "pairs": a.n, "index": idx}))
    sys.exit(0)
ix = GenomeIndex.load_from_directory(idx)
pa = al.ChimericPairedEndAligner(ix, abi.default_params(max_k=bargs.max_k, max_read_len=160), abi.default_paired_params())
res, _ = pa.align(pr["bases"], pr["quals"], pr["offsets"])
n = 2 * a.n
fc = np.zeros(n, np.int32); dl = np.full(n, 150, np.int32)
rates = []
for k in range(a.calls + 1):
    pa.kernel_time(reset=True)
    got = pa.samFieldsPaired(pr["bases"], pr["quals"], pr["offsets"], fc, dl, res)
    ms, _ = pa.kernel_time(reset=True)
    if k:
        rates.append(n / (ms / 1e3))
out = {"pairs": a.n, "genome_mb": a.genome_mb, "lib": al.LIB_PATH, "SNAPGPU_SAMF_DP8": os.environ.get("SNAPGPU_SAMF_DP8", "1"),
       "mapped_mates": int((got["flag"] & 4 == 0).sum()), "kernel_reads_per_s": rates, "median": float(np.median(rates)),
       "spread": float(max(rates) - min(rates))}
if hasattr(pa, "samf_pre_valid") and hasattr(pa.lib, "snapgpu_debug_samf_pre_valid"):
    out["valid_samf_pre_records"] = pa.samf_pre_valid()
pa.close()
print(json.dumps(out))
