"""Generate tests/golden/bam_records.npz: the BAM records the unmodified reference CLI wrote (oracle/_ref/snap-aligner single | paired ...
-o out.bam -t 1, so the file is in read order), decompressed, for the first reads of the workloads two other fixtures come from:
  single_<tag>   the first N_SINGLE reads of sam_records_single.npz (names r<i>), the seven option sets of make_golden_sam_records.py
  paired_<tag>   the first N_PAIRS pairs of sam_fields_paired.npz (names p<i>/1, p<i>/2), its three option sets
Each is one uint8 blob of records, block_size words included.  single_ref_id / paired_ref_id: the BAM reference number of every contig of
the index, from the reference's own header.  The reads, their names' rule and the fields of these records are the other fixtures': a
record of a read does not depend on the other reads of a run, which this script checks by count and by FLAG against those fixtures."""
import os, sys, shutil, subprocess
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from snap_amd import synth
from snap_amd.index import GenomeIndex
from oracle import ref
from tests import util
from tests.test_zz_gpu_native_sam import bam_parts

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden')
W = '/tmp/snap_golden_bam'
N_SINGLE, N_PAIRS = 200, 100
SINGLE_SETS = [('om1_omax4', ['-om', '1', '-omax', '4']), ('D2_om2_mpc2', ['-D', '2', '-om', '2', '-mpc', '2']), ('ea_om1', ['-ea', '-om', '1']), ('ea', ['-ea']),
               ('ae', ['-ae']), ('ae_om1', ['-ae', '-om', '1']), ('lvonly_eqx_om1', ['-G-', '-=', '-om', '1'])]
PAIRED_SETS = [('default', []), ('lvonly', ['-G-']), ('eqx', ['-='])]


def run(cmd):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-2000:]


def ref_ids(idx, refs):
    order = [name.rstrip(b'\0') for name, _ in refs]                          # (l_name counts the NUL)
    return np.array([order.index(c.name.encode()) for c in idx.contigs], np.int32)


def flags_of(recs):
    return np.array([int.from_bytes(r[16:20], 'little') >> 16 for r in recs], np.int32)


def main():
    shutil.rmtree(W, ignore_errors=True); os.makedirs(W)
    out = {}
    # ---- single end: the genome of make_golden_sam_records.py
    g = synth.make_genome(20260925, 100_000, n_contigs=2, repeat_frac=0.4, max_copies=60, repeat_len=(150, 1200), n_run_frac=0.004)
    rng = np.random.default_rng(99)
    alt = g[0][1][20_000:32_000].copy()
    mut = rng.random(alt.size) < 0.01
    alt[mut] = synth._ACGT[rng.integers(0, 4, size=int(mut.sum()))]
    g.append(('chrA_alt1', alt))
    synth.write_fasta(W + '/s.fa', g)
    ref.build_index(W + '/s.fa', W + '/sidx', 20, threads=4, extra=['-altContigName', 'chrA_alt1'])
    idx = GenomeIndex.load_from_directory(W + '/sidx')
    gold = util.load_golden_index()
    assert (idx.contig_begin == gold.contig_begin).all() and (idx.genome_padded == gold.genome_padded).all()
    z = np.load(OUT + '/sam_records_single.npz')
    o = z['offsets'].astype(np.int64)
    with open(W + '/s.fq', 'wb') as f:
        for i in range(N_SINGLE):
            f.write(b'@r%d\n' % i + z['bases'][o[i]:o[i + 1]].tobytes() + b'\n+\n' + z['quals'][o[i]:o[i + 1]].tobytes() + b'\n')
    for tag, cli in SINGLE_SETS:
        run([ref.CLI_PATH, 'single', W + '/sidx', W + '/s.fq', '-o', W + '/s_%s.bam' % tag, '-t', '1'] + cli)
        _, refs, recs = bam_parts(W + '/s_%s.bam' % tag)
        keep = z[tag + '_rec_read'] < N_SINGLE
        assert len(recs) == int(keep.sum()) and (flags_of(recs) == z[tag + '_flag'][keep]).all(), tag
        out['single_' + tag] = np.frombuffer(b''.join(recs), np.uint8)
        out['single_ref_id'] = ref_ids(idx, refs)
        print('single', tag, len(recs), 'records', out['single_' + tag].size, 'bytes')
    out['single_n'] = np.int32(N_SINGLE)
    # ---- paired end: the genome of make_golden_sam_fields_paired.py
    g = synth.make_genome(20260926, 240_000, n_contigs=3, repeat_frac=0.35, max_copies=40, repeat_len=(150, 1500), n_run_frac=0.003)
    synth.write_fasta(W + '/p.fa', g)
    ref.build_index(W + '/p.fa', W + '/pidx', 20, threads=4)
    idx = GenomeIndex.load_from_directory(W + '/pidx')
    gold = util.load_golden_index('paired_index.npz')
    assert (idx.contig_begin == gold.contig_begin).all() and (idx.genome_padded == gold.genome_padded).all()
    z = np.load(OUT + '/sam_fields_paired.npz')
    o = z['offsets'].astype(np.int64)
    for w in (0, 1):
        with open(W + '/p%d.fq' % (w + 1), 'wb') as f:
            for i in range(N_PAIRS):
                m = 2 * i + w
                f.write(b'@p%d/%d\n' % (i, w + 1) + z['bases'][o[m]:o[m + 1]].tobytes() + b'\n+\n' + z['quals'][o[m]:o[m + 1]].tobytes() + b'\n')
    for tag, cli in PAIRED_SETS:
        run([ref.CLI_PATH, 'paired', W + '/pidx', W + '/p1.fq', W + '/p2.fq', '-o', W + '/p_%s.bam' % tag, '-t', '1'] + cli)
        _, refs, recs = bam_parts(W + '/p_%s.bam' % tag)
        fw = z[tag + '_first_written'][:N_PAIRS]
        order = np.stack([2 * np.arange(N_PAIRS) + fw, 2 * np.arange(N_PAIRS) + 1 - fw], axis=1).reshape(-1)
        assert len(recs) == 2 * N_PAIRS and (flags_of(recs) == z[tag + '_flag'][order]).all(), tag
        out['paired_' + tag] = np.frombuffer(b''.join(recs), np.uint8)
        out['paired_ref_id'] = ref_ids(idx, refs)
        print('paired', tag, len(recs), 'records', out['paired_' + tag].size, 'bytes')
    out['paired_n'] = np.int32(N_PAIRS)
    np.savez_compressed(OUT + '/bam_records.npz', **out)
    print('written', OUT + '/bam_records.npz', os.path.getsize(OUT + '/bam_records.npz'), 'bytes')


if __name__ == '__main__':
    main()
