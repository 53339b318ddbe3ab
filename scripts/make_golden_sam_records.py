"""Generate tests/golden/sam_records_single.npz: every SAM record of a read set as the unmodified reference CLI printed them
(oracle/_ref/snap-aligner single ... -o out.sam -t 1, so the file is in read order), for the option sets that give a read more than one
record or adjust its alignment: -om / -omax / -mpc (secondary results), -ea (first-ALT records), -ae (AlignmentAdjuster).  Per option set:
the read each record belongs to, in file order, and FLAG / RNAME index / POS / MAPQ / CIGAR / NM.  What snapgpu_align_sam_single_records
needs to compute them is stored once: the reads as written to the FASTQ and Read::clip's outcome (ClipBack of '#', the CLI default).
Genome = the golden genome of make_golden.py (locations are tiny_index.npz's; it has one ALT contig)."""
import os, sys, shutil, subprocess
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from snap_amd import synth
from snap_amd.index import GenomeIndex
from oracle import ref
from tests import util

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden')
W = '/tmp/snap_golden_samrec'
# (tag, command line, snapgpu_params fields, (om, omax, mpc) or None, -ae, use_m): tests/samrec_util.py reads the same table from the file
SETS = [('om1_omax4', ['-om', '1', '-omax', '4'], {}, (1, 4, -1), 0, 1),
        ('D2_om2_mpc2', ['-D', '2', '-om', '2', '-mpc', '2'], dict(extra_search_depth=2), (2, 0x7fffffff, 2), 0, 1),
        ('ea_om1', ['-ea', '-om', '1'], dict(emit_alt_alignments=1), (1, 0x7fffffff, -1), 0, 1),
        ('ea', ['-ea'], dict(emit_alt_alignments=1), None, 0, 1),
        ('ae', ['-ae'], {}, None, 1, 1),
        ('ae_om1', ['-ae', '-om', '1'], {}, (1, 0x7fffffff, -1), 1, 1),
        ('lvonly_eqx_om1', ['-G-', '-=', '-om', '1'], dict(use_affine_gap=0), (1, 0x7fffffff, -1), 0, 0)]


def main():
    shutil.rmtree(W, ignore_errors=True); os.makedirs(W)
    g = synth.make_genome(20260925, 100_000, n_contigs=2, repeat_frac=0.4, max_copies=60, repeat_len=(150, 1200), n_run_frac=0.004)
    rng = np.random.default_rng(99)
    alt = g[0][1][20_000:32_000].copy()
    mut = rng.random(alt.size) < 0.01
    ACGT = synth._ACGT
    alt[mut] = ACGT[rng.integers(0, 4, size=int(mut.sum()))]
    g.append(('chrA_alt1', alt))
    synth.write_fasta(W + '/ref.fa', g)
    ref.build_index(W + '/ref.fa', W + '/idx', 20, threads=4, extra=['-altContigName', 'chrA_alt1'])
    idx = GenomeIndex.load_from_directory(W + '/idx')
    gold = util.load_golden_index()
    assert (idx.contig_begin == gold.contig_begin).all() and (idx.genome_padded == gold.genome_padded).all()
    z = np.load(OUT + '/tiny_reads.npz')
    rng = np.random.default_rng(20261017)
    reads = []          # (bases, quals) uint8 arrays
    for tag, n in (('100', 500), ('150', 300)):
        b, q = z['b' + tag], z['q' + tag]
        for i in range(n):
            bb, qq = b[i].copy(), q[i].copy()
            kind = i % 20
            if kind == 1: L = int(rng.integers(30, len(bb))); bb, qq = bb[:L], qq[:L]                   # ragged, some below -mrl 50
            elif kind == 2: qq[len(qq) - int(rng.integers(1, 40)):] = ord('#')                           # '#' tail: clipped by the reader
            elif kind == 3: k = int(rng.integers(1, 4)); bb = np.concatenate([ACGT[rng.integers(0, 4, size=k)], bb])[:len(qq)]   # bases prepended: leading insertion
            elif kind == 4: k = int(rng.integers(1, 4)); bb = np.concatenate([bb[k:], ACGT[rng.integers(0, 4, size=k)]])       # first bases dropped
            elif kind == 5: bb[rng.integers(0, len(bb), size=16)] = ord('N')                             # too many Ns: not aligned
            elif kind == 6: j = int(rng.integers(1, 6)); bb = np.delete(bb, j); qq = qq[:len(bb)]         # deletion right after the start: the adjuster moves it
            elif kind == 7: j = int(rng.integers(1, 6)); bb = np.insert(bb, j, ACGT[rng.integers(0, 4)])[:len(qq)]   # insertion right after the start: soft clip
            elif kind == 8: bb = ACGT[rng.integers(0, 4, size=len(bb))]                                  # unalignable
            reads.append((bb, qq))
    # reads from the ALT contig and from the stretch it copies (first-ALT records), reads inside the repeats come with tiny_reads
    nb = idx.n_bases
    G = idx.genome_padded[(idx.genome_padded.size - nb) // 2:]
    cb = [int(x) for x in idx.contig_begin] + [int(nb)]
    pad = idx.chromosome_padding
    a0 = cb[2]
    for i in range(150):
        L = 100 if i % 2 else 150
        start = (a0 if i % 3 else cb[0] + 20_000) + int(rng.integers(0, 12_000 - L))
        d = G[start:start + L].copy()
        e = rng.random(L) < 0.01
        d[e] = ACGT[rng.integers(0, 4, size=int(e.sum()))]
        if i % 4 == 0: d = synth._COMP[d[::-1]]
        reads.append((d, rng.integers(45, 74, size=L).astype(np.uint8)))
    for c in range(len(cb) - 1):                                  # contig ends: starting before the first base, ending past the last
        real_end = cb[c + 1] - pad
        for L in (100, 150):
            for k in (1, 5):
                reads.append((np.concatenate([ACGT[rng.integers(0, 4, size=k)], G[cb[c]:cb[c] + L - k]]), rng.integers(45, 74, size=L).astype(np.uint8)))
                reads.append((np.concatenate([G[real_end - (L - k):real_end], ACGT[rng.integers(0, 4, size=k)]]), rng.integers(45, 74, size=L).astype(np.uint8)))
    n = len(reads)
    with open(W + '/r.fq', 'wb') as f:
        for i, (b, q) in enumerate(reads):
            f.write(b'@r%d\n' % i + b.tobytes() + b'\n+\n' + q.tobytes() + b'\n')
    bases = np.concatenate([r[0] for r in reads]); quals = np.concatenate([r[1] for r in reads])
    offsets = np.concatenate([[0], np.cumsum([len(r[0]) for r in reads])]).astype(np.uint64)
    fc = np.zeros(n, np.int32); dl = np.zeros(n, np.int32)        # Read::clip, ClipBack: drop the trailing run of '#'
    for i, (b, q) in enumerate(reads):
        m = len(q)
        while m > 0 and q[m - 1] == ord('#'):
            m -= 1
        dl[i] = m
    out = dict(bases=bases, quals=quals, offsets=offsets, front_clip=fc, data_len=dl, sets=np.array([s[0] for s in SETS]))
    contig_of = {c.name: i for i, c in enumerate(idx.contigs)}
    CIG = {c: i for i, c in enumerate('MIDNSHP=X')}
    seen_multi = seen_alt = seen_adjusted = 0
    for tag, cli, kw, sec, ae, use_m in SETS:
        sam = W + '/out_%s.sam' % tag
        r = subprocess.run([ref.CLI_PATH, 'single', W + '/idx', W + '/r.fq', '-o', sam, '-t', '1'] + cli, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert r.returncode == 0, r.stdout.decode()[-2000:]
        rec = []
        for line in open(sam):
            if line.startswith('@'):
                continue
            t = line.rstrip('\n').split('\t')
            ops = []
            if t[5] != '*':
                num = ''
                for ch in t[5]:
                    if ch.isdigit(): num += ch
                    else: ops.append((int(num) << 4) | CIG[ch]); num = ''
            rec.append((int(t[0][1:]), int(t[1]), contig_of.get(t[2], -1), int(t[3]), int(t[4]), int([x for x in t[11:] if x.startswith('NM:i:')][0][5:]), ops))
        m = len(rec)
        width = max(3, max(len(x[6]) for x in rec))
        ops = np.zeros((m, width), np.uint32)
        for k, x in enumerate(rec):
            ops[k, :len(x[6])] = x[6]
        rd = np.array([x[0] for x in rec], np.uint32)
        assert (np.diff(rd.astype(np.int64)) >= 0).all() and np.unique(rd).size == n          # read order, every read there
        out[tag + '_rec_read'] = rd
        out[tag + '_flag'] = np.array([x[1] for x in rec], np.int32); out[tag + '_contig'] = np.array([x[2] for x in rec], np.int32)
        out[tag + '_pos'] = np.array([x[3] for x in rec], np.int64); out[tag + '_mapq'] = np.array([x[4] for x in rec], np.int32)
        out[tag + '_nm'] = np.array([x[5] for x in rec], np.int32); out[tag + '_n_ops'] = np.array([len(x[6]) if x[6] else -1 for x in rec], np.int32)
        out[tag + '_ops'] = ops
        per_read = np.bincount(rd, minlength=n)
        flags = out[tag + '_flag']
        n_sec = per_read - 1
        multi = int((n_sec >= 2).sum())
        if sec is None and '-ea' in cli:
            seen_alt += int((per_read == 2).sum())                # without -om the only second record is the first-ALT one
        if sec is not None:
            seen_multi += multi
        if ae and sec is None:                                    # against the run without -ae: reads the adjuster moved or soft-clipped
            base = subprocess.run([ref.CLI_PATH, 'single', W + '/idx', W + '/r.fq', '-o', W + '/noae.sam', '-t', '1'], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
            assert base.returncode == 0
            a = [l.split('\t')[:6] for l in open(sam) if not l.startswith('@')]
            b0 = [l.split('\t')[:6] for l in open(W + '/noae.sam') if not l.startswith('@')]
            seen_adjusted += sum(1 for x, y in zip(a, b0) if x[3] != y[3] or x[5] != y[5])
        print(tag, 'reads', n, 'records', m, 'reads with >= 2 secondary', multi, 'cigar width', width, 'unmapped', int((flags & 4 != 0).sum()))
    print('first-ALT records under -ea', seen_alt, 'adjusted by -ae', seen_adjusted, 'reads with several secondary results', seen_multi)
    assert seen_multi > 0 and seen_alt > 0 and seen_adjusted > 0
    np.savez_compressed(OUT + '/sam_records_single.npz', **out)
    print('written', OUT + '/sam_records_single.npz', os.path.getsize(OUT + '/sam_records_single.npz'), 'bytes')


if __name__ == '__main__':
    main()
