// sam_bam.h -- records -> the bytes of their BAM records (snapgpu_bam_records_single* / _paired*): what BAMFormat::writeRead and writePairs lay
// out for a record of a BAM file (Bam.cpp:1312-1508, 1033-1309), before BGZF compression, from the fields the SAM-field kernels left in HBM.
// Per record, little endian:
//   block_size | refID | pos - 1 | bin << 16 | (mapq & 0xff) << 8 | l_qname + 1 | flag << 16 | n_cigar | l_seq | next_refID | pnext - 1 | tlen
//   | QNAME NUL | cigar | SEQ | QUAL | aux
// refID / next_refID are the BAM numbers of the contigs (snapgpu_set_contig_bam_ids) or -1; QNAME is the read's name cut at its first space
// (a pair's names first lose "/1" / "/2" together, as in sam_text.h); the cigar is the record's row of ops as it stands (no operations for
// n_ops <= 0); SEQ is the whole (unclipped) read, two bases a byte, high nibble first, coded by "=ACMGRSVTWYHKDBN" with every other byte 15
// ('=' too: Bam.cpp:505-510 starts at code 1), QUAL is byte - 33; both in the record's orientation (under flag 0x10 the reverse complement that
// sam_text.h's kernels form, rc_base).  bin is reg2bin (Bam.cpp:523-535) over [pos - 1, pos - 1 + ref_len), ref_len the lengths of the
// operations that CigarCodeToRefBase (Bam.cpp:270: M D N P = X) counts, or l_seq without operations; an unmapped mate of a mapped one takes
// it from pnext, every other unmapped record gets reg2bin(-1, 0) (Bam.cpp:1473-1477).  tlen is masked to 31 bits with its sign.  aux: the
// default read group's RG PL PU LB SM, PG:Z:SNAP, NM:C (one byte: -1 reads as 255) and, for mates, QS:i (Bam.cpp:1510-1650).
// Single-end records: next_refID -1, next position -1, tlen 0.
//   k_sambam_len / k_sambam_pair_len        one lane per record: len[r] = 4 + block_size; the sum of every SAMREC_CHUNK-record tile
//   k_samtext_partials / k_samtext_begins   (sam_text.h, as they are) block_begin, the 64-bit exclusive scan, and where the last record that fits ends
//   k_samtext_qs                            (sam_text.h, as it is) QS of every mate, before the pair records' write pass
//   k_sambam_write / k_sambam_pair_write    one wavefront per record, for the records that lie wholly below the capacity
// As in sam_text.h: no LDS, no per-wave scratch, a record is never staged; both passes place a record's parts through sambam_at, so a store
// never leaves [block_begin[r], block_begin[r + 1]).  A record starts at any byte address: nothing here assumes an alignment.
#pragma once
#include "dev_common.h"
#include "cigar_args.h"
#include "sam_records.h"
#include "sam_text.h"

#define SAMBAM_AUX "RGZFASTQ\0PLZIllumina\0PUZpu\0LBZlb\0SMZsm\0PGZSNAP\0NMC"      // then NM's byte; mates: "QSi" and four bytes
#define SAMBAM_AUX_LEN ((uint32_t)sizeof(SAMBAM_AUX) - 1u)
#define SAMBAM_HEAD 36u                                                                 // block_size and the eight fixed words
static_assert(SAMBAM_AUX_LEN == 50u, "RG PL PU LB SM PG and NM's tag and type");
static_assert(SAMBAM_AUX_LEN + 1u + 7u <= 64u, "aux goes a byte a lane");

// the code of the letters 'A' + first .. 'A' + first + 15, a nibble each (Bam.cpp:505-510: SeqToCode, 15 where CodeToSeq[1..15] has no entry)
static constexpr unsigned long long sambam_code_table(int first) {
    unsigned long long t = 0;
    for (int i = 0; i < 16; i++) {
        unsigned long long code = 15;
        for (int k = 1; k < 16; k++) if ("=ACMGRSVTWYHKDBN"[k] == 'A' + first + i) code = (unsigned long long)k;
        t |= code << (4 * i);
    }
    return t;
}
static_assert(sambam_code_table(0) == 0xFFF3FCFFB4FFD2E1ull && sambam_code_table(16) == 0xFFFFFFFAF97F865Full, "A1 C2 M3 G4 R5 S6 V7 T8 W9 Y10 H11 K12 D13 B14 N15");
static __device__ __forceinline__ uint32_t sambam_code(uint32_t c) {
    const uint32_t i = c - (uint32_t)'A';
    if (i >= 32u) return 15u;
    const unsigned long long t = i < 16u ? sambam_code_table(0) : sambam_code_table(16);
    return (uint32_t)(t >> (4u * (i & 15u))) & 15u;
}
static __device__ __forceinline__ int sambam_reg2bin(int beg, int end) {                // Bam.cpp:523-535
    --end;
    if (beg >> 14 == end >> 14) return ((1 << 15) - 1) / 7 + (beg >> 14);
    if (beg >> 17 == end >> 17) return ((1 << 12) - 1) / 7 + (beg >> 17);
    if (beg >> 20 == end >> 20) return ((1 << 9) - 1) / 7 + (beg >> 20);
    if (beg >> 23 == end >> 23) return ((1 << 6) - 1) / 7 + (beg >> 23);
    if (beg >> 26 == end >> 26) return ((1 << 3) - 1) / 7 + (beg >> 26);
    return 0;
}
// what an operation adds to ref_len (CigarCodeToRefBase, Bam.cpp:270)
static __device__ __forceinline__ uint32_t sambam_ref_len(uint32_t op) { return ((0x1CDu >> (op & 15u)) & 1u) ? op >> 4 : 0u; }

// The fields of record j of a call but for the cut name and ref_len, which the passes find in their own ways.  PAIRED: record j is position
// j & 1 of unit j >> 1, as a pair line of sam_text.h.  A record that cannot be written (n_ops beyond its row, a contig or an rnext the index
// does not have, a first_written that is neither 0 nor 1) is laid out without that field and flagged.
struct SamBamRec {
    uint32_t rd, fi, U, name_len, bad;         // the read, where the fields are (the row of ops too), l_seq, the name up to its end (the space not looked for)
    uint64_t read_at, name_at;
    int flag, mapq, n_cig, nm, ref, pos0, next_ref, pnext0, tlen, qs;
};
template <bool PAIRED> static __device__ __forceinline__ SamBamRec sambam_record(const SamBamArgs &a, uint32_t j)
{
    SamBamRec l;
    l.bad = 0;
    uint32_t v = 0, u = j, k = 0;
    if (PAIRED) {
        u = j >> 1; k = a.rec_read ? a.rec_read[u] : u;
        int fw = a.first_written[u];
        if (fw != 0 && fw != 1) { fw = 0; l.bad |= SAMTEXT_BAD_RECORD; }
        v = (j & 1u) ? 1u - (uint32_t)fw : (uint32_t)fw;
        l.rd = 2u * k + v; l.fi = 2u * u + v;
    } else { l.rd = a.rec_read ? a.rec_read[j] : j; l.fi = j; }
    l.read_at = a.offsets[l.rd]; l.U = (uint32_t)(a.offsets[l.rd + 1] - l.read_at);
    l.name_at = a.name_off[l.rd]; l.name_len = (uint32_t)(a.name_off[l.rd + 1] - l.name_at);
    if (PAIRED) {
        // the suffix rule of samtext_layout(SamTextPairedArgs), on the two names of pair k (ReadWriter.cpp:405-420).  Restated, not shared: moving
        // it out of that function into a helper of both changed k_samtext_pair_len's registers (70 -> 71 VGPRs).
        const uint64_t n0 = a.name_off[2u * k], n1 = a.name_off[2u * k + 1u], n2 = a.name_off[2u * k + 2u];
        const uint32_t L = (uint32_t)(n1 - n0);
        if (L == (uint32_t)(n2 - n1) && L > 2u && a.names[n0 + L - 2u] == '/' && a.names[n1 + L - 2u] == '/') {
            const uint8_t c0 = a.names[n0 + L - 1u], c1 = a.names[n1 + L - 1u];
            if ((c0 == '1' || c0 == '2') && (c1 == '1' || c1 == '2') && c0 != c1) l.name_len -= 2u;
        }
    }
    l.flag = a.flag[l.fi]; l.mapq = a.mapq[l.fi]; l.nm = a.nm[l.fi]; l.pos0 = (int)((uint32_t)a.pos[l.fi] - 1u);
    if (l.nm == -2) l.bad |= SAMTEXT_NM_OVERFLOW;
    l.n_cig = a.n_ops[l.fi];
    if (l.n_cig > (int)a.ops_stride) { l.n_cig = 0; l.bad |= SAMTEXT_BAD_RECORD; }
    if (l.n_cig < 0) l.n_cig = 0;
    int contig = a.contig[l.fi];
    if (contig >= (int)a.n_contigs) { contig = -1; l.bad |= SAMTEXT_BAD_RECORD; }
    l.ref = contig >= 0 ? a.ref_id[contig] : -1;
    l.next_ref = -1; l.pnext0 = -1; l.tlen = 0; l.qs = 0;
    if (PAIRED) {
        int rnext = a.rnext[l.fi];
        if (rnext < -2 || rnext >= (int)a.n_contigs) { rnext = -1; l.bad |= SAMTEXT_BAD_RECORD; }
        l.next_ref = rnext == -2 ? l.ref : rnext >= 0 ? a.ref_id[rnext] : -1;
        l.pnext0 = (int)((uint32_t)a.pnext[l.fi] - 1u);
        const long long t = a.tlen[l.fi];
        l.tlen = t >= 0 ? (int)(t & 0x7fffffffll) : -(int)((0ull - (unsigned long long)t) & 0x7fffffffull);
        l.qs = a.qs[2u * u + 1u - v];
    }
    return l;
}

// Where the parts of a record stand, from the start of its block_size word, given the length of its cut name: the one layout of both passes.
struct SamBamAt { uint32_t cigar, seq, qual, aux, end; };
template <bool PAIRED> static __device__ __forceinline__ SamBamAt sambam_at(const SamBamRec &l, uint32_t qn)
{
    SamBamAt at;
    at.cigar = SAMBAM_HEAD + qn + 1u; at.seq = at.cigar + 4u * (uint32_t)l.n_cig; at.qual = at.seq + (l.U + 1u) / 2u; at.aux = at.qual + l.U;
    at.end = at.aux + SAMBAM_AUX_LEN + 1u + (PAIRED ? 7u : 0u);
    return at;
}

// the length pass over the records of a call
template <bool PAIRED> static __device__ __forceinline__ void sambam_len_body(const SamBamArgs &a)
{
    const int lane = lane_id();
    for (uint32_t c = samrec_wave_id(); c < a.n_chunks; c += samrec_n_waves()) {
        unsigned long long s = 0;
        uint32_t bad = 0;
        for (int k = 0; k < SAMREC_ROUNDS; k++) {
            const uint64_t r = (uint64_t)c * SAMREC_CHUNK + (uint64_t)k * 64 + (uint64_t)lane;
            if (r < a.n) {
                const SamBamRec l = sambam_record<PAIRED>(a, (uint32_t)r);
                uint32_t qn = 0;
                while (qn < l.name_len && a.names[l.name_at + qn] != ' ') qn++;
                if (qn > 254u) { bad |= SAMBAM_LONG_NAME; atomicMax(&a.summary->pad, ~(uint32_t)r); }      // (pad: ~ the first such record)
                const uint32_t len = sambam_at<PAIRED>(l, qn).end;
                a.len[r] = len;
                s += len; bad |= l.bad;
            }
        }
        if (bad) atomicOr(&a.summary->flags, bad);
        s = samtext_incl_scan64(s);
        if (lane == 63) a.partial[c] = s;
    }
}
__global__ __launch_bounds__(256) void k_sambam_len(SamBamArgs a) { sambam_len_body<false>(a); }
__global__ __launch_bounds__(256) void k_sambam_pair_len(SamBamArgs a) { sambam_len_body<true>(a); }

// a little-endian word at any byte address
static __device__ __forceinline__ void sambam_put32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

// n bytes to dst, all 64 lanes, byte j being get(j): the bytes up to the first dword boundary of dst and behind the last one go one by one,
// the dwords between them whole (samtext_copy's stores, over any source)
template <class G> static __device__ __forceinline__ void sambam_store(uint8_t *dst, uint32_t n, int lane, G get)
{
    uint32_t head = (4u - (uint32_t)((uintptr_t)dst & 3u)) & 3u;
    if (head > n) head = n;
    const uint32_t nd = (n - head) >> 2, tail_at = head + 4u * nd, tail = n - tail_at;
    if ((uint32_t)lane < head) dst[lane] = (uint8_t)get((uint32_t)lane);
    for (uint32_t d = (uint32_t)lane; d < nd; d += WAVE) {
        const uint32_t j = head + 4u * d;
        *(uint32_t *)(dst + j) = get(j) | (get(j + 1u) << 8) | (get(j + 2u) << 16) | (get(j + 3u) << 24);
    }
    if ((uint32_t)lane < tail) dst[tail_at + (uint32_t)lane] = (uint8_t)get(tail_at + (uint32_t)lane);
}

// the write pass over the records of a call
template <bool PAIRED> static __device__ __forceinline__ void sambam_write_body(const SamBamArgs &a)
{
    const int lane = lane_id();
    for (uint32_t r = first_u32(samrec_wave_id()); r < a.n; r += first_u32(samrec_n_waves())) {
        const uint64_t begin = first_u64(a.line_begin[r]), end = first_u64(a.line_begin[r + 1]);
        if (end > a.cap) continue;                                           // the record does not lie wholly below the capacity: not a byte of it
        const SamBamRec l = sambam_record<PAIRED>(a, r);
        uint8_t *p = a.text + begin;
        // ---- QNAME: copied as it is searched for its first space, 64 bytes a round
        uint32_t qn = l.name_len;
        for (uint32_t base = 0; base < l.name_len; base += WAVE) {
            const uint32_t j = base + (uint32_t)lane;
            const uint8_t c = j < l.name_len ? a.names[l.name_at + j] : (uint8_t)0;
            const unsigned long long sp = BALLOT(j < l.name_len && c == ' ');
            const uint32_t stop = sp ? base + (uint32_t)__builtin_ctzll(sp) : l.name_len;
            if (j < stop) p[SAMBAM_HEAD + j] = c;
            if (sp) { qn = stop; break; }
        }
        const SamBamAt at = sambam_at<PAIRED>(l, qn);
        // ---- the cigar: 64 operations a round as they stand, and the reference bases they span
        uint32_t ref_len = l.n_cig > 0 ? 0u : l.U;
        const bool cigar_aligned = ((uintptr_t)(p + at.cigar) & 3u) == 0;
        for (int base = 0; base < l.n_cig; base += WAVE) {
            const int j = base + lane;
            const uint32_t op = j < l.n_cig ? a.ops[(size_t)l.fi * a.ops_stride + (size_t)j] : 0u;
            if (j < l.n_cig) {
                uint8_t *q = p + at.cigar + 4u * (uint32_t)j;
                if (cigar_aligned) *(uint32_t *)q = op; else sambam_put32(q, op);
            }
            ref_len += (uint32_t)__shfl((int)samrec_incl_scan(sambam_ref_len(op)), 63);
        }
        // ---- the fixed head, a word a lane
        int bin;
        if (!(l.flag & 0x4)) bin = sambam_reg2bin(l.pos0, (int)((uint32_t)l.pos0 + ref_len));
        else if (PAIRED && !(l.flag & 0x8)) bin = sambam_reg2bin(l.pnext0, (int)((uint32_t)l.pnext0 + 1u));
        else bin = sambam_reg2bin(-1, 0);
        if (lane < 9) {
            const uint32_t w = lane == 0 ? at.end - 4u : lane == 1 ? (uint32_t)l.ref : lane == 2 ? (uint32_t)l.pos0
                             : lane == 3 ? ((uint32_t)bin << 16) | ((uint32_t)(l.mapq & 0xff) << 8) | ((qn + 1u) & 0xffu)
                             : lane == 4 ? ((uint32_t)l.flag << 16) | (uint32_t)l.n_cig : lane == 5 ? l.U : lane == 6 ? (uint32_t)l.next_ref
                             : lane == 7 ? (uint32_t)l.pnext0 : (uint32_t)l.tlen;
            sambam_put32(p + 4u * (uint32_t)lane, w);
        } else if (lane == 9) p[SAMBAM_HEAD + qn] = 0;
        // ---- aux, a byte a lane
        if ((uint32_t)lane < SAMBAM_AUX_LEN) p[at.aux + (uint32_t)lane] = (uint8_t)SAMBAM_AUX[lane];
        else if ((uint32_t)lane == SAMBAM_AUX_LEN) p[at.aux + SAMBAM_AUX_LEN] = (uint8_t)l.nm;
        else if (PAIRED && (uint32_t)lane < SAMBAM_AUX_LEN + 4u) p[at.aux + (uint32_t)lane] = (uint8_t)"QSi"[(uint32_t)lane - SAMBAM_AUX_LEN - 1u];
        else if (PAIRED && (uint32_t)lane < SAMBAM_AUX_LEN + 8u) p[at.aux + (uint32_t)lane] = (uint8_t)((uint32_t)l.qs >> (8u * ((uint32_t)lane - SAMBAM_AUX_LEN - 4u)));
        // ---- SEQ and QUAL: under 0x10 from the far end, the bases complemented, so that the stores ascend either way
        const bool rc = (l.flag & 0x10) != 0;
        const uint8_t *sb = a.bases + l.read_at, *sq = a.quals + l.read_at;
        const uint32_t U = l.U;
        auto base_code = [&](uint32_t i) -> uint32_t { return i < U ? sambam_code(rc ? (uint32_t)rc_base(sb[U - 1u - i]) : (uint32_t)sb[i]) : 0u; };
        sambam_store(p + at.seq, (U + 1u) / 2u, lane, [&](uint32_t j) -> uint32_t { return (base_code(2u * j) << 4) | base_code(2u * j + 1u); });
        sambam_store(p + at.qual, U, lane, [&](uint32_t j) -> uint32_t { return ((uint32_t)(rc ? sq[U - 1u - j] : sq[j]) - 33u) & 255u; });
        WAVE_SYNC();
    }
}
__global__ __launch_bounds__(256) void k_sambam_write(SamBamArgs a) { sambam_write_body<false>(a); }
__global__ __launch_bounds__(256) void k_sambam_pair_write(SamBamArgs a) { sambam_write_body<true>(a); }
