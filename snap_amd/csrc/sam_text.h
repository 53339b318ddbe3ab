// sam_text.h -- records -> the bytes of their SAM lines (snapgpu_sam_text_single*): what SAMFormat::writeRead and createSAMLine print for a
// single-end record in a SAM (not BAM) file (SAM.cpp:1424-1572, 1898-2352), from the fields the SAM-field kernels left in HBM:
//   QNAME \t FLAG \t RNAME|* \t POS \t MAPQ \t CIGAR|* \t * \t 0 \t 0 \t SEQ \t QUAL \t PG:Z:SNAP \t NM:i:<nm> \t RG:Z:FASTQ \t PL:Z:Illumina \t PU:Z:pu \t LB:Z:lb \t SM:Z:sm \n
// QNAME is the read's name cut at its first space (SAM.cpp:2001-2004); SEQ / QUAL are the whole (unclipped) read, reverse-complemented /
// reversed under flag 0x10; n_ops < 0 prints "*", n_ops == 0 nothing; integers as printf("%d") / ("%lld") would.
//   k_samtext_len        one lane per record: len[r], the line's length; the sum of every SAMREC_CHUNK-record tile
//   k_samtext_partials   one lane: the tile sums -> their exclusive scan, the batch's total
//   k_samtext_begins     line_begin[r], the exclusive scan of len (64-bit), and where the last line that fits the capacity ends
//   k_samtext_write      one wavefront per record, for the lines that lie wholly below the capacity
// Wave-level like sam_records.h (whose tile size and wave indexing it shares): no block barriers, no LDS -- a line is never staged, every
// byte goes from its source to its place in the text.  A store never leaves [line_begin[r], line_begin[r + 1]): both passes compute a
// line's layout from the same function (samtext_layout).
//
// The two lines of a paired-end result (snapgpu_sam_text_paired*: SAMFormat::writePairs, SAM.cpp:1575-1895, its snprintf at :1854-1875) are
// the same bodies over SamTextPairedArgs -- where line j finds its read, its fields and its name is the overload of samtext_layout:
//   ... CIGAR|* \t RNEXT \t PNEXT \t TLEN \t SEQ \t QUAL ... SM:Z:sm \t QS:i:<qs> \n
// QNAME loses "/1" / "/2" when both names of the pair carry them (ReadWriter.cpp:405-420) and is then cut at its first space; RNEXT is "="
// (rnext -2), "*" (-1) or a contig's name; TLEN the 64-bit value cast to int32; QS the sum of the MATE's qualities of 15 and more (SAM.cpp:1826-1834).
//   k_samtext_qs         one wavefront per mate: qs, before the length pass (a line's length has QS's digits in it)
//   k_samtext_pair_len / k_samtext_pair_write      the length pass and the write pass over pair lines; the scan kernels are the ones above
#pragma once
#include "dev_common.h"
#include "cigar_args.h"
#include "sam_records.h"

#define SAMTEXT_MID "\t*\t0\t0\t"
#define SAMTEXT_TAGS "\tPG:Z:SNAP\tNM:i:"
#define SAMTEXT_TAIL "\tRG:Z:FASTQ\tPL:Z:Illumina\tPU:Z:pu\tLB:Z:lb\tSM:Z:sm\n"
#define SAMTEXT_MID_LEN ((uint32_t)sizeof(SAMTEXT_MID) - 1u)
#define SAMTEXT_TAGS_LEN ((uint32_t)sizeof(SAMTEXT_TAGS) - 1u)
#define SAMTEXT_TAIL_LEN ((uint32_t)sizeof(SAMTEXT_TAIL) - 1u)
#define SAMTEXT_PAIR_TAIL "\tRG:Z:FASTQ\tPL:Z:Illumina\tPU:Z:pu\tLB:Z:lb\tSM:Z:sm\tQS:i:"      // then <qs> \n
#define SAMTEXT_PAIR_TAIL_LEN ((uint32_t)sizeof(SAMTEXT_PAIR_TAIL) - 1u)
static_assert(sizeof(SAMTEXT_PAIR_TAIL) - 1 < 63, "the pair line's tail goes a byte a lane, the last lane prints QS");

static __device__ __forceinline__ uint32_t samtext_digits(unsigned long long v) {
    if (v >> 32) { uint32_t n = 0; while (v) { v /= 10; n++; } return n; }
    const uint32_t x = (uint32_t)v;
    return 1u + (x >= 10u) + (x >= 100u) + (x >= 1000u) + (x >= 10000u) + (x >= 100000u) + (x >= 1000000u) + (x >= 10000000u) + (x >= 100000000u) +
           (x >= 1000000000u);
}
static __device__ __forceinline__ unsigned long long samtext_abs(long long v) { return v < 0 ? (unsigned long long)(-(v + 1)) + 1ull : (unsigned long long)v; }
static __device__ __forceinline__ uint32_t samtext_int_len(long long v) { return (v < 0 ? 1u : 0u) + samtext_digits(samtext_abs(v)); }
// v in decimal at p (samtext_int_len(v) bytes)
static __device__ __forceinline__ void samtext_put_int(uint8_t *p, long long v) {
    unsigned long long m = samtext_abs(v);
    uint32_t nd = samtext_digits(m);
    if (v < 0) *p++ = '-';
    while (m >> 32) { p[--nd] = (uint8_t)('0' + (uint32_t)(m % 10)); m /= 10; }
    uint32_t x = (uint32_t)m;
    while (nd) { p[--nd] = (uint8_t)('0' + x % 10u); x /= 10u; }
}
static __device__ __forceinline__ uint32_t samtext_op_len(uint32_t op) { return samtext_digits(op >> 4) + 1u; }
static __device__ __forceinline__ unsigned long long samtext_shfl_up64(unsigned long long v, int o) {
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, o), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), o);
    return ((unsigned long long)hi << 32) | lo;
}
static __device__ __forceinline__ unsigned long long samtext_incl_scan64(unsigned long long v) {
    const int lane = lane_id();
    for (int o = 1; o < WAVE; o <<= 1) { const unsigned long long t = samtext_shfl_up64(v, o); if (lane >= o) v += t; }
    return v;
}

// The fields of record r and the layout of its line but for the name and the cigar, whose lengths the two passes find in their own ways.
// A record that cannot be printed (n_ops beyond its row, a contig the index does not have) is laid out with "*" in that field and flagged.
struct SamTextLine {
    uint32_t rd, U, cn, bad;                 // the read, its length, the length of RNAME, SAMTEXT_* flags
    uint32_t d_flag, d_pos, d_mapq, d_nm;    // decimal lengths
    int flag, contig, mapq, n_ops, nm; long long pos;
    uint64_t read_at, name_at; uint32_t name_len, cname_at;      // (name_len: up to the end of the name, the space not looked for)
    uint32_t fi;                             // where the record's fields are (its row of ops too)
};
// the line of read rd with the fields at r
static __device__ __forceinline__ SamTextLine samtext_layout_at(const SamTextArgs &a, uint32_t rd, uint32_t r)
{
    SamTextLine l;
    l.rd = rd; l.fi = r;
    l.read_at = a.offsets[l.rd]; l.U = (uint32_t)(a.offsets[l.rd + 1] - l.read_at);
    l.name_at = a.name_off[l.rd]; l.name_len = (uint32_t)(a.name_off[l.rd + 1] - l.name_at);
    l.flag = a.flag[r]; l.contig = a.contig[r]; l.pos = a.pos[r]; l.mapq = a.mapq[r]; l.n_ops = a.n_ops[r]; l.nm = a.nm[r];
    l.bad = l.nm == -2 ? SAMTEXT_NM_OVERFLOW : 0u;
    if (l.n_ops > (int)a.ops_stride) { l.n_ops = -1; l.bad |= SAMTEXT_BAD_RECORD; }
    if (l.contig >= (int)a.n_contigs) { l.contig = -1; l.bad |= SAMTEXT_BAD_RECORD; }
    l.cname_at = 0; l.cn = 1;
    if (l.contig >= 0) { l.cname_at = a.contig_name_off[l.contig]; l.cn = a.contig_name_off[l.contig + 1] - l.cname_at; }
    l.d_flag = samtext_int_len(l.flag); l.d_pos = samtext_int_len(l.pos); l.d_mapq = samtext_int_len(l.mapq); l.d_nm = samtext_int_len(l.nm);
    return l;
}
static __device__ __forceinline__ SamTextLine samtext_layout(const SamTextArgs &a, uint32_t r) { return samtext_layout_at(a, a.rec_read ? a.rec_read[r] : r, r); }

// A pair line: line j is position j & 1 of unit j >> 1 (SamTextPairedArgs).  name_len is already without the "/1" / "/2" that both names of
// the pair lose together, so the space is looked for within the shortened name.  An rnext that is neither -2, -1 nor a contig, and a
// first_written that is neither 0 nor 1 (the line is then laid out as for 0), flag the record as the single-end fields do.
struct SamTextPairLine : SamTextLine {
    uint32_t rn, rnext_at, d_pnext, d_tlen, d_qs;      // RNEXT's length and (rnext >= 0) its place in the contig names; decimal lengths
    int rnext, tlen, qs; long long pnext;
};
static __device__ __forceinline__ SamTextPairLine samtext_layout(const SamTextPairedArgs &a, uint32_t j)
{
    const uint32_t u = j >> 1, k = a.rec_read ? a.rec_read[u] : u;
    int fw = a.first_written[u];
    const bool bad_order = fw != 0 && fw != 1;
    if (bad_order) fw = 0;
    const uint32_t v = (j & 1u) ? 1u - (uint32_t)fw : (uint32_t)fw;
    SamTextPairLine l;
    (SamTextLine &)l = samtext_layout_at(a, 2u * k + v, 2u * u + v);
    if (bad_order) l.bad |= SAMTEXT_BAD_RECORD;
    l.rnext = a.rnext[l.fi]; l.pnext = a.pnext[l.fi]; l.tlen = (int)(uint32_t)(unsigned long long)a.tlen[l.fi]; l.qs = a.qs[2u * u + 1u - v];
    if (l.rnext < -2 || l.rnext >= (int)a.n_contigs) { l.rnext = -1; l.bad |= SAMTEXT_BAD_RECORD; }
    l.rnext_at = 0; l.rn = 1;
    if (l.rnext >= 0) { l.rnext_at = a.contig_name_off[l.rnext]; l.rn = a.contig_name_off[l.rnext + 1] - l.rnext_at; }
    l.d_pnext = samtext_int_len(l.pnext); l.d_tlen = samtext_int_len(l.tlen); l.d_qs = samtext_int_len(l.qs);
    // the suffix rule, on the two names of pair k (ReadWriter.cpp:405-420)
    const uint64_t n0 = a.name_off[2u * k], n1 = a.name_off[2u * k + 1u], n2 = a.name_off[2u * k + 2u];
    const uint32_t L = (uint32_t)(n1 - n0);
    if (L == (uint32_t)(n2 - n1) && L > 2u && a.names[n0 + L - 2u] == '/' && a.names[n1 + L - 2u] == '/') {
        const uint8_t c0 = a.names[n0 + L - 1u], c1 = a.names[n1 + L - 1u];
        if ((c0 == '1' || c0 == '2') && (c1 == '1' || c1 == '2') && c0 != c1) l.name_len -= 2u;
    }
    return l;
}
// what stands between CIGAR and SEQ, and behind NM's digits
static __device__ __forceinline__ uint32_t samtext_mid_len(const SamTextLine &) { return SAMTEXT_MID_LEN; }
static __device__ __forceinline__ uint32_t samtext_mid_len(const SamTextPairLine &l) { return 1u + l.rn + 1u + l.d_pnext + 1u + l.d_tlen + 1u; }
static __device__ __forceinline__ uint32_t samtext_end_len(const SamTextLine &) { return SAMTEXT_TAIL_LEN; }
static __device__ __forceinline__ uint32_t samtext_end_len(const SamTextPairLine &l) { return SAMTEXT_PAIR_TAIL_LEN + l.d_qs + 1u; }
// the line's length, given the lengths of its QNAME and its CIGAR
template <class L> static __device__ __forceinline__ uint32_t samtext_line_len(const L &l, uint32_t qn, uint32_t cig) {
    return qn + 1u + l.d_flag + 1u + l.cn + 1u + l.d_pos + 1u + l.d_mapq + 1u + cig + samtext_mid_len(l) + 2u * l.U + 1u + SAMTEXT_TAGS_LEN + l.d_nm + samtext_end_len(l);
}

// the length pass over the lines of a call: SamTextArgs (k_samtext_len) or SamTextPairedArgs (k_samtext_pair_len)
template <class A> static __device__ __forceinline__ void samtext_len_body(const A &a)
{
    const int lane = lane_id();
    for (uint32_t c = samrec_wave_id(); c < a.n_chunks; c += samrec_n_waves()) {
        unsigned long long s = 0;
        uint32_t bad = 0;
        for (int k = 0; k < SAMREC_ROUNDS; k++) {
            const uint64_t r = (uint64_t)c * SAMREC_CHUNK + (uint64_t)k * 64 + (uint64_t)lane;
            if (r < a.n) {
                const auto l = samtext_layout(a, (uint32_t)r);
                uint32_t qn = 0, cig = l.n_ops < 0 ? 1u : 0u;
                while (qn < l.name_len && a.names[l.name_at + qn] != ' ') qn++;
                for (int j = 0; j < l.n_ops; j++) cig += samtext_op_len(a.ops[(size_t)l.fi * a.ops_stride + (size_t)j]);
                const uint32_t len = samtext_line_len(l, qn, cig);
                a.len[r] = len;
                s += len; bad |= l.bad;
            }
        }
        if (bad) atomicOr(&a.summary->flags, bad);
        s = samtext_incl_scan64(s);
        if (lane == 63) a.partial[c] = s;
    }
}
__global__ __launch_bounds__(256) void k_samtext_len(SamTextArgs a) { samtext_len_body(a); }
__global__ __launch_bounds__(256) void k_samtext_pair_len(SamTextPairedArgs a) { samtext_len_body(a); }

__global__ __launch_bounds__(64) void k_samtext_partials(SamTextArgs a)
{
    if (lane_id() != 0) return;
    unsigned long long carry = 0;
    for (uint32_t c = 0; c < a.n_chunks; c++) { const unsigned long long v = a.partial[c]; a.partial[c] = carry; carry += v; }
    a.summary->total = carry;
    a.line_begin[a.n] = carry;
}

__global__ __launch_bounds__(256) void k_samtext_begins(SamTextArgs a)
{
    for (uint32_t c = samrec_wave_id(); c < a.n_chunks; c += samrec_n_waves()) {
        unsigned long long carry = a.partial[c];
        for (int k = 0; k < SAMREC_ROUNDS; k++) {
            const uint64_t r = (uint64_t)c * SAMREC_CHUNK + (uint64_t)k * 64 + (uint64_t)lane_id();
            const unsigned long long v = r < a.n ? a.len[r] : 0u;
            const unsigned long long inc = samtext_incl_scan64(v);
            if (r < a.n) {
                const unsigned long long end = carry + inc;
                a.line_begin[r] = end - v;
                // (a line is never empty, so exactly one line is the last that fits)
                if (end <= a.cap && (r + 1 == a.n || end + a.len[r + 1] > a.cap)) a.summary->written = end;
            }
            carry += ((unsigned long long)(uint32_t)__shfl((int)(uint32_t)(inc >> 32), 63) << 32) | (uint32_t)__shfl((int)(uint32_t)inc, 63);
        }
    }
}

// n bytes of a read's bases or qualities to dst, all 64 lanes: forwards, or from the far end (rev) with the bases complemented (comp), so that
// the stores ascend either way.  dst is any byte address: the bytes up to the first dword boundary and behind the last one go one by one,
// the dwords between them whole.
static __device__ __forceinline__ void samtext_copy(uint8_t *dst, const uint8_t *src, uint32_t n, bool rev, bool comp, int lane)
{
    uint32_t head = (4u - (uint32_t)((uintptr_t)dst & 3u)) & 3u;
    if (head > n) head = n;
    const uint32_t nd = (n - head) >> 2, tail_at = head + 4u * nd, tail = n - tail_at;
    auto get = [&](uint32_t j) -> uint32_t { const uint8_t c = rev ? src[n - 1u - j] : src[j]; return comp ? (uint32_t)rc_base(c) : (uint32_t)c; };
    if ((uint32_t)lane < head) dst[lane] = (uint8_t)get((uint32_t)lane);
    for (uint32_t d = (uint32_t)lane; d < nd; d += WAVE) {
        const uint32_t j = head + 4u * d;
        *(uint32_t *)(dst + j) = get(j) | (get(j + 1u) << 8) | (get(j + 2u) << 16) | (get(j + 3u) << 24);
    }
    if ((uint32_t)lane < tail) dst[tail_at + (uint32_t)lane] = (uint8_t)get(tail_at + (uint32_t)lane);
}

__global__ __launch_bounds__(256) void k_samtext_write(SamTextArgs a)
{
    const int lane = lane_id();
    for (uint32_t r = first_u32(samrec_wave_id()); r < a.n; r += first_u32(samrec_n_waves())) {
        const uint64_t begin = first_u64(a.line_begin[r]), end = first_u64(a.line_begin[r + 1]);
        if (end > a.cap) continue;                                           // the line does not lie wholly below the capacity: not a byte of it
        const SamTextLine l = samtext_layout(a, r);
        uint8_t *p = a.text + begin;
        // ---- QNAME: copied as it is searched for its first space, 64 bytes a round
        uint32_t qn = l.name_len;
        for (uint32_t base = 0; base < l.name_len; base += WAVE) {
            const uint32_t j = base + (uint32_t)lane;
            const uint8_t c = j < l.name_len ? a.names[l.name_at + j] : (uint8_t)0;
            const unsigned long long sp = BALLOT(j < l.name_len && c == ' ');
            const uint32_t stop = sp ? base + (uint32_t)__builtin_ctzll(sp) : l.name_len;
            if (j < stop) p[j] = c;
            if (sp) { qn = stop; break; }
        }
        // ---- the cigar: 64 operations a round, each lane's place from a scan of the operations' lengths
        const uint32_t at_flag = qn + 1u, at_rname = at_flag + l.d_flag + 1u, at_pos = at_rname + l.cn + 1u, at_mapq = at_pos + l.d_pos + 1u;
        const uint32_t at_cigar = at_mapq + l.d_mapq + 1u;
        uint32_t cig = 0;
        for (int base = 0; base < l.n_ops; base += WAVE) {
            const int j = base + lane;
            const uint32_t op = j < l.n_ops ? a.ops[(size_t)r * a.ops_stride + (size_t)j] : 0u;
            const uint32_t ol = j < l.n_ops ? samtext_op_len(op) : 0u;
            const uint32_t inc = samrec_incl_scan(ol);
            if (j < l.n_ops) {
                uint8_t *q = p + at_cigar + cig + inc - ol;
                samtext_put_int(q, (long long)(op >> 4));
                q[ol - 1u] = (uint8_t)"MIDNSHP=X"[(op & 15u) < 9u ? (op & 15u) : 8u];
            }
            cig += (uint32_t)__shfl((int)inc, 63);
        }
        if (l.n_ops < 0) { cig = 1; if (lane == 3) p[at_cigar] = '*'; }
        const uint32_t at_mid = at_cigar + cig, at_seq = at_mid + SAMTEXT_MID_LEN, at_qual = at_seq + l.U + 1u, at_tags = at_qual + l.U;
        const uint32_t at_nm = at_tags + SAMTEXT_TAGS_LEN, at_tail = at_nm + l.d_nm;
        // ---- the numbers, one lane each
        if (lane == 0) { p[qn] = '\t'; samtext_put_int(p + at_flag, l.flag); p[at_rname - 1u] = '\t'; }
        else if (lane == 1) { p[at_pos - 1u] = '\t'; samtext_put_int(p + at_pos, l.pos); p[at_mapq - 1u] = '\t'; samtext_put_int(p + at_mapq, l.mapq); p[at_cigar - 1u] = '\t'; }
        else if (lane == 2) samtext_put_int(p + at_nm, l.nm);
        // ---- RNAME and the constant pieces, a byte a lane
        if (l.contig < 0) { if (lane == 4) p[at_rname] = '*'; }
        else for (uint32_t j = (uint32_t)lane; j < l.cn; j += WAVE) p[at_rname + j] = a.contig_names[l.cname_at + j];
        if ((uint32_t)lane < SAMTEXT_MID_LEN) p[at_mid + (uint32_t)lane] = (uint8_t)SAMTEXT_MID[lane];
        else if ((uint32_t)lane == SAMTEXT_MID_LEN) p[at_seq + l.U] = '\t';
        else if ((uint32_t)lane < SAMTEXT_MID_LEN + 1u + SAMTEXT_TAGS_LEN) p[at_tags + (uint32_t)lane - SAMTEXT_MID_LEN - 1u] = (uint8_t)SAMTEXT_TAGS[(uint32_t)lane - SAMTEXT_MID_LEN - 1u];
        if ((uint32_t)lane < SAMTEXT_TAIL_LEN) p[at_tail + (uint32_t)lane] = (uint8_t)SAMTEXT_TAIL[lane];
        // ---- SEQ and QUAL
        const bool rc = (l.flag & 0x10) != 0;
        samtext_copy(p + at_seq, a.bases + l.read_at, l.U, rc, rc, lane);
        samtext_copy(p + at_qual, a.quals + l.read_at, l.U, rc, false, lane);
        WAVE_SYNC();
    }
}

// a pair line's RNEXT, PNEXT and TLEN between CIGAR and SEQ, the tab behind SEQ, the tags up to NM's digits, and what follows them up to QS and the
// end of the line: a byte a lane, a number a lane
static __device__ __forceinline__ void samtext_put_pair_fixed(const SamTextPairedArgs &a, const SamTextPairLine &l, uint8_t *p, uint32_t at_mid, uint32_t at_seq,
                                                         uint32_t at_tags, uint32_t at_tail, int lane)
{
    const uint32_t at_rnext = at_mid + 1u, at_pnext = at_rnext + l.rn + 1u, at_tlen = at_pnext + l.d_pnext + 1u;      // (at_seq = at_tlen + d_tlen + 1)
    if (l.rnext < 0) { if (lane == 5) p[at_rnext] = l.rnext == -2 ? '=' : '*'; }
    else for (uint32_t j = (uint32_t)lane; j < l.rn; j += WAVE) p[at_rnext + j] = a.contig_names[l.rnext_at + j];
    if (lane == 6) { p[at_mid] = '\t'; p[at_pnext - 1u] = '\t'; samtext_put_int(p + at_pnext, l.pnext); p[at_tlen - 1u] = '\t'; }
    else if (lane == 7) { samtext_put_int(p + at_tlen, l.tlen); p[at_seq - 1u] = '\t'; p[at_seq + l.U] = '\t'; }
    else if (lane >= 8 && (uint32_t)lane < 8u + SAMTEXT_TAGS_LEN) p[at_tags + (uint32_t)lane - 8u] = (uint8_t)SAMTEXT_TAGS[lane - 8];
    if ((uint32_t)lane < SAMTEXT_PAIR_TAIL_LEN) p[at_tail + (uint32_t)lane] = (uint8_t)SAMTEXT_PAIR_TAIL[lane];
    else if (lane == 63) { samtext_put_int(p + at_tail + SAMTEXT_PAIR_TAIL_LEN, l.qs); p[at_tail + SAMTEXT_PAIR_TAIL_LEN + l.d_qs] = '\n'; }
}

// The write pass over pair lines.  k_samtext_write's steps with the pair line's layout; a kernel of its own because folding the two into one
// body moved k_samtext_write's register figures.  What the two share is what fixes the layout: samtext_layout_at,
// samtext_line_len, samtext_mid_len / samtext_end_len, samtext_put_int, samtext_copy.
__global__ __launch_bounds__(256) void k_samtext_pair_write(SamTextPairedArgs a)
{
    const int lane = lane_id();
    for (uint32_t r = first_u32(samrec_wave_id()); r < a.n; r += first_u32(samrec_n_waves())) {
        const uint64_t begin = first_u64(a.line_begin[r]), end = first_u64(a.line_begin[r + 1]);
        if (end > a.cap) continue;                                           // the line does not lie wholly below the capacity: not a byte of it
        const SamTextPairLine l = samtext_layout(a, r);
        uint8_t *p = a.text + begin;
        // ---- QNAME: copied as it is searched for its first space, 64 bytes a round
        uint32_t qn = l.name_len;
        for (uint32_t base = 0; base < l.name_len; base += WAVE) {
            const uint32_t j = base + (uint32_t)lane;
            const uint8_t c = j < l.name_len ? a.names[l.name_at + j] : (uint8_t)0;
            const unsigned long long sp = BALLOT(j < l.name_len && c == ' ');
            const uint32_t stop = sp ? base + (uint32_t)__builtin_ctzll(sp) : l.name_len;
            if (j < stop) p[j] = c;
            if (sp) { qn = stop; break; }
        }
        // ---- the cigar: 64 operations a round, each lane's place from a scan of the operations' lengths
        const uint32_t at_flag = qn + 1u, at_rname = at_flag + l.d_flag + 1u, at_pos = at_rname + l.cn + 1u, at_mapq = at_pos + l.d_pos + 1u;
        const uint32_t at_cigar = at_mapq + l.d_mapq + 1u;
        uint32_t cig = 0;
        for (int base = 0; base < l.n_ops; base += WAVE) {
            const int j = base + lane;
            const uint32_t op = j < l.n_ops ? a.ops[(size_t)l.fi * a.ops_stride + (size_t)j] : 0u;
            const uint32_t ol = j < l.n_ops ? samtext_op_len(op) : 0u;
            const uint32_t inc = samrec_incl_scan(ol);
            if (j < l.n_ops) {
                uint8_t *q = p + at_cigar + cig + inc - ol;
                samtext_put_int(q, (long long)(op >> 4));
                q[ol - 1u] = (uint8_t)"MIDNSHP=X"[(op & 15u) < 9u ? (op & 15u) : 8u];
            }
            cig += (uint32_t)__shfl((int)inc, 63);
        }
        if (l.n_ops < 0) { cig = 1; if (lane == 3) p[at_cigar] = '*'; }
        const uint32_t at_mid = at_cigar + cig, at_seq = at_mid + samtext_mid_len(l), at_qual = at_seq + l.U + 1u, at_tags = at_qual + l.U;
        const uint32_t at_nm = at_tags + SAMTEXT_TAGS_LEN, at_tail = at_nm + l.d_nm;
        // ---- the numbers, one lane each
        if (lane == 0) { p[qn] = '\t'; samtext_put_int(p + at_flag, l.flag); p[at_rname - 1u] = '\t'; }
        else if (lane == 1) { p[at_pos - 1u] = '\t'; samtext_put_int(p + at_pos, l.pos); p[at_mapq - 1u] = '\t'; samtext_put_int(p + at_mapq, l.mapq); p[at_cigar - 1u] = '\t'; }
        else if (lane == 2) samtext_put_int(p + at_nm, l.nm);
        // ---- RNAME and the constant pieces, a byte a lane
        if (l.contig < 0) { if (lane == 4) p[at_rname] = '*'; }
        else for (uint32_t j = (uint32_t)lane; j < l.cn; j += WAVE) p[at_rname + j] = a.contig_names[l.cname_at + j];
        samtext_put_pair_fixed(a, l, p, at_mid, at_seq, at_tags, at_tail, lane);
        // ---- SEQ and QUAL
        const bool rc = (l.flag & 0x10) != 0;
        samtext_copy(p + at_seq, a.bases + l.read_at, l.U, rc, rc, lane);
        samtext_copy(p + at_qual, a.quals + l.read_at, l.U, rc, false, lane);
        WAVE_SYNC();
    }
}

// QS of every mate a call's lines name: qs[2 u + v] = the sum over the whole (unclipped) quality string of mate v of unit u's pair of b - 33
// wherever b - 33 >= 15, the bytes read as unsigned (SAM.cpp:1826-1834).  One wavefront per mate; the string is read in whole dwords
// between a byte-wise head up to the first dword boundary of the source and a byte-wise tail, as samtext_copy stores.
__global__ __launch_bounds__(256) void k_samtext_qs(SamTextPairedArgs a)
{
    const int lane = lane_id();
    for (uint32_t i = first_u32(samrec_wave_id()); i < a.n; i += first_u32(samrec_n_waves())) {
        const uint32_t u = i >> 1, k = first_u32(a.rec_read ? a.rec_read[u] : u), rd = 2u * k + (i & 1u);
        const uint64_t at = first_u64(a.offsets[rd]);
        const uint32_t n = (uint32_t)(first_u64(a.offsets[rd + 1]) - at);
        const uint8_t *src = a.quals + at;
        uint32_t head = (4u - (uint32_t)((uintptr_t)src & 3u)) & 3u;
        if (head > n) head = n;
        const uint32_t nd = (n - head) >> 2, tail_at = head + 4u * nd, tail = n - tail_at;
        auto term = [](uint32_t b) -> uint32_t { return b >= 33u + 15u ? b - 33u : 0u; };
        uint32_t s = 0;
        if ((uint32_t)lane < head) s += term(src[lane]);
        for (uint32_t d = (uint32_t)lane; d < nd; d += WAVE) {
            const uint32_t w = *(const uint32_t *)(src + head + 4u * d);
            s += term(w & 255u) + term((w >> 8) & 255u) + term((w >> 16) & 255u) + term(w >> 24);
        }
        if ((uint32_t)lane < tail) s += term(src[tail_at + (uint32_t)lane]);
        s = (uint32_t)__shfl((int)samrec_incl_scan(s), 63);
        if (lane == 0) a.qs[i] = (int32_t)s;
    }
}
