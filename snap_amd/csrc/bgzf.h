// bgzf.h -- bytes -> BGZF blocks (snapgpu_bgzf_compress*): what the tool's bgzf_append (host/snapgpu_sam.cpp) and, on the reference's side, the
// BGZF writer of Bam.cpp with DataWriter's gzip filter do with the record bytes of a BAM file.  Member m of a call covers the input bytes
// [m * block_input, min((m + 1) * block_input, n_bytes)) and is one gzip member:
//   1f 8b 08 04 | MTIME 0 | XFL 0 | OS ff | XLEN 6 | 42 43 02 00 | BSIZE = size - 1 | raw DEFLATE | CRC32 | ISIZE
// The DEFLATE payload is one dynamic-Huffman block (BTYPE 10), one stored block (BTYPE 00) where that would not be smaller than len + 5
// bytes -- so a member never exceeds len + 31 bytes -- or, for an empty input, the fixed block 03 00 of the specification's end-of-file member.
//   k_bgzf_deflate       one wavefront per member, static stride: the member into its slot of a fixed stride, its size into size[m]
//   k_bgzf_sums          the sum of every SAMREC_CHUNK-member tile of size[]
//   k_samtext_partials / k_samtext_begins   (sam_text.h, as they are) member_begin, the 64-bit exclusive scan
//   k_bgzf_place         one wavefront per member that lies wholly below the capacity: slot -> out, through sambam_store
// A member's wavefront:
//   LZ77      64 positions a step.  A lane hashes the 4 bytes at its position, reads the candidate earlier STEPS left in head[] (LDS, position
//             + 1, 0 = none), extends it dword by dword to at most min(258, len - pos) bytes and a distance of at most 32768; then the lanes
//             publish their positions with atomicMax, so that head[h] is the highest position with that hash whatever the order of the lanes.
//             A wave-uniform pass picks matches (>= 4 bytes) greedily from a cursor that carries over; tokens go to the wave's HBM list.
//   Huffman   lit/len, distance and code-length codes from the LDS histograms: a rank sort by all lanes, then on lane 0 the in-place minimum-
//             redundancy lengths over the sorted counts, the counts per length folded to the limit (15, 15, 7) and repaired until the Kraft sum
//             is exactly 1, lengths handed out by rank, canonical codes.  One used symbol gets one bit; no distance symbol: one code of zero bits.
//   emission  every lane takes a contiguous run of tokens: their bits, a wave scan to bit offsets, then a 64-bit bit buffer.  The slot is zero
//             beforehand; a lane's first and last dword go in with atomicOr, the dwords between with plain stores, so no bit depends on an order.
//   CRC32     byte-wise table CRC over a lane's slice, the slices combined pairwise by x^(8 n) mod P (what zlib's crc32_combine computes).
// LDS per wave: BGZF_LDS_WORDS dwords (head[], three histograms, three code tables); the Huffman work arrays reuse head[] once LZ77 is done.
#pragma once
#include "dev_common.h"
#include "cigar_args.h"
#include "sam_records.h"
#include "sam_text.h"
#include "sam_bam.h"

#define BGZF_HASH_BITS 12u
#define BGZF_NHEAD (1u << BGZF_HASH_BITS)
#define BGZF_NLL 288u               // 286 lit/len symbols, rounded
#define BGZF_ND 32u                 // 30 distance symbols, rounded
#define BGZF_NCL 32u                // 19 code-length symbols, rounded
#define BGZF_MIN_MATCH 4u
#define BGZF_MAX_MATCH 258u
#define BGZF_WINDOW 32768u
#define BGZF_HEAD_BYTES 18u
#define BGZF_EOB 256u
// the work arrays inside head[]: the sorted counts, their symbols, counts per length / next code, the code-length sequence of the header
#define BGZF_W_KEY 0u
#define BGZF_W_SYM 288u
#define BGZF_W_CNT 576u
#define BGZF_W_SEQ 640u
#define BGZF_SEQ_MAX 320u
static_assert(BGZF_W_SEQ + BGZF_SEQ_MAX <= BGZF_NHEAD, "the Huffman work arrays fit head[]");
static_assert(BGZF_LDS_WORDS == BGZF_NHEAD + 2u * (BGZF_NLL + BGZF_ND + BGZF_NCL), "cigar_args.h sizes the launch's LDS");

struct BgzfCrcTable { uint32_t t[256]; };
static constexpr BgzfCrcTable bgzf_make_crc_table() {
    BgzfCrcTable r{};
    for (uint32_t n = 0; n < 256; n++) { uint32_t c = n; for (int k = 0; k < 8; k++) c = (c & 1u) ? 0xedb88320u ^ (c >> 1) : c >> 1; r.t[n] = c; }
    return r;
}
static __device__ const BgzfCrcTable bgzf_crc_table = bgzf_make_crc_table();
static_assert(bgzf_make_crc_table().t[1] == 0x77073096u && bgzf_make_crc_table().t[255] == 0x2d02ef8du, "the CRC-32 table of zlib");

// a * b mod P, polynomials over GF(2) in the CRC's reflected form (bit 31 is x^0)
static __device__ __forceinline__ uint32_t bgzf_mulmodp(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 32; i++) { if (a & 0x80000000u) p ^= b; a <<= 1; b = (b >> 1) ^ ((b & 1u) ? 0xedb88320u : 0u); }
    return p;
}
static __device__ __forceinline__ uint32_t bgzf_x8n(uint32_t n) {          // x^(8 n) mod P
    uint32_t r = 0x80000000u, p = 0x00800000u;
    while (n) { if (n & 1u) r = bgzf_mulmodp(r, p); p = bgzf_mulmodp(p, p); n >>= 1; }
    return r;
}
static __device__ __forceinline__ uint32_t bgzf_load32(const uint8_t *p) { uint32_t w; __builtin_memcpy(&w, p, 4); return w; }

// the lit/len symbol of a match of L bytes and the distance symbol of distance D, with their extra bits
static __device__ __forceinline__ uint32_t bgzf_len_sym(uint32_t L, uint32_t *eb, uint32_t *ev) {
    if (L == BGZF_MAX_MATCH) { *eb = 0; *ev = 0; return 285u; }
    const uint32_t l = L - 3u;
    if (l < 8u) { *eb = 0; *ev = 0; return 257u + l; }
    const uint32_t e = (31u - (uint32_t)__builtin_clz(l)) - 2u;
    *eb = e; *ev = l & ((1u << e) - 1u);
    return 257u + 4u * e + 4u + ((l >> e) & 3u);
}
static __device__ __forceinline__ uint32_t bgzf_dist_sym(uint32_t D, uint32_t *eb, uint32_t *ev) {
    const uint32_t d = D - 1u;
    if (d < 4u) { *eb = 0; *ev = 0; return d; }
    const uint32_t n = 31u - (uint32_t)__builtin_clz(d);
    *eb = n - 1u; *ev = d & ((1u << (n - 1u)) - 1u);
    return 2u * n + ((d >> (n - 1u)) & 1u);
}
// a token: a literal or end-of-block (0 .. 256), or bit 31 | (L - 3) << 16 | (D - 1)
static __device__ __forceinline__ uint32_t bgzf_token_bits(uint32_t t, const uint32_t *code_ll, const uint32_t *code_d) {
    if (!(t >> 31)) return code_ll[t] & 255u;
    uint32_t eb, ev, db, dv;
    const uint32_t ls = bgzf_len_sym(((t >> 16) & 255u) + 3u, &eb, &ev), ds = bgzf_dist_sym((t & 0xffffu) + 1u, &db, &dv);
    return (code_ll[ls] & 255u) + eb + (code_d[ds] & 255u) + db;
}

// bits into a zeroed slot, from any bit offset: the first dword a writer touches and its last, partial one may be shared with its neighbours
struct BgzfBits { uint32_t *w; unsigned long long acc; uint32_t n; bool first; };
static __device__ __forceinline__ BgzfBits bgzf_bits_at(uint8_t *slot, uint32_t bit) { return BgzfBits{(uint32_t *)slot + (bit >> 5), 0ull, bit & 31u, true}; }
static __device__ __forceinline__ void bgzf_put(BgzfBits &b, uint32_t v, uint32_t nb) {      // nb <= 32, v < 2^nb
    b.acc |= (unsigned long long)v << b.n; b.n += nb;
    if (b.n >= 32u) {
        if (b.first) { atomicOr(b.w, (uint32_t)b.acc); b.first = false; } else *b.w = (uint32_t)b.acc;
        b.w++; b.acc >>= 32; b.n -= 32u;
    }
}
static __device__ __forceinline__ void bgzf_finish(BgzfBits &b) { if (b.n) atomicOr(b.w, (uint32_t)b.acc); }
static __device__ __forceinline__ void bgzf_put_code(BgzfBits &b, uint32_t entry) { bgzf_put(b, entry >> 8, entry & 255u); }

// Code lengths of at most max_len bits and their canonical codes for the n_sym counts of freq[], into code[s] = bit-reversed code << 8 | length
// (0: the symbol is not coded).  All lanes call it; scr is the work area inside head[].
static __device__ __forceinline__ void bgzf_build_code(const uint32_t *freq, uint32_t n_sym, uint32_t max_len, uint32_t *code, uint32_t *scr, int lane)
{
    uint32_t *key = scr + BGZF_W_KEY, *sym = scr + BGZF_W_SYM, *cnt = scr + BGZF_W_CNT;
    uint32_t mine = 0;
    for (uint32_t i = (uint32_t)lane; i < n_sym; i += WAVE) {
        const uint32_t f = freq[i];
        code[i] = 0;
        if (f) {                                                             // the symbol's place among the used ones, by (count, symbol)
            uint32_t rank = 0;
            for (uint32_t j = 0; j < n_sym; j++) { const uint32_t g = freq[j]; if (g && (g < f || (g == f && j < i))) rank++; }
            key[rank] = f; sym[rank] = i; mine++;
        }
    }
    const uint32_t n = (uint32_t)__shfl((int)samrec_incl_scan(mine), 63);
    WAVE_SYNC();
    if (lane == 0 && n == 1u) code[sym[0]] = 1u;                             // one bit, code 0
    if (lane == 0 && n > 1u) {
        // minimum-redundancy code lengths in place over the ascending counts (Moffat and Katajainen)
        key[0] += key[1];
        uint32_t root = 0, leaf = 2;
        for (uint32_t next = 1; next < n - 1u; next++) {
            if (leaf >= n || key[root] < key[leaf]) { key[next] = key[root]; key[root++] = next; } else key[next] = key[leaf++];
            if (leaf >= n || (root < next && key[root] < key[leaf])) { key[next] += key[root]; key[root++] = next; } else key[next] += key[leaf++];
        }
        key[n - 2u] = 0;
        for (int next = (int)n - 3; next >= 0; next--) key[next] = key[key[next]] + 1u;
        {
            int avbl = 1, used = 0, r = (int)n - 2, next = (int)n - 1;
            uint32_t depth = 0;
            while (avbl > 0) {
                while (r >= 0 && key[r] == depth) { used++; r--; }
                while (avbl > used) { key[next--] = depth; avbl--; }
                avbl = 2 * used; depth++; used = 0;
            }
        }
        // symbols per length, every length beyond the limit folded into it; then codes move down until the Kraft sum is 1.  The loop relies on
        // two things: folding only ever raises the sum, so total >= 2^max_len, and while it is above, some length below max_len has a symbol
        // (n <= 2^max_len symbols: 286 at 15 bits, 30 at 15, 19 at 7 -- all of them at max_len would already sum to at most 1).
        // (The rank sort in front of this is n_sym^2 / 64 compares a lane: about 1 300 LDS reads for the 286 lit/len symbols.)
        for (uint32_t l = 0; l <= 16u; l++) cnt[l] = 0;
        for (uint32_t i = 0; i < n; i++) cnt[key[i] < max_len ? key[i] : max_len]++;
        uint32_t total = 0;
        for (uint32_t l = max_len; l > 0; l--) total += cnt[l] << (max_len - l);
        while (total != (1u << max_len)) {
            cnt[max_len]--;
            for (uint32_t l = max_len - 1u; l > 0; l--) if (cnt[l]) { cnt[l]--; cnt[l + 1u] += 2u; break; }
            total--;
        }
        // the shortest codes to the largest counts (the end of the sorted list)
        {
            uint32_t j = n;
            for (uint32_t l = 1; l <= max_len; l++) for (uint32_t k = cnt[l]; k > 0; k--) code[sym[--j]] = l;
        }
        // canonical codes, bit-reversed: DEFLATE sends a code from its most significant bit
        uint32_t c = 0;
        for (uint32_t l = 1; l <= max_len; l++) { c = (c + cnt[l - 1u]) << 1; cnt[16u + l] = c; }
        for (uint32_t s = 0; s < n_sym; s++) {
            const uint32_t l = code[s];
            if (l) { const uint32_t v = cnt[16u + l]++; code[s] = ((__brev(v) >> (32u - l)) << 8) | l; }
        }
    }
    WAVE_SYNC();
}
static_assert(BGZF_W_CNT + 16u + 15u < BGZF_W_SEQ, "counts per length and next codes fit their area");

// the order in which the header sends the lengths of the code-length code
static __device__ __forceinline__ uint32_t bgzf_cl_order(uint32_t i) { return (uint32_t)"\x10\x11\x12\x00\x08\x07\x09\x06\x0a\x05\x0b\x04\x0c\x03\x0d\x02\x0e\x01\x0f"[i]; }

static __device__ __forceinline__ void bgzf_member(const BgzfArgs &a, uint32_t m, uint32_t *lds, uint32_t *tok, int lane)
{
    const uint64_t at = (uint64_t)m * a.block_input;
    const uint32_t len = (uint32_t)(a.n_bytes - at < (uint64_t)a.block_input ? a.n_bytes - at : (uint64_t)a.block_input);      // (0 only for the one member of an empty input)
    const uint8_t *in = a.in + at;
    uint8_t *slot = a.slots + (uint64_t)m * a.slot_stride;
    uint32_t *head = lds, *freq_ll = head + BGZF_NHEAD, *freq_d = freq_ll + BGZF_NLL, *freq_cl = freq_d + BGZF_ND;
    uint32_t *code_ll = freq_cl + BGZF_NCL, *code_d = code_ll + BGZF_NLL, *code_cl = code_d + BGZF_ND;
    for (uint32_t i = (uint32_t)lane; i < BGZF_NHEAD + BGZF_NLL + BGZF_ND + BGZF_NCL; i += WAVE) head[i] = 0;      // head[] and the histograms
    // ---- CRC32 of the member's input
    uint32_t crc;
    {
        const uint32_t S = (len + 63u) / 64u;
        const uint32_t b = (uint32_t)lane * S < len ? (uint32_t)lane * S : len, e = b + S < len ? b + S : len;
        uint32_t c = 0xffffffffu, nb = e - b;
        for (uint32_t i = b; i < e; i++) c = bgzf_crc_table.t[(c ^ in[i]) & 255u] ^ (c >> 8);
        c = ~c;
        for (int o = 1; o < WAVE; o <<= 1) {
            const uint32_t c2 = (uint32_t)__shfl_down((int)c, (unsigned)o), n2 = (uint32_t)__shfl_down((int)nb, (unsigned)o);
            if ((lane & (2 * o - 1)) == 0) { c = bgzf_mulmodp(bgzf_x8n(n2), c) ^ c2; nb += n2; }
        }
        crc = (uint32_t)__shfl((int)c, 0);
    }
    WAVE_SYNC();
    // ---- LZ77
    uint32_t ntok = 0, cursor = 0;
    for (uint32_t base = 0; base < len; base += WAVE) {
        const uint32_t pos = base + (uint32_t)lane;
        const bool hashed = pos + 4u <= len;
        uint32_t h = 0, mlen = 0, mdist = 0;
        if (hashed) {
            h = (bgzf_load32(in + pos) * 2654435761u) >> (32u - BGZF_HASH_BITS);
            const uint32_t cand = head[h];
            if (cand && pos - (cand - 1u) <= BGZF_WINDOW) {
                const uint32_t cp = cand - 1u, maxl = len - pos < BGZF_MAX_MATCH ? len - pos : BGZF_MAX_MATCH;
                uint32_t l = 0;
                while (l + 4u <= maxl) {
                    const uint32_t x = bgzf_load32(in + cp + l) ^ bgzf_load32(in + pos + l);
                    if (x) { l += (uint32_t)__builtin_ctz(x) >> 3; break; }
                    l += 4u;
                }
                if (l + 4u > maxl) while (l < maxl && in[cp + l] == in[pos + l]) l++;
                if (l >= BGZF_MIN_MATCH) { mlen = l; mdist = pos - cp; }
            }
        }
        WAVE_SYNC();
        if (hashed) atomicMax(&head[h], pos + 1u);
        WAVE_SYNC();
        // the tokens of this step: greedily from the cursor, which a match may carry beyond the step
        const unsigned long long has = BALLOT(mlen != 0u);
        const uint32_t end = len - base < (uint32_t)WAVE ? len - base : (uint32_t)WAVE;
        unsigned long long sel = 0;
        uint32_t c = cursor - base;                                          // (cursor >= base)
        while (c < end) {
            const unsigned long long rest = has >> c;
            const uint32_t nl = rest ? c + (uint32_t)__builtin_ctzll(rest) : end;
            if (nl > c) sel |= (nl - c >= 64u ? ~0ull : ((1ull << (nl - c)) - 1ull)) << c;      // literals up to the next match
            if (nl >= end) { c = end; break; }
            sel |= 1ull << nl;
            c = nl + (uint32_t)__shfl((int)mlen, (int)nl);
        }
        cursor = base + c;
        if ((sel >> lane) & 1ull) {
            const bool match = ((has >> lane) & 1ull) != 0ull;
            const uint32_t idx = ntok + (uint32_t)__builtin_popcountll(sel & ((1ull << lane) - 1ull));
            if (match) {
                uint32_t eb, ev;
                tok[idx] = 0x80000000u | ((mlen - 3u) << 16) | (mdist - 1u);
                atomicAdd(&freq_ll[bgzf_len_sym(mlen, &eb, &ev)], 1u);
                atomicAdd(&freq_d[bgzf_dist_sym(mdist, &eb, &ev)], 1u);
            } else {
                const uint32_t b = in[pos];
                tok[idx] = b;
                atomicAdd(&freq_ll[b], 1u);
            }
        }
        ntok += (uint32_t)__builtin_popcountll(sel);
    }
    if (lane == 0) { tok[ntok] = BGZF_EOB; freq_ll[BGZF_EOB] += 1u; }
    WAVE_SYNC();
    __threadfence();                                                         // the tokens are read back by other lanes
    // ---- the codes
    bgzf_build_code(freq_ll, 286u, 15u, code_ll, head, lane);
    bgzf_build_code(freq_d, 30u, 15u, code_d, head, lane);
    uint32_t *seq = head + BGZF_W_SEQ;
    uint32_t hdr[4] = {0u, 0u, 0u, 0u};                                       // lane 0: nll, nd, n_seq, hclen
    if (lane == 0) {
        uint32_t nll = 286u, nd = 30u;
        while (nll > 257u && !(code_ll[nll - 1u] & 255u)) nll--;
        while (nd > 1u && !(code_d[nd - 1u] & 255u)) nd--;
        const uint32_t total = nll + nd;
        auto len_at = [&](uint32_t i) -> uint32_t { return (i < nll ? code_ll[i] : code_d[i - nll]) & 255u; };
        uint32_t ns = 0;
        for (uint32_t i = 0; i < total;) {
            const uint32_t v = len_at(i);
            uint32_t run = 1;
            while (i + run < total && len_at(i + run) == v) run++;
            uint32_t r = run;
            if (v == 0u) {
                while (r >= 11u) { const uint32_t t = r < 138u ? r : 138u; seq[ns++] = 18u | ((t - 11u) << 8); r -= t; }
                if (r >= 3u) { seq[ns++] = 17u | ((r - 3u) << 8); r = 0; }
            } else {
                seq[ns++] = v; r--;
                while (r >= 3u) { const uint32_t t = r < 6u ? r : 6u; seq[ns++] = 16u | ((t - 3u) << 8); r -= t; }
            }
            while (r) { seq[ns++] = v; r--; }
            i += run;
        }
        uint32_t used = 0, one = 0;
        for (uint32_t i = 0; i < ns; i++) { const uint32_t s = seq[i] & 255u; if (!freq_cl[s]) { used++; one = s; } freq_cl[s]++; }
        if (used == 1u) freq_cl[one == 0u ? 1u : 0u] = 1u;                   // the code-length code must be complete: two symbols at least
        hdr[0] = nll; hdr[1] = nd; hdr[2] = ns;
    }
    WAVE_SYNC();
    bgzf_build_code(freq_cl, 19u, 7u, code_cl, head, lane);
    uint32_t hdr_bits = 0;
    if (lane == 0) {
        uint32_t hclen = 19u;
        while (hclen > 4u && !(code_cl[bgzf_cl_order(hclen - 1u)] & 255u)) hclen--;
        hdr[3] = hclen;
        hdr_bits = 3u + 5u + 5u + 4u + 3u * hclen;
        for (uint32_t i = 0; i < hdr[2]; i++) {
            const uint32_t s = seq[i] & 255u;
            hdr_bits += (code_cl[s] & 255u) + (s == 16u ? 2u : s == 17u ? 3u : s == 18u ? 7u : 0u);
        }
    }
    hdr_bits = (uint32_t)__shfl((int)hdr_bits, 0);
    // ---- the bits of every lane's run of tokens (end-of-block is the last token)
    const uint32_t nt = ntok + 1u, per = (nt + 63u) / 64u;
    const uint32_t t0 = (uint32_t)lane * per < nt ? (uint32_t)lane * per : nt, t1 = t0 + per < nt ? t0 + per : nt;
    uint32_t my_bits = 0;
    for (uint32_t t = t0; t < t1; t++) my_bits += bgzf_token_bits(tok[t], code_ll, code_d);
    const uint32_t incl = samrec_incl_scan(my_bits);
    const uint32_t payload_bits = hdr_bits + (uint32_t)__shfl((int)incl, 63);
    uint32_t payload = (payload_bits + 7u) >> 3;
    const bool stored = len != 0u && payload >= len + 5u;
    if (len == 0u) payload = 2u; else if (stored) payload = len + 5u;
    const uint32_t size = BGZF_HEAD_BYTES + payload + 8u;
    if (len == 0u || stored) {
        // the gzip header, the block, the trailer: plain bytes (the wave owns the slot)
        for (uint32_t j = (uint32_t)lane; j < size; j += WAVE) {
            uint32_t v;
            if (j < BGZF_HEAD_BYTES) v = j == 16u ? (size - 1u) & 255u : j == 17u ? (size - 1u) >> 8 : (uint32_t)(uint8_t)"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00\x42\x43\x02\x00"[j];
            else if (j >= BGZF_HEAD_BYTES + payload) { const uint32_t k = j - BGZF_HEAD_BYTES - payload; v = ((k < 4u ? crc : len) >> (8u * (k & 3u))) & 255u; }
            else if (len == 0u) v = j == BGZF_HEAD_BYTES ? 3u : 0u;
            else {
                const uint32_t k = j - BGZF_HEAD_BYTES;
                v = k == 0u ? 1u : k == 1u ? len & 255u : k == 2u ? len >> 8 : k == 3u ? ~len & 255u : k == 4u ? (~len >> 8) & 255u : (uint32_t)in[k - 5u];
            }
            slot[j] = (uint8_t)v;
        }
    } else {
        if (lane == 0) {
            BgzfBits b = bgzf_bits_at(slot, 0u);
            bgzf_put(b, 0x04088b1fu, 32u); bgzf_put(b, 0u, 32u); bgzf_put(b, 0x0006ff00u, 32u); bgzf_put(b, 0x00024342u, 32u); bgzf_put(b, size - 1u, 16u);
            bgzf_put(b, 1u | (2u << 1), 3u); bgzf_put(b, hdr[0] - 257u, 5u); bgzf_put(b, hdr[1] - 1u, 5u); bgzf_put(b, hdr[3] - 4u, 4u);
            for (uint32_t i = 0; i < hdr[3]; i++) bgzf_put(b, code_cl[bgzf_cl_order(i)] & 255u, 3u);
            for (uint32_t i = 0; i < hdr[2]; i++) {
                const uint32_t s = seq[i] & 255u;
                bgzf_put_code(b, code_cl[s]);
                if (s >= 16u) bgzf_put(b, seq[i] >> 8, s == 16u ? 2u : s == 17u ? 3u : 7u);
            }
            bgzf_finish(b);
            BgzfBits t = bgzf_bits_at(slot, 8u * (BGZF_HEAD_BYTES + payload));
            bgzf_put(t, crc, 32u); bgzf_put(t, len, 32u);
            bgzf_finish(t);
        }
        if (t0 < t1) {
            BgzfBits b = bgzf_bits_at(slot, 8u * BGZF_HEAD_BYTES + hdr_bits + incl - my_bits);
            for (uint32_t t = t0; t < t1; t++) {
                const uint32_t k = tok[t];
                if (!(k >> 31)) bgzf_put_code(b, code_ll[k]);
                else {
                    uint32_t eb, ev, db, dv;
                    const uint32_t ls = bgzf_len_sym(((k >> 16) & 255u) + 3u, &eb, &ev), ds = bgzf_dist_sym((k & 0xffffu) + 1u, &db, &dv);
                    bgzf_put_code(b, code_ll[ls]); if (eb) bgzf_put(b, ev, eb);
                    bgzf_put_code(b, code_d[ds]); if (db) bgzf_put(b, dv, db);
                }
            }
            bgzf_finish(b);
        }
    }
    if (lane == 0) a.size[m] = size;
    WAVE_SYNC();
}

__global__ __launch_bounds__(64) void k_bgzf_deflate(BgzfArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int lane = lane_id();
    const uint32_t wave = first_u32(samrec_wave_id()), n_waves = first_u32(samrec_n_waves());
    uint32_t *tok = a.tok + (uint64_t)wave * a.tok_stride;
    for (uint32_t m = wave; m < a.n_members; m += n_waves) bgzf_member(a, m, (uint32_t *)lds, tok, lane);
}

// the tile sums of size[] that k_samtext_partials scans
__global__ __launch_bounds__(256) void k_bgzf_sums(BgzfArgs a)
{
    const int lane = lane_id();
    const uint32_t n_chunks = (a.n_members + SAMREC_CHUNK - 1u) / SAMREC_CHUNK;
    for (uint32_t c = samrec_wave_id(); c < n_chunks; c += samrec_n_waves()) {
        unsigned long long s = 0;
        for (int k = 0; k < SAMREC_ROUNDS; k++) {
            const uint64_t r = (uint64_t)c * SAMREC_CHUNK + (uint64_t)k * 64 + (uint64_t)lane;
            if (r < a.n_members) s += a.size[r];
        }
        s = samtext_incl_scan64(s);
        if (lane == 63) a.partial[c] = s;
    }
}

// slot -> its place in the output, for the members that lie wholly below the capacity: no store leaves [member_begin[m], member_begin[m + 1])
__global__ __launch_bounds__(256) void k_bgzf_place(BgzfArgs a)
{
    const int lane = lane_id();
    for (uint32_t m = first_u32(samrec_wave_id()); m < a.n_members; m += first_u32(samrec_n_waves())) {
        const uint64_t begin = first_u64(a.member_begin[m]), end = first_u64(a.member_begin[m + 1]);
        if (end > a.cap) continue;
        const uint8_t *src = a.slots + (uint64_t)m * a.slot_stride;
        sambam_store(a.out + begin, (uint32_t)(end - begin), lane, [&](uint32_t j) -> uint32_t { return (uint32_t)src[j]; });
    }
}
