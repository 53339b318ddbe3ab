// bam_sort.h -- the BAM records of a batch into coordinate order (snapgpu_bam_sort*, the _bam_sorted fused calls): what the reference's -so
// does per sort block with a qsort of (location, offset) entries (SortedDataWriter.cpp), here over the record bytes where sam_bam.h left them.
//   key = (uint64)(uint32)refID << 32 | (uint32)(pos + 1)      refID: the int32 at record offset 4, pos: the int32 at offset 8
// both read from the record's own bytes, whatever the writer put there: an unmapped mate that carries its mate's coordinates sorts with its
// mate, and refID -1 (0xffffffff) sorts behind every contig, pos -1 before position 0 of its contig -- the SAM specification's coordinate order.
// The output is the STABLE sort by that key (ties keep the input order), so it is a function of the input alone.
//   k_bamsort_keys        key[i], index[i] = i; which key bits vary over the batch (only passes over such bits run); the extents are checked
//   k_bamsort_hist / k_bamsort_scan_* / k_bamsort_scatter     one LSD pass of radix_pass.h (the index builder's), no element dropped
//   k_bamsort_len         len[r] of the record at sorted place r, the sum of every SAMREC_CHUNK-record tile
//   k_samtext_partials / k_samtext_begins   (sam_text.h, as they are) sorted_begin, the 64-bit exclusive scan
//   k_bamsort_gather      one wavefront per record: its bytes to their place
// A record starts at any byte address on both sides.  The gather stores as sambam_store does (bytes up to the first dword boundary of the
// destination, whole dwords, bytes behind the last one), each dword put together from four byte loads, or from one dword load where source and
// destination have the same residue mod 4: a shortcut nothing depends on.  No store leaves [sorted_begin[r], sorted_begin[r + 1]).
#pragma once
#include "dev_common.h"
#include "cigar_args.h"
#include "radix_pass.h"
#include "sam_records.h"
#include "sam_text.h"

static __device__ __forceinline__ uint32_t bamsort_get32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
static __device__ __forceinline__ uint64_t bamsort_key(const uint8_t *rec)
{
    const uint32_t ref = bamsort_get32(rec + 4), pos = bamsort_get32(rec + 8);
    return ((uint64_t)ref << 32) | (uint64_t)(uint32_t)(pos + 1u);
}
static __device__ __forceinline__ uint32_t bamsort_wave_or(uint32_t v) {
    for (int o = 1; o < WAVE; o <<= 1) v |= (uint32_t)__shfl_xor((int)v, o);
    return v;
}

__global__ __launch_bounds__(256) void k_bamsort_keys(BamSortArgs a)
{
    const int lane = lane_id();
    const uint64_t total = a.block_begin[a.n];
    uint64_t ones = 0, zeros = 0;
    uint32_t bad = 0;
    for (uint64_t base = (uint64_t)ib_wave_id() * 64; base < a.n; base += (uint64_t)ib_n_waves() * 64) {
        const uint64_t i = base + (uint64_t)lane;
        if (i < a.n) {
            const uint64_t b = a.block_begin[i], e = a.block_begin[i + 1];
            uint32_t f = 0;
            if (e < b || e > total) f = BAMSORT_DECREASING;
            else if (e - b < 12u) f = BAMSORT_SHORT;
            else if (e - b > 0xFFFFFFFFull) f = BAMSORT_LONG;
            uint64_t key = 0;
            if (f) { bad |= f; atomicMax(&a.summary->first_bad[f == BAMSORT_DECREASING ? 0 : f == BAMSORT_SHORT ? 1 : 2], ~(uint32_t)i); }
            else { key = bamsort_key(a.bytes + b); ones |= key; zeros |= ~key; }      // (only a record that lies inside the bytes is read)
            a.key[i] = key; a.index[i] = (uint32_t)i;
        }
    }
    const uint32_t o_lo = bamsort_wave_or((uint32_t)ones), o_hi = bamsort_wave_or((uint32_t)(ones >> 32));
    const uint32_t z_lo = bamsort_wave_or((uint32_t)zeros), z_hi = bamsort_wave_or((uint32_t)(zeros >> 32));
    bad = bamsort_wave_or(bad);
    if (lane == 0) {
        if (o_lo) atomicOr(&a.summary->ones_lo, o_lo);
        if (o_hi) atomicOr(&a.summary->ones_hi, o_hi);
        if (z_lo) atomicOr(&a.summary->zeros_lo, z_lo);
        if (z_hi) atomicOr(&a.summary->zeros_hi, z_hi);
        if (bad) atomicOr(&a.summary->flags, bad);
    }
}

// ---- one pass of the sort: radix_pass.h's bodies, every key an element
__global__ __launch_bounds__(256) void k_bamsort_hist(const uint64_t *keys, uint64_t n, uint32_t shift, uint32_t *hist, uint32_t n_tiles)
{
    static __shared__ uint32_t sh[4][64];
    ib_hist_body<false>(keys, n, shift, hist, n_tiles, sh[(threadIdx.x >> 6) & 3]);
}
__global__ __launch_bounds__(256) void k_bamsort_scatter(const uint64_t *keys_in, const uint32_t *vals_in, uint64_t n, uint32_t shift,
                                                         const uint32_t *offs, uint32_t n_tiles, uint64_t *keys_out, uint32_t *vals_out)
{
    static __shared__ uint32_t sh[4][64];
    ib_scatter_body<false>(keys_in, vals_in, n, shift, offs, n_tiles, keys_out, vals_out, sh[(threadIdx.x >> 6) & 3]);
}
__global__ __launch_bounds__(256) void k_bamsort_scan_sums(const uint32_t *in, uint64_t n, uint32_t *partial, uint32_t n_chunks) { ib_scan_sums_body(in, n, partial, n_chunks); }
__global__ __launch_bounds__(64) void k_bamsort_scan_partials(uint32_t *partial, uint32_t n_chunks, uint32_t *total) { ib_scan_partials_body(partial, n_chunks, total); }
__global__ __launch_bounds__(256) void k_bamsort_scan_apply(const uint32_t *in, uint64_t n, const uint32_t *partial, uint32_t n_chunks, uint32_t *out)
{
    ib_scan_apply_body(in, n, partial, n_chunks, out);
}

// ---- the lengths of the records in sorted order, for sam_text.h's scan
__global__ __launch_bounds__(256) void k_bamsort_len(BamSortArgs a)
{
    const int lane = lane_id();
    for (uint32_t c = samrec_wave_id(); c < a.n_chunks; c += samrec_n_waves()) {
        unsigned long long s = 0;
        for (int k = 0; k < SAMREC_ROUNDS; k++) {
            const uint64_t r = (uint64_t)c * SAMREC_CHUNK + (uint64_t)k * 64 + (uint64_t)lane;
            if (r < a.n) {
                const uint32_t i = a.perm[r];
                const uint32_t len = (uint32_t)(a.block_begin[i + 1] - a.block_begin[i]);
                a.len[r] = len;
                s += len;
            }
        }
        s = samtext_incl_scan64(s);
        if (lane == 63) a.partial[c] = s;
    }
}

// ---- every record to its place
__global__ __launch_bounds__(256) void k_bamsort_gather(BamSortArgs a)
{
    const int lane = lane_id();
    for (uint64_t r = first_u32(samrec_wave_id()); r < a.n; r += first_u32(samrec_n_waves())) {      // (64 bits: n may be 2^32 - 1)
        const uint32_t i = first_u32(a.perm[r]);
        const uint64_t from = first_u64(a.block_begin[i]), to = first_u64(a.sorted_begin[r]);
        const uint32_t n = (uint32_t)(first_u64(a.sorted_begin[r + 1]) - to);
        const uint8_t *src = a.bytes + from;
        uint8_t *dst = a.sorted + to;
        const bool same = (((uintptr_t)src ^ (uintptr_t)dst) & 3u) == 0;      // a dword boundary of dst is then one of src
        uint32_t head = (4u - (uint32_t)((uintptr_t)dst & 3u)) & 3u;
        if (head > n) head = n;
        const uint32_t nd = (n - head) >> 2, tail_at = head + 4u * nd, tail = n - tail_at;
        if ((uint32_t)lane < head) dst[lane] = src[lane];
        for (uint32_t d = (uint32_t)lane; d < nd; d += WAVE) {
            const uint32_t j = head + 4u * d;
            *(uint32_t *)(dst + j) = same ? *(const uint32_t *)(src + j) : bamsort_get32(src + j);
        }
        if ((uint32_t)lane < tail) dst[tail_at + (uint32_t)lane] = src[tail_at + (uint32_t)lane];
    }
}
