// radix_pass.h -- one pass of the stable LSD radix sort over (64-bit key, 32-bit value) and the 32-bit exclusive scan it needs, as bodies that
// the kernels of two translation units wrap: index_build.h (k_ib_*: (seed, location) by seed) and bam_sort.h (k_bamsort_*: (coordinate key,
// record index) by key).  6 bits per pass, one bin per lane: counts, offsets and running ranks are wave operations.
//   ib_hist_body      hist[bin * n_tiles + tile] = elements of the tile whose digit is bin (bin-major, so ONE exclusive scan over the whole
//                     array yields the output offset of every (bin, tile))
//   ib_scan_*_body    that scan: tile sums, their scan by one wavefront, the apply pass
//   ib_scatter_body   every element to offs[bin][tile] + its rank among the tile's elements of the same bin: ranks ascend with the input
//                     index, which is what makes the pass stable
// DROP: elements whose key is IB_INVALID_KEY are neither counted nor scattered (the index builder's first pass drops the locations without
// a seed that way); without it every key is an element, all ones included.
// Everything is wave-level: no block barriers; `bins` is 64 words of LDS of the calling wave's own.
#pragma once
#include "dev_common.h"

#define IB_INVALID_KEY 0xFFFFFFFFFFFFFFFFull
#define IB_TILE 1024u            // elements per wavefront tile: 16 rounds of 64
#define IB_ROUNDS 16
#define IB_BITS 6                // radix bits per pass: one bin per lane

static __device__ __forceinline__ uint32_t ib_wave_id()  { return (uint32_t)((blockIdx.x * blockDim.x + threadIdx.x) >> 6); }
static __device__ __forceinline__ uint32_t ib_n_waves()  { return (uint32_t)((gridDim.x * blockDim.x) >> 6); }

// inclusive prefix sum over the 64 lanes
static __device__ __forceinline__ uint32_t ib_wave_incl_scan(uint32_t v) {
    const int lane = lane_id();
    for (int o = 1; o < WAVE; o <<= 1) { const uint32_t t = (uint32_t)__shfl_up((int)v, o); if (lane >= o) v += t; }
    return v;
}

// lanes with the same (valid) digit as this one
static __device__ __forceinline__ uint64_t ib_peers(uint32_t d, bool valid) {
    uint64_t p = BALLOT(valid);
#pragma unroll
    for (int b = 0; b < IB_BITS; b++) {
        const bool bit = (d >> b) & 1u;
        const uint64_t m = BALLOT(bit);
        p &= bit ? m : ~m;
    }
    return valid ? p : 0ull;
}

template <bool DROP> static __device__ __forceinline__ void ib_hist_body(const uint64_t *keys, uint64_t n, uint32_t shift, uint32_t *hist, uint32_t n_tiles, uint32_t *h)
{
    const int lane = lane_id();
    for (uint32_t tile = ib_wave_id(); tile < n_tiles; tile += ib_n_waves()) {
        h[lane] = 0;
        WAVE_SYNC();
        for (int r = 0; r < IB_ROUNDS; r++) {
            const uint64_t i = (uint64_t)tile * IB_TILE + (uint64_t)r * 64 + (uint64_t)lane;
            const uint64_t key = i < n ? keys[i] : IB_INVALID_KEY;
            const bool valid = DROP ? key != IB_INVALID_KEY : i < n;
            const uint32_t d = (uint32_t)(key >> shift) & 63u;
            const uint64_t peers = ib_peers(d, valid);
            if (valid && (peers & ((1ull << lane) - 1ull)) == 0) h[d] += (uint32_t)__popcll(peers);      // the lowest peer speaks for all
            WAVE_SYNC();
        }
        hist[(size_t)lane * n_tiles + tile] = h[lane];
        WAVE_SYNC();
    }
}

template <bool DROP> static __device__ __forceinline__ void ib_scatter_body(const uint64_t *keys_in, const uint32_t *vals_in, uint64_t n, uint32_t shift,
                                                                            const uint32_t *offs, uint32_t n_tiles, uint64_t *keys_out, uint32_t *vals_out, uint32_t *run)
{
    const int lane = lane_id();
    for (uint32_t tile = ib_wave_id(); tile < n_tiles; tile += ib_n_waves()) {
        run[lane] = offs[(size_t)lane * n_tiles + tile];          // where the tile's elements of bin `lane` start in the output
        WAVE_SYNC();
        for (int r = 0; r < IB_ROUNDS; r++) {
            const uint64_t i = (uint64_t)tile * IB_TILE + (uint64_t)r * 64 + (uint64_t)lane;
            const uint64_t key = i < n ? keys_in[i] : IB_INVALID_KEY;
            const bool valid = DROP ? key != IB_INVALID_KEY : i < n;
            const uint32_t val = valid ? (vals_in ? vals_in[i] : (uint32_t)i) : 0u;
            const uint32_t d = (uint32_t)(key >> shift) & 63u;
            const uint64_t peers = ib_peers(d, valid);
            const uint64_t below = peers & ((1ull << lane) - 1ull);
            const uint32_t base = valid ? run[d] : 0u;
            WAVE_SYNC();
            if (valid) {
                const uint32_t pos = base + (uint32_t)__popcll(below);
                keys_out[pos] = key; vals_out[pos] = val;
                if (below == 0) run[d] = base + (uint32_t)__popcll(peers);
            }
            WAVE_SYNC();
        }
    }
}

// ---------------------------------------------------------------- exclusive scan of a u32 array (three kernels; chunk = 1024 per wave)
static __device__ __forceinline__ void ib_scan_sums_body(const uint32_t *in, uint64_t n, uint32_t *partial, uint32_t n_chunks)
{
    const int lane = lane_id();
    for (uint32_t c = ib_wave_id(); c < n_chunks; c += ib_n_waves()) {
        uint32_t s = 0;
        for (int r = 0; r < IB_ROUNDS; r++) {
            const uint64_t i = (uint64_t)c * IB_TILE + (uint64_t)r * 64 + (uint64_t)lane;
            s += i < n ? in[i] : 0u;
        }
        s = ib_wave_incl_scan(s);
        if (lane == 63) partial[c] = s;
    }
}
// one wavefront: partial[] -> its exclusive scan in place; total[0] = the sum
static __device__ __forceinline__ void ib_scan_partials_body(uint32_t *partial, uint32_t n_chunks, uint32_t *total)
{
    const int lane = lane_id();
    uint32_t carry = 0;
    for (uint32_t c0 = 0; c0 < n_chunks; c0 += 64) {
        const uint32_t c = c0 + (uint32_t)lane;
        const uint32_t v = c < n_chunks ? partial[c] : 0u;
        const uint32_t inc = ib_wave_incl_scan(v);
        if (c < n_chunks) partial[c] = carry + inc - v;
        carry += (uint32_t)__shfl((int)inc, 63);
    }
    if (lane == 0) total[0] = carry;
}
static __device__ __forceinline__ void ib_scan_apply_body(const uint32_t *in, uint64_t n, const uint32_t *partial, uint32_t n_chunks, uint32_t *out)
{
    const int lane = lane_id();
    for (uint32_t c = ib_wave_id(); c < n_chunks; c += ib_n_waves()) {
        uint32_t carry = partial[c];
        for (int r = 0; r < IB_ROUNDS; r++) {
            const uint64_t i = (uint64_t)c * IB_TILE + (uint64_t)r * 64 + (uint64_t)lane;
            const uint32_t v = i < n ? in[i] : 0u;
            const uint32_t inc = ib_wave_incl_scan(v);
            if (i < n) out[i] = carry + inc - v;
            carry += (uint32_t)__shfl((int)inc, 63);
        }
    }
}
