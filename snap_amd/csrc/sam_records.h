// sam_records.h -- the record list of snapgpu_align_sam_single_records: which SAM records a batch of single-end reads has, in the order
// the reference writes them (SingleAligner.cpp:250-325 -> SimpleReadWriter::writeReads): per read its primary, its secondary results in
// the order finalizeSecondaryResults left them, then its first-ALT result when the aligner produced one (altAwareness && status != NotFound,
// SingleAligner.cpp:312).
//   k_samrec_count      count[i] = 1 + n_secondary[i] + has_alt[i], the sum of every 1024-read chunk, and the reads whose secondary results
//                       outgrew the align launch's stride (they are rerun on their own, cigar_args.h: SamRecSrc)
//   k_samrec_partials   one wavefront: the chunk sums -> their exclusive scan, the batch's total
//   k_samrec_begins     rec_begin[i], the exclusive scan of count
//   k_samrec_list       rec_read / rec_kind of the records the caller has room for
// Wave-level like index_build.h: no block barriers, no LDS.
#pragma once
#include "dev_common.h"
#include "cigar_args.h"

#define SAMREC_ROUNDS 16            // SAMREC_CHUNK (cigar_args.h) reads per wavefront tile: 16 rounds of 64

static __device__ __forceinline__ uint32_t samrec_wave_id() { return (uint32_t)((blockIdx.x * blockDim.x + threadIdx.x) >> 6); }
static __device__ __forceinline__ uint32_t samrec_n_waves() { return (uint32_t)((gridDim.x * blockDim.x) >> 6); }
static __device__ __forceinline__ uint32_t samrec_incl_scan(uint32_t v) {
    const int lane = lane_id();
    for (int o = 1; o < WAVE; o <<= 1) { const uint32_t t = (uint32_t)__shfl_up((int)v, o); if (lane >= o) v += t; }
    return v;
}

// the result record r of read i is written from (k = r - rec_begin[i])
static __device__ __forceinline__ const snapgpu_single_result *samrec_result(const SamRecSrc &s, uint32_t i, uint32_t kind, uint32_t k)
{
    if (kind == SAMREC_PRIMARY) return &s.primary[i];
    if (kind == SAMREC_FIRST_ALT) return &s.first_alt[i];
    const uint32_t slot = s.sec_slot[i];
    return slot == 0xFFFFFFFFu ? &s.secondary[(size_t)i * s.sec_stride + (k - 1)] : &s.sec_ovf[(size_t)slot * s.ovf_stride + (k - 1)];
}

__global__ __launch_bounds__(256) void k_samrec_count(SamRecArgs a)
{
    const int lane = lane_id();
    for (uint32_t c = samrec_wave_id(); c < a.n_chunks; c += samrec_n_waves()) {
        uint32_t s = 0;
        for (int r = 0; r < SAMREC_ROUNDS; r++) {
            const uint64_t i = (uint64_t)c * SAMREC_CHUNK + (uint64_t)r * 64 + (uint64_t)lane;
            uint32_t cnt = 0;
            if (i < a.n) {
                cnt = 1;
                uint32_t slot = 0xFFFFFFFFu;
                if (a.n_secondary) {
                    const uint32_t ns = a.n_secondary[i];
                    if (ns == 0xFFFFFFFFu) atomicOr(&a.summary->cand_overflow, 1u);
                    else {
                        cnt += ns;
                        if (ns > a.src.sec_stride) {
                            slot = atomicAdd(&a.summary->n_overflow, 1u);
                            a.ovf_list[slot] = (uint32_t)i;
                            atomicMax(&a.summary->max_secondary, ns);
                        }
                    }
                }
                if (a.alt_aware && a.src.first_alt[i].status != SNAPGPU_NotFound) cnt++;
                a.count[i] = cnt; a.sec_slot[i] = slot;
            }
            s += cnt;
        }
        s = samrec_incl_scan(s);
        if (lane == 63) a.partial[c] = s;
    }
}

__global__ __launch_bounds__(64) void k_samrec_partials(SamRecArgs a)
{
    if (lane_id() != 0) return;
    unsigned long long carry = 0;
    for (uint32_t c = 0; c < a.n_chunks; c++) { const unsigned long long v = a.partial[c]; a.partial[c] = carry; carry += v; }
    a.summary->total = carry;
    a.rec_begin[a.n] = carry;
}

__global__ __launch_bounds__(256) void k_samrec_begins(SamRecArgs a)
{
    for (uint32_t c = samrec_wave_id(); c < a.n_chunks; c += samrec_n_waves()) {
        unsigned long long carry = a.partial[c];
        for (int r = 0; r < SAMREC_ROUNDS; r++) {
            const uint64_t i = (uint64_t)c * SAMREC_CHUNK + (uint64_t)r * 64 + (uint64_t)lane_id();
            const uint32_t v = i < a.n ? a.count[i] : 0u;
            const uint32_t inc = samrec_incl_scan(v);
            if (i < a.n) a.rec_begin[i] = carry + inc - v;
            carry += (uint32_t)__shfl((int)inc, 63);
        }
    }
}

// One thread per read.  check_clipped (-ae): a read the reader clipped whose adjusted alignment reaches the end of its contig is one the
// adjuster does not reproduce (adjust.h; include/snapgpu.h: snapgpu_adjust_alignments) -- the call is refused, as its callers did per batch.
__global__ __launch_bounds__(256) void k_samrec_list(SamRecArgs a)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (uint64_t)gridDim.x * blockDim.x) {
        const unsigned long long begin = a.rec_begin[i];
        const uint32_t cnt = a.count[i];
        uint32_t ns = a.n_secondary ? a.n_secondary[i] : 0u; if (ns == 0xFFFFFFFFu) ns = 0;
        for (uint32_t k = 0; k < cnt; k++) {
            if (begin + k >= a.cap) break;
            a.rec_read[begin + k] = (uint32_t)i;
            a.rec_kind[begin + k] = (uint8_t)(k == 0 ? SAMREC_PRIMARY : (k <= ns ? SAMREC_SECONDARY : SAMREC_FIRST_ALT));
        }
        if (a.sec_slot[i] != 0xFFFFFFFFu && a.ovf_n_secondary[a.sec_slot[i]] != ns) atomicOr(&a.summary->refused, SAMREC_RERUN_MISMATCH);
        const long long U = (long long)(a.offsets[i + 1] - a.offsets[i]);
        if (a.check_clipped && (a.front_clip[i] != 0 || (long long)a.data_len[i] != U)) {
            for (uint32_t k = 0; k <= ns; k++) {
                const snapgpu_single_result *r = samrec_result(a.src, (uint32_t)i, k == 0 ? SAMREC_PRIMARY : SAMREC_SECONDARY, k);
                if (r->status == SNAPGPU_NotFound) continue;
                const long long loc = (long long)r->location;
                int lo = 0, hi = (int)a.ix.n_contigs - 1, ct = -1;                  // Genome::getContigAtLocation
                while (lo <= hi) { const int mid = (lo + hi) >> 1; if ((long long)a.ix.contig_begin[mid] <= loc) { ct = mid; lo = mid + 1; } else hi = mid - 1; }
                if (ct < 0) continue;
                const long long cend = ct == (int)a.ix.n_contigs - 1 ? (long long)a.ix.n_bases : (long long)a.ix.contig_begin[ct + 1];
                if (loc + a.data_len[i] + (long long)a.max_k + 2 > cend - (long long)a.ix.chromosome_padding) atomicOr(&a.summary->refused, SAMREC_AE_CLIPPED);
            }
        }
    }
}

// the overflowed reads as a batch of their own: read j of the rerun is read ovf_list[j] of the batch (launched over a.summary->n_overflow reads)
__global__ __launch_bounds__(256) void k_samrec_gather(SamRecArgs a, uint32_t m)
{
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j <= m; j += (uint64_t)gridDim.x * blockDim.x) {
        if (j == m) { a.ovf_offsets[m] = a.offsets[a.n]; continue; }
        const uint32_t i = a.ovf_list[j];
        a.ovf_offsets[j] = a.offsets[i]; a.ovf_front_clip[j] = a.front_clip[i]; a.ovf_data_len[j] = a.data_len[i];
    }
}

// where the read the aligner was given starts (the adjuster's `off`)
__global__ __launch_bounds__(256) void k_samrec_clip_off(SamRecArgs a)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (uint64_t)gridDim.x * blockDim.x)
        a.clip_off[i] = a.offsets[i] + (uint64_t)a.front_clip[i];
}
