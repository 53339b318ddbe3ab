// TEST INFRASTRUCTURE: bgzf_build_code (snap_amd/csrc/bgzf.h) on histograms of the test's choosing.  The routine has no entry of its own in
// the product and gets none: this translation unit includes bgzf.h through the emulator's headers, holds one test kernel around the call and
// is built by tests/emu/build.py's build_coder_harness() into a shared object of its own (with wave_emu.o), never into libsnapgpu_emu.so or
// the product.  The kernel sets the LDS up the way bgzf_member does: head[] first, which the routine uses as its work area, the histogram and
// the code table behind it.
#include <hip/hip_runtime.h>
#include "bgzf.h"

struct BgzfCoderArgs { const uint32_t *freq; uint32_t *code; uint32_t n_hist, n_sym, max_len; };

__global__ __launch_bounds__(64) void k_bgzf_test_build_code(BgzfCoderArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int lane = lane_id();
    uint32_t *head = (uint32_t *)lds, *freq = head + BGZF_NHEAD, *code = freq + BGZF_NLL;
    for (uint32_t h = blockIdx.x; h < a.n_hist; h += gridDim.x) {
        for (uint32_t i = (uint32_t)lane; i < BGZF_NHEAD; i += WAVE) head[i] = 0xa5a5a5a5u;      // (what LZ77 leaves there is of no concern to it)
        for (uint32_t i = (uint32_t)lane; i < BGZF_NLL; i += WAVE) { freq[i] = i < a.n_sym ? a.freq[(uint64_t)h * a.n_sym + i] : 0u; code[i] = 0xffffffffu; }
        WAVE_SYNC();
        bgzf_build_code(freq, a.n_sym, a.max_len, code, head, lane);
        for (uint32_t i = (uint32_t)lane; i < a.n_sym; i += WAVE) a.code[(uint64_t)h * a.n_sym + i] = code[i];
        WAVE_SYNC();
    }
}

// code[h * n_sym + s] = bit-reversed code << 8 | length for the n_hist histograms of n_sym counts each; -1: arguments out of range
extern "C" int bgzf_coder_build(const uint32_t *freq, uint32_t n_hist, uint32_t n_sym, uint32_t max_len, uint32_t *code, uint32_t blocks)
{
    if (!freq || !code || n_sym == 0u || n_sym > BGZF_NLL || max_len == 0u || max_len > 15u || blocks == 0u) return -1;
    BgzfCoderArgs a{freq, code, n_hist, n_sym, max_len};
    hipLaunchKernelGGL(k_bgzf_test_build_code, dim3(blocks), dim3(64), (size_t)(BGZF_NHEAD + 2u * BGZF_NLL) * 4, nullptr, a);
    return hipDeviceSynchronize() == hipSuccess ? 0 : -2;
}
