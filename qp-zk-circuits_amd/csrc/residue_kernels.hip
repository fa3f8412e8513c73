// residue_kernels.hip — the device side of the residue scan (residue.hpp): does any of up to 16 needle words occur in a buffer?
//
// One grid-stride pass per buffer, bound by HBM bandwidth: every lane loads 128 bits (two words) at a time, four such loads in
// flight per iteration. The needles are kernel arguments, so they are uniform and stay in scalar registers; a compare costs one
// v_cmp_eq_u64 against an SGPR pair and no vector register per needle. Matches are rare by construction (a scrubbed buffer has
// none): they leave through an ordinary atomicAdd on the result block's counter and plain vector stores of the first few.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "residue_kernels.hpp"

namespace {

__device__ __forceinline__ void rk_check(uint64_t w, uint64_t index, const ResidueNeedles &nd, ResidueResult *res) {
    bool m = false;
#pragma unroll
    for (uint32_t k = 0; k < QPGPU_RESIDUE_MAX_NEEDLES; k++)
        if (k < nd.n) m = m || w == nd.v[k];      // k < nd.n is uniform: a scalar branch
    if (m) {
        const unsigned long long at = atomicAdd(&res->count, 1ull);
        if (at < RESIDUE_DEV_CAP) { res->found[at].word = w; res->found[at].offset_words = index; }
    }
}

__global__ __launch_bounds__(256) void rk_scan_kernel(const ulonglong2 *__restrict__ buf, uint64_t words, ResidueNeedles nd, ResidueResult *res) {
    const uint64_t pairs = words / 2, stride = (uint64_t)gridDim.x * blockDim.x;
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i + 3 * stride < pairs; i += 4 * stride) {
        const ulonglong2 a = buf[i], b = buf[i + stride], c = buf[i + 2 * stride], d = buf[i + 3 * stride];
        rk_check(a.x, 2 * i, nd, res); rk_check(a.y, 2 * i + 1, nd, res);
        rk_check(b.x, 2 * (i + stride), nd, res); rk_check(b.y, 2 * (i + stride) + 1, nd, res);
        rk_check(c.x, 2 * (i + 2 * stride), nd, res); rk_check(c.y, 2 * (i + 2 * stride) + 1, nd, res);
        rk_check(d.x, 2 * (i + 3 * stride), nd, res); rk_check(d.y, 2 * (i + 3 * stride) + 1, nd, res);
    }
    for (; i < pairs; i += stride) {
        const ulonglong2 a = buf[i];
        rk_check(a.x, 2 * i, nd, res); rk_check(a.y, 2 * i + 1, nd, res);
    }
    if ((words & 1) && blockIdx.x == 0 && threadIdx.x == 0)      // an odd last word
        rk_check(((const uint64_t *)buf)[words - 1], words - 1, nd, res);
}

__global__ __launch_bounds__(256) void rk_zero_kernel(uint64_t *dst, uint64_t words, uint64_t tail_bytes) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += stride) dst[i] = 0;
    if (tail_bytes && blockIdx.x == 0 && threadIdx.x == 0)
        for (uint64_t k = 0; k < tail_bytes; k++) ((unsigned char *)(dst + words))[k] = 0;
}

unsigned grid_for(uint64_t items) {
    const uint64_t blocks = (items + 255) / 256;
    return (unsigned)std::min<uint64_t>(std::max<uint64_t>(blocks, 1), 256 * 8);     // 256 CUs, 8 workgroups of 256 lanes each
}

}  // namespace

hipError_t rk_scan(const uint64_t *buf, uint64_t words, const ResidueNeedles &needles, ResidueResult *res, hipStream_t st) {
    if (words == 0) return hipSuccess;
    if (((uintptr_t)buf & 15) != 0 || needles.n == 0 || needles.n > QPGPU_RESIDUE_MAX_NEEDLES) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rk_scan_kernel, dim3(grid_for((words / 2 + 3) / 4)), dim3(256), 0, st, (const ulonglong2 *)buf, words, needles, res);
    return hipGetLastError();
}

hipError_t rk_zero(void *dst, size_t bytes, hipStream_t st) {
    if (bytes == 0) return hipSuccess;
    if ((uintptr_t)dst & 7) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rk_zero_kernel, dim3(grid_for(bytes / 8)), dim3(256), 0, st, (uint64_t *)dst, (uint64_t)(bytes / 8), (uint64_t)(bytes % 8));
    return hipGetLastError();
}
