// ntt_lde_column.hip — column-resident coset LDE for proof-sized columns (2^11..2^13 coefficients, any rate_bits the planner sends: 1..8).
//
// The generic plan (ntt_plan.cpp) runs every transform above 2^10 points as two launches with an intermediate of the output's
// size in HBM. A zero-padded transform of 2^(d+r) points on the coset g<w_(d+r)> is 2^r independent 2^d-point transforms:
// for LDE point i = k + 2^r t the evaluation point is (g w_(d+r)^k) w_d^t, so coset k is the 2^d-point transform of the
// coefficients scaled by (g w_(d+r)^k)^i, and its values fill LDE slots brev_(d+r)(i) = brev_r(k) 2^d + brev_d(t): one
// contiguous block of the output in exactly the order a decimation-in-frequency transform leaves behind. A workgroup owns one
// (column, coset): it reads the 2^d coefficients once (the 2^r workgroups of a column run side by side, so all but the first
// read is served by a cache), runs the d levels on chip as three register rounds (2^(d-8), 16 and 16 points per thread) with
// two LDS exchanges, and writes the coset's block. No intermediate, one launch.
//
// Round structure for element index n = n1 2^8 + n2 2^4 + n3 and output k = k1 + 2^K1 k2 + 2^(K1+4) k3:
//   round 1  thread m = (n2, n3) transforms over n1 (K1 = d - 8 levels), then x *= w_(2^d)^(m k1)
//   round 2  thread (k1, n3) transforms over n2 (4 levels), then y *= w_256^(n3 k2)
//   round 3  thread (k1, k2) transforms over n3 (4 levels) and stores 16 consecutive slots at brev(k1) 2^8 + brev(k2) 2^4
// The exchanges pass the low and the high 32-bit halves through the same 4-byte slots one after the other (as the split
// passes of ntt_kernel_impl.hpp do): 34 KB of LDS per workgroup at d = 13, so four 256-thread workgroups share a CU and the
// register budget is pinned to four wavefronts per SIMD.
// this unit keeps the schoolbook product: with the single-addend form ntt_lde_column_kernel<5> measured 17.5 % slower (profiles/mul_wide_notes.txt item 6)
#define GL_MUL_WIDE_CLASSIC
#include <hip/hip_runtime.h>
#include "gl64.hpp"
#include "ntt_pass.hpp"
#include "ntt_kernel_impl.hpp"

namespace {

constexpr int LDE_COL_THREADS = 256;
// LDS words between two k1 rows of an exchange image. 256 + 16: a half-wave of round 2 or 3 covers 16 lanes of one k1 and 16
// of the next, which land on the two halves of the 32 banks.
constexpr int LDE_COL_PITCH = 272;
// words between two k2 rows of the second image: 16 lanes with k2 = 0..15 read banks 17 k2 mod 32, all distinct, and disjoint
// from those of the neighbouring k1 (offset 16).
constexpr int LDE_COL_PITCH2 = 17;

template <int K1>
__global__ void __launch_bounds__(LDE_COL_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4))) ntt_lde_column_kernel(const NttLdeColumnArgs a) {
    constexpr int NA = 1 << K1, D = K1 + 8;
    constexpr int NBLK = NA * 16;                                       // 16-point blocks of rounds 2 and 3
    constexpr int BPT = NBLK >= LDE_COL_THREADS ? NBLK / LDE_COL_THREADS : 1;   // blocks per thread
    constexpr int ACT = NBLK / BPT;                                     // threads that take part in rounds 2 and 3
    __shared__ u32 lds[NA * LDE_COL_PITCH];

    const u32 tid = threadIdx.x;
    const u32 r = a.rate_bits, nc = 1u << r;
    u32 col, k;
    if (a.xcd_map) {
        // consecutive workgroups go to different XCDs: give the cosets of a column the same residue mod 8, so that one L2
        // serves all reads of a column's coefficients (a placement that changes speed only)
        const u32 grp = blockIdx.x / (8u * nc), w = blockIdx.x % (8u * nc);
        col = grp * 8u + (w & 7u);
        k = w >> 3;
    } else {
        col = blockIdx.x >> r;
        k = blockIdx.x & (nc - 1);
    }
    const u64 *in = a.in + (u64)col * a.in_col_stride + (u64)blockIdx.z * a.in_proof_stride;
    const u64 *sc = a.scale + ((u64)k << D);
    u32 kr = 0;                                                          // brev_r(k): the coset's block of the output
    for (u32 i = 0; i < r; i++) kr |= ((k >> i) & 1u) << (r - 1 - i);
    u64 *out = a.out + (u64)col * a.out_col_stride + (u64)blockIdx.z * a.out_proof_stride + ((u64)kr << D);

    // ---- round 1 ----
    u64 x[NA];
#pragma unroll
    for (int i = 0; i < NA; i++) {
        const u32 idx = (u32)i * LDE_COL_THREADS + tid;
        x[i] = gl::mul(in[idx], sc[idx]);
    }
    dif_regs<K1, false>(x);
#pragma unroll
    for (int j = 1; j < NA; j++) x[j] = gl::mul(x[j], a.tw_outer[(u32)j * LDE_COL_THREADS + tid]);

    // ---- exchange 1: element (j1, m) at word j1 * PITCH + m ----
    const u32 lo4 = tid & 15u, hi4 = tid >> 4;
    const bool act = tid < (u32)ACT;
    u64 y[BPT][16];
    {
#pragma unroll
        for (int j = 0; j < NA; j++) lds[(u32)j * LDE_COL_PITCH + tid] = (u32)x[j];
        __syncthreads();
        if (act) {
#pragma unroll
            for (int b = 0; b < BPT; b++)
#pragma unroll
                for (int i = 0; i < 16; i++) y[b][i] = lds[(hi4 + 16u * b) * LDE_COL_PITCH + (u32)i * 16u + lo4];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NA; j++) lds[(u32)j * LDE_COL_PITCH + tid] = (u32)(x[j] >> 32);
        __syncthreads();
        if (act) {
#pragma unroll
            for (int b = 0; b < BPT; b++)
#pragma unroll
                for (int i = 0; i < 16; i++)
                    y[b][i] |= (u64)lds[(hi4 + 16u * b) * LDE_COL_PITCH + (u32)i * 16u + lo4] << 32;
        }
    }

    // ---- round 2: thread (k1 = hi4 + 16 b, n3 = lo4) ----
    if (act) {
#pragma unroll
        for (int b = 0; b < BPT; b++) {
            dif_regs<4, false>(y[b]);
#pragma unroll
            for (int j = 1; j < 16; j++) y[b][j] = gl::mul(y[b][j], a.tw_inner[(u32)j * 16u + lo4]);
        }
    }
    __syncthreads();   // every thread has read the first image

    // ---- exchange 2: element (j1, j2, n3) at word j1 * PITCH + j2 * PITCH2 + n3 ----
    u64 z[BPT][16];
    {
        if (act) {
#pragma unroll
            for (int b = 0; b < BPT; b++)
#pragma unroll
                for (int j = 0; j < 16; j++) lds[(hi4 + 16u * b) * LDE_COL_PITCH + (u32)j * LDE_COL_PITCH2 + lo4] = (u32)y[b][j];
        }
        __syncthreads();
        if (act) {
#pragma unroll
            for (int b = 0; b < BPT; b++)
#pragma unroll
                for (int i = 0; i < 16; i++) z[b][i] = lds[(hi4 + 16u * b) * LDE_COL_PITCH + lo4 * LDE_COL_PITCH2 + (u32)i];
        }
        __syncthreads();
        if (act) {
#pragma unroll
            for (int b = 0; b < BPT; b++)
#pragma unroll
                for (int j = 0; j < 16; j++) lds[(hi4 + 16u * b) * LDE_COL_PITCH + (u32)j * LDE_COL_PITCH2 + lo4] = (u32)(y[b][j] >> 32);
        }
        __syncthreads();
        if (act) {
#pragma unroll
            for (int b = 0; b < BPT; b++)
#pragma unroll
                for (int i = 0; i < 16; i++)
                    z[b][i] |= (u64)lds[(hi4 + 16u * b) * LDE_COL_PITCH + lo4 * LDE_COL_PITCH2 + (u32)i] << 32;
        }
    }

    // ---- round 3: thread (k1 = hi4 + 16 b, k2 = lo4) writes slots j1 * 256 + j2 * 16 + 0..15, 16 bytes at a time ----
    if (act) {
#pragma unroll
        for (int b = 0; b < BPT; b++) {
            dif_regs<4, false>(z[b]);
            ulonglong2 *o = reinterpret_cast<ulonglong2 *>(out + (((hi4 + 16u * b) << 8) | (lo4 << 4)));
#pragma unroll
            for (int j = 0; j < 16; j += 2) o[j >> 1] = make_ulonglong2(gl::canon(z[b][j]), gl::canon(z[b][j + 1]));
        }
    }
}

}  // namespace

hipError_t ntt_lde_column_launch(const NttLdeColumnArgs &a, unsigned log_n_in, uint32_t n_proofs, hipStream_t st) {
    if (a.rate_bits + log_n_in > 23 || a.ncols == 0 || n_proofs == 0 || n_proofs > 65535) return hipErrorInvalidValue;
    if (a.xcd_map && a.ncols % 8) return hipErrorInvalidValue;
    const uint64_t blocks = (uint64_t)a.ncols << a.rate_bits;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    dim3 grid((unsigned)blocks, 1, n_proofs), block(LDE_COL_THREADS, 1, 1);
    switch (log_n_in) {
        case 11: hipLaunchKernelGGL((ntt_lde_column_kernel<3>), grid, block, 0, st, a); break;
        case 12: hipLaunchKernelGGL((ntt_lde_column_kernel<4>), grid, block, 0, st, a); break;
        case 13: hipLaunchKernelGGL((ntt_lde_column_kernel<5>), grid, block, 0, st, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
