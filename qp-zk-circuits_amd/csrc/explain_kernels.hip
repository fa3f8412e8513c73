// explain_kernels.hip — the kernels qpgpu_circuit_explain_witness (explain_api.cpp) adds around the gate kernels of the witness
// check, for gfx950, 256-thread blocks, one thread per item, every index checked against its bound:
//   explain_failing_rows_kernel     bitmap of the trace rows whose weighted gate sums are not all zero
//   explain_gather_rows_kernel      the chosen rows' columns into a compact trace [cols][stride]
//   explain_one_hot_kernel          the weight table whose column c is the indicator of one constraint
//   explain_copy_kernel             bitmap of the routed cells that differ from their copy class's source cell
//   explain_fetch_cells_kernel      the two values and the source of each reported cell
// None of them evaluates a gate. The bitmaps are set with atomicOr on 32-bit words (a vector atomic): which bits end up set does
// not depend on the order the threads run in, so the findings are the same on every run.
#include <hip/hip_runtime.h>
#include "explain_kernels.hpp"
#include "gl64.hpp"

using gl::u32;
using gl::u64;

namespace {

__global__ void __launch_bounds__(256) explain_failing_rows_kernel(const u64 *acc, u64 n, u32 nch, u32 *bitmap) {
    const u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (i >= n) return;
    bool bad = false;
    for (u32 c = 0; c < nch; c++) bad |= gl::canon(acc[(u64)c * n + i]) != 0;
    if (bad) atomicOr(&bitmap[i >> 5], 1u << (i & 31));
}

__global__ void __launch_bounds__(256) explain_gather_rows_kernel(const u64 *src, u64 n, u32 cols, const u32 *rows, u32 count, u32 stride, u64 *dst) {
    const u32 k = blockIdx.x * blockDim.x + threadIdx.x, col = blockIdx.y;
    if (k >= stride || col >= cols) return;
    u64 v = 0;
    if (k < count) {
        const u64 r = rows[k];
        if (r < n) v = src[(u64)col * n + r];
    }
    dst[(u64)col * stride + k] = v;
}

__global__ void __launch_bounds__(256) explain_one_hot_kernel(u64 *table, u32 nch, u32 nterms, u32 t0, u32 k0, u32 num_constraints) {
    const u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (i >= (u64)nch * nterms) return;
    const u32 c = (u32)(i / nterms), t = (u32)(i % nterms);
    const u64 k = (u64)k0 + c;
    table[i] = (k < num_constraints && (u64)t == (u64)t0 + k) ? 1 : 0;
}

__global__ void __launch_bounds__(256) explain_copy_kernel(const u64 *wires, const u32 *src_of, u64 n, u32 num_routed, u32 *bitmap) {
    const u64 cell = blockIdx.x * (u64)blockDim.x + threadIdx.x;      // row * num_routed + wire
    if (cell >= n * num_routed) return;
    const u64 row = cell / num_routed, wire = cell % num_routed;
    const u64 src = src_of[cell];
    if (src >= n * num_routed) return;                                // (a source is a routed cell: nothing else is read)
    if (gl::canon(wires[wire * n + row]) != gl::canon(wires[src])) atomicOr(&bitmap[cell >> 5], 1u << (cell & 31));
}

__global__ void __launch_bounds__(256) explain_fetch_cells_kernel(const u64 *wires, const u32 *src_of, u64 n, u32 num_routed, const u64 *cells, u32 count, u64 *out) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const u64 cell = cells[i];
    u64 own = 0, other = 0, src = 0;
    if (cell < n * num_routed) {
        src = src_of[cell];
        own = gl::canon(wires[(cell % num_routed) * n + cell / num_routed]);
        if (src < n * num_routed) other = gl::canon(wires[src]);
    }
    out[3 * (u64)i] = own; out[3 * (u64)i + 1] = other; out[3 * (u64)i + 2] = src;
}

unsigned blocks_for(u64 items) { return (unsigned)((items + 255) / 256); }

}  // namespace

hipError_t ek_failing_rows(const u64 *acc, u64 n, u32 nch, u32 *bitmap, hipStream_t st) {
    if (n == 0) return hipSuccess;
    if (n > (1ull << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(explain_failing_rows_kernel, dim3(blocks_for(n)), dim3(256), 0, st, acc, n, nch, bitmap);
    return hipGetLastError();
}

hipError_t ek_gather_rows(const u64 *src, u64 n, u32 cols, const u32 *rows, u32 count, u32 stride, u64 *dst, hipStream_t st) {
    if (cols == 0 || stride == 0) return hipSuccess;
    if (count > stride || cols > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(explain_gather_rows_kernel, dim3(blocks_for(stride), cols), dim3(256), 0, st, src, n, cols, rows, count, stride, dst);
    return hipGetLastError();
}

hipError_t ek_one_hot(u64 *table, u32 nch, u32 nterms, u32 t0, u32 k0, u32 num_constraints, hipStream_t st) {
    if (nch == 0 || nterms == 0) return hipSuccess;
    hipLaunchKernelGGL(explain_one_hot_kernel, dim3(blocks_for((u64)nch * nterms)), dim3(256), 0, st, table, nch, nterms, t0, k0, num_constraints);
    return hipGetLastError();
}

hipError_t ek_copy_mismatches(const u64 *wires, const u32 *src_of, u64 n, u32 num_routed, u32 *bitmap, hipStream_t st) {
    const u64 cells = n * num_routed;
    if (cells == 0) return hipSuccess;
    if (cells >= (1ull << 32)) return hipErrorInvalidValue;           // src_of holds 32-bit cells (witness_plan.cpp refuses larger circuits)
    hipLaunchKernelGGL(explain_copy_kernel, dim3(blocks_for(cells)), dim3(256), 0, st, wires, src_of, n, num_routed, bitmap);
    return hipGetLastError();
}

hipError_t ek_fetch_cells(const u64 *wires, const u32 *src_of, u64 n, u32 num_routed, const u64 *cells, u32 count, u64 *out, hipStream_t st) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(explain_fetch_cells_kernel, dim3(blocks_for(count)), dim3(256), 0, st, wires, src_of, n, num_routed, cells, count, out);
    return hipGetLastError();
}
