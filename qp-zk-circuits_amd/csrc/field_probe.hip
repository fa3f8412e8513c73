// field_probe.hip — test hook: every primitive of gl64.hpp (and the NTT's register transforms) on caller-chosen operands.
//
// The kernels reach the field code with pseudo-random data, on which the second borrow of sub, the borrow and the carry of
// reduce128 or the fold branch of mul_group fire about once in 2^32 operations. qpgpu_field_probe runs ONE primitive per launch,
// one thread per index, on operands the caller chose to force those branches, and returns the raw 64-bit results (not
// canonicalised here), so that a test can compare them with plain integer arithmetic modulo p. The same operation table runs
// through the host versions of gl64.hpp with on_device = 0.
//
// What this proves: each primitive's contract, for every branch, in this unit's compile context. Inline assembly inlined into
// another kernel gets another register allocation; the bit-exact kernel parity tests stay the check on that.
#include <hip/hip_runtime.h>
#include <vector>
#include "ctx.hpp"
#include "gl64.hpp"
#include "ntt_kernel_impl.hpp"

namespace {

// words per thread read from a and from b (0: b is not read) and written to out; false for a bad op / param
struct ProbeShape { unsigned wa, wb, wo; };

bool probe_shape(unsigned op, unsigned param, bool on_device, ProbeShape &s) {
    switch (op) {
        case QPGPU_FP_CANON: case QPGPU_FP_NEG: case QPGPU_FP_SQR: case QPGPU_FP_MUL_EPS: case QPGPU_FP_MUL7: case QPGPU_FP_INV:
            s = {1, 0, 1}; return true;
        case QPGPU_FP_ADD: case QPGPU_FP_SUB: case QPGPU_FP_MUL: case QPGPU_FP_REDUCE128: case QPGPU_FP_REDUCE96:
        case QPGPU_FP_ADD_CANONICAL: case QPGPU_FP_POW:
            s = {1, 1, 1}; return true;
        case QPGPU_FP_MUL_POW2: s = {1, 0, 1}; return param < 192;
        case QPGPU_FP_MUL_POW2_DYN: s = {1, 0, 1}; return param < 96;
        case QPGPU_FP_MUL_GROUP: s = {param, param, param}; return param == 1 || param == 2 || param == 12;
        case QPGPU_FP_ACC: s = {param, param, 1}; return param >= 1 && param <= 4096;
        case QPGPU_FP_E2_ADD: case QPGPU_FP_E2_SUB: case QPGPU_FP_E2_MUL: s = {2, 2, 2}; return true;
        case QPGPU_FP_E2_SCALE: case QPGPU_FP_E2_POW: s = {2, 1, 2}; return true;
        case QPGPU_FP_E2_INV: s = {2, 0, 2}; return true;
        case QPGPU_FP_DIF_REGS: {
            const unsigned k = param & 0xFF;
            s = {1u << (k & 7), 0, 1u << (k & 7)};
            return on_device && k >= 1 && k <= 6 && (param >> 8) <= 1;
        }
        case QPGPU_FP_DIF_SPARSE: {
            // the instances of the LDE pass kernels (lde_sparse_lv in ntt_kernel_impl.hpp): forward, (K, LV) = (4, 1) and (5, 2)
            const unsigned k = param & 0xFF, inv = (param >> 8) & 0xFF, lv = param >> 16;
            s = {1u << (k & 7), 0, 1u << (k & 7)};
            return on_device && inv == 0 && ((k == 4 && lv == 1) || (k == 5 && lv == 2));
        }
        default: return false;
    }
}

template <int S>
GL_HD u64 pow2_arm(u64 x, unsigned s) {
    if constexpr (S >= 192) return 0;
    else return s == (unsigned)S ? gl::mul_pow2<S>(x) : pow2_arm<S + 1>(x, s);
}
// mul_pow2_dyn as the register transforms call it: the shift is a constant at every call site
template <int S>
GL_HD u64 pow2_dyn_arm(u64 x, unsigned s) {
    if constexpr (S >= 96) return 0;
    else return s == (unsigned)S ? mul_pow2_dyn(x, S) : pow2_dyn_arm<S + 1>(x, s);
}

template <int N>
GL_HD void group_case(const u64 *a, const u64 *b, u64 *out) {
    u64 x[N], y[N], r[N];
    for (int k = 0; k < N; k++) { x[k] = a[k]; y[k] = b[k]; }
    gl::mul_group(r, x, y);
    for (int k = 0; k < N; k++) out[k] = r[k];
}

#if defined(__HIP_DEVICE_COMPILE__)
template <int K, bool INV>
__device__ __forceinline__ void dif_case(const u64 *a, u64 *out) {
    u64 x[1 << K];
#pragma unroll
    for (int j = 0; j < (1 << K); j++) x[j] = a[j];
    dif_regs<K, INV>(x);
#pragma unroll
    for (int j = 0; j < (1 << K); j++) out[j] = x[j];
}
template <int K, int LV>
__device__ __forceinline__ void sparse_case(const u64 *a, u64 *out) {
    u64 x[1 << K];
#pragma unroll
    for (int j = 0; j < (1 << K); j++) x[j] = a[j];
    dif_sparse<K, false, LV>(x);
#pragma unroll
    for (int j = 0; j < (1 << K); j++) out[j] = x[j];
}
template <int K>
__device__ __forceinline__ void dif_dispatch(unsigned k, bool inv, const u64 *a, u64 *out) {
    if constexpr (K <= 6) {
        if (k == (unsigned)K) { if (inv) dif_case<K, true>(a, out); else dif_case<K, false>(a, out); }
        else dif_dispatch<K + 1>(k, inv, a, out);
    }
}
#endif

// one index of one operation: a, b and out point at this index's words
template <unsigned OP>
GL_HD void probe_eval(unsigned param, const u64 *a, const u64 *b, u64 *out) {
    if constexpr (OP == QPGPU_FP_CANON) out[0] = gl::canon(a[0]);
    else if constexpr (OP == QPGPU_FP_ADD) out[0] = gl::add(a[0], b[0]);
    else if constexpr (OP == QPGPU_FP_SUB) out[0] = gl::sub(a[0], b[0]);
    else if constexpr (OP == QPGPU_FP_NEG) out[0] = gl::neg(a[0]);
    else if constexpr (OP == QPGPU_FP_MUL) out[0] = gl::mul(a[0], b[0]);
    else if constexpr (OP == QPGPU_FP_SQR) out[0] = gl::sqr(a[0]);
    else if constexpr (OP == QPGPU_FP_REDUCE128) out[0] = gl::reduce128(a[0], b[0]);
    else if constexpr (OP == QPGPU_FP_REDUCE96) out[0] = gl::reduce96(a[0], (u32)b[0]);
    else if constexpr (OP == QPGPU_FP_MUL_EPS) out[0] = gl::mul_eps((u32)a[0]);
    else if constexpr (OP == QPGPU_FP_ADD_CANONICAL) out[0] = gl::add_canonical(a[0], b[0]);
    else if constexpr (OP == QPGPU_FP_MUL7) out[0] = gl::mul7(a[0]);
    else if constexpr (OP == QPGPU_FP_INV) out[0] = gl::inv(a[0]);
    else if constexpr (OP == QPGPU_FP_POW) out[0] = gl::pow(a[0], b[0]);
    else if constexpr (OP == QPGPU_FP_MUL_POW2) out[0] = pow2_arm<0>(a[0], param);
    else if constexpr (OP == QPGPU_FP_MUL_POW2_DYN) out[0] = pow2_dyn_arm<0>(a[0], param);
    else if constexpr (OP == QPGPU_FP_MUL_GROUP) {
        if (param == 1) group_case<1>(a, b, out);
        else if (param == 2) group_case<2>(a, b, out);
        else group_case<12>(a, b, out);
    } else if constexpr (OP == QPGPU_FP_ACC) {
        gl::Acc192 acc = gl::acc_zero();
        for (unsigned t = 0; t < param; t++) gl::acc_mul(acc, a[t], b[t]);
        out[0] = gl::acc_reduce(acc);
    } else if constexpr (OP == QPGPU_FP_E2_ADD || OP == QPGPU_FP_E2_SUB || OP == QPGPU_FP_E2_MUL) {
        const gl::e2 x = gl::e2_make(a[0], a[1]), y = gl::e2_make(b[0], b[1]);
        const gl::e2 r = OP == QPGPU_FP_E2_ADD ? gl::e2_add(x, y) : OP == QPGPU_FP_E2_SUB ? gl::e2_sub(x, y) : gl::e2_mul(x, y);
        out[0] = r.a; out[1] = r.b;
    } else if constexpr (OP == QPGPU_FP_E2_SCALE || OP == QPGPU_FP_E2_POW) {
        const gl::e2 x = gl::e2_make(a[0], a[1]);
        const gl::e2 r = OP == QPGPU_FP_E2_SCALE ? gl::e2_scale(x, b[0]) : gl::e2_pow(x, b[0]);
        out[0] = r.a; out[1] = r.b;
    } else if constexpr (OP == QPGPU_FP_E2_INV) {
        const gl::e2 r = gl::e2_inv(gl::e2_make(a[0], a[1]));
        out[0] = r.a; out[1] = r.b;
    }
#if defined(__HIP_DEVICE_COMPILE__)
    else if constexpr (OP == QPGPU_FP_DIF_REGS) dif_dispatch<1>(param & 0xFF, (param >> 8) != 0, a, out);
    else if constexpr (OP == QPGPU_FP_DIF_SPARSE) {
        if ((param & 0xFF) == 4) sparse_case<4, 1>(a, out);
        else sparse_case<5, 2>(a, out);
    }
#endif
}

// one thread per index; consecutive indices are consecutive lanes of a wave (mul_group's branch is per wave)
template <unsigned OP>
__global__ void __launch_bounds__(256) field_probe_kernel(unsigned param, ProbeShape s, const u64 *a, const u64 *b, size_t n, u64 *out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    probe_eval<OP>(param, a + i * s.wa, b + i * s.wb, out + i * s.wo);
}

template <unsigned OP>
void probe_host(unsigned param, ProbeShape s, const u64 *a, const u64 *b, size_t n, u64 *out) {
    for (size_t i = 0; i < n; i++) probe_eval<OP>(param, a + i * s.wa, b ? b + i * s.wb : nullptr, out + i * s.wo);
}

template <unsigned OP>
hipError_t probe_launch(unsigned param, ProbeShape s, const u64 *a, const u64 *b, size_t n, u64 *out, hipStream_t st) {
    hipLaunchKernelGGL((field_probe_kernel<OP>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, param, s, a, b, n, out);
    return hipGetLastError();
}

// OP is a template argument everywhere: one table from the run-time op to the instance
template <unsigned OP>
int probe_run(unsigned op, bool dev, unsigned param, ProbeShape s, const u64 *a, const u64 *b, size_t n, u64 *out, hipStream_t st, hipError_t &he) {
    if constexpr (OP >= QPGPU_FP_OP_COUNT) return QPGPU_EINVAL;
    else {
        if (op != OP) return probe_run<OP + 1>(op, dev, param, s, a, b, n, out, st, he);
        if (dev) he = probe_launch<OP>(param, s, a, b, n, out, st);
        else if constexpr (OP != QPGPU_FP_DIF_REGS && OP != QPGPU_FP_DIF_SPARSE) probe_host<OP>(param, s, a, b, n, out);
        return QPGPU_OK;
    }
}

}  // namespace

extern "C" int qpgpu_field_probe(qpgpu_ctx *ctx, unsigned op, unsigned param, const uint64_t *a, const uint64_t *b, size_t n,
                                 uint64_t *out, size_t out_words, int on_device) {
    ProbeShape s;
    if (!probe_shape(op, param, on_device != 0, s)) return QPGPU_EINVAL;
    if (!a || !out || (s.wb && !b) || n == 0 || n > ((size_t)1 << 24) || out_words < n * s.wo) return QPGPU_EINVAL;
    if (on_device && !ctx) return QPGPU_EINVAL;
    // operand preconditions of the primitives themselves: a 32-bit word where the signature takes one, a canonical addend
    for (size_t i = 0; i < n; i++) {
        if ((op == QPGPU_FP_REDUCE96 && (b[i] >> 32)) || (op == QPGPU_FP_MUL_EPS && (a[i] >> 32)) ||
            (op == QPGPU_FP_ADD_CANONICAL && b[i] >= gl::P))
            return QPGPU_EINVAL;
    }
    hipError_t he = hipSuccess;
    if (!on_device) return probe_run<0>(op, false, param, s, a, b, n, out, nullptr, he);

    QP_DEV(ctx);
    const size_t na = n * s.wa, nb = n * s.wb, no = n * s.wo;
    uint64_t *d = nullptr;
    QP_HIP(ctx, hipMalloc((void **)&d, (na + nb + no) * 8));
    uint64_t *d_a = d, *d_b = d + na, *d_o = d + na + nb;
    int rc = QPGPU_OK;
    he = hipMemcpyAsync(d_a, a, na * 8, hipMemcpyHostToDevice, ctx->stream);
    if (he == hipSuccess && nb) he = hipMemcpyAsync(d_b, b, nb * 8, hipMemcpyHostToDevice, ctx->stream);
    if (he == hipSuccess) he = hipMemsetAsync(d_o, 0, no * 8, ctx->stream);
    if (he == hipSuccess) rc = probe_run<0>(op, true, param, s, d_a, d_b, n, d_o, ctx->stream, he);
    if (he == hipSuccess && rc == QPGPU_OK) he = hipMemcpyAsync(out, d_o, no * 8, hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t hs = hipStreamSynchronize(ctx->stream);
    if (he == hipSuccess) he = hs;
    (void)hipFree(d);
    if (he != hipSuccess) return ctx->hip_fail(he, "qpgpu_field_probe");
    return rc;
}
