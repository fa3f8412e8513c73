// explain_api.cpp — qpgpu_circuit_explain_witness and qpgpu_witness_finding_format (include/qpgpu.h): which gate constraints and
// which copy constraints an unsatisfied witness violates, and where.
//
// There is ONE statement of the gates: the kernels that judge a witness in the witness check (pk_gate_sums on value arrays, the
// hash gates' weights from pk_quotient_fold_sweep when the circuit runs them folded, exactly as stage_quotient_prepare does).
// This file only chooses the weights those kernels multiply the constraints with:
//   (a) detection: one pass over the whole trace under a FIXED weight table (explain_select.hpp: column c = the powers of a
//       constant from a SplitMix64 stream with a fixed seed), then explain_failing_rows_kernel marks the rows with a non-zero sum.
//       The table depends on no transcript, so the call needs none. A row whose constraints are not all zero is missed only if
//       its constraint vector, read as a polynomial of degree < num_gate_constraints, vanishes at every column's constant: for a
//       witness that was not built against these constants at most num_gate_constraints / p < 2^-56 per column, columns
//       multiplying. (The witness check itself uses the transcript's alphas and is what decides QPGPU_EUNSAT.)
//   (b) gather: the first max_rows failing rows' wire, selector and constant columns into a compact trace. Gates are row-local,
//       so the compact trace is a valid input of the gate kernels.
//   (c) expansion: ceil(num_gate_constraints / num_challenges) passes of the same gate kernels over the compact trace, column c
//       of the weight table being the indicator of constraint k0 + c: the sums ARE the filtered constraint values. The hash gates
//       run in the form the circuit runs them in (folded unless QPGPU_QUOTIENT_FOLD=0 at load): the fold is linear in the weights
//       (tools/host_checks/explain_one_hot_check.cpp compares one-hot folds with the round-by-round constraints, exactly).
//   (d) copy constraints: every routed cell against the source cell of its copy class (the witness plan's src_of).
// Ordered results come from bitmaps read in ascending order on the host, never from "first thread wins".
//
// Everything allocated here is registered with the residue registry and is overwritten and released before the call returns,
// on every exit path (Work's destructor).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "circuit_state.hpp"
#include "explain_kernels.hpp"
#include "explain_select.hpp"
#include "poseidon.hpp"
#include "quotient_kernels.hpp"
#include "witness.hpp"

using gl::u64;

namespace {

// the buffers of one call: device and pinned memory of the circuit-workspace region, zeroed when taken, overwritten and freed
// when the call ends
struct Work {
    qpgpu_ctx *ctx;
    std::vector<std::pair<void *, size_t>> dev;
    void *pin = nullptr;
    static constexpr size_t PIN_BYTES = 1u << 20;
    explicit Work(qpgpu_ctx *c) : ctx(c) {}
    Work(const Work &) = delete;
    Work &operator=(const Work &) = delete;
    ~Work() {
        for (auto &d : dev) (void)hipMemsetAsync(d.first, 0, d.second, ctx->stream);
        (void)hipStreamSynchronize(ctx->stream);
        if (pin) std::memset(pin, 0, PIN_BYTES);
        for (auto &d : dev) ctx->track_free(d.first);
        ctx->track_free(pin);
    }
    template <class T> int take(T **p, size_t count) {
        void *v = nullptr;
        const size_t bytes = std::max<size_t>(count * sizeof(T), 8);
        const hipError_t e = ctx->track_malloc(&v, bytes, residue::CIRCUIT_WORKSPACE);
        if (e == hipErrorOutOfMemory) return ctx->fail(QPGPU_ENOMEM, "explain_witness: out of device memory");
        if (e != hipSuccess) return ctx->hip_fail(e, "hipMalloc(explain_witness)");
        dev.push_back({v, bytes});
        QP_HIP(ctx, hipMemsetAsync(v, 0, bytes, ctx->stream));
        *p = (T *)v;
        return QPGPU_OK;
    }
    // device -> host through the call's own pinned buffer, a piece at a time (a copy kernel writes it in place, as qpgpu_ctx::read_back does)
    int read(void *dst, const void *src, size_t bytes) {
        if (!pin) {
            const hipError_t e = ctx->track_host_malloc(&pin, PIN_BYTES, residue::CIRCUIT_WORKSPACE);
            if (e != hipSuccess) { pin = nullptr; return ctx->hip_fail(e, "hipHostMalloc(explain_witness)"); }
        }
        for (size_t off = 0; off < bytes; off += PIN_BYTES) {
            const size_t len = std::min(PIN_BYTES, bytes - off);
            QP_HIP(ctx, pk_copy(pin, (const char *)src + off, len, ctx->stream));
            QP_HIP(ctx, hipStreamSynchronize(ctx->stream));
            std::memcpy((char *)dst + off, pin, len);
        }
        return QPGPU_OK;
    }
};

void wipe(std::vector<u64> &v) {
    volatile u64 *z = v.data();
    for (size_t i = 0; i < v.size(); i++) z[i] = 0;
}

// the gate a trace row selects: the one whose filter does not vanish there (0xFFFFFFFF: none, which a loaded pack does not have)
uint32_t gate_of_row(const CircuitPack &p, u64 row) {
    const u64 n = p.n();
    for (size_t gi = 0; gi < p.gates.size(); gi++)
        if (p.constants_sigmas[p.gates[gi].selector_index * n + row] == gi) return (uint32_t)gi;
    return 0xFFFFFFFFu;
}

int explain_run(qpgpu_circuit *c, Work &w, const u64 *wires, bool on_device, const u64 *public_inputs, uint32_t max_rows,
            qpgpu_witness_finding *out, size_t cap, size_t *count, u64 *failing_rows, u64 *copy_mismatches) {
    qpgpu_ctx *ctx = c->ctx;
    const CircuitPack &p = c->pack;
    const StageTables &t = c->tab;
    hipStream_t st = ctx->stream;
    const u64 n = p.n(), NW = p.num_wires, R = p.num_routed_wires;
    const uint32_t nch = (uint32_t)p.num_challenges, nchunks = (uint32_t)p.num_chunks(), C = (uint32_t)p.num_gate_constraints;
    const uint32_t t0 = nch + nch * nchunks, nterms = t0 + C;
    const uint32_t nsc = (uint32_t)(p.num_selectors + p.num_constants);
    size_t written = 0;

    const u64 *d_wires = wires;
    if (!on_device) {
        u64 *up = nullptr;
        QP_TRY(w.take(&up, NW * n));
        QP_TRY(h2d_sync(ctx, up, wires, NW * n * 8));
        d_wires = up;
    }

    // ---- (a) detection ----
    u64 *d_small = nullptr, *d_fold = nullptr, *d_acc = nullptr;
    uint32_t *d_bitmap = nullptr;
    QP_TRY(w.take(&d_small, (size_t)nch * nterms + 4));
    if (t.fold_words) QP_TRY(w.take(&d_fold, t.fold_words));
    QP_TRY(w.take(&d_acc, (size_t)nch * n));
    QP_TRY(w.take(&d_bitmap, explain::bitmap_words(n)));
    {
        std::vector<u64> tab((size_t)nch * nterms + 4);
        for (uint32_t k = 0; k < nch; k++) {
            const u64 base = explain::detect_constant(k);
            u64 a = 1;
            for (uint32_t i = 0; i < nterms; i++) { tab[(size_t)k * nterms + i] = gl::canon(a); a = gl::mul(a, base); }
        }
        hasher::hash_no_pad(ctx->hasher, public_inputs, p.num_public_inputs, tab.data() + (size_t)nch * nterms);
        QP_TRY(h2d_sync(ctx, d_small, tab.data(), tab.size() * 8));
    }
    QuotientArgs ta{};       // as stage_quotient_prepare builds it for the witness check, one proof
    ta.wires = d_wires; ta.cs = t.cs_values; ta.alpha_pows = d_small; ta.pi_hash = d_small + (size_t)nch * nterms; ta.gates = t.d_gates;
    ta.acc = d_acc; ta.out = d_acc; ta.poseidon_rc = t.d_poseidon_rc; ta.p2_gate = ctx->d_p2_app; ta.p2_layout = p.p2_layout;
    ta.zh_inv = t.d_zh_inv; ta.lde_n = n; ta.q_n = n; ta.q_shift = 0; ta.log_lde = (uint32_t)p.degree_bits; ta.rate = 1; ta.nch = nch;
    ta.num_routed = (uint32_t)R; ta.chunk = (uint32_t)p.quotient_degree_factor; ta.nchunks = nchunks; ta.sig0 = nsc;
    ta.num_selectors = (uint32_t)p.num_selectors; ta.num_gates = (uint32_t)p.gates.size(); ta.nterms = nterms;
    ta.batch = 1; ta.ps_wires = NW * n; ta.ps_zs = 0; ta.ps_small = (u64)nch * nterms + 4; ta.ps_acc = (u64)nch * n; ta.ps_out = (u64)nch * n;
    ta.fold = d_fold; ta.ps_fold = t.fold_words; ta.pair = t.quotient_pair ? 1 : 0;
    QP_HIP(ctx, pk_quotient_fold_sweep(ta, t.h_gates.data(), st));
    QP_HIP(ctx, pk_gate_sums(ta, t.h_gates.data(), st));
    QP_HIP(ctx, ek_failing_rows(d_acc, n, nch, d_bitmap, st));
    std::vector<uint32_t> bitmap(explain::bitmap_words(n));
    QP_TRY(w.read(bitmap.data(), d_bitmap, bitmap.size() * 4));
    std::vector<u64> rows(max_rows);
    u64 n_failing = 0;
    const uint32_t K = (uint32_t)explain::select_first(bitmap.data(), n, max_rows, rows.data(), &n_failing);
    if (failing_rows) *failing_rows = n_failing;

    // ---- (b) gather, (c) expansion ----
    if (K > 0) {
        const uint32_t S = (K + 63) & ~63u;               // column stride of the compact trace
        const uint32_t passes = (C + nch - 1) / nch;
        std::vector<uint32_t> rows32(K);
        for (uint32_t k = 0; k < K; k++) rows32[k] = (uint32_t)rows[k];
        uint32_t *d_rows = nullptr;
        u64 *d_cw = nullptr, *d_ccs = nullptr, *d_vals = nullptr;
        QP_TRY(w.take(&d_rows, K));
        QP_TRY(w.take(&d_cw, (size_t)NW * S));
        QP_TRY(w.take(&d_ccs, (size_t)std::max<uint32_t>(nsc, 1) * S));
        QP_TRY(w.take(&d_vals, (size_t)passes * nch * S));
        QP_TRY(h2d_sync(ctx, d_rows, rows32.data(), (size_t)K * 4));
        QP_HIP(ctx, ek_gather_rows(d_wires, n, (uint32_t)NW, d_rows, K, S, d_cw, st));
        QP_HIP(ctx, ek_gather_rows(t.cs_values, n, nsc, d_rows, K, S, d_ccs, st));
        QuotientArgs te = ta;
        te.wires = d_cw; te.cs = d_ccs; te.lde_n = S; te.q_n = K; te.ps_wires = NW * S; te.ps_acc = (u64)nch * S; te.ps_out = (u64)nch * S;
        for (uint32_t pass = 0; pass < passes; pass++) {
            const uint32_t k0 = pass * nch;
            QP_HIP(ctx, ek_one_hot(d_small, nch, nterms, t0, k0, C, st));
            QP_HIP(ctx, pk_quotient_fold_sweep(te, t.h_gates.data(), st));
            te.acc = d_vals + (size_t)k0 * S; te.out = te.acc;
            QP_HIP(ctx, pk_gate_sums(te, t.h_gates.data(), st));
        }
        std::vector<u64> vals((size_t)C * S);
        const int rc = w.read(vals.data(), d_vals, vals.size() * 8);
        if (rc == QPGPU_OK)
            for (uint32_t k = 0; k < K && written < cap; k++) {
                const uint32_t gate = gate_of_row(p, rows[k]);
                for (uint32_t q = 0; q < C && written < cap; q++) {
                    const u64 v = gl::canon(vals[(size_t)q * S + k]);
                    if (v == 0) continue;
                    qpgpu_witness_finding f{};
                    f.kind = QPGPU_FINDING_GATE; f.gate = gate; f.constraint = q; f.row = rows[k]; f.value = v;
                    out[written++] = f;
                }
            }
        wipe(vals);
        QP_TRY(rc);
    }

    // ---- (d) copy constraints ----
    if (R > 0) {
        const uint32_t *d_src_of = nullptr;
        QP_TRY(witness_plan_src_of(c, &d_src_of));
        const u64 cells = n * R;
        uint32_t *d_cbits = nullptr;
        QP_TRY(w.take(&d_cbits, explain::bitmap_words(cells)));
        QP_HIP(ctx, ek_copy_mismatches(d_wires, d_src_of, n, (uint32_t)R, d_cbits, st));
        std::vector<uint32_t> cbits(explain::bitmap_words(cells));
        QP_TRY(w.read(cbits.data(), d_cbits, cbits.size() * 4));
        u64 total = 0;
        (void)explain::select_first(cbits.data(), cells, 0, nullptr, &total);
        if (copy_mismatches) *copy_mismatches = total;
        const size_t m = (size_t)std::min<u64>(total, cap - written);
        if (m > 0) {
            std::vector<u64> list(m), got(3 * m);
            (void)explain::select_first(cbits.data(), cells, m, list.data(), nullptr);
            u64 *d_list = nullptr, *d_got = nullptr;
            QP_TRY(w.take(&d_list, m));
            QP_TRY(w.take(&d_got, 3 * m));
            QP_TRY(h2d_sync(ctx, d_list, list.data(), m * 8));
            QP_HIP(ctx, ek_fetch_cells(d_wires, d_src_of, n, (uint32_t)R, d_list, (uint32_t)m, d_got, st));
            const int rc = w.read(got.data(), d_got, got.size() * 8);
            if (rc == QPGPU_OK)
                for (size_t i = 0; i < m; i++) {
                    qpgpu_witness_finding f{};
                    f.kind = QPGPU_FINDING_COPY;
                    f.row = list[i] / R; f.wire = (uint32_t)(list[i] % R);
                    f.row_b = got[3 * i + 2] % n; f.wire_b = (uint32_t)(got[3 * i + 2] / n);
                    f.value = got[3 * i]; f.value_b = got[3 * i + 1];
                    out[written++] = f;
                }
            wipe(got);
            QP_TRY(rc);
        }
    }
    *count = written;
    return QPGPU_OK;
}

// tools/pack_dump.py's names, by QPCP gate type code
const char *const GATE_NAMES[] = {"Noop", "Constant", "PublicInput", "Arithmetic", "Poseidon", "BaseSum", "ArithmeticExtension", "MulExtension", "Reducing",
                                  "ReducingExtension", "RandomAccess", "Exponentiation", "PoseidonMds", "CosetInterpolation", "Poseidon2"};

}  // namespace

extern "C" {

int qpgpu_circuit_explain_witness(qpgpu_circuit *c, const uint64_t *wires, int wires_on_device, const uint64_t *public_inputs, uint32_t max_rows,
                                  unsigned flags, qpgpu_witness_finding *out, size_t cap, size_t *count, uint64_t *failing_rows, uint64_t *copy_mismatches) {
    if (!c) return QPGPU_EINVAL;
    qpgpu_ctx *ctx = c->ctx;
    QP_DEV(ctx);
    if (count) *count = 0;
    if (failing_rows) *failing_rows = 0;
    if (copy_mismatches) *copy_mismatches = 0;
    if (!wires || !count || (cap && !out) || (!public_inputs && c->pack.num_public_inputs)) return ctx->fail(QPGPU_EINVAL, "explain_witness: null argument");
    if (max_rows == 0 || max_rows > 1024) return ctx->fail(QPGPU_EINVAL, "explain_witness: max_rows must be 1..1024");
    if (flags != 0) return ctx->fail(QPGPU_EINVAL, "explain_witness: flags must be 0");
    int rc;
    std::string keep;
    {
        Work w(ctx);
        rc = explain_run(c, w, wires, wires_on_device != 0, public_inputs, max_rows, out, cap, count, failing_rows, copy_mismatches);
        keep = ctx->err;
    }   // the buffers are overwritten and released here, whatever rc is
    ctx->err = keep;
    return rc;
}

int qpgpu_witness_finding_format(const uint64_t *pack_words, size_t n_words, const qpgpu_witness_finding *f, char *buf, size_t cap) {
    if (!pack_words || !f || !buf || cap == 0) return QPGPU_EINVAL;
    buf[0] = 0;
    CircuitPack p;
    if (!p.parse_stage(pack_words, n_words).empty()) return QPGPU_EINVAL;
    int len;
    if (f->kind == QPGPU_FINDING_GATE) {
        if (f->gate >= p.gates.size() || f->row >= p.n()) return QPGPU_EINVAL;
        const GateInfo &g = p.gates[f->gate];
        if (f->constraint >= g.num_constraints) return QPGPU_EINVAL;
        const char *name = g.type < sizeof(GATE_NAMES) / sizeof(GATE_NAMES[0]) ? GATE_NAMES[g.type] : "?";
        len = std::snprintf(buf, cap, "gate constraint fails at row %llu: gate %u (%s), constraint %u of %llu, filtered value %llu",
                            (unsigned long long)f->row, f->gate, name, f->constraint, (unsigned long long)g.num_constraints, (unsigned long long)f->value);
    } else if (f->kind == QPGPU_FINDING_COPY) {
        if (f->wire >= p.num_routed_wires || f->wire_b >= p.num_routed_wires || f->row >= p.n() || f->row_b >= p.n()) return QPGPU_EINVAL;
        len = std::snprintf(buf, cap, "copy constraint violated: wire %u of row %llu holds %llu, the source of its copy class, wire %u of row %llu, holds %llu",
                            f->wire, (unsigned long long)f->row, (unsigned long long)f->value, f->wire_b, (unsigned long long)f->row_b, (unsigned long long)f->value_b);
    } else {
        return QPGPU_EINVAL;
    }
    return len >= 0 && (size_t)len < cap ? QPGPU_OK : QPGPU_EBUFSIZE;
}

}  // extern "C"
