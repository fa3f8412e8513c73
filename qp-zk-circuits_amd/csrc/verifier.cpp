// verifier.cpp — host-side proof verification over a circuit pack (include/qpgpu_verify.h): qp-plonky2's
// `VerifierCircuitData::verify` as the reference applies it at every hand-over of a proof (leaf proofs entering a private
// batch, private-batch proofs entering a public batch, self-verification after proving). Pure host code: extension-field
// arithmetic from gl64.hpp, the context-independent hasher, the pack parser. The gate constraints are the verifier-side
// (extension field, one point) counterparts of the prover-side kernels in prover_kernels.hip, written separately from them.
#include "../../include/qpgpu.h"
#include "../../include/qpgpu_verify.h"
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <atomic>
#include <thread>
#include <string>
#include <vector>
#include "challenger.hpp"
#include "circuit.hpp"
#include "gl64.hpp"
#include "poseidon.hpp"
#include "verifier.hpp"
#include "verify_math.hpp"

using gl::e2;
using gl::u64;

int verify::fail(char *err, int code, const char *fmt, ...) {
    if (err) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(err, QPGPU_VERIFY_ERR_CAP, fmt, ap);
        va_end(ap);
    }
    return code;
}
using verify::fail;

int verify::parse_hasher(int hasher_kind, const uint64_t *hasher_params, size_t n_params, hasher::Config &out, char *err) {
    if (hasher_kind == hasher::POSEIDON) { out.kind = hasher::POSEIDON; return QPGPU_OK; }
    if (hasher_kind != hasher::POSEIDON2) return fail(err, QPGPU_EINVAL, "unknown hasher kind");
    out.kind = hasher::POSEIDON2;
    if (!hasher_params && n_params == 0) { out.p2 = poseidon2::qp_params(); return QPGPU_OK; }
    if (!hasher_params || n_params != (size_t)poseidon2::PARAM_WORDS) return fail(err, QPGPU_EINVAL, "bad Poseidon2 parameter block");
    for (size_t i = 0; i < n_params; i++) if (hasher_params[i] >= gl::P) return fail(err, QPGPU_EINVAL, "Poseidon2 parameter %zu is not canonical", i);
    std::memcpy(out.p2.rc_ext, hasher_params, 96 * 8);
    std::memcpy(out.p2.rc_int, hasher_params + 96, 22 * 8);
    std::memcpy(out.p2.diag_m1, hasher_params + 118, 12 * 8);
    std::memcpy(out.p2.m4, hasher_params + 130, 16 * 8);
    return QPGPU_OK;
}

bool verify::same_hasher(const hasher::Config &a, const hasher::Config &b) {
    if (a.kind != b.kind) return false;
    if (a.kind != hasher::POSEIDON2) return true;
    return memcmp(a.p2.rc_ext, b.p2.rc_ext, sizeof a.p2.rc_ext) == 0 && memcmp(a.p2.rc_int, b.p2.rc_int, sizeof a.p2.rc_int) == 0 &&
           memcmp(a.p2.diag_m1, b.p2.diag_m1, sizeof a.p2.diag_m1) == 0 && memcmp(a.p2.m4, b.p2.m4, sizeof a.p2.m4) == 0;
}

namespace {

// ---- extension-field shorthands (F[x]/(x^2 - 7)) ----
inline e2 E(u64 a) { return gl::e2_from(a); }
using gl::scale;       // + - * scale sadd madd on e2: verify_math.hpp
inline bool same(e2 x, e2 y) { x = gl::e2_canon(x); y = gl::e2_canon(y); return x.a == y.a && x.b == y.b; }

// ---- hashing under the proof system's permutation ----
struct Hash {
    const hasher::Config *h;
    void leaf(const u64 *row, size_t width, u64 out[4]) const {     // hash_or_noop
        if (width <= 4) { for (size_t i = 0; i < 4; i++) out[i] = i < width ? row[i] : 0; return; }
        hasher::hash_no_pad(*h, row, width, out);
    }
    void two_to_one(const u64 *l, const u64 *r, u64 out[4]) const {
        u64 st[12] = {l[0], l[1], l[2], l[3], r[0], r[1], r[2], r[3], 0, 0, 0, 0};
        h->permute(st);
        std::memcpy(out, st, 32);
    }
};

inline uint32_t bitrev(uint32_t x, unsigned bits) {
    uint32_t r = 0;
    for (unsigned i = 0; i < bits; i++) r |= ((x >> i) & 1u) << (bits - 1 - i);
    return r;
}

// in-place radix-2 transform of 2^log_n values by powers of `root` (natural order in and out)
void ntt(std::vector<u64> &a, unsigned log_n, u64 root) {
    const size_t n = (size_t)1 << log_n;
    for (size_t i = 0; i < n; i++) { const size_t j = bitrev((uint32_t)i, log_n); if (j > i) std::swap(a[i], a[j]); }
    for (unsigned s = 1; s <= log_n; s++) {
        const size_t m = (size_t)1 << s, half = m >> 1;
        const u64 wm = gl::pow(root, n >> s);
        for (size_t k = 0; k < n; k += m) {
            u64 w = 1;
            for (size_t j = 0; j < half; j++) {
                const u64 t = gl::mul(w, a[k + j + half]), u = a[k + j];
                a[k + j] = gl::add(u, t); a[k + j + half] = gl::sub(u, t);
                w = gl::mul(w, wm);
            }
        }
    }
}

// the gate constraints and the vanishing polynomial at one point: verify_math.hpp (shared with the in-circuit verifier)
using vmath::gate_constraints;

}  // namespace

namespace {
bool path_ok(const Hash &H, const u64 *leaf, size_t width, size_t index, const u64 *path, size_t plen, const u64 *cap) {
    u64 cur[4], nxt[4];
    H.leaf(leaf, width, cur);
    for (size_t i = 0; i < plen; i++) {
        if (index & 1) H.two_to_one(path + 4 * i, cur, nxt); else H.two_to_one(cur, path + 4 * i, nxt);
        std::memcpy(cur, nxt, 32);
        index >>= 1;
    }
    return std::memcmp(cur, cap + 4 * index, 32) == 0;
}
}  // namespace

// ---- the query rounds of any FRI instance (fri_verify.hpp): verify_impl below and qpgpu_fri_verify (fri_verify.cpp) ----
namespace friv {

void reduced_openings(const Instance &in, const e2 *openings, e2 alpha, e2 *out) {
    for (size_t b = 0; b < in.batches.size(); b++) {
        const size_t n = in.batch_count(b);
        e2 red = E(0);
        for (size_t j = n; j-- > 0;) red = red * alpha + openings[j];
        out[b] = red;
        openings += n;
    }
}

void query_reason(char *out, size_t qi, uint32_t code) {
    const unsigned kind = code >> 8, at = code & 0xff;
    switch (kind) {
    case VQ_ORACLE_PLEN: fail(out, 0, "query %zu: Merkle path length of oracle %d out of range", qi, (int)at); break;
    case VQ_ORACLE_PATH: fail(out, 0, "query %zu: Merkle path of initial oracle %d does not lead to its cap", qi, (int)at); break;
    case VQ_ROUND_PLEN: fail(out, 0, "query %zu: Merkle path length of FRI round %zu out of range", qi, (size_t)at); break;
    case VQ_ROUND_CONT: fail(out, 0, "query %zu: FRI round %zu does not continue the previous evaluation", qi, (size_t)at); break;
    case VQ_ROUND_PATH: fail(out, 0, "query %zu: Merkle path of FRI round %zu does not lead to its cap", qi, (size_t)at); break;
    default: fail(out, 0, "query %zu: the final polynomial does not match the last FRI round", qi); break;
    }
}

// A query round has one layout (proof_layout::Fri): a path-length byte that differs from the layout's is a verdict, never a
// length, so every read is at a fixed offset inside the round.
uint32_t query_rounds(const hasher::Config &h, const Instance &in, const QueryInput &q, const uint8_t *queries, size_t *query) {
    const Hash H{&h};
    const proof_layout::Fri &lay = in.lay;
    const proof_layout::Opening *op = lay.op.data();     // the initial oracles, then the FRI rounds
    const size_t n_oracles = in.widths.size(), n_rounds = in.arity_bits.size(), n_batches = in.batches.size(), cap_words = in.cap_words();
    const unsigned L = in.degree_bits + in.rate_bits;
    std::vector<size_t> row_at(n_oracles);
    size_t row_words = 0;
    for (size_t o = 0; o < n_oracles; o++) { row_at[o] = row_words; row_words += in.widths[o]; }
    std::vector<u64> row(row_words + 1), path(64 * 4), ev(2 << 8);
    std::vector<e2> shift(n_batches);                    // ReducingFactor::shift of a batch: alpha^(its polynomials)
    for (size_t b = 0; b < n_batches; b++) shift[b] = gl::e2_pow(q.alpha, in.batch_count(b));
    const u64 w_lde = gl::root_of_unity(L);
    auto words = [](u64 *out, const uint8_t *p, size_t n) { std::memcpy(out, p, 8 * n); };
    for (size_t qi = 0; qi < lay.num_query_rounds; qi++) {
        *query = qi;
        const uint8_t *base = queries + qi * lay.round_bytes;
        size_t x_index = (size_t)q.indices[qi];
        for (size_t o = 0; o < n_oracles; o++) {
            u64 *r = row.data() + row_at[o];
            const uint8_t *at = base + op[o].off;
            words(r, at, in.widths[o]);
            const size_t plen = at[8 * in.widths[o]];
            if (plen > 60) return VQ_ORACLE_PLEN << 8 | (uint32_t)o;
            if (plen != op[o].path_len) return VQ_ORACLE_PATH << 8 | (uint32_t)o;
            words(path.data(), at + 8 * in.widths[o] + 1, plen * 4);
            if (!path_ok(H, r, in.widths[o], x_index, path.data(), plen, q.caps[o])) return VQ_ORACLE_PATH << 8 | (uint32_t)o;
        }
        u64 subgroup_x = gl::mul(gl::MULT_GEN, gl::pow(w_lde, bitrev((uint32_t)x_index, L)));
        const e2 sx = E(subgroup_x);
        e2 sum = E(0);                                   // fri_combine_initial: salts are not opened
        for (size_t b = 0; b < n_batches; b++) {
            e2 e = E(0);
            const std::vector<Range> &rg = in.batches[b];
            for (size_t k = rg.size(); k-- > 0;) {
                const u64 *r = row.data() + row_at[rg[k].oracle] + rg[k].first;
                for (size_t j = rg[k].count; j-- > 0;) e = e * q.alpha + E(r[j]);
            }
            sum = sum * shift[b] + (e - q.reduced[b]) * gl::e2_inv(sx - q.points[b]);
        }
        e2 old_eval = sum;
        for (size_t r = 0; r < n_rounds; r++) {
            const unsigned ab = (unsigned)in.arity_bits[r];
            const size_t arity = (size_t)1 << ab;
            const uint8_t *at = base + op[n_oracles + r].off;
            words(ev.data(), at, 2 * arity);
            const size_t plen = at[16 * arity];
            if (plen > 60) return VQ_ROUND_PLEN << 8 | (uint32_t)r;
            const size_t coset_index = x_index >> ab, within = x_index & (arity - 1);
            if (!same(gl::e2_make(ev[2 * within], ev[2 * within + 1]), old_eval)) return VQ_ROUND_CONT << 8 | (uint32_t)r;
            if (plen != op[n_oracles + r].path_len) return VQ_ROUND_PATH << 8 | (uint32_t)r;
            words(path.data(), at + 16 * arity + 1, plen * 4);
            if (!path_ok(H, ev.data(), 2 * arity, coset_index, path.data(), plen, q.round_caps + r * cap_words)) return VQ_ROUND_PATH << 8 | (uint32_t)r;
            // compute_evaluation: interpolate the coset's 2^ab evaluations and evaluate at beta
            const u64 g = gl::root_of_unity(ab);
            const size_t rev_within = bitrev((uint32_t)within, ab);
            const u64 coset_start = gl::mul(subgroup_x, gl::pow(g, arity - rev_within));
            std::vector<u64> px(arity); std::vector<e2> py(arity);
            for (size_t i = 0; i < arity; i++) {
                const size_t src = bitrev((uint32_t)i, ab);
                py[i] = gl::e2_make(ev[2 * src], ev[2 * src + 1]);
                px[i] = gl::mul(coset_start, gl::pow(g, i));
            }
            const e2 beta = q.betas[r];
            e2 acc = E(0);
            if (ab <= 5) {
                for (size_t i = 0; i < arity; i++) {      // Lagrange form
                    e2 num = E(1); u64 den = 1;
                    for (size_t j = 0; j < arity; j++) if (j != i) { num = num * (beta - E(px[j])); den = gl::mul(den, gl::sub(px[i], px[j])); }
                    acc = acc + py[i] * scale(num, gl::inv(den));
                }
            } else {
                // the same value in barycentric form (the points are a coset of the 2^ab-th roots of unity): beyond arity 32 the
                // quadratic Lagrange loop is 2^16 multiplications per round and query
                //   p(beta) = (beta^n - s^n) / (n s^n) * sum_i y_i x_i / (beta - x_i)
                const u64 s_n = gl::pow(coset_start, arity);
                bool hit = false;
                for (size_t i = 0; i < arity && !hit; i++) if (same(beta, E(px[i]))) { acc = py[i]; hit = true; }
                if (!hit) {
                    for (size_t i = 0; i < arity; i++) acc = acc + scale(py[i], px[i]) * gl::e2_inv(beta - E(px[i]));
                    acc = scale(acc * (gl::e2_pow(beta, arity) - E(s_n)), gl::inv(gl::mul(s_n, (u64)arity)));
                }
            }
            old_eval = acc;
            subgroup_x = gl::pow(subgroup_x, arity);
            x_index = coset_index;
        }
        e2 fe = E(0);
        const e2 sxe = E(subgroup_x);
        for (size_t i = lay.final_len; i-- > 0;) fe = fe * sxe + q.final_poly[i];
        if (!same(fe, old_eval)) return VQ_FINAL << 8;
    }
    return 0;
}

}  // namespace friv

namespace {

// constants/sigmas cap from the pack: per column values -> coefficients -> coset LDE in leaf order; leaves hashed, tree to the cap
void host_cs_cap(const CircuitPack &p, const Hash &H, std::vector<u64> &cap) {
    const unsigned d = (unsigned)p.degree_bits, L = d + (unsigned)p.rate_bits;
    const size_t n = (size_t)1 << d, lde_n = (size_t)1 << L, ncs = p.num_cs_cols();
    std::vector<u64> lde(ncs * lde_n), col(n), ext(lde_n);
    const u64 w_inv = gl::inv(gl::root_of_unity(d)), n_inv = gl::inv(n), w_lde = gl::root_of_unity(L);
    for (size_t c = 0; c < ncs; c++) {
        std::copy(p.constants_sigmas.begin() + c * n, p.constants_sigmas.begin() + (c + 1) * n, col.begin());
        ntt(col, d, w_inv);
        u64 shift = 1;
        std::fill(ext.begin(), ext.end(), 0);
        for (size_t i = 0; i < n; i++) { ext[i] = gl::mul(gl::mul(col[i], n_inv), shift); shift = gl::mul(shift, gl::MULT_GEN); }
        ntt(ext, L, w_lde);
        for (size_t j = 0; j < lde_n; j++) lde[c * lde_n + j] = gl::canon(ext[bitrev((uint32_t)j, L)]);   // leaf j = point g w^rev(j)
    }
    std::vector<u64> level(lde_n * 4), row(ncs);
    for (size_t j = 0; j < lde_n; j++) {
        for (size_t c = 0; c < ncs; c++) row[c] = lde[c * lde_n + j];
        H.leaf(row.data(), ncs, &level[4 * j]);
    }
    size_t cnt = lde_n;
    while (cnt > ((size_t)1 << p.cap_height)) {
        for (size_t i = 0; i < cnt / 2; i++) { u64 o[4]; H.two_to_one(&level[8 * i], &level[8 * i + 4], o); std::memcpy(&level[4 * i], o, 32); }
        cnt >>= 1;
    }
    cap.assign(level.begin(), level.begin() + 4 * cnt);
}

using proof_layout::Reader;
void read_exts(Reader &b, std::vector<e2> &v, size_t n) { v.resize(n); b.vec((u64 *)v.data(), 2 * n); }

}  // namespace

extern "C" {

int qpgpu_verifier_create(const uint64_t *pack_words, size_t n_words, const uint64_t *cs_cap, size_t cap_words, int hasher_kind,
                          const uint64_t *hasher_params, size_t n_params, qpgpu_verifier **out, char *err) {
    if (!pack_words || !out) return fail(err, QPGPU_EINVAL, "null argument");
    qpgpu_verifier *v = new (std::nothrow) qpgpu_verifier();
    if (!v) return fail(err, QPGPU_ENOMEM, "out of memory");
    const std::string why = v->pack.parse(pack_words, n_words);
    if (!why.empty()) { delete v; return fail(err, QPGPU_EINVAL, "circuit pack: %s", why.c_str()); }
    if (int rc = verify::parse_hasher(hasher_kind, hasher_params, n_params, v->hash, err)) { delete v; return rc; }
    const CircuitPack &p = v->pack;
    if (p.num_challenges > 4 || p.arity_bits.size() > 16) { delete v; return fail(err, QPGPU_EINVAL, "circuit outside the supported range"); }
    for (u64 ab : p.arity_bits) if (ab == 0 || ab > 5) { delete v; return fail(err, QPGPU_EINVAL, "FRI arity outside 2..32"); }
    {   // every FRI round's tree must still be at least as tall as the cap (the proof layout subtracts the two)
        u64 lvl = p.degree_bits + p.rate_bits;
        for (u64 ab : p.arity_bits) {
            if (ab > lvl || lvl - ab < p.cap_height) { delete v; return fail(err, QPGPU_EINVAL, "FRI reduction schedule is inconsistent with degree_bits / cap_height"); }
            lvl -= ab;
        }
    }
    const size_t want = ((size_t)1 << p.cap_height) * 4;
    if (cs_cap) {
        if (cap_words != want) { delete v; return fail(err, QPGPU_EINVAL, "constants/sigmas cap has %zu words, the circuit's cap height needs %zu", cap_words, want); }
        v->cs_cap.assign(cs_cap, cs_cap + want);
    } else {
        if (p.degree_bits + p.rate_bits > 20) { delete v; return fail(err, QPGPU_EINVAL, "constants/sigmas cap not given and the circuit is too large to rebuild it on the host"); }
        const Hash H{&v->hash};
        host_cs_cap(p, H, v->cs_cap);
    }
    v->layout = proof_layout::of(p);
    {   // the FRI part as fri::verifier sees it: batch 0 opens every polynomial at zeta, batch 1 the Zs at g zeta
        friv::Instance &f = v->fri;
        f.degree_bits = (unsigned)p.degree_bits; f.rate_bits = (unsigned)p.rate_bits; f.cap_height = (unsigned)p.cap_height;
        f.pow_bits = (unsigned)p.proof_of_work_bits;
        f.widths.assign(v->layout.widths, v->layout.widths + 4);
        f.polys.assign(v->layout.polys, v->layout.polys + 4);
        f.arity_bits = p.arity_bits;
        f.batches.resize(2);
        for (uint32_t o = 0; o < 4; o++) f.batches[0].push_back({o, 0, (uint32_t)f.polys[o]});
        f.batches[1].push_back({2, 0, (uint32_t)p.num_challenges});
        f.lay = v->layout.fri;
    }
    {   // the consistency check vanishing_at_zeta makes of the gate table does not read the openings: asked once, on zeros, for
        // the device head (verify_device.cpp), which reports it where verify_head does
        const size_t nch = p.num_challenges;
        const std::vector<e2> zero(std::max<size_t>(std::max<size_t>(p.num_cs_cols(), p.num_wires), nch * (1 + p.num_partial_products)) + 8, E(0));
        const e2 z = E(0), four[4] = {z, z, z, z};
        std::vector<e2> van;
        v->pack_why = vmath::vanishing_at_zeta<e2>(p, z, z, zero.data(), zero.data(), zero.data(), zero.data(), zero.data(), four, four, four, four, van);
    }
    *out = v;
    return QPGPU_OK;
}

void qpgpu_verifier_free(qpgpu_verifier *v) { delete v; }
size_t qpgpu_verifier_proof_size(const qpgpu_verifier *v) { return v ? v->layout.total : 0; }
int qpgpu_verifier_constants_sigmas_cap(const qpgpu_verifier *v, uint64_t *out, size_t out_words) {
    if (!v || !out || out_words < v->cs_cap.size()) return QPGPU_EINVAL;
    std::memcpy(out, v->cs_cap.data(), v->cs_cap.size() * 8);
    return QPGPU_OK;
}

static int verify_impl(const qpgpu_verifier *v, const uint8_t *proof, size_t len, char *err, uint64_t *indices_out);
int qpgpu_verifier_verify(const qpgpu_verifier *v, const uint8_t *proof, size_t len, char *err) { return verify_impl(v, proof, len, err, nullptr); }
// The FRI query indices of a proof: the transcript replayed up to the proof of work, then num_query_rounds challenges reduced
// mod the LDE size. Everything the transcript absorbs is checked on the way (sizes, canonical elements, quotient identity,
// proof of work); the query rounds themselves are NOT looked at, so the indices of a proof whose opened rows or paths were
// tampered with are still returned (they are what a recursive verifier circuit derives in-circuit, wormhole/aggregator/src/
// common/recursive.rs:91-97).
int qpgpu_verifier_query_indices(const qpgpu_verifier *v, const uint8_t *proof, size_t len, uint64_t *out, size_t cap, char *err) {
    if (!v || !out || cap < v->pack.num_query_rounds) return fail(err, QPGPU_EINVAL, "query_indices: null argument or room for fewer than num_query_rounds indices");
    return verify_impl(v, proof, len, err, out);
}
}  // extern "C"

// the head of verification: parse, transcript, proof of work, quotient identity at zeta, the query indices
int verify_head(const qpgpu_verifier *v, const uint8_t *proof, size_t len, char *err, VerifyHead &h) {
    if (!v || !proof) return fail(err, QPGPU_EINVAL, "null argument");
    const CircuitPack &c = v->pack;
    const proof_layout::Proof &lay = v->layout;
    if (len != lay.total) return fail(err, QPGPU_EVERIFY, "proof has %zu bytes, this circuit's proofs have %zu", len, lay.total);
    const unsigned d = (unsigned)c.degree_bits, rb = (unsigned)c.rate_bits;
    const size_t n = (size_t)1 << d, lde_n = n << rb, nch = c.num_challenges;
    const size_t cap_words = lay.cap_bytes / 8, n_rounds = c.arity_bits.size();

    Reader b{proof, len};
    std::vector<u64> &wires_cap = h.wires_cap, &zs_cap = h.zs_cap, &q_cap = h.q_cap;
    wires_cap.assign(cap_words, 0); zs_cap.assign(cap_words, 0); q_cap.assign(cap_words, 0);
    b.vec(wires_cap.data(), cap_words); b.vec(zs_cap.data(), cap_words); b.vec(q_cap.data(), cap_words);
    std::vector<e2> o_cs, o_w, o_zs, o_zn, o_pp, o_q;
    const proof_layout::Vec *ov = lay.openings;      // constants and sigmas are one vector here, as in the oracle that holds them
    read_exts(b, o_cs, ov[0].count + ov[1].count); read_exts(b, o_w, ov[2].count); read_exts(b, o_zs, ov[3].count); read_exts(b, o_zn, ov[4].count);
    read_exts(b, o_pp, ov[5].count); read_exts(b, o_q, ov[6].count);
    std::vector<u64> &fri_caps = h.fri_caps;
    fri_caps.assign(cap_words * n_rounds, 0);
    b.vec(fri_caps.data(), cap_words * n_rounds);
    b.pos = lay.final_pos;                           // over the query rounds
    std::vector<e2> &final_poly = h.final_poly;
    read_exts(b, final_poly, lay.fri.final_len);
    u64 pow_witness = b.word();
    std::vector<u64> pis(c.num_public_inputs + 1);
    b.vec(pis.data(), c.num_public_inputs);
    if (b.bad || b.pos != len) return fail(err, QPGPU_EVERIFY, "proof layout does not match the circuit");
    if (b.noncanonical) return fail(err, QPGPU_EVERIFY, "proof holds a non-canonical field element");

    // ---- challenges: the prover's transcript, replayed ----
    u64 pih[4];
    hasher::hash_no_pad(v->hash, pis.data(), c.num_public_inputs, pih);
    Challenger ch(v->hash);
    auto observe = [&ch](const std::vector<e2> &x) { ch.observe((const u64 *)x.data(), 2 * x.size()); };
    ch.observe_raw(c.circuit_digest, 4);
    ch.observe(pih, 4);
    ch.observe(wires_cap.data(), cap_words);
    u64 betas[4], gammas[4], alphas[4];
    for (size_t k = 0; k < nch; k++) betas[k] = ch.get();
    for (size_t k = 0; k < nch; k++) gammas[k] = ch.get();
    ch.observe(zs_cap.data(), cap_words);
    for (size_t k = 0; k < nch; k++) alphas[k] = ch.get();
    ch.observe(q_cap.data(), cap_words);
    const e2 zeta = h.zeta = ch.get_ext();
    observe(o_cs); observe(o_w); observe(o_zs); observe(o_pp); observe(o_q); observe(o_zn);
    const e2 fri_alpha = h.fri_alpha = ch.get_ext();
    std::vector<e2> &fri_betas = h.fri_betas;
    fri_betas.assign(n_rounds, E(0));
    for (size_t r = 0; r < n_rounds; r++) { ch.observe(fri_caps.data() + r * cap_words, cap_words); fri_betas[r] = ch.get_ext(); }
    observe(final_poly);
    ch.observe(&pow_witness, 1);
    const u64 pow_response = ch.get();
    if (c.proof_of_work_bits && (pow_response >> (64 - c.proof_of_work_bits)) != 0)
        return fail(err, QPGPU_EVERIFY, "proof-of-work response has fewer than %llu leading zero bits", (unsigned long long)c.proof_of_work_bits);

    // ---- vanishing polynomial at zeta against Z_H(zeta) * quotient(zeta) ----
    {
        e2 zeta_n = zeta;
        for (unsigned i = 0; i < d; i++) zeta_n = zeta_n * zeta_n;
        const e2 zh = zeta_n - E(1);
        const e2 l0 = zh * gl::e2_inv(scale(zeta - E(1), (u64)n));
        e2 xb[4], xg[4], xa[4], xpih[4];
        for (size_t k = 0; k < nch; k++) { xb[k] = E(betas[k]); xg[k] = E(gammas[k]); xa[k] = E(alphas[k]); }
        for (int i = 0; i < 4; i++) xpih[i] = E(pih[i]);
        std::vector<e2> van;
        const std::string why = vmath::vanishing_at_zeta<e2>(c, zeta, l0, o_cs.data(), o_w.data(), o_zs.data(), o_zn.data(), o_pp.data(), xb, xg, xa, xpih, van);
        if (!why.empty()) return fail(err, QPGPU_EVERIFY, "%s", why.c_str());
        for (size_t k = 0; k < nch; k++) {
            e2 qv = E(0);
            for (size_t j = c.quotient_degree_factor; j-- > 0;) qv = qv * zeta_n + o_q[k * c.quotient_degree_factor + j];
            if (!same(van[k], zh * qv)) return fail(err, QPGPU_EVERIFY, "quotient identity fails at zeta (challenge %zu): the openings do not satisfy the circuit", k);
        }
    }

    // ---- FRI ----
    e2 &red0 = h.red0, &red1 = h.red1;     // reduced openings: sum_j opening_j alpha^j, batch 0 in oracle order, batch 1 = Zs at g zeta
    {
        red0 = red1 = E(0);
        const std::vector<e2> *parts[5] = {&o_cs, &o_w, &o_zs, &o_pp, &o_q};
        for (int p = 5; p-- > 0;) for (size_t j = parts[p]->size(); j-- > 0;) red0 = red0 * fri_alpha + (*parts[p])[j];
        for (size_t j = nch; j-- > 0;) red1 = red1 * fri_alpha + o_zn[j];
    }
    h.g_zeta = scale(zeta, gl::root_of_unity(d));
    h.alpha_nch = gl::e2_pow(fri_alpha, nch);
    h.x_indices.resize(c.num_query_rounds);      // the query rounds do not touch the transcript: draw them all first
    for (size_t qi = 0; qi < c.num_query_rounds; qi++) h.x_indices[qi] = (size_t)(ch.get() % lde_n);
    return QPGPU_OK;
}

extern "C" {

static int verify_impl(const qpgpu_verifier *v, const uint8_t *proof, size_t len, char *err, uint64_t *indices_out) {
    VerifyHead h;
    const int head = verify_head(v, proof, len, err, h);
    if (head != QPGPU_OK) return head;
    if (indices_out) { for (size_t qi = 0; qi < h.x_indices.size(); qi++) indices_out[qi] = h.x_indices[qi]; return QPGPU_OK; }
    // the query rounds: fri::verifier::verify_fri_proof's loop (friv::query_rounds above), shared with qpgpu_fri_verify
    const u64 *caps0[4] = {v->cs_cap.data(), h.wires_cap.data(), h.zs_cap.data(), h.q_cap.data()};
    const e2 points[2] = {h.zeta, h.g_zeta}, reduced[2] = {h.red0, h.red1};
    static_assert(sizeof(size_t) == sizeof(uint64_t), "query indices are passed on as 64-bit words");
    const friv::QueryInput q{caps0, h.fri_caps.data(), points, reduced, h.fri_alpha, h.fri_betas.data(), h.final_poly.data(),
                             reinterpret_cast<const uint64_t *>(h.x_indices.data())};
    size_t qi = 0;
    const uint32_t code = friv::query_rounds(v->hash, v->fri, q, proof + v->layout.queries_pos, &qi);
    if (!code) return QPGPU_OK;
    friv::query_reason(err, qi, code);
    return QPGPU_EVERIFY;
}

int qpgpu_verifier_verify_many(const qpgpu_verifier *v, const uint8_t *const *proofs, const size_t *lens, size_t count, unsigned threads,
                               int *results, char *err) {
    if (!v || !proofs || !lens || !results) return fail(err, QPGPU_EINVAL, "null argument");
    if (threads == 0) threads = std::max(1u, std::thread::hardware_concurrency());
    threads = (unsigned)std::min<size_t>(threads, std::max<size_t>(count, 1));
    std::atomic<size_t> next{0};
    std::vector<std::string> reasons(count);
    auto work = [&] {
        char local[QPGPU_VERIFY_ERR_CAP];
        for (size_t i = next.fetch_add(1); i < count; i = next.fetch_add(1)) {
            local[0] = 0;
            results[i] = proofs[i] ? qpgpu_verifier_verify(v, proofs[i], lens[i], local) : QPGPU_EINVAL;
            if (results[i]) reasons[i] = local;
        }
    };
    std::vector<std::thread> pool;
    try {
        for (unsigned t = 1; t < threads; t++) pool.emplace_back(work);
    } catch (...) {}                 // no more threads to be had: the ones that started (and this one) drain the queue
    work();
    for (auto &t : pool) t.join();
    for (size_t i = 0; i < count; i++)
        if (results[i]) return fail(err, QPGPU_EVERIFY, "proof %zu: %.170s", i, reasons[i].c_str());
    return QPGPU_OK;
}

}  // extern "C"
