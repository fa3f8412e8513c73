// poseidon_mfma.hpp — the 22 partial rounds of the Poseidon permutation (poseidon.hpp) as one constant matrix on the matrix pipe.
//
// Same function as poseidon::permute (plonky2::hash::poseidon::Poseidon::poseidon for GoldilocksField; reference
// common/src/circuit.rs:17), bit for bit; only the schedule of the partial rounds differs. In a partial round lane 0 alone goes
// through the S-box, so with N = M P (M the MDS matrix, P = "zero lane 0"), m0 = M e0 and y_k the S-box output of round k, the S-box
// input of every round and the state after the last one are affine in (s, y_0 .. y_{k-1}):
//     x_k = (e0^T N^k)(s + c') + sum_{j<k} (e0^T N^{k-1-j} m0) y_j + c_k         out = N^22 (s + c') + sum_j y_j N^{21-j} m0 + c''
// (c' the lanes-1..11 constants before the first partial round, c'' the constants of the full round that follows: both folded into
// the additive terms; and s = M t for the S-box outputs t of the fourth full round, so that round's MDS layer is in the matrix too). That is one matrix of dense 64-bit field constants with 34 columns; a 64-bit modular matrix product is an
// int8 GEMM on byte digits, and v_mfma_i32_32x32x32_i8 runs beside the vector ALU, which the rest of the permutation saturates:
//   * B operand = the inputs as 8 signed base-256 digits per element. The state of lane n is column n, an element's 8 digits are 8
//     consecutive k: the registers already hold the operand, up to one v_permlane32_swap per register pair (lanes 32..63 of a
//     32-column tile carry the second half of K).
//   * A operand: column (element e, digit b) of output o holds the 8 signed digits of the constant w[o][e] 256^b mod p (the
//     representative in the balanced range: w or w - p always fits 8 digits in [-128, 127]), one digit per output limb: 8 limbs per
//     output, 4 outputs per 32-row tile. Tiles live in LDS (60 KB), one ds_read_b128 per MFMA pair.
//   * C operand = 2^23 + the additive constant's bytes: every limb comes out in [3 670 016, 13 107 455] (|sum| <= 288 x 2^14), and
//     any two limbs up to 16 711 935 = (2^32 - 1) / 257 join at 8-bit spacing in one 32-bit shift-add. Recombining 8 limbs is four
//     such shift-adds and three words with two carries (recombine_wide, 14 to 15 vector instructions), then one reduce96: about 20
//     vector instructions per output where an MDS layer in the spectral form costs about 270. The table builder proves the limb
//     bound from the table bytes before a table may be uploaded (host::chain_limb_max).
//   * The K dimension only ever holds complete groups of four y; the y of the running group reach the rounds of that group through
//     three small integer coefficients (25, 5 017, 1 259 209) on the VALU.
// The accumulator layout gives a lane 16 rows of its own column and 16 of the partner lane's (lane +-32): 16 swaps give every lane
// the 32 rows of its own column. Every register of both accumulators is read by those swaps: nothing may be written into the
// destination of an MFMA that is still in flight (measured: a wave sharing its SIMD's matrix pipe with other waves sees its MFMAs
// finish later than the fixed distance the compiler's hazard table assumes when it reuses a dead destination register for an LDS
// load; wrong results on every wave but one per SIMD).
#pragma once
#include <string.h>
#include <utility>
#include "poseidon.hpp"

namespace pmf {
using gl::u32;
using gl::u64;
#if defined(__HIPCC__)
typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));
#endif

constexpr int LIMBS = 8, N_GROUP = 6, N_FIN = 3, FIN_STEPS = 9, N_ELEM = 36;   // 12 state elements + 22 y + 2 zero
constexpr int group_steps(int g) { return 3 + g; }                  // group g = rounds 4g .. 4g+3: elements 12 + 4g known
constexpr int group_base(int g) { int b = 0; for (int i = 0; i < g; i++) b += group_steps(i); return b; }
constexpr int N_GROUP_TILES = group_base(N_GROUP);                  // 33
constexpr int N_TILES = N_GROUP_TILES + N_FIN * FIN_STEPS;          // 60
constexpr int CINIT_OFF = N_TILES * 1024;
constexpr int G_OFF = CINIT_OFF + (N_GROUP + N_FIN) * 128;         // three 64-bit coefficients of the running group's y
constexpr int TABLE_BYTES = G_OFF + 32;
static_assert(N_GROUP_TILES == 33 && TABLE_BYTES % 16 == 0, "table layout");
constexpr u64 DIGIT_BIAS = 0x8080808080808080ull;

// coefficients of the running group's y: G[d] = e0^T N^d m0 for d = 0, 1, 2 (integers, no reduction)
constexpr u64 mds_entry(int r, int j) {
    constexpr u32 C[12] = {17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20};
    return C[(j - r + 12) % 12] + ((r == 0 && j == 0) ? 8 : 0);
}
constexpr u64 small_g(int d) {
    u64 R[12] = {1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int it = 0; it < d; it++) {
        u64 T[12] = {};
        for (int j = 1; j < 12; j++)
            for (int i = 0; i < 12; i++) T[j] += R[i] * mds_entry(i, j);
        for (int j = 0; j < 12; j++) R[j] = T[j];
    }
    u64 g = 0;
    for (int i = 0; i < 12; i++) g += R[i] * mds_entry(i, 0);
    return g;
}
constexpr u32 G0 = (u32)small_g(0), G1 = (u32)small_g(1), G2 = (u32)small_g(2);
static_assert(small_g(0) == 25 && small_g(1) < small_g(2) && small_g(2) < (1ull << 21), "group coefficients: the bound of reduce96_terms");

// ---- pieces shared by the device code and the host emulation ----
// v -> eight signed digits d_b in [-128, 127] packed in a u64: d_b = byte b of v, minus 128, i.e. byte ^ 0x80 read as signed. As
// integers sum d_b 256^b = v - BIAS for EVERY 64-bit v: no carry, no wrap, no representative to choose. The gemm is linear, so
// output row o comes out short of the constant BIAS sum_e w[o][e] over the elements whose digits are in; host::build_tables puts
// that constant into the row's accumulator start (Rows::addc). Elements that are not known yet and the two pad elements keep the
// literal digits 0 (not 0 ^ BIAS): their weights are zero.
GL_HD u64 to_digits(u64 v) { return v ^ DIGIT_BIAS; }
// The largest limb a join may see: 16 711 935 x 257 = 2^32 - 1, so z + 256 z' fits 32 bits for any two limbs up to it. What a
// chain can reach is far below: an accumulator starts at 2^23 + one byte and collects at most 288 products of two digits of
// magnitude <= 128, 2^23 + 255 + 288 x 2^14 = 13 107 455. host::fill_tiles proves the bound for every row from the table bytes
// themselves (a table that cannot hold it is never uploaded); host::emu_gemm checks every limb it computes against it.
constexpr u32 LIMB_MAX = 16711935u;
static_assert((u64)LIMB_MAX * 257 == 0xFFFFFFFFull, "two limbs at 8-bit spacing fit one word");
// sum_l z[l] 2^(8 l) as a 96-bit integer (lo + top 2^64) for 8 limbs in [0, LIMB_MAX]: neighbours pair up in one 32-bit
// shift-add each (t1..t4, no overflow, above), and t1 + t2 2^16 + t3 2^32 + t4 2^48 is three words with two carries: word 0 =
// t1 + (t2 << 16), word 1 = t3 + (lo16(t4) : hi16(t2)) + carry (one v_alignbit_b32 makes the middle term), top = (t4 >> 16) +
// carry. One text for host and device; the gfx950 compiler makes 14 to 15 vector instructions of it (about 22 for the three byte
// concatenations and the 96-bit add chain it replaces). Two other forms were counted and are not used, profiles/mds_gemm_isa.txt:
// two multiply-adds by 2^16 (X = t1 + t2 2^16, Y = t3 + t4 2^16, joined as X + Y 2^32; 8 instructions on paper, 14 compiled: the
// multiplications become 64-bit shifts and every 64-bit addend pays a v_mov for its zero upper half), and the same three words
// as an explicit add-with-carry chain (10 instructions, all full rate, but 16 more bytes of scratch per lane in the proof-of-work
// kernel and 4 in Poseidon2's node kernel, which no change to these kernels may cost).
// The sum is below 2^24 (2^56 + 2^48 + ...) < 2^81 (so below 2^82): the top word stays below 2^18.
GL_HD void recombine_wide(const u32 (&z)[LIMBS], u64 &lo, u32 &top) {
    const u32 t1 = z[0] + (z[1] << 8), t2 = z[2] + (z[3] << 8), t3 = z[4] + (z[5] << 8), t4 = z[6] + (z[7] << 8);
    const u32 m = (t4 << 16) | (t2 >> 16);     // v_alignbit_b32: the two halves do not overlap
    const u64 s0 = (u64)t1 + (t2 << 16), s1 = (u64)t3 + m + (s0 >> 32);
    const u32 w0 = (u32)s0, w1 = (u32)s1, c1 = (u32)(s1 >> 32);
    lo = ((u64)w1 << 32) | w0; top = (t4 >> 16) + c1;
}
// the same mod p: one reduce96
GL_HD u64 recombine(const u32 (&z)[LIMBS]) {
    u64 lo; u32 top;
    recombine_wide(z, lo, top);
    return gl::reduce96(lo, top);
}
// (lo + top 2^64 + sum_{i<n} y[i] g[i]) mod p with ONE reduction: the S-box input of a round of the running group, from the
// gemm's recombined sum and the group's earlier y with their small integer coefficients. Exact for any (loose) 64-bit y as long
// as the integer stays below 2^96, which reduce96 needs (top word < 2^32): the recombined sum is below 2^82, each term below
// 2^64 2^21 = 2^85 (G2 = 1 259 209 < 2^21), there are at most three terms: the total is below 2^82 + 3 2^85 < 2^87, top < 2^23.
// (A term reduced on its own, two multiply-adds + reduce96 + gl::add, is 15 to 16 vector instructions; a term added here is two multiply-adds and
// a carry.)
constexpr int MAX_GROUP_TERMS = 3;
// The terms go onto two 64-bit halves, one multiply-add each (v_mad_u64_u32 takes a 64-bit addend): al = the sum's low word + sum
// of lo32(y) g < 2^32 + 3 2^53, ah = the sum's upper 64 bits + sum of hi32(y) g < 2^50 + 3 2^53; neither can wrap, and the join
// is the MDS layer's (poseidon::join_halves). Counted in the gfx950 node kernel: 2 n + 3 vector instructions for n terms, where
// adding 128-bit products with unsigned __int128 gave 6 n.
GL_HD u64 reduce96_terms(u64 lo, u32 top, const u64 *y, const u32 *g, int n) {
    if (n == 0) return gl::reduce96(lo, top);
    u64 al = (u32)lo, ah = ((u64)top << 32) | (lo >> 32);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < n; i++) { al += (u64)(u32)y[i] * g[i]; ah += (y[i] >> 32) * g[i]; }
    const u64 low = al + (ah << 32);
    return gl::reduce96(low, (u32)(ah >> 32) + (low < al ? 1u : 0u));
}
// Tile rows. After the swaps a lane holds the 32 rows of its column in two register sets: X[i] = row (i&3) + 8 (i>>2), Y[i] = that
// row + 4. Outputs 0, 1 of a tile are X[0..7], X[8..15]; outputs 2, 3 are Y[0..7], Y[8..15]; limb = i & 7.
constexpr int row_of(int output, int limb) { const int i = 8 * (output & 1) + limb; return (i & 3) + 8 * (i >> 2) + 4 * (output >> 1); }

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- host: table construction (once per process) and an integer emulation of the device schedule ----
namespace host {
typedef unsigned __int128 u128;
inline u64 fmul(u64 a, u64 b) { return (u64)((u128)a * b % gl::P); }
inline u64 fadd(u64 a, u64 b) { return (u64)(((u128)a + b) % gl::P); }
inline u64 fsub(u64 a, u64 b) { return (u64)(((u128)a + gl::P - b % gl::P) % gl::P); }
// eight signed digits in [-128, 127] of the representative of w mod p in the balanced range
inline bool const_digits(u64 w, signed char (&d)[LIMBS]) {
    w %= gl::P;
    __int128 rep = w <= 0x7F7F7F7F7F7F7F7Full ? (__int128)w : (__int128)w - (__int128)gl::P;
    for (int a = 0; a < LIMBS; a++) {
        int dg = (int)(rep & 255);
        if (dg >= 128) dg -= 256;
        d[a] = (signed char)dg;
        rep = (rep - dg) / 256;
    }
    return rep == 0;
}
struct Rows { u64 w[4][N_ELEM]; u64 addc[4]; };   // the four outputs of a tile
// The largest limb one tile chain can produce, from the table bytes alone: over its 32 rows, start + 128 sum |a| (a B digit has
// magnitude at most 128, whatever the inputs). A row that could go below zero (start - 128 sum |a| < 0) counts as unbounded.
inline u64 chain_limb_max(const unsigned char *tiles, const unsigned char *cinit, int steps) {
    u64 worst = 0;
    for (int row = 0; row < 32; row++) {
        u64 mag = 0;
        for (int q = 0; q < steps; q++)
            for (int k = 0; k < 32; k++) {
                const int a = (signed char)tiles[(size_t)q * 1024 + (row + 32 * (k >> 4)) * 16 + (k & 15)];
                mag += (u64)(a < 0 ? -a : a);
            }
        u32 start; memcpy(&start, cinit + (row >> 2 & 1) * 64 + ((row & 3) + 4 * (row >> 3)) * 4, 4);   // row = (i&3) + 8 (i>>2) + 4 h
        if (start < 128 * mag) return ~0ull;
        if (start + 128 * mag > worst) worst = start + 128 * mag;
    }
    return worst;
}
inline bool fill_tiles(const Rows &rw, int steps, unsigned char *tiles, unsigned char *cinit) {
    static signed char dig[4][N_ELEM][8][LIMBS];
    for (int o = 0; o < 4; o++)
        for (int e = 0; e < N_ELEM; e++) {
            u64 w = rw.w[o][e] % gl::P;
            for (int b = 0; b < 8; b++) { if (!const_digits(w, dig[o][e][b])) return false; w = fmul(w, 256); }
        }
    for (int q = 0; q < steps; q++)
        for (int o = 0; o < 4; o++)
            for (int limb = 0; limb < LIMBS; limb++)
                for (int k = 0; k < 32; k++) {
                    const int lane = row_of(o, limb) + 32 * (k >> 4), j = k & 15, e = 4 * q + (k >> 3), b = k & 7;
                    tiles[(size_t)q * 1024 + lane * 16 + j] = (unsigned char)dig[o][e][b][limb];
                }
    // accumulator start: 2^23 + byte l of (addc - BIAS), BIAS = sum_{l<LIMBS} 2^23 2^(8l); register i of lane half h is row
    // (i&3) + 8 (i>>2) + 4 h = row_of(2 h + (i >> 3), i & 7)
    u64 bias = 0, pw = 1u << 23;
    for (int l = 0; l < LIMBS; l++) { bias = fadd(bias, pw); pw = fmul(pw, 256); }
    for (int h = 0; h < 2; h++)
        for (int i = 0; i < 16; i++) {
            const u64 c = fsub(rw.addc[2 * h + (i >> 3)], bias);
            const u32 v = (1u << 23) + (u32)((c >> (8 * (i & 7))) & 0xFF);
            memcpy(cinit + h * 64 + i * 4, &v, 4);
        }
    return chain_limb_max(tiles, cinit, steps) <= LIMB_MAX;
}
// to_digits hands the gemm v - BIAS for every element whose digits are in: row o gets BIAS sum_e w[o][e] back through its additive
// constant. A tile's rows carry weights only on elements that are known when the tile runs (the twelve state elements and the y
// of the groups before it; all 34 in the final tiles) and zero on the rest, whose digits are the literal 0: the sum over all
// columns is the sum over exactly the biased ones.
inline void fold_digit_bias(Rows &rw) {
    for (int o = 0; o < 4; o++) {
        u64 sw = 0;
        for (int e = 0; e < N_ELEM; e++) sw = fadd(sw, rw.w[o][e] % gl::P);
        rw.addc[o] = fadd(rw.addc[o], fmul(DIGIT_BIAS % gl::P, sw));
    }
}
// The partial-round block of a Poseidon-family permutation as the builder sees it: 22 rounds of `lane 0 <- (lane 0 + c_k)^7, state
// <- M state`, entered with `pre t + cvec` (t = the S-box outputs of the full round before: that round's linear layer is `pre`)
// and left with `+ after` (the constants of the full round behind).
struct Linear {
    u64 M[12][12], pre[12][12];
    u64 rc[22][12], after[12];      // rc[k]: the constants added to the state before round k's S-box (all twelve lanes)
};
inline bool build_tables(const Linear &L, unsigned char *tab) {
    static u64 R[23][12], G[22], Q[22][12], NP[12][12];
    const auto &M = L.M;
    for (int j = 0; j < 12; j++) R[0][j] = j == 0;
    for (int k = 0; k < 22; k++)
        for (int j = 0; j < 12; j++) {
            u64 a = 0;
            if (j >= 1) for (int i = 0; i < 12; i++) a = fadd(a, fmul(R[k][i], M[i][j]));
            R[k + 1][j] = a;
        }
    for (int d = 0; d < 22; d++) { u64 a = 0; for (int i = 0; i < 12; i++) a = fadd(a, fmul(R[d][i], M[i][0])); G[d] = a; }
    for (int i = 0; i < 12; i++) Q[0][i] = M[i][0] % gl::P;
    for (int d = 0; d + 1 < 22; d++)
        for (int i = 0; i < 12; i++) { u64 a = 0; for (int j = 1; j < 12; j++) a = fadd(a, fmul(M[i][j], Q[d][j])); Q[d + 1][i] = a; }
    for (int i = 0; i < 12; i++) for (int j = 0; j < 12; j++) NP[i][j] = i == j;
    for (int it = 0; it < 22; it++) {
        u64 T[12][12];
        for (int i = 0; i < 12; i++) for (int e = 0; e < 12; e++) { u64 a = 0; for (int j = 1; j < 12; j++) a = fadd(a, fmul(M[i][j], NP[j][e])); T[i][e] = a; }
        memcpy(NP, T, sizeof T);
    }
    // additive parts: acc_k = what the constants of rounds < k have put into the state before round k (acc_0 = 0,
    // acc_{k+1} = N (acc_k + rc_k)); round k's S-box input carries acc_k[0] + rc_k[0], the final state acc_22 + after
    static u64 accv[23][12];
    memset(accv, 0, sizeof accv);
    for (int k = 0; k < 22; k++)
        for (int i = 0; i < 12; i++) { u64 a = 0; for (int j = 1; j < 12; j++) a = fadd(a, fmul(M[i][j], fadd(accv[k][j], L.rc[k][j] % gl::P))); accv[k + 1][i] = a; }
    memset(tab, 0, TABLE_BYTES);
    for (int g = 0; g < N_GROUP; g++) {
        Rows rw{};
        for (int o = 0; o < 4; o++) {
            const int k = 4 * g + o;
            if (k >= 22) continue;                            // the last group has two rounds
            for (int e = 0; e < 12; e++) { u64 a = 0; for (int i = 0; i < 12; i++) a = fadd(a, fmul(R[k][i], L.pre[i][e])); rw.w[o][e] = a; }   // (e0^T N^k) pre
            for (int j = 0; j < 4 * g; j++) rw.w[o][12 + j] = G[k - 1 - j];
            rw.addc[o] = fadd(accv[k][0], L.rc[k][0] % gl::P);
        }
        fold_digit_bias(rw);
        if (!fill_tiles(rw, group_steps(g), tab + (size_t)group_base(g) * 1024, tab + CINIT_OFF + g * 128)) return false;
    }
    for (int f = 0; f < N_FIN; f++) {
        Rows rw{};
        for (int o = 0; o < 4; o++) {
            const int i = 4 * f + o;
            for (int e = 0; e < 12; e++) { u64 a = 0; for (int j = 0; j < 12; j++) a = fadd(a, fmul(NP[i][j], L.pre[j][e])); rw.w[o][e] = a; }   // N^22 pre
            for (int j = 0; j < 22; j++) rw.w[o][12 + j] = Q[21 - j][i];
            rw.addc[o] = fadd(accv[22][i], L.after[i] % gl::P);
        }
        fold_digit_bias(rw);
        if (!fill_tiles(rw, FIN_STEPS, tab + (size_t)(N_GROUP_TILES + f * FIN_STEPS) * 1024, tab + CINIT_OFF + (N_GROUP + f) * 128)) return false;
    }
    memcpy(tab + G_OFF, G, 3 * sizeof(u64));                  // the running group's coefficients (Poseidon: 25, 5 017, 1 259 209)
    return true;
}
// plonky2's Poseidon; rc: the 360-entry table poseidon::permute takes (host_hash_round_constants layout)
inline bool build_tables(const u64 *rc, unsigned char *tab) {
    static Linear L;
    memset(&L, 0, sizeof L);
    for (int r = 0; r < 12; r++) for (int j = 0; j < 12; j++) L.M[r][j] = L.pre[r][j] = mds_entry(r, j);
    for (int k = 0; k < 22; k++) L.rc[k][0] = rc[(4 + k) * 12];
    for (int i = 1; i < 12; i++) L.rc[0][i] = rc[4 * 12 + i];
    for (int i = 0; i < 12; i++) L.after[i] = rc[26 * 12 + i];
    if (!build_tables(L, tab)) return false;
    u64 g[3]; memcpy(g, tab + G_OFF, sizeof g);
    return g[0] == G0 && g[1] == G1 && g[2] == G2;            // the device code has them as immediates
}
// plonky2's PoseidonGate (quotient kernel): the same matrices with the PLAIN round constants (ALL_ROUND_CONSTANTS: twelve lanes in
// every partial round), as the gate's constraints are written against the textbook schedule; rcp: poseidon::host_round_constants()
inline bool build_tables_gate(const u64 *rcp, unsigned char *tab) {
    static Linear L;
    memset(&L, 0, sizeof L);
    for (int r = 0; r < 12; r++) for (int j = 0; j < 12; j++) L.M[r][j] = L.pre[r][j] = mds_entry(r, j);
    for (int k = 0; k < 22; k++) for (int i = 0; i < 12; i++) L.rc[k][i] = rcp[(4 + k) * 12 + i];
    for (int i = 0; i < 12; i++) L.after[i] = rcp[26 * 12 + i];
    return build_tables(L, tab);
}
// qp-poseidon-core's Poseidon2 (poseidon2::permute_qp): internal layer J + diag, the external layer before it folded in; both
// matrices are read off the layer functions themselves (columns = images of the unit vectors)
inline bool build_tables_p2(const poseidon2::Params &p, unsigned char *tab) {
    static Linear L;
    memset(&L, 0, sizeof L);
    for (int j = 0; j < 12; j++) {
        u64 e[12] = {}, f[12] = {};
        e[j] = f[j] = 1;
        poseidon2::int_layer(e, p); poseidon2::ext_layer_qp(f);
        for (int i = 0; i < 12; i++) { L.M[i][j] = gl::canon(e[i]); L.pre[i][j] = gl::canon(f[i]); }
    }
    for (int k = 0; k < 22; k++) L.rc[k][0] = p.rc_int[k];
    for (int i = 0; i < 12; i++) L.after[i] = p.rc_ext[4 * 12 + i];
    return build_tables(L, tab);
}
// the largest limb any chain of a finished table can produce (chain_limb_max over every chain the device runs)
inline u64 table_limb_max(const unsigned char *tab) {
    u64 worst = 0;
    for (int g = 0; g < N_GROUP; g++) {
        const u64 m = chain_limb_max(tab + (size_t)group_base(g) * 1024, tab + CINIT_OFF + g * 128, group_steps(g));
        if (m > worst) worst = m;
    }
    for (int f = 0; f < N_FIN; f++) {
        const u64 m = chain_limb_max(tab + (size_t)(N_GROUP_TILES + f * FIN_STEPS) * 1024, tab + CINIT_OFF + (N_GROUP + f) * 128, FIN_STEPS);
        if (m > worst) worst = m;
    }
    return worst;
}
// what one MFMA chain computes for one column, from the table bytes (layout assumptions as the device code's)
inline bool emu_gemm(const unsigned char *tab, int tile0, int cidx, int steps, const u64 *D, u32 (&Z)[4][LIMBS]) {
    for (int o = 0; o < 4; o++)
        for (int limb = 0; limb < LIMBS; limb++) {
            const int row = row_of(o, limb);
            u32 c; memcpy(&c, tab + CINIT_OFF + cidx * 128 + (o >> 1) * 64 + (8 * (o & 1) + limb) * 4, 4);
            long long acc = c;
            for (int q = 0; q < steps; q++)
                for (int k = 0; k < 32; k++) {
                    const int lane = row + 32 * (k >> 4), j = k & 15;
                    const int a = (signed char)tab[(size_t)(tile0 + q) * 1024 + lane * 16 + j];
                    const int bdig = (signed char)(D[4 * q + (k >> 3)] >> (8 * (k & 7)));
                    acc += (long long)a * bdig;
                }
            if (acc < 0 || acc > (long long)LIMB_MAX) return false;
            Z[o][limb] = (u32)acc;
        }
    return true;
}
// the partial-round block as the device runs it: s = S-box outputs of the full round before -> the state the S-box layer of the
// full round behind applies to
inline bool emu_partial_rounds(u64 (&s)[12], const unsigned char *tab) {
    u64 D[N_ELEM] = {}, y[24], G[3];
    memcpy(G, tab + G_OFF, sizeof G);
    const bool small = G[0] == G0 && G[1] == G1 && G[2] == G2;    // Poseidon's three small integers (the kernels have them as immediates)
    for (int e = 0; e < 12; e++) D[e] = to_digits(s[e]);
    for (int g = 0; g < N_GROUP; g++) {
        u32 Z[4][LIMBS];
        if (!emu_gemm(tab, group_base(g), g, group_steps(g), D, Z)) return false;
        for (int o = 0; o < 4 && 4 * g + o < 22; o++) {
            const int k = 4 * g + o;
            u64 x;
            if (small) {                                      // the device's SMALL_G schedule: unreduced terms, one reduction
                u64 lo; u32 top, gg[MAX_GROUP_TERMS];
                recombine_wide(Z[o], lo, top);
                for (int i = 0; i < o; i++) gg[i] = (u32)G[o - 1 - i];
                x = reduce96_terms(lo, top, y + 4 * g, gg, o);
            } else {
                x = recombine(Z[o]);
                for (int j = 4 * g; j < k; j++) x = gl::add(x, gl::mul(y[j], G[k - 1 - j]));
            }
            y[k] = poseidon::sbox7_lane(x);
        }
        for (int o = 0; o < 4 && 4 * g + o < 22; o++) D[12 + 4 * g + o] = to_digits(y[4 * g + o]);
    }
    for (int f = 0; f < N_FIN; f++) {
        u32 Z[4][LIMBS];
        if (!emu_gemm(tab, N_GROUP_TILES + f * FIN_STEPS, N_GROUP + f, FIN_STEPS, D, Z)) return false;
        for (int o = 0; o < 4; o++) s[4 * f + o] = recombine(Z[o]);
    }
    return true;
}
// textbook permutation (plain constants) through the gate table: what the PoseidonGate kernel's matrix form computes when every
// S-box input equals its wire (a satisfied row)
inline bool emu_permute_textbook(u64 (&s)[12], const u64 *rcp, const unsigned char *tab) {
    using namespace poseidon;
    int r = 0;
    for (int k = 0; k < HALF_FULL; k++, r++) {
        for (int i = 0; i < WIDTH; i++) s[i] = sbox7(gl::add_canonical(s[i], rcp[r * WIDTH + i]));
        if (k + 1 < HALF_FULL) mds_layer(s);
    }
    if (!emu_partial_rounds(s, tab)) return false;
    r += 1 + PARTIAL;
    for (int i = 0; i < WIDTH; i++) s[i] = sbox7(s[i]);
    mds_layer(s);
    for (int k = 1; k < HALF_FULL; k++, r++) {
        for (int i = 0; i < WIDTH; i++) s[i] = sbox7(gl::add_canonical(s[i], rcp[r * WIDTH + i]));
        mds_layer(s);
    }
    for (int i = 0; i < WIDTH; i++) s[i] = gl::canon(s[i]);
    return true;
}
inline bool emu_permute(u64 (&s)[12], const u64 *rc, const unsigned char *tab) {
    using namespace poseidon;
    int r = 0;
    for (int k = 0; k < HALF_FULL; k++, r++) {
        for (int i = 0; i < WIDTH; i++) s[i] = gl::add_canonical(s[i], rc[r * WIDTH + i]);
        sbox7_layer(s);
        if (k + 1 < HALF_FULL) mds_layer(s);          // the fourth round's MDS layer is part of the matrix
    }
    if (!emu_partial_rounds(s, tab)) return false;
    r += 1 + PARTIAL;
    sbox7_layer(s); mds_layer(s);
    for (int k = 1; k < HALF_FULL; k++, r++) {
        for (int i = 0; i < WIDTH; i++) s[i] = gl::add_canonical(s[i], rc[r * WIDTH + i]);
        sbox7_layer(s);
        mds_layer(s);
    }
    for (int i = 0; i < WIDTH; i++) s[i] = gl::canon(s[i]);
    return true;
}
inline bool emu_permute_p2(u64 (&s)[12], const poseidon2::Params &p, const unsigned char *tab) {
    poseidon2::ext_layer_qp(s);
    for (int r = 0; r < 4; r++) {
        for (int i = 0; i < 12; i++) s[i] = gl::add(s[i], p.rc_ext[r * 12 + i]);
        poseidon::sbox7_layer(s);
        if (r < 3) poseidon2::ext_layer_qp(s);        // the fourth round's external layer is part of the matrix
    }
    if (!emu_partial_rounds(s, tab)) return false;
    poseidon::sbox7_layer(s); poseidon2::ext_layer_qp(s);
    for (int r = 5; r < 8; r++) {
        for (int i = 0; i < 12; i++) s[i] = gl::add(s[i], p.rc_ext[r * 12 + i]);
        poseidon::sbox7_layer(s);
        poseidon2::ext_layer_qp(s);
    }
    for (int i = 0; i < 12; i++) s[i] = gl::canon(s[i]);
    return true;
}
template <class F, class Gf>
inline bool selfcheck_with(F plain, Gf emu, int n) {
    u64 seed = 0x243F6A8885A308D3ull;
    for (int t = 0; t < n; t++) {
        u64 a[12], b[12];
        for (int i = 0; i < 12; i++) {
            seed = seed * 6364136223846793005ull + 1442695040888963407ull;
            u64 v = seed ^ (seed >> 29);
            if (t % 7 == 0) v = (i & 1) ? ~0ull - (v & 0xFF) : (v & 0xFF);            // extremes: near 0 and near 2^64
            if (t % 11 == 0) v = gl::P - 1 - (v & 3);
            a[i] = b[i] = v;
        }
        plain(a);
        if (!emu(b)) return false;
        for (int i = 0; i < 12; i++) if (a[i] != b[i]) return false;
    }
    return true;
}
inline bool selfcheck(const u64 *rc, const unsigned char *tab, int n = 2000) {
    return selfcheck_with([&](u64 (&s)[12]) { poseidon::permute(s, rc); }, [&](u64 (&s)[12]) { return emu_permute(s, rc, tab); }, n);
}
inline bool selfcheck_gate(const u64 *rcp, const unsigned char *tab, int n = 2000) {
    return selfcheck_with([&](u64 (&s)[12]) { for (int i = 0; i < 12; i++) s[i] = gl::canon(s[i]); poseidon::permute_textbook(s, rcp); },
                          [&](u64 (&s)[12]) { for (int i = 0; i < 12; i++) s[i] = gl::canon(s[i]); return emu_permute_textbook(s, rcp, tab); }, n);
}
inline bool selfcheck_p2(const poseidon2::Params &p, const unsigned char *tab, int n = 2000) {
    return selfcheck_with([&](u64 (&s)[12]) { poseidon2::permute_qp(s, p); }, [&](u64 (&s)[12]) { return emu_permute_p2(s, p, tab); }, n);
}
}  // namespace host
inline bool build_tables(const u64 *rc, unsigned char *tab) { return host::build_tables(rc, tab); }
inline bool host_selfcheck(const u64 *rc, const unsigned char *tab, int n = 2000) { return host::selfcheck(rc, tab, n); }
inline bool build_tables_gate(const u64 *rcp, unsigned char *tab) { return host::build_tables_gate(rcp, tab); }
inline bool host_selfcheck_gate(const u64 *rcp, const unsigned char *tab, int n = 2000) { return host::selfcheck_gate(rcp, tab, n); }
inline bool build_tables_p2(const poseidon2::Params &p, unsigned char *tab) { return host::build_tables_p2(p, tab); }
inline bool host_selfcheck_p2(const poseidon2::Params &p, const unsigned char *tab, int n = 2000) { return host::selfcheck_p2(p, tab, n); }
#else
bool build_tables(const u64 *, unsigned char *);          // host functions: declared only in the device pass
bool host_selfcheck(const u64 *, const unsigned char *, int n = 2000);
bool build_tables_p2(const poseidon2::Params &, unsigned char *);
bool build_tables_gate(const u64 *, unsigned char *);
bool host_selfcheck_gate(const u64 *, const unsigned char *, int n = 2000);
bool host_selfcheck_p2(const poseidon2::Params &, const unsigned char *, int n = 2000);
#endif

#if defined(__HIP_DEVICE_COMPILE__)
// ---- device ----
__device__ __forceinline__ void swap32(u32 &x, u32 &y) {     // lanes 32..63 of x <-> lanes 0..31 of y
    auto r = __builtin_amdgcn_permlane32_swap(x, y, false, false);
    x = r[0]; y = r[1];
}
struct Run {
    u32 Dlo[N_ELEM], Dhi[N_ELEM];     // digits, natural layout until their K-step is formed
    v4i B0[FIN_STEPS], B1[FIN_STEPS];  // B operands of the columns of lanes 0..31 / 32..63
    u64 y[24];
    u64 Gd[3];                         // the running group's coefficients when they are not Poseidon's three small integers
    const unsigned char *lds;
};
__device__ __forceinline__ void form_step(Run &st, int q) {
    swap32(st.Dlo[4 * q], st.Dlo[4 * q + 2]); swap32(st.Dhi[4 * q], st.Dhi[4 * q + 2]);
    swap32(st.Dlo[4 * q + 1], st.Dlo[4 * q + 3]); swap32(st.Dhi[4 * q + 1], st.Dhi[4 * q + 3]);
    st.B0[q] = v4i{(int)st.Dlo[4 * q], (int)st.Dhi[4 * q], (int)st.Dlo[4 * q + 1], (int)st.Dhi[4 * q + 1]};
    st.B1[q] = v4i{(int)st.Dlo[4 * q + 2], (int)st.Dhi[4 * q + 2], (int)st.Dlo[4 * q + 3], (int)st.Dhi[4 * q + 3]};
}
// one tile: Z[o] = the 8 limbs of output o for this lane's column
template <int STEPS>
__device__ __forceinline__ void gemm(const Run &st, int tile0, int cidx, u32 (&Z)[4][LIMBS]) {
    const int lane = threadIdx.x & 63;
    const v4i *cp = (const v4i *)(st.lds + CINIT_OFF + cidx * 128 + (lane >> 5) * 64);
    v16i a0, a1;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const v4i c = cp[i];
        a0[4 * i] = c[0]; a0[4 * i + 1] = c[1]; a0[4 * i + 2] = c[2]; a0[4 * i + 3] = c[3];
    }
    a1 = a0;
    const v4i *ap = (const v4i *)(st.lds + (size_t)tile0 * 1024) + lane;
#pragma unroll
    for (int q = 0; q < STEPS; q++) {
        const v4i a = ap[q * 64];
        a0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, st.B0[q], a0, 0, 0, 0);
        a1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, st.B1[q], a1, 0, 0, 0);
    }
#ifndef PMF_NO_KEEPALIVE   // (defined only by tools/mfma_hazard_check.py --first-layout, to show what the compiler does without it)
    asm volatile("" : "+v"(a0), "+v"(a1));    // both destinations stay allocated as a whole until the chain has been issued
#endif
#pragma unroll
    for (int i = 0; i < 16; i++) {
        u32 x = (u32)a0[i], yv = (u32)a1[i];
        swap32(x, yv);
        Z[i >> 3][i & 7] = x; Z[2 + (i >> 3)][i & 7] = yv;
    }
}
// what a round does with its S-box input: the permutation sends it through the S-box; a gate's quotient kernel compares it with
// the wire that holds it and sends the WIRE through (poseidon quotient kernels)
struct SboxOfInput { __device__ __forceinline__ u64 operator()(int, u64 x) const { return poseidon::sbox7_lane(x); } };
template <int G, bool SMALL_G, class F>
__device__ __forceinline__ void group_step(Run &st, F &f) {
    u32 Z[4][LIMBS];
    gemm<group_steps(G)>(st, group_base(G), G, Z);
    constexpr int n = 4 * G + 4 <= 22 ? 4 : 22 - 4 * G;
#pragma unroll
    for (int o = 0; o < n; o++) {
        const int k = 4 * G + o;
        u64 x;
        if constexpr (SMALL_G) {
            constexpr u32 Gc[3] = {G0, G1, G2};
            u64 lo, yy[MAX_GROUP_TERMS] = {};
            u32 top, gg[MAX_GROUP_TERMS] = {};
            recombine_wide(Z[o], lo, top);
#pragma unroll
            for (int i = 0; i < o; i++) { yy[i] = st.y[4 * G + i]; gg[i] = Gc[o - 1 - i]; }
            x = reduce96_terms(lo, top, yy, gg, o);
        } else {
            x = recombine(Z[o]);
#pragma unroll
            for (int j = 4 * G; j < k; j++) x = gl::add(x, gl::mul(st.y[j], st.Gd[k - 1 - j]));
        }
        st.y[k] = f(k, x);
    }
#pragma unroll
    for (int o = 0; o < n; o++) {
        const u64 t = to_digits(st.y[4 * G + o]);
        st.Dlo[12 + 4 * G + o] = (u32)t; st.Dhi[12 + 4 * G + o] = (u32)(t >> 32);
    }
    form_step(st, 3 + G);
}
template <bool SMALL_G, class F, int... G>
__device__ __forceinline__ void all_groups(Run &st, F &f, std::integer_sequence<int, G...>) { (group_step<G, SMALL_G>(st, f), ...); }

// s: the S-box outputs of the fourth full round (its MDS layer is part of the matrix) -> the state the S-box layer of the first
// closing full round applies to (that round's constants are already in)
template <bool SMALL_G, class F>
__device__ __forceinline__ void partial_rounds(u64 (&s)[12], const unsigned char *lds, F &f) {
    Run st;
    st.lds = lds;
    if (!SMALL_G) {
#pragma unroll
        for (int d = 0; d < 3; d++) {      // wave-uniform: scalar registers
            const u64 g = *(const u64 *)(lds + G_OFF + 8 * d);
            st.Gd[d] = ((u64)(u32)__builtin_amdgcn_readfirstlane((int)(g >> 32)) << 32) | (u32)__builtin_amdgcn_readfirstlane((int)(u32)g);
        }
    }
#pragma unroll
    for (int e = 0; e < N_ELEM; e++) {
        const u64 t = e < 12 ? to_digits(s[e]) : 0;
        st.Dlo[e] = (u32)t; st.Dhi[e] = (u32)(t >> 32);
    }
    form_step(st, 0); form_step(st, 1); form_step(st, 2);
    all_groups<SMALL_G>(st, f, std::make_integer_sequence<int, N_GROUP>{});
#pragma unroll
    for (int f = 0; f < N_FIN; f++) {
        u32 Z[4][LIMBS];
        gemm<FIN_STEPS>(st, N_GROUP_TILES + f * FIN_STEPS, N_GROUP + f, Z);
#pragma unroll
        for (int o = 0; o < 4; o++) s[4 * f + o] = recombine(Z[o]);
    }
}
// poseidon::permute with the partial rounds on the matrix pipe, in two halves so that a caller can place loads between them (the
// closing full rounds need the fewest registers). Every lane of the wave must be here (MFMA and the lane swaps ignore or need the
// whole wave); lds: the table of build_tables, 16-byte aligned.
__device__ __forceinline__ void permute_head(u64 (&s)[12], const u64 *rc, const unsigned char *lds) {
    using namespace poseidon;
#pragma unroll
    for (int i = 0; i < WIDTH; i++) s[i] = gl::add_canonical(s[i], rc[i]);
    for (int k = 0; k < HALF_FULL; k++) {          // a round's layer brings the next round's constants (the fourth round's layer is part of the matrix)
        sbox7_layer(s);
        if (k + 1 < HALF_FULL) mds_layer_words_rc(s, rc + (k + 1) * WIDTH);
    }
    SboxOfInput f;
    partial_rounds<true>(s, lds, f);
}
// The four closing full rounds in two parts. permute_tail_rounds: three times [S-box layer, MDS layer, the next round's constants]
// and the last round's S-box layer. The last linear layer is the caller's: a sponge reads only a few rows of it (plonky2 overwrites
// the rate lanes with the next block, a digest is lanes 0..3, the proof of work reads lane 7), and mds_layer_rows joins and
// reduces only the rows it is asked for. permute_tail_rows<FIRST, COUNT, CANON> ends in rows [FIRST, FIRST + COUNT), canonical if
// they leave the kernel; the other lanes of s mean nothing afterwards. A loose row may feed the next permutation (its first
// step is add_canonical, exact for any 64-bit left operand).
__device__ __forceinline__ void permute_tail_rounds(u64 (&s)[12], const u64 *rc) {
    using namespace poseidon;
    int r = HALF_FULL + 1 + PARTIAL;
    for (int k = 1; k < HALF_FULL; k++, r++) {
        sbox7_layer(s);
        mds_layer_words_rc(s, rc + r * WIDTH);
    }
    sbox7_layer(s);
}
template <int FIRST, int COUNT, bool CANON>
__device__ __forceinline__ void last_layer_rows(u64 (&s)[12]) {
    poseidon::mds_layer_rows_words<FIRST, COUNT>(s);
    if (CANON) {
#pragma unroll
        for (int i = FIRST; i < FIRST + COUNT; i++) s[i] = gl::canon(s[i]);
    }
}
template <int FIRST, int COUNT, bool CANON>
__device__ __forceinline__ void permute_tail_rows(u64 (&s)[12], const u64 *rc) {
    permute_tail_rounds(s, rc);
    last_layer_rows<FIRST, COUNT, CANON>(s);
}
__device__ __forceinline__ void permute_tail(u64 (&s)[12], const u64 *rc) { permute_tail_rows<0, 12, true>(s, rc); }
__device__ __forceinline__ void permute(u64 (&s)[12], const u64 *rc, const unsigned char *lds) {
    permute_head(s, rc, lds);
    permute_tail(s, rc);
}
// poseidon2::permute_qp (qp-poseidon-core's parameter set) with the 22 internal rounds, the external layer before them and the
// constants of the external round behind them on the matrix pipe; lds: the table of build_tables_p2 for the same parameters
__device__ __forceinline__ void permute_p2qp(u64 (&s)[12], const poseidon2::Params &p, const unsigned char *lds) {
    poseidon2::ext_layer_qp(s);
    for (int r = 0; r < 4; r++) {
#pragma unroll
        for (int i = 0; i < 12; i++) s[i] = gl::add_canonical(s[i], p.rc_ext[r * 12 + i]);   // the block's constants are canonical (parse_p2, qp_params)
        poseidon::sbox7_layer(s);
        if (r < 3) poseidon2::ext_layer_qp(s);
    }
    SboxOfInput f;
    partial_rounds<false>(s, lds, f);
    poseidon::sbox7_layer(s);
    poseidon2::ext_layer_qp(s);
    for (int r = 5; r < 8; r++) {
#pragma unroll
        for (int i = 0; i < 12; i++) s[i] = gl::add_canonical(s[i], p.rc_ext[r * 12 + i]);   // the block's constants are canonical (parse_p2, qp_params)
        poseidon::sbox7_layer(s);
        poseidon2::ext_layer_qp(s);
    }
#pragma unroll
    for (int i = 0; i < 12; i++) s[i] = gl::canon(s[i]);
}
#elif defined(__HIPCC__)
__device__ void permute(u64 (&s)[12], const u64 *rc, const unsigned char *lds);   // host pass of a .hip unit: names only
__device__ void permute_head(u64 (&s)[12], const u64 *rc, const unsigned char *lds);
__device__ void permute_tail(u64 (&s)[12], const u64 *rc);
__device__ void permute_tail_rounds(u64 (&s)[12], const u64 *rc);
template <int FIRST, int COUNT, bool CANON> __device__ void last_layer_rows(u64 (&)[12]) {}
template <int FIRST, int COUNT, bool CANON> __device__ void permute_tail_rows(u64 (&)[12], const u64 *) {}
__device__ void permute_p2qp(u64 (&s)[12], const poseidon2::Params &p, const unsigned char *lds);
template <bool SMALL_G, class F> __device__ void partial_rounds(u64 (&)[12], const unsigned char *, F &) {}   // body: device pass only
#endif

}  // namespace pmf
