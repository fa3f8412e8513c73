// proof_layout.hpp — the byte layout of a proof, the only place that knows it. Host only.
//
// A proof of a circuit is ProofWithPublicInputs::to_bytes (qp-plonky2 1.5.5 util::serialization), little-endian u64 words:
//   1. three Merkle caps (wires, Zs / partial products, quotient), 2^cap_height digests each
//   2. the openings, extension elements: constants, plonk_sigmas, wires, plonk_zs, plonk_zs_next, partial_products, quotient_polys
//      (the lookup vectors are empty)
//   3. one cap per FRI round
//   4. num_query_rounds query rounds: an opening of each initial oracle, then one per FRI round; an opening is the row, a
//      one-byte sibling count and the siblings (write_merkle_proof)
//   5. the final polynomial, 6. the proof-of-work witness, 7. the public inputs
// 3..6 are the FriProof (write_fri_proof): the stage-level ABI builds it over any list of oracles, so it has a layer of its own.
#pragma once
#include <vector>
#include "circuit.hpp"
#include "gl64.hpp"

namespace proof_layout {

// Proof bytes, read in order. A read past the end sets `bad`, yields 0 and leaves nothing more to read; a word that is not
// below the field order sets `noncanonical` (Field::from_canonical_u64 on read: a proof carries canonical elements only).
struct Reader {
    const uint8_t *p; size_t len, pos = 0; bool bad = false, noncanonical = false;
    uint64_t word() {
        if (pos + 8 > len) { bad = true; pos = len; return 0; }
        uint64_t v; std::memcpy(&v, p + pos, 8); pos += 8;
        if (v >= gl::P) noncanonical = true;
        return v;
    }
    uint8_t byte() { if (pos + 1 > len) { bad = true; return 0; } return p[pos++]; }
    void vec(uint64_t *out, size_t n) { for (size_t i = 0; i < n; i++) out[i] = word(); }
};

// one Merkle opening of a query round
struct Opening {
    size_t row_words;   // the opened row (an initial oracle's leaf, salt included; a FRI round's coset of 2^arity extension values)
    size_t path_len;    // siblings: log2 leaves - cap_height
    size_t off;         // byte offset of the row from the start of its query round
    size_t shift;       // leaf index = x_index >> shift
};

struct Fri {
    size_t n_initial = 0, num_query_rounds = 0, cap_bytes = 0;
    std::vector<Opening> op;            // the initial oracles, then the FRI rounds
    size_t round_bytes = 0;             // one query round
    size_t final_len = 0;               // coefficients of the final polynomial (extension elements)
    size_t total = 0;                   // caps, query rounds, final polynomial, proof-of-work witness
    size_t n_rounds() const { return op.size() - n_initial; }
    size_t queries_bytes() const { return num_query_rounds * round_bytes; }
};

// leaf_widths: words of a leaf of every initial oracle, salt included
inline Fri fri_part(size_t degree_bits, size_t rate_bits, size_t cap_height, const std::vector<uint64_t> &arity_bits,
                    size_t num_query_rounds, const std::vector<size_t> &leaf_widths) {
    Fri f;
    f.n_initial = leaf_widths.size(); f.num_query_rounds = num_query_rounds; f.cap_bytes = ((size_t)1 << cap_height) * 32;
    size_t lvl = degree_bits + rate_bits, fin = degree_bits, shift = 0, off = 0;
    auto add = [&](size_t row_words) {
        f.op.push_back({row_words, lvl - cap_height, off, shift});
        off += row_words * 8 + 1 + (lvl - cap_height) * 32;
    };
    for (size_t w : leaf_widths) add(w);
    for (uint64_t ab : arity_bits) { lvl -= ab; fin -= ab; shift += ab; add((size_t)2 << ab); }
    f.round_bytes = off;
    f.final_len = (size_t)1 << fin;
    f.total = arity_bits.size() * f.cap_bytes + f.queries_bytes() + f.final_len * 16 + 8;
    return f;
}

struct Vec { size_t pos, count; };      // byte offset in the proof, extension elements

struct Proof {
    size_t cap_bytes = 0;
    Vec openings[7] = {};               // in byte order: constants, sigmas, wires, zs, zs_next, partial products, quotient
    size_t widths[4] = {}, polys[4] = {};   // constants/sigmas, wires, Zs / partial products, quotient: leaf words, opened polynomials
    Fri fri;
    size_t fri_caps_pos = 0, queries_pos = 0, final_pos = 0, pow_pos = 0, pis_pos = 0, total = 0;
};

inline Proof of(const CircuitPack &c) {
    Proof p;
    const size_t nch = c.num_challenges, salt = c.zero_knowledge ? 4 : 0;   // a blinded oracle's leaves end in four salt words
    const size_t polys[4] = {c.num_cs_cols(), c.num_wires, c.num_zs_pp_cols(), c.num_quotient_cols()};
    for (int o = 0; o < 4; o++) { p.polys[o] = polys[o]; p.widths[o] = polys[o] + (o ? salt : 0); }
    p.fri = fri_part(c.degree_bits, c.rate_bits, c.cap_height, c.arity_bits, c.num_query_rounds, std::vector<size_t>(p.widths, p.widths + 4));
    p.cap_bytes = p.fri.cap_bytes;
    const size_t counts[7] = {c.num_selectors + c.num_constants, c.num_routed_wires, c.num_wires, nch, nch, nch * c.num_partial_products, c.num_quotient_cols()};
    size_t pos = 3 * p.cap_bytes;
    for (int i = 0; i < 7; i++) { p.openings[i] = {pos, counts[i]}; pos += counts[i] * 16; }
    p.fri_caps_pos = pos;
    p.queries_pos = p.fri_caps_pos + p.fri.n_rounds() * p.cap_bytes;
    p.final_pos = p.queries_pos + p.fri.queries_bytes();
    p.pow_pos = p.final_pos + p.fri.final_len * 16;
    p.pis_pos = p.pow_pos + 8;
    p.total = p.pis_pos + c.num_public_inputs * 8;
    return p;
}

}  // namespace proof_layout
