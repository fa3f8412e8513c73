// verify_dev.hpp — device functions the two query-round units share (verify_kernels.hip: the Plonk proof layout;
// fri_verify_kernels.hip: any FRI instance): unaligned word loads from proof bytes, hash_or_noop of an opened row, the climb of a
// Merkle path, the coset interpolation at beta and the final polynomial's value. Included inside the unit's namespace, after
// its permutation plugs (merkle_hash_impl.hpp with MERKLE_HASH_PLUGS_ONLY). Proof bytes are read in place: a one-byte path
// length precedes every path, so most words of a query round are not 8-byte aligned; words are assembled from the two aligned
// words they straddle (each proof starts on a word and is followed by a word of padding).

// the little-endian word at byte offset `off` of a word array
__device__ __forceinline__ u64 ld(const u64 *w, u32 off) {
    const u64 *p = w + (off >> 3);
    const u32 sh = (off & 7) * 8;
    const u64 lo = p[0], hi = p[1];
    return sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
}
__device__ __forceinline__ e2 ld_ext(const u64 *w, u32 off) { return gl::e2_make(ld(w, off), ld(w, off + 8)); }
__device__ __forceinline__ e2 rec_ext(const u64 *rec, u32 i) { return gl::e2_make(rec[i], rec[i + 1]); }
__device__ __forceinline__ bool same(e2 x, e2 y) { x = gl::e2_canon(x); y = gl::e2_canon(y); return x.a == y.a && x.b == y.b; }
__device__ __forceinline__ u32 bitrev(u32 x, u32 bits) { return __brev(x) >> (32 - bits); }

// hash_or_noop of the `width` words at byte offset `row`: the digest in s[0..3]
template <class Perm>
__device__ __forceinline__ void hash_row(u64 (&s)[12], const u64 *pw, u32 row, u32 width, const poseidon2::Params *p2) {
#pragma unroll
    for (int i = 0; i < 12; i++) s[i] = 0;
    if (width <= 4) {                                           // a short row is its own digest
#pragma unroll
        for (u32 i = 0; i < 4; i++) s[i] = i < width ? ld(pw, row + 8 * i) : 0;
    } else {
        for (u32 c = 0; c < width; c += 8) {                    // hash_n_to_hash_no_pad: overwrite absorption, rate 8
#pragma unroll
            for (u32 i = 0; i < 8; i++)
                if (c + i < width) s[i] = ld(pw, row + 8 * (c + i));
            Perm::permute(s, p2);
        }
    }
}

// the digest in s[0..3] taken up `plen` levels through the siblings at byte offset `at`; index: the leaf's, the cap entry's on return
template <class Perm>
__device__ __forceinline__ void climb_path(u64 (&s)[12], const u64 *pw, u32 at, u32 plen, u64 &index, const poseidon2::Params *p2) {
    for (u32 l = 0; l < plen; l++, at += 32) {
        u64 sib[4];
#pragma unroll
        for (int i = 0; i < 4; i++) sib[i] = ld(pw, at + 8 * i);
        const bool right = index & 1;
#pragma unroll
        for (int i = 0; i < 4; i++) { const u64 cur = s[i]; s[i] = right ? sib[i] : cur; s[4 + i] = right ? cur : sib[i]; s[8 + i] = 0; }
        Perm::permute(s, p2);
        index >>= 1;
    }
}

// compute_evaluation: the coset's points x_i = start g^i carry the values ev[bitrev(i)] (2^ab extension values at byte offset
// `ev`); barycentric form
//   p(beta) = (beta^n - start^n) / (n start^n) * sum_i y_i x_i / (beta - x_i),  accumulated as one fraction num / den
__device__ __forceinline__ e2 coset_interpolate(const u64 *pw, u32 ev, u32 ab, u32 within, u64 subgroup_x, e2 beta) {
    const u32 arity = 1u << ab;
    const u64 g = gl::root_of_unity(ab);
    const u64 start = gl::mul(subgroup_x, gl::pow(g, arity - bitrev(within, ab)));
    e2 num = gl::e2_from(0), den = gl::e2_from(1), hit = gl::e2_from(0);
    bool at_point = false;
    u64 x = start;
    for (u32 i = 0; i < arity; i++, x = gl::mul(x, g)) {
        const e2 y = ld_ext(pw, ev + 16 * bitrev(i, ab));
        const e2 d = gl::e2_canon(gl::e2_sub(beta, gl::e2_from(x)));
        if (d.a == 0 && d.b == 0) { at_point = true; hit = y; continue; }
        num = gl::e2_add(gl::e2_mul(num, d), gl::e2_mul(gl::e2_scale(y, x), den));
        den = gl::e2_mul(den, d);
    }
    const u64 start_n = gl::pow(start, arity);
    e2 beta_n = beta;
    for (u32 i = 0; i < ab; i++) beta_n = gl::e2_mul(beta_n, beta_n);
    const e2 zb = gl::e2_sub(beta_n, gl::e2_from(start_n));
    const e2 val = gl::e2_scale(gl::e2_mul(gl::e2_mul(zb, num), gl::e2_inv(den)), gl::inv(gl::mul(start_n, arity)));
    return at_point ? hit : val;
}

// Horner value at x of the `n` extension coefficients at byte offset `off`
__device__ __forceinline__ e2 final_poly_at(const u64 *pw, u32 off, u32 n, u64 x) {
    e2 fe = gl::e2_from(0);
    const e2 sxe = gl::e2_from(x);
    for (u32 i = n; i-- > 0;) fe = gl::e2_add(gl::e2_mul(fe, sxe), ld_ext(pw, off + 16 * i));
    return fe;
}
