// ec_encode_kernels.h — the text interface behind a curve session (csrc/ec_encode_layout.h): lines of text <-> points.
//
// Encoding:  (k_textlines_records   encode_kernels.h, unchanged, with nbytes = L + 4: the records T of all components)
//            k_ec_encode_search     one lane per record: x = 256 T + c for the least counter c whose x^3 + a x + b is a nonzero
//                                   square -- the light, divergent part: two products, one squaring and one binary Jacobi symbol
//                                   per counter; a lane leaves at its first +1, a wave runs as long as its unluckiest lane
//            k_ec_encode_root       one lane per record: y = the smaller root of that value (f_sqrt) -- the heavy, uniform part,
//                                   ~bits(p) products once per record, every lane the same power when p = 3 mod 4
// Decoding:  (export_rows_launch    the point records x || y)
//            k_ec_textlines_fold    one lane per record: the ill-formedness tests on x, T into a compact record of L + 4 bytes
//            (k_textlines_lengths, k_jsonlines_offsets, k_textlines_emit: unchanged, with nbytes = L + 4)
// Records are component-major, as in encode_kernels.h; the two encoding kernels work on one component's array at a time.
#pragma once
#include "ec_encode_layout.h"
#include "encode_kernels.h"
#include "ec_kernels.h"

namespace vmn {

// v < 2 p -> v mod p, by one conditional subtraction
template <int S>
__device__ __forceinline__ void f_once_below_p(u32 (&v)[S], const ECDev& E) {
    u32 pp[S], d[S];
#pragma unroll
    for (int k = 0; k < S; ++k) pp[k] = E.p[k];
    const bool below = borrow_sweep<S>(d, v, pp, 0) != 0;
#pragma unroll
    for (int k = 0; k < S; ++k) v[k] = below ? v[k] : d[k];
}

// rows[r] = (x, rhs, one) for record r of one component: x = 256 T + c in Montgomery form, canonical, rhs = x^3 + a x + b
// likewise, for the least c in 0..255 with (rhs / p) = +1.  The row is Montgomery form times R = 2^(28 S), an even power of two,
// so the symbol of the row is the symbol of the value; a zero rhs has the symbol 0 and is passed over ("nonzero square").
// THE LOOP IS BOUNDED by encode::COUNTER_ROUNDS whatever the data: a lane that finds no counter -- chance 2^-256, each x being
// a nonzero square with chance ~1/2 independently enough; not reachable in a test -- names its line in *first_fail (atomicMin) and
// the host returns a format error and frees the arrays.  It cannot spin.  rec: records of tbytes = L + 4 bytes, 256 T < p.
template <int S, int NW, int KIND = EC_NIST>
__global__ void __launch_bounds__(BLOCK, ECfg<S>::MINW)
k_ec_encode_search(u32* __restrict__ rows, const uint8_t* __restrict__ rec, size_t n, u32 tbytes, ECDev E, u32* __restrict__ first_fail) {
    using C1 = Cfg<S, 1>;
    constexpr int ROW = ECfg<S>::ROW;
    const size_t r = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (r >= n) return;
    Lane<C1> ln(nullptr);
    u32 x[S], t[S], t2[S], rhs[S], one[S];
    limbs_from_be<C1, NW>(t, rec + r * tbytes, (long)tbytes, ln);
    // 256 T as an integer (below 2^(8 (L + 5)) < p: nothing leaves the top limb), then into Montgomery form by one product
#pragma unroll
    for (int k = S - 1; k >= 0; --k) t[k] = ((t[k] << 8) | (k ? t[k - 1] >> (LIMB_BITS - 8) : 0u)) & LIMB_MASK;
#pragma unroll
    for (int k = 0; k < S; ++k) {
        t2[k] = E.rr[k];
        one[k] = E.one[k];
    }
    f_mul<S, false, KIND>(x, t, t2, E);
    f_once_below_p<S>(x, E);
    bool found = false;
    for (unsigned c = 0; c < encode::COUNTER_ROUNDS && !found; ++c) {
        if (c) {
            f_add<S>(x, x, one);                           // both canonical: < 2 p
            f_once_below_p<S>(x, E);
        }
        f_sqr<S, false, KIND>(t, x, E);
        f_mul<S, false, KIND>(t2, t, x, E);                // x^3
#pragma unroll
        for (int k = 0; k < S; ++k) t[k] = E.b[k];
        f_add<S>(rhs, t2, t);
        if constexpr (KIND == EC_GENERAL) {
            if (!E.a_zero) {                               // (wave-uniform)
#pragma unroll
                for (int k = 0; k < S; ++k) t2[k] = E.a[k];
                f_mul<S, false, KIND>(t, t2, x, E);
                f_add<S>(rhs, rhs, t);                     // x^3 + a x + b
            }
        } else {
            f_small<S, 3>(t, x);
            f_sub<S>(rhs, rhs, t, E);                      // x^3 - 3x + b
        }
        f_canon<S, KIND>(rhs, rhs, E);
#pragma unroll
        for (int k = 0; k < S; ++k) {
            t[k] = rhs[k];
            t2[k] = E.p[k];
        }
        found = jacobi_symbol<S>(t, t2) == 1;
    }
    if (!found) atomicMin(first_fail, (u32)r);
    Pt<S> P;
#pragma unroll
    for (int k = 0; k < S; ++k) {
        P.X[k] = x[k];
        P.Y[k] = rhs[k];
        P.Z[k] = one[k];
    }
    P.inf = 0;
    pt_store<S>(rows + r * ROW, P);
}

// rows[r] = (x, rhs, one) -> the point (x, y, one), y the smaller root of rhs as integers (the choice of k_ec_random_points).
// z^2 = rhs is checked: a mismatch -- the search found no counter, or a defect of ours -- names the line in *first_fail and
// stores the point at infinity, never a point off the curve.  TS: the curve has p = 1 mod 4 (E.ts_s != 0; the host chooses, and
// builds that form for the 9-limb fields alone, where the library's only such primes are): without Tonelli-Shanks' constants
// beside the rest the kernel of 15 limbs spills no scalar register.
template <int S, int KIND = EC_NIST, bool TS = false>
__global__ void __launch_bounds__(BLOCK, ECfg<S>::MINW)
k_ec_encode_root(u32* __restrict__ rows, size_t n, ECDev E, u32* __restrict__ first_fail) {
    constexpr int ROW = ECfg<S>::ROW;
    const size_t r = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (r >= n) return;
    Pt<S> P;
    pt_load_normalised<S>(P, rows + r * ROW);             // Y holds rhs
    u32 z[S], t[S], zs[S], zn[S];
    if constexpr (TS) f_sqrt<S, KIND>(z, P.Y, E);          // p = 1 mod 4 (the 224-bit curves): Tonelli-Shanks, data-dependent loops
    else f_pow_words<S, KIND>(z, P.Y, E.pp14, E.pwords, E);    // p = 3 mod 4: the (p + 1) / 4 power alone, the same on every lane
    f_canon<S, KIND>(z, z, E);
    f_sqr<S, false, KIND>(t, z, E);
    f_canon<S, KIND>(t, t, E);                             // both sides canonical (the search stored rhs so): compared limb by limb
    u32 differ = 0, znz = 0;
#pragma unroll
    for (int k = 0; k < S; ++k) {
        differ |= t[k] ^ P.Y[k];
        znz |= z[k];
    }
    const bool ok = differ == 0 && znz != 0;
    // the smaller root: compare the standard representatives of z and p - z; the rows keep the Montgomery forms z and p - z
#pragma unroll
    for (int k = 0; k < S; ++k) t[k] = k == 0 ? 1u : 0u;
    f_mul<S, false, KIND>(zs, z, t, E);                    // z / R: standard representative, < 2p
    f_once_below_p<S>(zs, E);
#pragma unroll
    for (int k = 0; k < S; ++k) t[k] = E.p[k];
    borrow_sweep<S>(zn, t, zs, 0);                         // p - z  (z != 0: checked above)
    const bool neg_smaller = borrow_sweep<S>(zs, zn, zs, 0) != 0;      // p - z < z (a borrow chain: no indexed register array)
    borrow_sweep<S>(zn, t, z, 0);                          // the Montgomery form of p - z, canonical
#pragma unroll
    for (int k = 0; k < S; ++k) {
        P.Y[k] = neg_smaller ? zn[k] : z[k];
        P.Z[k] = E.one[k];
    }
    P.inf = 0;
    if (!ok) {
        atomicMin(first_fail, (u32)r);
        pt_set_inf<S>(P, E);
    }
    pt_store<S>(rows + r * ROW, P);
}

// trec[r] = T of point record r (x || y at stride 2 nbytes), plen[r] = its message length (encode::ILL_FORMED: none, reported
// in flags); trec has stride L + 4
__global__ void __launch_bounds__(BLOCK) k_ec_textlines_fold(uint8_t* __restrict__ trec, u32* __restrict__ plen, const uint8_t* __restrict__ rec,
                                                             size_t total, u32 nbytes, u32 L, u32* __restrict__ flags) {
    const size_t r = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (r >= total) return;
    const u32 len = encode::fold_point_record(trec + r * (L + encode::LENGTH_BYTES), rec + r * 2 * (size_t)nbytes, nbytes, L);
    plen[r] = len;
    if (len == encode::ILL_FORMED) atomicOr(flags, TEXTLINES_ILL_FORMED);
}

}  // namespace vmn
