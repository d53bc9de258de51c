// modp_kernels.h — gfx950 kernels over arrays of residues in M28 form (see mont28.h).
//
// Device array layout ("AoS"): element i occupies W consecutive 32-bit words at base + i*W, limb j
// (28 bits) in one word, padding words zero.  Elements are contiguous so that gathers / permutations /
// sharding by contiguous ranges move whole 16-byte-aligned rows.
//
// Two execution geometries, chosen by the modulus size (struct Cfg):
//   LPE = 1  one element per lane (moduli up to 2072 bits, S <= 74 limbs): the lane's multiplicand sits
//            in VGPRs, its multiplier is staged in LDS as lds[limb*256 + tid], the modulus limbs are
//            wave-uniform SGPRs.
//   LPE = 2  two lanes per element (3072-bit moduli, S = 110): a lane holds L = S/2 limbs and columns
//            (a + columns + modulus half = 4L = 220 VGPRs; one lane would need 330 > the 256
//            architectural VGPRs).  The lanes of a pair exchange the reduction factor and one column
//            per row through DPP (mont28.h / the generator).  In memory a lane's share is LW = 56
//            words (16-byte aligned), W = 2*LW.
//   LPE = 4  four lanes per element (4096-bit moduli, S = 148, L = 37: two lanes would need 4*74 = 296
//            VGPRs).  Same scheme inside a quad of lanes (quad_perm DPP); carries / borrows cross the
//            three lane boundaries by repeated sweeps.
//   LPE = 8 / 16  moduli up to 8192 / 16384 bits (S = 296 / 592, L = 37): half a DPP row resp. a whole one (row shifts
//            with bank masks); the same kernels, the columns relieved every 74 rows.  Built for completeness -- the
//            reference offers safe primes up to 15 424 bits and benchmarks with a 15 492-bit group -- not tuned.
#pragma once
#include "mont28.h"

namespace vmn {

constexpr int BLOCK = 256;   // threads per workgroup: 4 waves, one per SIMD

// "Wide" geometries for SMALL arrays (fewer elements than the chip has lanes at one element per lane): the same
// element rows -- same R, same words in memory -- are worked on by four lanes, so that a chain of dependent products is
// ~2.5 times shorter and four times as many waves are in flight.
//   Cfg<76, 4>   the wide form of Cfg<74, 1> (2048-bit moduli): four shares of 19 columns = 76 columns, the two above the 74
//                limbs are zero; a product still takes ROWS = 74 reduction rows, so R = 2^(28*74).
//   Cfg<112, 4>  the wide form of Cfg<110, 2> (3072-bit moduli): four shares of 28 columns, ROWS = 110.
// A wide geometry reads and writes the rows of its BASE geometry: limb g of the element is word
// (g / BASE_L) * BASE_LW + g % BASE_L of the row (BASE_L limbs per share of the base layout, BASE_LW words apart), the
// columns g >= ROWS exist in registers only.
//   Cfg<80, 8>   the widest form of Cfg<74, 1>, for the smallest arrays: eight shares of 10 columns, ROWS = 74.
__host__ __device__ constexpr int rows_for(int S, int LPE) {
    return ((S == 76 && LPE == 4) || (S == 80 && LPE == 8)) ? 74 : (S == 112 && LPE == 4) ? 110 : S;
}
__host__ __device__ constexpr int base_lpe_for(int S, int LPE) {
    return ((S == 76 && LPE == 4) || (S == 80 && LPE == 8)) ? 1 : (S == 112 && LPE == 4) ? 2 : LPE;
}

template <int S_, int LPE_>
struct Cfg {
    static constexpr int S = S_;                        // columns per element (limbs, plus the zero columns of a wide geometry)
    static constexpr int LPE = LPE_;                    // lanes per element
    static constexpr int L = S_ / LPE_;                 // limbs per lane
    static constexpr int ROWS = rows_for(S_, LPE_);     // reduction rows of a product: R = 2^(28 ROWS)
    static constexpr int BASE_LPE = base_lpe_for(S_, LPE_);
    static constexpr bool WIDE = BASE_LPE != LPE_;      // works on the rows of another geometry's layout
    static constexpr int BASE_L = ROWS / BASE_LPE;      // limbs per share of the memory layout
    static constexpr int BASE_LW = stride_for_limbs(BASE_L);
    static constexpr int LW = WIDE ? 0 : BASE_LW;       // words of one lane's share in memory (own layout only)
    static constexpr int W = BASE_LPE * BASE_LW;        // words per element in memory
    static constexpr int EPB = BLOCK / LPE_;            // elements per workgroup
    static constexpr int MINW = 2;                      // waves per SIMD the kernels are built for
    static constexpr int BITS = LIMB_BITS;              // bits per limb
    static_assert(S_ % LPE_ == 0 && ROWS % BASE_LPE == 0, "limbs must split evenly over the lanes of an element");
    // word of limb g (< ROWS) in the row
    static __host__ __device__ constexpr int word_of(int g) { return (g / BASE_L) * BASE_LW + g % BASE_L; }
};

// The geometry the two variable-base power kernels of Cfg<74, 1> work in (k_modpow, k_modpow_phased; no other kernel): one
// element per lane on 71 limbs of 29 bits, R' = 2^(29*71) = 2^2059 > 4N for every modulus of up to 2048 bits.  A product is
// 2 * 71^2 multiply-adds where 74 limbs of 28 bits take 2 * 74^2, and the kernels are bound by their instruction count.
// Only registers, the LDS column, the table rows and -- between the phases of the phased kernel -- the running value in out[]
// hold this form, 71 (stored: 72) of the 76 words of a row; arrays stay in M28 form.  A power enters with one product by
// c_in = R'^2 / R mod N (x R -> x R') and leaves with one by c_out = R mod N (y R' -> y R).
// SHORT: the same geometry on the short rows of mont28.h, for a modulus N = -1 mod 2^58 (the host decides per modulus and
// launches k_modpow<C, true> / k_modpow_phased<C, true>); form, constants and results are the same, only the rows differ.
template <bool SHORT_>
struct Cfg29T {
    static constexpr bool SHORT = SHORT_;               // the short rows of mont28.h: the kernel's nn[] holds the limbs of N''
    static constexpr int S = 71, LPE = 1, L = 71, ROWS = 71, BASE_LPE = 1;
    static constexpr bool WIDE = false;
    static constexpr int BASE_L = 71, BASE_LW = stride_for_limbs(71), LW = BASE_LW;
    static constexpr int W = Cfg<74, 1>::W;             // its rows are the rows of Cfg<74, 1>
    static constexpr int EPB = BLOCK, MINW = 2;
    static constexpr int BITS = 29;
    static __host__ __device__ constexpr int word_of(int g) { return g; }
    // the constants of a modulus in this form, rows of W words one after the other (the kernels' nmod argument: ROW_N, or ROW_NS
    // for the short rows -- N'' = (N + 1) >> 58, all zero where N is not -1 mod 2^58)
    static constexpr int ROW_N = 0, ROW_ONE = 1, ROW_CIN = 2, ROW_COUT = 3, ROW_NS = 4, CONST_ROWS = 5;
};
using Cfg29 = Cfg29T<false>;
using Cfg29S = Cfg29T<true>;
static_assert(Cfg29::LW <= Cfg29::W && 29 * Cfg29::S >= 2048 + 2, "71 limbs of 29 bits: a row of Cfg<74, 1>, R' > 4N");
// PowGeom<C, SHORT>::type: the geometry k_modpow<C, SHORT> and k_modpow_phased<C, SHORT> run in -- C itself, except for Cfg<74, 1>,
// the only one with short rows
template <class C, bool SHORT = false> struct PowGeom {
    static_assert(!SHORT, "short rows: Cfg<74, 1> only");
    using type = C;
};
template <bool SHORT> struct PowGeom<Cfg<74, 1>, SHORT> { using type = Cfg29T<SHORT>; };
template <class C> constexpr bool POW29 = !__is_same(typename PowGeom<C>::type, C);

// What a lane needs to know about its place: element slot in the workgroup, which half it holds, its
// LDS column (limb i of the element's multiplier is bl[i*EPB]).
template <class C>
struct Lane {
    int eslot;        // element slot within the workgroup
    int half;         // 0 .. LPE-1: which share of the element this lane holds
    u32 lowmask;      // LPE > 1: 0xffffffff on lane 0 of the element, 0 elsewhere
    u32 nottopmask;   // LPE > 1: 0xffffffff on every lane of the element but the last
    u32* bl;
    __device__ __forceinline__ explicit Lane(u32* lds) {
        eslot = threadIdx.x / C::LPE;
        half = threadIdx.x % C::LPE;
        lowmask = half == 0 ? 0xffffffffu : 0u;
        nottopmask = half == C::LPE - 1 ? 0u : 0xffffffffu;
        bl = lds + eslot;
    }
};

// Cross-lane moves inside an element (DPP; elements are aligned groups of 2, 4 or 8 lanes: quad_perm within a quad, row
// shifts with bank masks for the two quads of an 8-lane element -- bank k of a DPP row = its lanes 4k .. 4k+3).
// from_below: the value of lane h-1 (lane 0 gets its own / a neighbour's: mask with ~lowmask); from_top: the last lane's
// value on all lanes; or_all: OR over the element's lanes, on all lanes.
template <int LPE>
__device__ __forceinline__ u32 from_below(u32 x) { return lane_below<LPE>(x); }
// lower quads <- upper quads (row_shl:4 into banks 0, 2) resp. upper <- lower (row_shr:4 into banks 1, 3); other lanes keep old
__device__ __forceinline__ u32 quad_from_upper(u32 old, u32 x) { return (u32)__builtin_amdgcn_update_dpp((int)old, (int)x, 0x104, 0xf, 0x5, false); }
__device__ __forceinline__ u32 quad_from_lower(u32 old, u32 x) { return (u32)__builtin_amdgcn_update_dpp((int)old, (int)x, 0x114, 0xf, 0xA, false); }
// (sixteen lanes per element = a whole DPP row: one more step of each kind)
template <int LPE>
__device__ __forceinline__ u32 from_top(u32 x) {
    if constexpr (LPE == 2) return (u32)__builtin_amdgcn_mov_dpp((int)x, 0xF5, 0xf, 0xf, true);     // [1,1,3,3]
    else {
        u32 t = (u32)__builtin_amdgcn_mov_dpp((int)x, 0xFF, 0xf, 0xf, true);                        // [3,3,3,3]
        if constexpr (LPE == 8) t = quad_from_upper(t, t);
        if constexpr (LPE == 16) {
            t = (u32)__builtin_amdgcn_update_dpp((int)t, (int)t, 0x104, 0xf, 0x4, false);           // lanes 8-11 <- 12-15 (row_shl:4, bank 2)
            t = (u32)__builtin_amdgcn_update_dpp((int)t, (int)t, 0x108, 0xf, 0x3, false);           // lanes 0-7 <- 8-15 (row_shl:8, banks 0, 1)
        }
        return t;
    }
}
// the value of lane h+1 of the element (the last lane receives its own / a neighbour's: mask with nottopmask); lane 0's value on all lanes
template <int LPE>
__device__ __forceinline__ u32 from_above(u32 x) {
    if constexpr (LPE == 2) return (u32)__builtin_amdgcn_mov_dpp((int)x, 0xF5, 0xf, 0xf, true);     // [1,1,3,3]
    else if constexpr (LPE == 4) return (u32)__builtin_amdgcn_mov_dpp((int)x, 0xF9, 0xf, 0xf, true);   // [1,2,3,3]
    else return (u32)__builtin_amdgcn_update_dpp(0, (int)x, 0x101, 0xf, 0xf, true);                 // row_shl:1 (8 or 16 lanes)
}
template <int LPE>
__device__ __forceinline__ u32 from_lane0(u32 x) {
    if constexpr (LPE == 2) return (u32)__builtin_amdgcn_mov_dpp((int)x, 0xA0, 0xf, 0xf, true);     // [0,0,2,2]
    else {
        u32 t = (u32)__builtin_amdgcn_mov_dpp((int)x, 0x00, 0xf, 0xf, true);                        // [0,0,0,0]
        if constexpr (LPE == 8) t = quad_from_lower(t, t);
        if constexpr (LPE == 16) {
            t = (u32)__builtin_amdgcn_update_dpp((int)t, (int)t, 0x114, 0xf, 0x2, false);           // lanes 4-7 <- 0-3 (row_shr:4, bank 1)
            t = (u32)__builtin_amdgcn_update_dpp((int)t, (int)t, 0x118, 0xf, 0xC, false);           // lanes 8-15 <- 0-7 (row_shr:8, banks 2, 3)
        }
        return t;
    }
}
template <int LPE>
__device__ __forceinline__ u32 or_all(u32 x) {
    x |= (u32)__builtin_amdgcn_mov_dpp((int)x, 0xB1, 0xf, 0xf, true);                               // [1,0,3,2]
    if constexpr (LPE >= 4) x |= (u32)__builtin_amdgcn_mov_dpp((int)x, 0x4E, 0xf, 0xf, true);       // [2,3,0,1]
    if constexpr (LPE == 8) x |= quad_from_upper(0u, x) | quad_from_lower(0u, x);
    if constexpr (LPE == 16) {
        x |= (u32)__builtin_amdgcn_update_dpp(0, (int)x, 0x124, 0xf, 0xf, false);                   // row_ror:4
        x |= (u32)__builtin_amdgcn_update_dpp(0, (int)x, 0x128, 0xf, 0xf, false);                   // row_ror:8
    }
    return x;
}

// ---------------------------------------------------------------------------------------------
// element movement helpers
// ---------------------------------------------------------------------------------------------
template <class C>
__device__ __forceinline__ void load_elem(u32 (&a)[C::L], const u32* __restrict__ p, const Lane<C>& ln) {
    if constexpr (C::WIDE) {                            // shares cut across the base layout: dword loads by limb index
#pragma unroll
        for (int j = 0; j < C::L; ++j) {
            const int g = ln.half * C::L + j;
            a[j] = g < C::ROWS ? p[C::word_of(g)] : 0u;
        }
        return;
    }
    const uint4* q = reinterpret_cast<const uint4*>(p + ln.half * C::LW);
#pragma unroll
    for (int k = 0; k < C::LW / 4; ++k) {
        uint4 v = q[k];
        if (4 * k + 0 < C::L) a[4 * k + 0] = v.x;
        if (4 * k + 1 < C::L) a[4 * k + 1] = v.y;
        if (4 * k + 2 < C::L) a[4 * k + 2] = v.z;
        if (4 * k + 3 < C::L) a[4 * k + 3] = v.w;
    }
}
template <class C>
__device__ __forceinline__ void store_elem(u32* __restrict__ p, const u32 (&a)[C::L], const Lane<C>& ln) {
    if constexpr (C::WIDE) {                            // (the columns above the limbs are zero: value < 2N < 2^(28 ROWS))
#pragma unroll
        for (int j = 0; j < C::L; ++j) {
            const int g = ln.half * C::L + j;
            if (g < C::ROWS) p[C::word_of(g)] = a[j];
        }
        if (ln.half < C::BASE_LPE) {                    // the padding words of the base layout stay zero
#pragma unroll
            for (int k = C::BASE_L; k < C::BASE_LW; ++k) p[ln.half * C::BASE_LW + k] = 0u;
        }
        return;
    }
    uint4* q = reinterpret_cast<uint4*>(p + ln.half * C::LW);
#pragma unroll
    for (int k = 0; k < C::LW / 4; ++k) {
        uint4 v;
        v.x = 4 * k + 0 < C::L ? a[4 * k + 0] : 0;
        v.y = 4 * k + 1 < C::L ? a[4 * k + 1] : 0;
        v.z = 4 * k + 2 < C::L ? a[4 * k + 2] : 0;
        v.w = 4 * k + 3 < C::L ? a[4 * k + 3] : 0;
        q[k] = v;
    }
}
// global element -> the element's LDS column (multiplier operand); each lane moves its own share
template <class C>
__device__ __forceinline__ void load_elem_to_lds(const Lane<C>& ln, const u32* __restrict__ p) {
    u32* dst = ln.bl + ln.half * C::L * C::EPB;
    if constexpr (C::WIDE) {
#pragma unroll
        for (int j = 0; j < C::L; ++j) {
            const int g = ln.half * C::L + j;
            dst[j * C::EPB] = g < C::ROWS ? p[C::word_of(g)] : 0u;
        }
        return;
    }
    const uint4* q = reinterpret_cast<const uint4*>(p + ln.half * C::LW);
#pragma unroll
    for (int k = 0; k < C::LW / 4; ++k) {
        uint4 v = q[k];
        if (4 * k + 0 < C::L) dst[(4 * k + 0) * C::EPB] = v.x;
        if (4 * k + 1 < C::L) dst[(4 * k + 1) * C::EPB] = v.y;
        if (4 * k + 2 < C::L) dst[(4 * k + 2) * C::EPB] = v.z;
        if (4 * k + 3 < C::L) dst[(4 * k + 3) * C::EPB] = v.w;
    }
}
template <class C>
__device__ __forceinline__ void regs_to_lds(const Lane<C>& ln, const u32 (&a)[C::L]) {
    u32* dst = ln.bl + ln.half * C::L * C::EPB;
#pragma unroll
    for (int j = 0; j < C::L; ++j) dst[j * C::EPB] = a[j];
}
// a small constant element (value v < 2^28) into the LDS column: limb 0 = v, the rest 0
template <class C>
__device__ __forceinline__ void small_to_lds(const Lane<C>& ln, u32 v) {
    u32* dst = ln.bl + ln.half * C::L * C::EPB;
#pragma unroll
    for (int j = 0; j < C::L; ++j) dst[j * C::EPB] = (j == 0 && ln.half == 0) ? v : 0u;
}
// device constant (modulus-like layout) -> LDS column
template <class C>
__device__ __forceinline__ void const_to_lds(const Lane<C>& ln, const u32* __restrict__ c) {
    u32* dst = ln.bl + ln.half * C::L * C::EPB;
#pragma unroll
    for (int j = 0; j < C::L; ++j) {
        if constexpr (C::WIDE) {
            const int g = ln.half * C::L + j;
            dst[j * C::EPB] = g < C::ROWS ? c[C::word_of(g)] : 0u;
        } else {
            dst[j * C::EPB] = c[ln.half * C::LW + j];
        }
    }
}
// this lane's share of a constant in modulus layout.  LPE = 1: uniform address => scalar loads into SGPRs.
template <class C>
__device__ __forceinline__ void load_modulus(u32 (&n)[C::L], const u32* __restrict__ nmod, const Lane<C>& ln) {
#pragma unroll
    for (int j = 0; j < C::L; ++j) {
        if constexpr (C::WIDE) {
            const int g = ln.half * C::L + j;
            n[j] = g < C::ROWS ? nmod[C::word_of(g)] : 0u;
        } else {
            n[j] = C::LPE == 1 ? nmod[j] : nmod[ln.half * C::LW + j];
        }
    }
}

// ---------------------------------------------------------------------------------------------
// carry / borrow chains (within a lane, and across the two lanes of a pair)
// ---------------------------------------------------------------------------------------------
// out = limbs of sum_j v[j] 2^(28j) (+ carry-in), v[j] arbitrary 64-bit columns; returns the carry out
template <int L, int BITS = LIMB_BITS>
__device__ __forceinline__ u64 carry_sweep(u32 (&out)[L], const u64 (&v)[L], u64 cin) {
    u64 c = cin;
#pragma unroll
    for (int j = 0; j < L; ++j) {
        c += v[j];
        out[j] = (u32)c & ((1u << BITS) - 1);
        c >>= BITS;
    }
    return c;
}
// Resolve lazy columns into 28-bit limbs.  Several lanes per element: a lane's carry-out enters column 0 of the
// lane above; after sweep t the lanes 0..t are final (lane 0 repeats its sweep with carry 0 = same result), so
// LPE sweeps settle the element.
template <class C>
__device__ __forceinline__ void normalize(u32 (&out)[C::L], const u64 (&T)[C::L], const Lane<C>& ln) {
    u64 c = carry_sweep<C::L, C::BITS>(out, T, 0);
    if constexpr (C::LPE > 1) {
#pragma unroll
        for (int t = 1; t < C::LPE; ++t) {
            u32 lo = from_below<C::LPE>((u32)c) & ~ln.lowmask, hi = from_below<C::LPE>((u32)(c >> 32)) & ~ln.lowmask;
            c = carry_sweep<C::L>(out, T, ((u64)hi << 32) | lo);
        }
    }
}
// d = x - n (limbs, borrow-in bin = 0 / -1); returns borrow-out (0 / -1)
template <int L, int BITS = LIMB_BITS>
__device__ __forceinline__ int32_t borrow_sweep(u32 (&d)[L], const u32 (&x)[L], const u32 (&n)[L], int32_t bin) {
    int32_t borrow = bin;
#pragma unroll
    for (int j = 0; j < L; ++j) {
        int32_t v = (int32_t)x[j] - (int32_t)n[j] + borrow;      // limbs < 2^29: no int32 overflow
        d[j] = (u32)v & ((1u << BITS) - 1);
        borrow = v >> BITS;
    }
    return borrow;
}
// element-wide x - n: d and the final borrow (0: x >= n, -1: x < n), identical on all lanes of the element
template <class C>
__device__ __forceinline__ int32_t sub_full(u32 (&d)[C::L], const u32 (&x)[C::L], const u32 (&n)[C::L], const Lane<C>& ln) {
    int32_t b = borrow_sweep<C::L, C::BITS>(d, x, n, 0);
    if constexpr (C::LPE > 1) {
#pragma unroll
        for (int t = 1; t < C::LPE; ++t) {
            int32_t bin = (int32_t)(from_below<C::LPE>((u32)b) & ~ln.lowmask);
            b = borrow_sweep<C::L>(d, x, n, bin);
        }
        b = (int32_t)from_top<C::LPE>((u32)b);
    }
    return b;
}
// x (limbs, value < 2N) -> canonical x mod N (< N), branch-free
template <class C>
__device__ __forceinline__ void canonicalize(u32 (&x)[C::L], const u32 (&n)[C::L], const Lane<C>& ln) {
    u32 d[C::L];
    bool ge = sub_full<C>(d, x, n, ln) == 0;
#pragma unroll
    for (int j = 0; j < C::L; ++j) x[j] = ge ? d[j] : x[j];
}
// r = a + b mod N (a, b canonical).  32-bit sums (limbs < 2^28, so a[j] + b[j] + carry < 2^30): the 64-bit
// column sweep would double the live registers, which the pair geometry (modulus half in VGPRs) cannot afford.
template <class C>
__device__ __forceinline__ void mod_add(u32 (&r)[C::L], const u32 (&a)[C::L], const u32 (&b)[C::L], const u32 (&n)[C::L],
                                        const Lane<C>& ln) {
    // r may alias a or b: sums first (own registers), then the carry sweep(s), then r is written
    u32 s[C::L];
#pragma unroll
    for (int j = 0; j < C::L; ++j) s[j] = a[j] + b[j];
    u32 cin = 0;
    if constexpr (C::LPE > 1) {
#pragma unroll
        for (int t = 1; t < C::LPE; ++t) {              // carry into this lane, settled from lane 0 upwards
            u32 c = cin;
#pragma unroll
            for (int j = 0; j < C::L; ++j) c = (c + s[j]) >> LIMB_BITS;
            cin = from_below<C::LPE>(c) & ~ln.lowmask;
        }
    }
    u32 c = cin;
#pragma unroll
    for (int j = 0; j < C::L; ++j) {
        c += s[j];
        r[j] = c & LIMB_MASK;
        c >>= LIMB_BITS;
    }
    canonicalize<C>(r, n, ln);
}
// r = -a mod N
template <class C>
__device__ __forceinline__ void mod_neg(u32 (&r)[C::L], const u32 (&a)[C::L], const u32 (&n)[C::L], const Lane<C>& ln) {
    u32 d[C::L];
    sub_full<C>(d, n, a, ln);                    // N - a  (a < N)
    u32 nz = 0;
#pragma unroll
    for (int j = 0; j < C::L; ++j) nz |= a[j];
    if constexpr (C::LPE > 1) nz = or_all<C::LPE>(nz);
#pragma unroll
    for (int j = 0; j < C::L; ++j) r[j] = nz ? d[j] : 0u;
}

// r = a * (element's LDS column) / R mod N, limbs normalised, value < 2N
template <class C>
__device__ __forceinline__ void mont_mul(u32 (&r)[C::L], const u32 (&a)[C::L], const Lane<C>& ln, const u32 (&n)[C::L], u32 n0inv) {
    u64 T[C::L];
    if constexpr (C::BITS == 29) {
        mont29_mul_columns<C::L, C::SHORT>(T, a, ln.bl, C::EPB, n, n0inv);
    } else if constexpr (C::LPE == 1) {
        mont_mul_columns<C::L>(T, a, ln.bl, C::EPB, n, n0inv);
    } else {
        mont_mul_columns_lanes<C::L, C::LPE, C::ROWS>(T, a, ln.bl, C::EPB, n, n0inv, ln.lowmask, ln.nottopmask);
    }
    normalize<C>(r, T, ln);
}
// r = a^2 / R mod N.  SQR_FROM_LDS<C>: the element's LDS column must hold a copy of a (the row's own limb needs a dynamic
// index); the 29-bit rows are unrolled one by one and read it from a's registers -- they leave the column alone.  sqr_times asks;
// odd_power_table (never instantiated on Cfg29) writes the column anyway, its product reads it next.
template <class C> constexpr bool SQR_FROM_LDS = C::BITS != 29;
template <class C>
__device__ __forceinline__ void mont_sqr(u32 (&r)[C::L], const u32 (&a)[C::L], const Lane<C>& ln, const u32 (&n)[C::L], u32 n0inv) {
    u64 T[C::L];
    if constexpr (C::BITS == 29) {
        mont29_sqr_columns<C::L, C::SHORT>(T, a, n, n0inv);
    } else if constexpr (C::LPE == 1) {
        mont_sqr_columns<C::L>(T, a, ln.bl, C::EPB, n, n0inv);
    } else {
        mont_sqr_columns_lanes<C::L, C::LPE, C::ROWS>(T, a, ln.bl, C::EPB, n, n0inv, ln.lowmask, ln.nottopmask);
    }
    normalize<C>(r, T, ln);
}

// ---------------------------------------------------------------------------------------------
// radix conversion between packed 32-bit words (NW words, little-endian) and 28-bit limbs
// ---------------------------------------------------------------------------------------------
template <int S, int NW>
__device__ __forceinline__ void words_to_limbs(u32 (&l)[S], const u32 (&w)[NW]) {
#pragma unroll
    for (int j = 0; j < S; ++j) {
        const int bit = 28 * j, k = bit / 32, sh = bit % 32;
        u32 lo = k < NW ? w[k] : 0, hi = k + 1 < NW ? w[k + 1] : 0;
        u64 both = ((u64)hi << 32) | lo;
        l[j] = (u32)(both >> sh) & LIMB_MASK;
    }
}
template <int S, int NW>
__device__ __forceinline__ void limbs_to_words(u32 (&w)[NW], const u32 (&l)[S]) {
#pragma unroll
    for (int k = 0; k < NW; ++k) {
        const int bit = 32 * k, j = bit / 28, sh = bit % 28;      // word k starts inside limb j
        u64 acc = 0;
        if (j < S) acc = (u64)l[j] >> sh;
        if (j + 1 < S) acc |= (u64)l[j + 1] << (28 - sh);
        if (j + 2 < S) acc |= (u64)l[j + 2] << (56 - sh);
        w[k] = (u32)acc;
    }
}
// word k of the element whose S limbs sit in the LDS column (any lane of the element may ask for any word)
template <class C>
__device__ __forceinline__ u32 word_from_lds(const Lane<C>& ln, int k) {
    int bit = 32 * k, j = bit / 28, sh = bit % 28;
    u64 acc = 0;
    if (j < C::S) acc = (u64)ln.bl[j * C::EPB] >> sh;
    if (j + 1 < C::S) acc |= (u64)ln.bl[(j + 1) * C::EPB] << (28 - sh);
    if (j + 2 < C::S) acc |= (u64)ln.bl[(j + 2) * C::EPB] << (56 - sh);
    return (u32)acc;
}

// ---------------------------------------------------------------------------------------------
// import / export:  big-endian fixed-width bytes  <->  M28 form
// ---------------------------------------------------------------------------------------------
// Word k (little-endian significance) of a big-endian integer of nbytes bytes at p; bytes beyond
// the integer read as zero.  nbytes need not be a multiple of 4 (Java's BigInteger encoding of a
// 2048-bit modulus is 257 bytes wide): whole words use one unaligned 4-byte load.
__device__ __forceinline__ u32 load_be_word(const uint8_t* __restrict__ p, long nbytes, int k) {
    long off = nbytes - 4L * (k + 1);
    if (off >= 0) {
        u32 v;
        __builtin_memcpy(&v, p + off, 4);
        return __builtin_bswap32(v);
    }
    u32 v = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        long o = nbytes - 1 - (4L * k + b);
        if (o >= 0) v |= (u32)p[o] << (8 * b);
    }
    return v;
}
__device__ __forceinline__ void store_be_word(uint8_t* __restrict__ p, long nbytes, int k, u32 w) {
    long off = nbytes - 4L * (k + 1);
    if (off >= 0) {
        u32 v = __builtin_bswap32(w);
        __builtin_memcpy(p + off, &v, 4);
        return;
    }
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        long o = nbytes - 1 - (4L * k + b);
        if (o >= 0) p[o] = (uint8_t)(w >> (8 * b));
    }
}

// this lane's limbs of the big-endian integer at src
template <class C, int NW>
__device__ __forceinline__ void limbs_from_be(u32 (&a)[C::L], const uint8_t* __restrict__ src, long nbytes, const Lane<C>& ln) {
    if constexpr (C::LPE == 1) {
        u32 w[NW];
#pragma unroll
        for (int k = 0; k < NW; ++k) w[k] = load_be_word(src, nbytes, k);
        words_to_limbs<C::L, NW>(a, w);
    } else {
#pragma unroll 1
        for (int j = 0; j < C::L; ++j) {            // the word index depends on the lane's half: read from memory per limb
            int bit = 28 * (ln.half * C::L + j), k = bit >> 5, sh = bit & 31;
            u32 lo = k < NW ? load_be_word(src, nbytes, k) : 0u;
            u32 hi = k + 1 < NW ? load_be_word(src, nbytes, k + 1) : 0u;
            a[j] = (u32)((((u64)hi << 32) | lo) >> sh) & LIMB_MASK;
        }
    }
}

// flags[0] |= 1 if some value >= N ; flags[0] |= 2 if some value == 0 (only reported).
// Out-of-range values are replaced by `one` (x = 1) -- the reference substitutes trivial values
// for malformed input (P/hvzk/PoSBasicTW.java:794-815).
template <class C, int NW>
__global__ void __launch_bounds__(BLOCK, C::MINW)
k_import_be(u32* __restrict__ out, const uint8_t* __restrict__ be, size_t nbytes, size_t stride, int mode, size_t n,
            const u32* __restrict__ nmod, u32 n0inv, const u32* __restrict__ rr, u32* __restrict__ flags) {
    // mode bit 0: every value is preceded by a byte-tree leaf header; bit 1: values >= N are REDUCED mod N instead of
    // being reported and replaced (pseudo-random integers wider than the modulus: a * RR / R is a mod N for every a < R)
    const int leaf_hdr = mode & 1;
    const bool reduce = (mode & 2) != 0;
    extern __shared__ u32 lds[];
    Lane<C> ln(lds);
    u32 nn[C::L];
    load_modulus<C>(nn, nmod, ln);
    size_t el = (size_t)blockIdx.x * C::EPB + ln.eslot;
    bool live = el < n;
    size_t ec = live ? el : n - 1;
    const uint8_t* src = be + ec * stride;             // stride = nbytes, or nbytes + 5 with byte-tree leaf headers
    if (leaf_hdr) {                                   // 01 | uint32_be(nbytes) in front of every value
        bool hdr_ok = src[0] == 1 && src[1] == (uint8_t)(nbytes >> 24) && src[2] == (uint8_t)(nbytes >> 16) &&
                      src[3] == (uint8_t)(nbytes >> 8) && src[4] == (uint8_t)nbytes;
        if (live && !hdr_ok) atomicOr(flags, 4u);
        src += 5;
    }
    u32 extra = 0;                                    // leading bytes beyond NW words must be zero
    for (long o = (long)nbytes - 4L * NW - 1; o >= 0; --o) extra |= src[o];
    u32 a[C::L];
    limbs_from_be<C, NW>(a, src, (long)nbytes, ln);
    u32 d[C::L];
    bool bad = !reduce && (sub_full<C>(d, a, nn, ln) == 0 || extra != 0);     // a >= N
    u32 nz = 0;
#pragma unroll
    for (int j = 0; j < C::L; ++j) nz |= a[j];
    if constexpr (C::LPE > 1) nz = or_all<C::LPE>(nz);
    if (live && bad) atomicOr(flags, 1u);
    if (live && nz == 0) atomicOr(flags, 2u);
    if (bad) {
#pragma unroll
        for (int j = 0; j < C::L; ++j) a[j] = (j == 0 && ln.half == 0) ? 1u : 0u;
    }
    const_to_lds<C>(ln, rr);                          // to Montgomery form: a * RR / R
    u32 r[C::L];
    mont_mul<C>(r, a, ln, nn, n0inv);
    canonicalize<C>(r, nn, ln);
    if (live) store_elem<C>(out + el * C::W, r, ln);
}

// r (canonical standard representative, limbs) -> words; pair mode goes through the LDS column
template <class C, int NW, typename F>
__device__ __forceinline__ void emit_words(const u32 (&r)[C::L], const Lane<C>& ln, F&& put) {
    if constexpr (C::LPE == 1) {
        u32 w[NW];
        limbs_to_words<C::L, NW>(w, r);
#pragma unroll
        for (int k = 0; k < NW; ++k) put(k, w[k]);
    } else {
        regs_to_lds<C>(ln, r);
#pragma unroll 1
        for (int k = ln.half; k < NW; k += C::LPE) put(k, word_from_lds<C>(ln, k));
    }
}

template <class C, int NW>
__global__ void __launch_bounds__(BLOCK, C::MINW)
k_export_be(uint8_t* __restrict__ be, size_t nbytes, size_t stride, int leaf_hdr, const u32* __restrict__ in, size_t n,
            const u32* __restrict__ nmod, u32 n0inv) {
    extern __shared__ u32 lds[];
    Lane<C> ln(lds);
    u32 nn[C::L];
    load_modulus<C>(nn, nmod, ln);
    size_t el = (size_t)blockIdx.x * C::EPB + ln.eslot;
    bool live = el < n;
    size_t ec = live ? el : n - 1;
    u32 a[C::L];
    load_elem<C>(a, in + ec * C::W, ln);
    small_to_lds<C>(ln, 1u);                          // multiply by 1: leaves the Montgomery domain
    u32 r[C::L];
    mont_mul<C>(r, a, ln, nn, n0inv);
    canonicalize<C>(r, nn, ln);
    uint8_t* dst = be + ec * stride;
    if (leaf_hdr) {
        if (live && ln.half == 0) {
            dst[0] = 1;
            dst[1] = (uint8_t)(nbytes >> 24);
            dst[2] = (uint8_t)(nbytes >> 16);
            dst[3] = (uint8_t)(nbytes >> 8);
            dst[4] = (uint8_t)nbytes;
        }
        dst += 5;
    }
    emit_words<C, NW>(r, ln, [&](int k, u32 w) { if (live) store_be_word(dst, (long)nbytes, k, w); });
    if (live && ln.half == 0) {
        for (long o = (long)nbytes - 4L * NW - 1; o >= 0; --o) dst[o] = 0;
    }
}

// M28 form -> packed little-endian words of the standard representative (exponent use)
template <class C, int NW>
__global__ void __launch_bounds__(BLOCK, C::MINW)
k_to_words(u32* __restrict__ out, const u32* __restrict__ in, size_t n, const u32* __restrict__ nmod, u32 n0inv) {
    extern __shared__ u32 lds[];
    Lane<C> ln(lds);
    u32 nn[C::L];
    load_modulus<C>(nn, nmod, ln);
    size_t el = (size_t)blockIdx.x * C::EPB + ln.eslot;
    bool live = el < n;
    size_t ec = live ? el : n - 1;
    u32 a[C::L];
    load_elem<C>(a, in + ec * C::W, ln);
    small_to_lds<C>(ln, 1u);
    u32 r[C::L];
    mont_mul<C>(r, a, ln, nn, n0inv);
    canonicalize<C>(r, nn, ln);
    u32* dst = out + ec * NW;
    emit_words<C, NW>(r, ln, [&](int k, u32 w) { if (live) dst[k] = w; });
}

// ---------------------------------------------------------------------------------------------
// K4: out[i] = x[i] * y[i]        (ystride = 0: every x[i] times the single element y)
// ---------------------------------------------------------------------------------------------
template <class C>
__global__ void __launch_bounds__(BLOCK, C::MINW)
k_mul(u32* __restrict__ out, const u32* __restrict__ x, const u32* __restrict__ y, size_t ystride, size_t n,
      const u32* __restrict__ nmod, u32 n0inv) {
    extern __shared__ u32 lds[];
    Lane<C> ln(lds);
    u32 nn[C::L];
    load_modulus<C>(nn, nmod, ln);
    size_t el = (size_t)blockIdx.x * C::EPB + ln.eslot;
    bool live = el < n;
    size_t ec = live ? el : n - 1;
    u32 a[C::L];
    load_elem<C>(a, x + ec * C::W, ln);
    load_elem_to_lds<C>(ln, y + ec * ystride);
    u32 r[C::L];
    mont_mul<C>(r, a, ln, nn, n0inv);
    canonicalize<C>(r, nn, ln);
    if (live) store_elem<C>(out + el * C::W, r, ln);
}

// ---------------------------------------------------------------------------------------------
// K1a / K1b: out[i] = x[i] ^ e[i]   fixed-window (wbits), left to right, per-element exponents.
//   e: packed little-endian words, element i at e + i*estride (estride = 0: one shared exponent)
//   tab: scratch of gridDim.x*EPB*(2^wbits)*W words: the element's table of x^0..x^(2^w-1), one
//        contiguous row per entry (gathered with 16-byte loads).
// Persistent grid: a workgroup loops over tiles of EPB elements.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ u32 exp_digit(const u32* __restrict__ ep, int ewords, int pos, int wbits) {
    int k = pos >> 5, sh = pos & 31;
    u32 lo = k < ewords ? ep[k] : 0;
    u32 hi = k + 1 < ewords ? ep[k + 1] : 0;
    u64 both = ((u64)hi << 32) | lo;
    return (u32)(both >> sh) & ((1u << wbits) - 1);
}

// The pieces every power kernel is made of (k_modpow, k_modpow2, k_modpow_shared of modp_shared_exp.h, their phased forms and
// modpow_job_tile): each table build and each window loop is written here once, the kernels differ in where a tile's table
// lives and in which windows of the power one pass over a tile runs.
// a = a^(2^count)
template <class C>
__device__ __forceinline__ void sqr_times(u32 (&a)[C::L], int count, const Lane<C>& ln, const u32 (&nn)[C::L], u32 n0inv) {
#pragma unroll 1
    for (int s = 0; s < count; ++s) {
        if constexpr (SQR_FROM_LDS<C>) regs_to_lds<C>(ln, a);
        mont_sqr<C>(a, a, ln, nn, n0inv);
    }
}
// a = a * (the table row at `row`)
template <class C>
__device__ __forceinline__ void mul_by_row(u32 (&a)[C::L], const u32* __restrict__ row, const Lane<C>& ln, const u32 (&nn)[C::L],
                                           u32 n0inv) {
    load_elem_to_lds<C>(ln, row);
    mont_mul<C>(a, a, ln, nn, n0inv);
}
// fixed-window table of the element at `base`: tb[0] = 1, tb[1] = base, tb[k] = tb[k-1] * base (a: work registers, = base after)
template <class C>
__device__ __forceinline__ void window_table(u32 (&a)[C::L], u32* __restrict__ tb, int tsize, const u32* __restrict__ base,
                                             const u32* __restrict__ one_m, const Lane<C>& ln, const u32 (&nn)[C::L], u32 n0inv) {
    constexpr int W = C::W;
    load_elem<C>(a, base, ln);
    {
        u32 o[C::L];
        load_modulus<C>(o, one_m, ln);
        store_elem<C>(tb, o, ln);
    }
    store_elem<C>(tb + W, a, ln);
    regs_to_lds<C>(ln, a);
#pragma unroll 1
    for (int k = 2; k < tsize; ++k) {
        u32 r[C::L];
        mont_mul<C>(r, a, ln, nn, n0inv);              // base * tb[k-1]
        store_elem<C>(tb + (size_t)k * W, r, ln);
        regs_to_lds<C>(ln, r);
    }
}
// sliding-window table of the element at `base`, the odd powers only: tb[0] = x, tb[k] = tb[k-1] * x^2 (a: work registers)
template <class C>
__device__ __forceinline__ void odd_power_table(u32 (&a)[C::L], u32* __restrict__ tb, int tsize, const u32* __restrict__ base,
                                                const Lane<C>& ln, const u32 (&nn)[C::L], u32 n0inv) {
    constexpr int W = C::W;
    u32 x2[C::L];
    load_elem<C>(a, base, ln);
    store_elem<C>(tb, a, ln);
    regs_to_lds<C>(ln, a);
    mont_sqr<C>(x2, a, ln, nn, n0inv);
#pragma unroll 1
    for (int k = 1; k < tsize; ++k) {
        regs_to_lds<C>(ln, a);
        u32 r[C::L];
        mont_mul<C>(r, x2, ln, nn, n0inv);             // x^2 * tb[k-1]
        store_elem<C>(tb + (size_t)k * W, r, ln);
#pragma unroll
        for (int j = 0; j < C::L; ++j) a[j] = r[j];
    }
}
// windows hi .. lo (downwards) of a fixed-window power: wbits squarings, then the product by the window's table row
// (counted by k = wi - lo, here and in straus_windows: with `wi` itself as the counter the compiler lays the loop out differently once
// two kernels share this function, and k_modpow<Cfg<80, 8>> loses a wave per SIMD to the copies at the loop's edges)
template <class C>
__device__ __forceinline__ void fixed_windows(u32 (&a)[C::L], const u32* __restrict__ ep, int ewords, int wbits, int hi, int lo,
                                              const u32* __restrict__ tb, const Lane<C>& ln, const u32 (&nn)[C::L], u32 n0inv) {
#pragma unroll 1
    for (int k = hi - lo; k >= 0; --k) {
        const int wi = lo + k;
        sqr_times<C>(a, wbits, ln, nn, n0inv);
        const u32 d = exp_digit(ep, ewords, wi * wbits, wbits);
        mul_by_row<C>(a, tb + (size_t)d * C::W, ln, nn, n0inv);
    }
}
// windows hi .. lo of the simultaneous power of two bases (Straus): the squarings shared, none in front of the top window, and
// a product for each exponent that reaches the window (uniform over the launch: window counts, not digits, decide)
template <class C>
__device__ __forceinline__ void straus_windows(u32 (&a)[C::L], const u32* __restrict__ ep1, int ewords1, int nwin1,
                                               const u32* __restrict__ ep2, int ewords2, int nwin2, int wbits, int hi, int lo,
                                               const u32* __restrict__ tab1, const u32* __restrict__ tab2, const Lane<C>& ln,
                                               const u32 (&nn)[C::L], u32 n0inv) {
    const int nwin = nwin1 > nwin2 ? nwin1 : nwin2;
#pragma unroll 1
    for (int k = hi - lo; k >= 0; --k) {
        const int wi = lo + k;
        if (wi != nwin - 1) sqr_times<C>(a, wbits, ln, nn, n0inv);
        if (wi < nwin1) mul_by_row<C>(a, tab1 + (size_t)exp_digit(ep1, ewords1, wi * wbits, wbits) * C::W, ln, nn, n0inv);
        if (wi < nwin2) mul_by_row<C>(a, tab2 + (size_t)exp_digit(ep2, ewords2, wi * wbits, wbits) * C::W, ln, nn, n0inv);
    }
}

// The same value on limbs of the other width (static indices: shifts and ors in registers).  A limb of either width lies in at
// most two limbs of the other; the value must fit the target (callers: canonical values, < 2^2048).
template <int SD, int BD, int SS, int BS>
__device__ __forceinline__ void repack_limbs(u32 (&d)[SD], const u32 (&s)[SS]) {
    static_assert(BD < 32 && BS < 32 && 2 * BS >= BD + BS - 1, "two source limbs cover a target limb");
#pragma unroll
    for (int i = 0; i < SD; ++i) {
        const int bit = BD * i, j = bit / BS, sh = bit % BS;
        u32 v = j < SS ? s[j] >> sh : 0u;
        if (j + 1 < SS) v |= s[j + 1] << (BS - sh);                 // (bits shifted out of the word lie above the mask)
        d[i] = v & ((1u << BD) - 1);
    }
}
// The first and the last step of k_modpow / k_modpow_phased where they work in Cfg29 (K; C = Cfg<74, 1>): the table of the
// element at `base` (an M28 row of C), and the running value to its row -- finished: out of K's domain, canonical, an M28 row
// again.  one_m is the row ROW_ONE of the modulus' constants in that form; c_in and c_out are found from it (the kernels keep
// one_m anyway, a second pointer held across the row loops is a pair of SGPRs they do not have).
template <class C, class K>
__device__ __forceinline__ void pow29_table(u32 (&a)[K::L], u32* __restrict__ tb, int tsize, const u32* __restrict__ base,
                                            const u32* __restrict__ one_m, const Lane<K>& ln, const u32 (&nn)[K::L], u32 n0inv) {
    constexpr int W = K::W;
    {
        u32 x[C::L];
        load_elem<C>(x, base, Lane<C>(ln.bl - ln.eslot));
        repack_limbs<K::L, K::BITS, C::L, C::BITS>(a, x);
    }
    const_to_lds<K>(ln, one_m + (Cfg29::ROW_CIN - Cfg29::ROW_ONE) * W);
    mont_mul<K>(a, a, ln, nn, n0inv);                              // x R -> x R'; from here on window_table's steps
    {
        u32 o[K::L];
        load_modulus<K>(o, one_m, ln);
        store_elem<K>(tb, o, ln);
    }
    store_elem<K>(tb + W, a, ln);
    regs_to_lds<K>(ln, a);
#pragma unroll 1
    for (int k = 2; k < tsize; ++k) {
        u32 r[K::L];
        mont_mul<K>(r, a, ln, nn, n0inv);                          // x R' * tb[k-1]
        store_elem<K>(tb + (size_t)k * W, r, ln);
        regs_to_lds<K>(ln, r);
    }
}
template <class C, class K>
__device__ __forceinline__ void pow29_store(u32* __restrict__ dst, u32 (&a)[K::L], bool finished, bool live,
                                            const u32* __restrict__ one_m, const Lane<K>& ln, const u32 (&nn)[K::L], u32 n0inv) {
    if (finished) {
        const_to_lds<K>(ln, one_m + (Cfg29::ROW_COUT - Cfg29::ROW_ONE) * K::W);
        mont_mul<K>(a, a, ln, nn, n0inv);                          // y R' -> y R
        if constexpr (K::SHORT) {                                  // nn[] is N'': N itself from its row, once per element
            u32 nfull[K::L];
            load_modulus<K>(nfull, one_m + (Cfg29::ROW_N - Cfg29::ROW_ONE) * K::W, ln);
            canonicalize<K>(a, nfull, ln);
        } else {
            canonicalize<K>(a, nn, ln);
        }
        u32 y[C::L];
        repack_limbs<C::L, C::BITS, K::L, K::BITS>(y, a);
        if (live) store_elem<C>(dst, y, Lane<C>(ln.bl - ln.eslot));
    } else if (live) {
        store_elem<K>(dst, a, ln);
    }
}

// The queue of a phased kernel.  Every tile of k_modpow takes the same time T, so an array of r = ntiles / slots rounds finishes
// after ceil(r) T: 10^6 elements are 7.63 rounds of the 512 workgroup slots and cost 8 -- 4.6 % of the launch is the idle tail of
// its last round (measured: 0.632 of the roof at exactly 2 rounds, 0.603 at 7.63).  A phased kernel cuts a tile's power into
// `phases` runs of windows and its workgroups take (phase, tile) units from this queue in phase-major order: P x 7.63 rounds of
// units of T / P each, the tail is at most one UNIT.  Between its phases a tile's running value lives in out[], its table in a
// table of its OWN (per element, not per lane slot: another workgroup continues it).  Unit u = (phase, tile) needs
// (phase - 1, tile), which is unit u - ntiles: handed out earlier, to a workgroup that is therefore running and waits for
// nothing later than itself -- the spin in take() always ends, whatever part of the grid is resident.
//     UnitQueue q(queue, done, &s_unit, ntiles, phases);          (s_unit: a __shared__ word of the kernel)
//     while (q.take()) { ... unit (q.ph, q.t) ...; q.hand_over(); }
// ONE thread-0 region per turn -- the hand-over of the finished unit and the fetch of the next, between the two barriers of
// hand_over().  (With the fetch at the top of the loop and the hand-over at its bottom, two thread-0 regions sit around the back
// edge: the compiler lets the other lanes of wave 0 run ahead into the next turn's barrier while lane 0 is still signalling, the
// barrier counts go out of step and the kernel hangs -- tools/micro/queue_handoff.hip reproduces both forms.)
struct UnitQueue {
    u32* queue;       // units handed out so far
    u32* done;        // done[t]: phases of tile t that are finished and visible
    u32* s_unit;      // the workgroup's current unit
    u32 ntiles, nunits;
    int phases;
    int ph;           // the unit take() returned: phase ...
    u32 t;            // ... and tile
    __device__ __forceinline__ UnitQueue(u32* queue_, u32* done_, u32* s_unit_, u32 ntiles_, int phases_)
        : queue(queue_), done(done_), s_unit(s_unit_), ntiles(ntiles_), nunits(ntiles_ * (u32)phases_), phases(phases_), ph(0), t(0) {
        if (threadIdx.x == 0) fetch();
        __syncthreads();
    }
    // the next unit of this workgroup, once its tile's previous phase is finished; false: the queue is empty
    __device__ __forceinline__ bool take() {
        const u32 u = (u32)__builtin_amdgcn_readfirstlane((int)*s_unit);
        ph = (int)(u / ntiles);                          // (split before the test: no path leaves ph and t undefined -- with
        t = u - (u32)ph * ntiles;                        // them set after it the compiler keeps both in vector registers)
        if (u >= nunits) return false;
        if (ph > 0) {                                    // the tile's previous phase, run by another workgroup
            if (threadIdx.x == 0) {
                long spins = 0;                          // (a unit lasts milliseconds: 2^28 polls are minutes -- a bug, and then a trap, not a hang)
                while (__hip_atomic_load(done + t, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < (u32)ph) {
                    if (++spins > (1L << 28)) __builtin_trap();
                    __builtin_amdgcn_s_sleep(16);
                }
            }
            __syncthreads();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        }
        return true;
    }
    __device__ __forceinline__ bool last() const { return ph == phases - 1; }
    // the unit's stores are issued: publish them to the workgroup that continues the tile, and fetch the next unit
    __device__ __forceinline__ void hand_over() {
        const bool hand_on = !last();                    // another workgroup continues this tile
        if (hand_on) __threadfence();
        __syncthreads();                                 // every store of the unit is out; everybody has read s_unit
        if (threadIdx.x == 0) {
            if (hand_on) (void)__hip_atomic_exchange(done + t, (u32)(ph + 1), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            fetch();
        }
        __syncthreads();
    }

private:
    __device__ __forceinline__ void fetch() { *s_unit = atomicAdd(queue, 1u); }     // (thread 0 only)
};

template <class C, bool SHORT = false>
__global__ void __launch_bounds__(BLOCK, C::MINW)
k_modpow(u32* __restrict__ out, const u32* __restrict__ x, const u32* __restrict__ e, int ewords, size_t estride,
         int ebits, int wbits, size_t n, const u32* __restrict__ nmod, u32 n0inv, const u32* __restrict__ one_m,
         u32* __restrict__ tab) {
    using K = typename PowGeom<C, SHORT>::type;          // (Cfg29: nmod, n0inv and one_m are that form's; SHORT: nmod is N'')
    constexpr int W = C::W;
    extern __shared__ u32 lds[];
    Lane<K> ln(lds);
    u32 nn[K::L];
    load_modulus<K>(nn, nmod, ln);
    const size_t ntiles = (n + C::EPB - 1) / C::EPB;
    const int tsize = 1 << wbits;
    u32* mytab = tab + ((size_t)blockIdx.x * C::EPB + ln.eslot) * (size_t)tsize * W;
    const int nwin = (ebits + wbits - 1) / wbits;

    for (size_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        size_t el = t * C::EPB + ln.eslot;
        bool live = el < n;
        size_t ec = live ? el : n - 1;
        const u32* ep = e + ec * estride;
        u32 a[K::L];
        if constexpr (POW29<C>) pow29_table<C, K>(a, mytab, tsize, x + ec * W, one_m, ln, nn, n0inv);
        else window_table<C>(a, mytab, tsize, x + ec * W, one_m, ln, nn, n0inv);
        load_elem<K>(a, mytab + (size_t)exp_digit(ep, ewords, (nwin - 1) * wbits, wbits) * W, ln);     // the top window
        fixed_windows<K>(a, ep, ewords, wbits, nwin - 2, 0, mytab, ln, nn, n0inv);
        if constexpr (POW29<C>) {
            pow29_store<C, K>(out + el * W, a, true, live, one_m, ln, nn, n0inv);
        } else {
            canonicalize<C>(a, nn, ln);
            if (live) store_elem<C>(out + el * W, a, ln);
        }
    }
}

// k_modpow for arrays of MORE than one round of tiles, in phases from a queue of (phase, tile) units (UnitQueue has the
// reasons).  Same products in the same order as k_modpow: bit-identical results.
template <class C, bool SHORT = false>
__global__ void __launch_bounds__(BLOCK, C::MINW)
k_modpow_phased(u32* __restrict__ out, const u32* __restrict__ x, const u32* __restrict__ e, int ewords, size_t estride,
                int ebits, int wbits, size_t n, const u32* __restrict__ nmod, u32 n0inv, const u32* __restrict__ one_m,
                u32* __restrict__ tab, int phases, u32* __restrict__ queue, u32* __restrict__ done) {
    using K = typename PowGeom<C, SHORT>::type;          // (Cfg29: nmod, n0inv and one_m are that form's; so are the table and,
    constexpr int W = C::W;                              // between a tile's phases, its running value in out[])
    extern __shared__ u32 lds[];
    __shared__ u32 s_unit;
    Lane<K> ln(lds);
    u32 nn[K::L];
    load_modulus<K>(nn, nmod, ln);
    const int tsize = 1 << wbits;
    const int nwin = (ebits + wbits - 1) / wbits;
    const int M = nwin - 1;                              // windows of the main loop (the top one is the first table read)
    UnitQueue q(queue, done, &s_unit, (u32)((n + C::EPB - 1) / C::EPB), phases);
    while (q.take()) {
        const int ph = q.ph;
        size_t el = (size_t)q.t * C::EPB + ln.eslot;
        bool live = el < n;
        size_t ec = live ? el : n - 1;
        const u32* ep = e + ec * estride;
        u32* mytab = tab + el * (size_t)tsize * W;
        u32 a[K::L];
        if (ph == 0) {
            if constexpr (POW29<C>) pow29_table<C, K>(a, mytab, tsize, x + ec * W, one_m, ln, nn, n0inv);
            else window_table<C>(a, mytab, tsize, x + ec * W, one_m, ln, nn, n0inv);
            load_elem<K>(a, mytab + (size_t)exp_digit(ep, ewords, (nwin - 1) * wbits, wbits) * W, ln);
        } else {
            load_elem<K>(a, out + ec * W, ln);
        }
        // the windows of this phase: M - 1 - M ph / P  down to  M - M (ph + 1) / P
        const int hi = M - 1 - (int)((long)M * ph / phases), lo = M - (int)((long)M * (ph + 1) / phases);
        fixed_windows<K>(a, ep, ewords, wbits, hi, lo, mytab, ln, nn, n0inv);
        if constexpr (POW29<C>) {
            pow29_store<C, K>(out + el * W, a, q.last(), live, one_m, ln, nn, n0inv);
        } else {
            if (q.last()) canonicalize<C>(a, nn, ln);
            if (live) store_elem<C>(out + el * W, a, ln);
        }
        q.hand_over();
    }
}

// ---------------------------------------------------------------------------------------------
// Simultaneous power of two bases (Straus): out[i] = x[i]^e1 * y[i]^e2 with the squarings shared -- max(ebits1, ebits2)
// squarings instead of their sum.  Either exponent may be shared (stride 0) or per element.  Per-lane tables of both bases
// in scratch (2 * 2^w rows).  Used by the verifiers' check (B) in the form B_i^v (B_{i-1}^{-1})^{k_E,i}.
// ---------------------------------------------------------------------------------------------
template <class C>
__global__ void __launch_bounds__(BLOCK, C::MINW)
k_modpow2(u32* __restrict__ out, const u32* __restrict__ x, const u32* __restrict__ e1, int ewords1, size_t estride1, int ebits1,
          const u32* __restrict__ y, const u32* __restrict__ e2, int ewords2, size_t estride2, int ebits2, int wbits, size_t n,
          const u32* __restrict__ nmod, u32 n0inv, const u32* __restrict__ one_m, u32* __restrict__ tab) {
    constexpr int W = C::W;
    extern __shared__ u32 lds[];
    Lane<C> ln(lds);
    u32 nn[C::L];
    load_modulus<C>(nn, nmod, ln);
    const size_t ntiles = (n + C::EPB - 1) / C::EPB;
    const int tsize = 1 << wbits;
    u32* tab1 = tab + ((size_t)blockIdx.x * C::EPB + ln.eslot) * (size_t)(2 * tsize) * W;
    u32* tab2 = tab1 + (size_t)tsize * W;
    const int nwin1 = (ebits1 + wbits - 1) / wbits, nwin2 = (ebits2 + wbits - 1) / wbits;
    const int nwin = nwin1 > nwin2 ? nwin1 : nwin2;

    for (size_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        size_t el = t * C::EPB + ln.eslot;
        bool live = el < n;
        size_t ec = live ? el : n - 1;
        u32 a[C::L];
#pragma unroll 1
        for (int which = 0; which < 2; ++which)
            window_table<C>(a, which ? tab2 : tab1, tsize, (which ? y : x) + ec * W, one_m, ln, nn, n0inv);
        load_modulus<C>(a, one_m, ln);
        straus_windows<C>(a, e1 + ec * estride1, ewords1, nwin1, e2 + ec * estride2, ewords2, nwin2, wbits, nwin - 1, 0, tab1, tab2,
                          ln, nn, n0inv);
        canonicalize<C>(a, nn, ln);
        if (live) store_elem<C>(out + el * W, a, ln);
    }
}

// k_modpow2 for arrays of more than one round of tiles: the same simultaneous power in phases from a queue of (phase, tile)
// units (UnitQueue); both tables of a tile live in a table of its own (2 * 2^w rows per element).
template <class C>
__global__ void __launch_bounds__(BLOCK, C::MINW)
k_modpow2_phased(u32* __restrict__ out, const u32* __restrict__ x, const u32* __restrict__ e1, int ewords1, size_t estride1, int ebits1,
                 const u32* __restrict__ y, const u32* __restrict__ e2, int ewords2, size_t estride2, int ebits2, int wbits, size_t n,
                 const u32* __restrict__ nmod, u32 n0inv, const u32* __restrict__ one_m, u32* __restrict__ tab, int phases,
                 u32* __restrict__ queue, u32* __restrict__ done) {
    constexpr int W = C::W;
    extern __shared__ u32 lds[];
    __shared__ u32 s_unit;
    Lane<C> ln(lds);
    u32 nn[C::L];
    load_modulus<C>(nn, nmod, ln);
    const int tsize = 1 << wbits;
    const int nwin1 = (ebits1 + wbits - 1) / wbits, nwin2 = (ebits2 + wbits - 1) / wbits;
    const int nwin = nwin1 > nwin2 ? nwin1 : nwin2;
    UnitQueue q(queue, done, &s_unit, (u32)((n + C::EPB - 1) / C::EPB), phases);
    while (q.take()) {
        const int ph = q.ph;
        size_t el = (size_t)q.t * C::EPB + ln.eslot;
        bool live = el < n;
        size_t ec = live ? el : n - 1;
        u32* tab1 = tab + el * (size_t)(2 * tsize) * W;
        u32* tab2 = tab1 + (size_t)tsize * W;
        u32 a[C::L];
        if (ph == 0) {
#pragma unroll 1
            for (int which = 0; which < 2; ++which)
                window_table<C>(a, which ? tab2 : tab1, tsize, (which ? y : x) + ec * W, one_m, ln, nn, n0inv);
            load_modulus<C>(a, one_m, ln);
        } else {
            load_elem<C>(a, out + ec * W, ln);
        }
        // the windows of this phase: nwin - 1 - nwin ph / P  down to  nwin - nwin (ph + 1) / P
        const int hi = nwin - 1 - (int)((long)nwin * ph / phases), lo = nwin - (int)((long)nwin * (ph + 1) / phases);
        straus_windows<C>(a, e1 + ec * estride1, ewords1, nwin1, e2 + ec * estride2, ewords2, nwin2, wbits, hi, lo, tab1, tab2, ln,
                          nn, n0inv);
        if (q.last()) canonicalize<C>(a, nn, ln);
        if (live) store_elem<C>(out + el * W, a, ln);
        q.hand_over();
    }
}

// =============================================================================================
// second part: fixed-base tables (K2), multi-exponentiation (K3), reductions (K5), comparison
// (K6), data movement (K7) and the ring kernels over Z_q (K8).
// =============================================================================================

// ---------------------------------------------------------------------------------------------
// K5 and friends: strided reduction.  out[seg][j] = OP_k x[seg][j + k*L], k = 0 .. ceil(len/L)-1,
// for j < L.  OP = Montgomery product (MUL = true) or modular sum.  nseg segments of `len`
// elements each; the output has nseg segments of L elements.
// ---------------------------------------------------------------------------------------------
template <class C, bool MUL>
__global__ void __launch_bounds__(BLOCK, C::MINW)
k_reduce_strided(u32* __restrict__ out, const u32* __restrict__ x, size_t len, size_t Lout, size_t nseg,
                 const u32* __restrict__ nmod, u32 n0inv) {
    constexpr int W = C::W;
    extern __shared__ u32 lds[];
    Lane<C> ln(lds);
    u32 nn[C::L];
    load_modulus<C>(nn, nmod, ln);
    size_t t = (size_t)blockIdx.x * C::EPB + ln.eslot;
    bool live = t < nseg * Lout;
    size_t tc = live ? t : nseg * Lout - 1;
    size_t seg = tc / Lout, j = tc % Lout;
    const u32* base = x + seg * len * W;
    u32 acc[C::L];
    load_elem<C>(acc, base + j * W, ln);
    size_t cnt = (len - j + Lout - 1) / Lout;            // elements j, j+Lout, ... < len
    for (size_t k = 1; k < cnt; ++k) {
        const u32* src = base + (j + k * Lout) * W;
        if constexpr (MUL) {
            load_elem_to_lds<C>(ln, src);
            mont_mul<C>(acc, acc, ln, nn, n0inv);
        } else {
            u32 b[C::L];
            load_elem<C>(b, src, ln);
            mod_add<C>(acc, acc, b, nn, ln);
        }
    }
    if constexpr (MUL) canonicalize<C>(acc, nn, ln);
    if (live) store_elem<C>(out + t * W, acc, ln);
}

// ---------------------------------------------------------------------------------------------
// K8 element-wise ring kernels:  op 0: x + y   op 1: -x   op 2: x*v + y (v one element)   op 3: x*v
// ---------------------------------------------------------------------------------------------
template <class C>
__global__ void __launch_bounds__(BLOCK, C::MINW)
k_ring_elementwise(u32* __restrict__ out, const u32* __restrict__ x, const u32* __restrict__ y, const u32* __restrict__ v,
                   int op, size_t n, const u32* __restrict__ nmod, u32 n0inv) {
    constexpr int W = C::W;
    extern __shared__ u32 lds[];
    Lane<C> ln(lds);
    u32 nn[C::L];
    load_modulus<C>(nn, nmod, ln);
    size_t el = (size_t)blockIdx.x * C::EPB + ln.eslot;
    bool live = el < n;
    size_t ec = live ? el : n - 1;
    u32 a[C::L], r[C::L];
    load_elem<C>(a, x + ec * W, ln);
    if (op == 0) {
        u32 b[C::L];
        load_elem<C>(b, y + ec * W, ln);
        mod_add<C>(r, a, b, nn, ln);
    } else if (op == 1) {
        mod_neg<C>(r, a, nn, ln);
    } else {
        load_elem_to_lds<C>(ln, v);
        u32 t[C::L];
        mont_mul<C>(t, a, ln, nn, n0inv);
        canonicalize<C>(t, nn, ln);
        if (op == 2) {
            u32 b[C::L];
            load_elem<C>(b, y + ec * W, ln);
            mod_add<C>(r, t, b, nn, ln);
        } else {
#pragma unroll
            for (int j = 0; j < C::L; ++j) r[j] = t[j];
        }
    }
    if (live) store_elem<C>(out + el * W, r, ln);
}

// ---------------------------------------------------------------------------------------------
// K8 scans.  An affine recurrence x[i] = x[i-1]*e[i] + b[i] (recLin; b == nullptr: prods,
// y[i] = y[i-1]*e[i]) over segments of `seglen` elements (seglen % Cc == 0 or one segment),
// processed in chunks of Cc consecutive elements per lane (pair):
//   k_scan_totals : per chunk, the composed map (E = prod e, X = value reached from 0)
//   (recursion on the totals gives every chunk's incoming value)
//   k_scan_apply  : per chunk, replay the recurrence from the incoming value and store x[i]
// `rev`: element i of a segment is read/written at position seglen-1-i (suffix scans of K3).
// ---------------------------------------------------------------------------------------------
// WANT_X = false: tot[c] = prod of the chunk's e.   WANT_X = true: tot[c] = value reached from 0.
// (Two launches for recLin: one accumulator per kernel keeps a + columns + accumulator within 256 VGPRs.)
template <class C, bool WANT_X>
__global__ void __launch_bounds__(BLOCK, C::MINW)
k_scan_totals(u32* __restrict__ tot, const u32* __restrict__ e, const u32* __restrict__ b,
              size_t n, size_t Cc, size_t seglen, int rev, const u32* __restrict__ nmod, u32 n0inv,
              const u32* __restrict__ one_m) {
    constexpr int W = C::W;
    extern __shared__ u32 lds[];
    Lane<C> ln(lds);
    u32 nn[C::L];
    load_modulus<C>(nn, nmod, ln);
    size_t nchunks = (n + Cc - 1) / Cc;
    size_t c = (size_t)blockIdx.x * C::EPB + ln.eslot;
    bool live = c < nchunks;
    size_t cc = live ? c : nchunks - 1;
    size_t lo = cc * Cc, hi = lo + Cc < n ? lo + Cc : n;
    u32 A[C::L];
    if constexpr (WANT_X) {
#pragma unroll
        for (int j = 0; j < C::L; ++j) A[j] = 0u;
    } else {
        load_modulus<C>(A, one_m, ln);
    }
    for (size_t i = lo; i < lo + Cc; ++i) {          // uniform trip count; short chunks idle at the end
        if (i < hi) {
            size_t pos = rev ? (i / seglen) * seglen + (seglen - 1 - i % seglen) : i;
            load_elem_to_lds<C>(ln, e + pos * W);
            mont_mul<C>(A, A, ln, nn, n0inv);
            if constexpr (WANT_X) {
                canonicalize<C>(A, nn, ln);
                u32 bb[C::L];
                load_elem<C>(bb, b + pos * W, ln);
                mod_add<C>(A, A, bb, nn, ln);
            }
        }
    }
    canonicalize<C>(A, nn, ln);
    if (live) store_elem<C>(tot + c * W, A, ln);
}

// incoming: per-chunk inclusive results of the level above (chunk c starts from incoming[c-1]),
// nullptr = every chunk starts fresh.  A chunk that begins a segment starts fresh (0 / one).
template <class C>
__global__ void __launch_bounds__(BLOCK, C::MINW)
k_scan_apply(u32* __restrict__ out, const u32* __restrict__ e, const u32* __restrict__ b, const u32* __restrict__ incoming,
             size_t n, size_t Cc, size_t seglen, int rev, const u32* __restrict__ nmod, u32 n0inv,
             const u32* __restrict__ one_m) {
    constexpr int W = C::W;
    extern __shared__ u32 lds[];
    Lane<C> ln(lds);
    u32 nn[C::L];
    load_modulus<C>(nn, nmod, ln);
    size_t nchunks = (n + Cc - 1) / Cc;
    size_t c = (size_t)blockIdx.x * C::EPB + ln.eslot;
    bool live = c < nchunks;
    size_t cc = live ? c : nchunks - 1;
    size_t lo = cc * Cc, hi = lo + Cc < n ? lo + Cc : n;
    bool fresh = incoming == nullptr || (lo % seglen) == 0;
    u32 X[C::L];
    if (fresh) {
        if (b) {
#pragma unroll
            for (int j = 0; j < C::L; ++j) X[j] = 0u;
        } else {
            load_modulus<C>(X, one_m, ln);
        }
    } else {
        load_elem<C>(X, incoming + (cc - 1) * W, ln);
    }
    for (size_t i = lo; i < lo + Cc; ++i) {
        if (i < hi) {
            size_t pos = rev ? (i / seglen) * seglen + (seglen - 1 - i % seglen) : i;
            load_elem_to_lds<C>(ln, e + pos * W);
            u32 t[C::L];
            mont_mul<C>(t, X, ln, nn, n0inv);
            canonicalize<C>(t, nn, ln);
            if (b) {
                u32 bb[C::L];
                load_elem<C>(bb, b + pos * W, ln);
                mod_add<C>(X, t, bb, nn, ln);
            } else {
#pragma unroll
                for (int j = 0; j < C::L; ++j) X[j] = t[j];
            }
            if (live) store_elem<C>(out + pos * W, X, ln);
        }
    }
}

template <class C>
__global__ void __launch_bounds__(BLOCK, C::MINW)
k_fixed_level(u32* __restrict__ T, int w, int nwin, int l, const u32* __restrict__ nmod, u32 n0inv) {
    constexpr int W = C::W;
    extern __shared__ u32 lds[];
    Lane<C> ln(lds);
    u32 nn[C::L];
    load_modulus<C>(nn, nmod, ln);
    size_t per = ((size_t)1 << l) - 1;                 // d = 2^l + 1 .. 2^(l+1) - 1
    size_t t = (size_t)blockIdx.x * C::EPB + ln.eslot;
    bool live = t < per * nwin;
    size_t tc = live ? t : per * nwin - 1;
    size_t k = tc / per, r = tc % per + 1;             // r = d - 2^l in [1, 2^l)
    u32* row = T + (k << w) * W;
    u32 a[C::L];
    load_elem<C>(a, row + r * W, ln);
    load_elem_to_lds<C>(ln, row + ((size_t)1 << l) * W);
    u32 o[C::L];
    mont_mul<C>(o, a, ln, nn, n0inv);
    canonicalize<C>(o, nn, ln);
    if (live) store_elem<C>(row + (((size_t)1 << l) + r) * W, o, ln);
}

// out[i] = prod_k T[k][digit_k(e[i])].  parts > 1 (small arrays): the chain of nwin - 1 dependent products of an element is cut
// into `parts` independent pieces -- item t = part * n + i multiplies the windows [part nwin / parts, (part + 1) nwin / parts)
// of element i into out[t] -- and the caller multiplies the pieces together by a tree of element-wise products: a chain of
// nwin / parts + log2(parts) products instead of nwin, on `parts` times as many lanes (which a small array leaves idle anyway).
template <class C>
__global__ void __launch_bounds__(BLOCK, C::MINW)
k_fixed_exp(u32* __restrict__ out, const u32* __restrict__ T, int w, int nwin, const u32* __restrict__ e, int ewords,
            size_t n, int parts, const u32* __restrict__ nmod, u32 n0inv) {
    constexpr int W = C::W;
    extern __shared__ u32 lds[];
    Lane<C> ln(lds);
    u32 nn[C::L];
    load_modulus<C>(nn, nmod, ln);
    const size_t items = n * (size_t)parts;
    const size_t ntiles = (items + C::EPB - 1) / C::EPB;
    for (size_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        size_t it = t * C::EPB + ln.eslot;
        bool live = it < items;
        size_t ic = live ? it : items - 1;
        const int part = (int)(ic / n);
        const size_t ec = ic % n;
        const int k0 = (int)((long)part * nwin / parts), k1 = (int)((long)(part + 1) * nwin / parts);
        const u32* ep = e + ec * ewords;
        u32 a[C::L];
        u32 d = exp_digit(ep, ewords, k0 * w, w);
        load_elem<C>(a, T + (((size_t)k0 << w) + d) * W, ln);
#pragma unroll 1
        for (int k = k0 + 1; k < k1; ++k) {
            d = exp_digit(ep, ewords, k * w, w);
            load_elem_to_lds<C>(ln, T + (((size_t)k << w) + d) * W);
            mont_mul<C>(a, a, ln, nn, n0inv);
        }
        canonicalize<C>(a, nn, ln);
        if (live) store_elem<C>(out + it * W, a, ln);
    }
}

// One level of the per-bucket product tree.  Bucket b owns cnt_in[b] items at off_in[b]; output item
// (b, j) = product of its input items [jF, (j+1)F) and lands at off_out[b] + j.  One lane (pair) per output
// item, so a bucket of any size is spread over ceil(size/F) lanes: no lane ever walks a long bucket
// (skewed digits -- a short top window, equal exponents -- would otherwise serialise on one lane).
// FIRST: input items are rows of x selected through `sorted`; otherwise rows of `in`.
// The arrays of one launch (a multi-exponentiation of k arrays under ONE exponent vector builds k trees of the same shape:
// counts and offsets are shared, so one launch per level serves up to LEVEL_ARRAYS of them -- a seventh of the launches over
// curves, and k times as many items in the thin upper levels).  Block b works for array b / blocks_per_array.
constexpr int LEVEL_ARRAYS = 8;
struct LevelInputs {
    const u32* p[LEVEL_ARRAYS];
};
template <class C, bool FIRST>
__global__ void __launch_bounds__(BLOCK, C::MINW)
k_bucket_level(u32* __restrict__ out, size_t out_stride, LevelInputs ins, unsigned blocks_per_array, const u32* __restrict__ sorted,
               const u32* __restrict__ off_in, const u32* __restrict__ cnt_in, const u32* __restrict__ off_out,
               size_t nbuckets, size_t total_out, u32 F, const u32* __restrict__ nmod, u32 n0inv) {
    constexpr int W = C::W;
    extern __shared__ u32 lds[];
    Lane<C> ln(lds);
    u32 nn[C::L];
    load_modulus<C>(nn, nmod, ln);
    const unsigned arr = blockIdx.x / blocks_per_array;          // (wave-uniform)
    const u32* __restrict__ in = ins.p[arr];
    out += (size_t)arr * out_stride;
    size_t t = (size_t)(blockIdx.x % blocks_per_array) * C::EPB + ln.eslot;
    bool live = t < total_out;
    size_t tc = live ? t : total_out - 1;
    // b = last bucket with off_out[b] <= tc  (empty buckets share their successor's offset)
    size_t lo = 0, hi = nbuckets;                 // invariant: off_out[lo] <= tc < off_out[hi] (off_out[nbuckets] = total)
    while (hi - lo > 1) {
        size_t mid = (lo + hi) >> 1;
        if (off_out[mid] <= tc) lo = mid; else hi = mid;
    }
    size_t b = lo;
    u32 j = (u32)(tc - off_out[b]);
    u32 start = off_in[b] + j * F;
    u32 end = off_in[b] + cnt_in[b];
    if (end > start + F) end = start + F;
    u32 acc[C::L];
    auto row = [&](u32 k) -> const u32* { return FIRST ? in + (size_t)sorted[k] * W : in + (size_t)k * W; };
    load_elem<C>(acc, row(start), ln);
    for (u32 k = start + 1; k < end; ++k) {
        load_elem_to_lds<C>(ln, row(k));
        mont_mul<C>(acc, acc, ln, nn, n0inv);
    }
    canonicalize<C>(acc, nn, ln);
    if (live) store_elem<C>(out + t * W, acc, ln);
}

// ---------------------------------------------------------------------------------------------
// K10: membership in the order-q subgroup of a safe-prime group (p = 2q + 1): x is a member iff it is a quadratic
// residue iff the Jacobi symbol (x / p) = 1.  Binary Jacobi algorithm on 28-bit limbs, one element per lane (moduli
// up to 2048 bits; above that the element's own lanes, k_jacobi_member_lanes), no multiplications: a few limb passes per
// step, at most 2 * bits(p) steps -- about a tenth of the instructions of the x^q = 1 test.  The rows are in Montgomery form x R mod p; (R / p) = 1 because R is an even
// power of two, so the symbol of the row is the symbol of x.  flags[0] |= 1 when some element is not a member
// (zero included).  ref: the membership test VCR makes when an array is read (pGroup.toElementArray), e.g.
// P/hvzk/PoSBasicTW.java:787-792.
// ---------------------------------------------------------------------------------------------
// The row of element ec and the modulus, all S limbs of each in ONE lane's registers (2 S <= 148 VGPRs).  (The loads also read
// the two-share layout of Cfg<110, 2>; 3072-bit moduli use the lanes form since that proved three times faster.)
template <class C>
__device__ __forceinline__ void jacobi_load_one_lane(u32 (&a)[C::S], u32 (&m)[C::S], const u32* __restrict__ x, size_t ec,
                                                     const u32* __restrict__ nmod) {
    static_assert(C::LPE <= 2, "the element must fit one lane");
    constexpr int L = C::L, LW = C::LW;
#pragma unroll
    for (int h = 0; h < C::LPE; ++h) {
        const uint4* q = reinterpret_cast<const uint4*>(x + ec * C::W + h * LW);
        const uint4* qm = reinterpret_cast<const uint4*>(nmod + h * LW);
#pragma unroll
        for (int k = 0; k < LW / 4; ++k) {
            uint4 v = q[k], w = qm[k];
            if (4 * k + 0 < L) { a[h * L + 4 * k + 0] = v.x; m[h * L + 4 * k + 0] = w.x; }
            if (4 * k + 1 < L) { a[h * L + 4 * k + 1] = v.y; m[h * L + 4 * k + 1] = w.y; }
            if (4 * k + 2 < L) { a[h * L + 4 * k + 2] = v.z; m[h * L + 4 * k + 2] = w.z; }
            if (4 * k + 3 < L) { a[h * L + 4 * k + 3] = v.w; m[h * L + 4 * k + 3] = w.w; }
        }
    }
}
// The Jacobi symbol (a / m): 1, -1, or 0 when the two share a factor (a = 0 included); m odd, 0 <= a < m.  The binary algorithm
// in place: both arrays are destroyed.  The one copy of the loop for one lane per element (k_jacobi_member, k_jacobi_fix).
// The registers hold a and m and little else at 74 limbs: the parity is a predicate, not a vector register, and the limb passes
// are scheduled eight limbs at a time (sched_barrier) -- free to reorder a whole pass the compiler spills.  The same form in
// every geometry: with the parity a word and no pacing below 20 limbs, hipcc (ROCm 7.2) compiled the comparison chain of
// Cfg<10, 1> to read limb 6 from a register it had just reused for the borrow (tests/test_gpu_jacobi_edges.py, 256 bits, found it).
template <int S>
__device__ __forceinline__ int jacobi_symbol(u32 (&a)[S], u32 (&m)[S]) {
    bool t = false;                              // parity of the sign flips: symbol = (-1)^t (a predicate: no vector register)
    u32 nz = 0;
#pragma unroll
    for (int j = 0; j < S; ++j) nz |= a[j];
    bool zero_in = nz == 0;
    // invariant: m odd, 0 <= a < m at loop entry (a < p on input)
    while (nz != 0) {
        // strip the factors of two of a: (2 / m) = -1 iff m = 3, 5 mod 8
        u32 low = a[0];
        if (low == 0) {                          // a whole zero limb: shift by one limb (28 bits: even count, no flip)
#pragma unroll
            for (int j = 0; j + 1 < S; ++j) a[j] = a[j + 1];
            a[S - 1] = 0;
            continue;
        }
        int k = __builtin_ctz(low);
        if (k) {
            u32 m8 = m[0] & 7u;
            if ((k & 1) && (m8 == 3u || m8 == 5u)) t = !t;
#pragma unroll
            for (int j = 0; j < S; ++j) {
                u32 hi = j + 1 < S ? a[j + 1] : 0u;
                a[j] = ((a[j] >> k) | (hi << (LIMB_BITS - k))) & LIMB_MASK;
                if (j % 8 == 7) __builtin_amdgcn_sched_barrier(0);
            }
        }
        // a odd now: compare (borrow of a - m), then subtract in place in the right direction
        int32_t borrow = 0;
#pragma unroll
        for (int j = 0; j < S; ++j) borrow = ((int32_t)a[j] - (int32_t)m[j] + borrow) >> LIMB_BITS;
        if (borrow == 0) {                       // a >= m: a := a - m (even; the symbol is unchanged)
            int32_t c = 0;
#pragma unroll
            for (int j = 0; j < S; ++j) {
                int32_t v = (int32_t)a[j] - (int32_t)m[j] + c;
                a[j] = (u32)v & LIMB_MASK;
                c = v >> LIMB_BITS;
                if (j % 8 == 7) __builtin_amdgcn_sched_barrier(0);
            }
        } else {                                 // a < m: swap by reciprocity, (a, m) := (m - a, a)
            if ((a[0] & 3u) == 3u && (m[0] & 3u) == 3u) t = !t;
            int32_t c = 0;
#pragma unroll
            for (int j = 0; j < S; ++j) {
                u32 old = a[j];
                int32_t v = (int32_t)m[j] - (int32_t)old + c;
                a[j] = (u32)v & LIMB_MASK;
                c = v >> LIMB_BITS;
                m[j] = old;
                if (j % 8 == 7) __builtin_amdgcn_sched_barrier(0);
            }
        }
        nz = 0;
#pragma unroll
        for (int j = 0; j < S; ++j) nz |= a[j];
    }
    // a = 0: the symbol is (-1)^t when m = 1 (coprime), 0 otherwise
    u32 rest = m[0] ^ 1u;
#pragma unroll
    for (int j = 1; j < S; ++j) rest |= m[j];
    return (zero_in || rest != 0) ? 0 : t ? -1 : 1;
}
template <class C>
__global__ void __launch_bounds__(BLOCK, 2)
k_jacobi_member(const u32* __restrict__ x, size_t n, const u32* __restrict__ nmod, u32* __restrict__ flags) {
    // ONE lane holds the whole element: a and m in registers, updated in place
    size_t el = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    bool live = el < n;
    size_t ec = live ? el : n - 1;
    u32 a[C::S], m[C::S];
    jacobi_load_one_lane<C>(a, m, x, ec, nmod);
    bool member = jacobi_symbol<C::S>(a, m) == 1;
    if (live && !member) atomicOr(flags, 1u);
}

// The same test with the element spread over LPE lanes (4096-bit moduli: a and m do not fit one lane's registers).  The
// lanes of an element run the binary algorithm in lockstep: every decision is taken from lane 0's low limbs (broadcast),
// the right shifts pull the next lane's low limb in (DPP), comparison and subtraction are the element-wide borrow chains
// of canonicalize() (sub_full: LPE sweeps).  ~1200 instructions per step, at most 2 * bits(p) steps: a tenth of x^q.
// (jacobi_symbol_lanes: the one copy of that loop -- k_jacobi_member_lanes, k_jacobi_fix_lanes; the symbol on every lane of the
// element, a and m destroyed)
template <class C>
__device__ __forceinline__ int jacobi_symbol_lanes(u32 (&a)[C::L], u32 (&m)[C::L], const Lane<C>& ln) {
    static_assert(C::LPE > 1 && !C::WIDE, "one lane per element uses jacobi_symbol");
    constexpr int L = C::L, LPE = C::LPE;
    u32 d[L];
    bool t = false;
    auto any = [&](const u32 (&v)[L]) {
        u32 nz = 0;
#pragma unroll
        for (int j = 0; j < L; ++j) nz |= v[j];
        return or_all<LPE>(nz);
    };
    u32 nz = any(a);
    const bool zero_in = nz == 0;
    // invariant: m odd, 0 <= a < m at loop entry (a < p on input)
    while (nz != 0) {
        const u32 low = from_lane0<LPE>(a[0]);
        const u32 up = from_above<LPE>(a[0]) & ln.nottopmask;       // the limb above this lane's share (0 above the element)
        if (low == 0) {                          // a whole zero limb: shift by one limb (28 bits: even count, no flip)
#pragma unroll
            for (int j = 0; j + 1 < L; ++j) a[j] = a[j + 1];
            a[L - 1] = up;
            continue;
        }
        const int k = __builtin_ctz(low);
        if (k) {
            const u32 m8 = from_lane0<LPE>(m[0]) & 7u;
            if ((k & 1) && (m8 == 3u || m8 == 5u)) t = !t;
#pragma unroll
            for (int j = 0; j < L; ++j) {
                const u32 hi = j + 1 < L ? a[j + 1] : up;
                a[j] = ((a[j] >> k) | (hi << (LIMB_BITS - k))) & LIMB_MASK;
            }
        }
        // a odd now: a - m over the whole element; borrow = -1 when a < m
        if (sub_full<C>(d, a, m, ln) == 0) {     // a >= m: a := a - m (even; the symbol is unchanged)
#pragma unroll
            for (int j = 0; j < L; ++j) a[j] = d[j];
        } else {                                 // a < m: swap by reciprocity, (a, m) := (m - a, a)
            const u32 a0 = from_lane0<LPE>(a[0]), m0 = from_lane0<LPE>(m[0]);
            if ((a0 & 3u) == 3u && (m0 & 3u) == 3u) t = !t;
            sub_full<C>(d, m, a, ln);
#pragma unroll
            for (int j = 0; j < L; ++j) {
                m[j] = a[j];
                a[j] = d[j];
            }
        }
        nz = any(a);
    }
    // a = 0: the symbol is (-1)^t when m = 1 (coprime), 0 otherwise
    u32 rest = m[0] ^ (ln.half == 0 ? 1u : 0u);
#pragma unroll
    for (int j = 1; j < L; ++j) rest |= m[j];
    rest = or_all<LPE>(rest);
    return (zero_in || rest != 0) ? 0 : t ? -1 : 1;
}
template <class C>
__global__ void __launch_bounds__(BLOCK, 2)
k_jacobi_member_lanes(const u32* __restrict__ x, size_t n, const u32* __restrict__ nmod, u32* __restrict__ flags) {
    constexpr int L = C::L;
    Lane<C> ln(nullptr);
    size_t el = (size_t)blockIdx.x * C::EPB + ln.eslot;
    bool live = el < n;
    size_t ec = live ? el : n - 1;
    u32 a[L], m[L];
    load_elem<C>(a, x + ec * C::W, ln);
    load_modulus<C>(m, nmod, ln);
    const bool member = jacobi_symbol_lanes<C>(a, m, ln) == 1;
    if (live && ln.half == 0 && !member) atomicOr(flags, 1u);
}

// The residue fix of the safe-prime encoding (csrc/encode_layout.h): row i := p - row i where the Jacobi symbol of the row is -1,
// in place, so that every row is a quadratic residue (-1 is none: p = 3 mod 4).  Rows are in Montgomery form: (R / p) = 1, and
// negation is p - row in either form.  The symbol's loop destroys its copy of the row, which is therefore read again for the
// store -- no second copy in registers.  A row whose symbol is 0 (zero; never an encoded value) stays.
// (reread: the same address, but one the compiler knows nothing about -- it would otherwise keep the values of the first loads
// alive across the loop, the second copy the registers have no room for, instead of loading them again)
__device__ __forceinline__ const u32* reread(const u32* p) {
    asm volatile("" : "+v"(p));
    return p;
}
__device__ __forceinline__ const u32* reread_uniform(const u32* p) {         // (a wave-uniform address stays in scalar registers)
    asm volatile("" : "+s"(p));
    return p;
}
template <class C>
__global__ void __launch_bounds__(BLOCK, 2)
k_jacobi_fix(u32* __restrict__ x, size_t n, const u32* __restrict__ nmod) {
    static_assert(C::LPE == 1, "one lane per element");
    constexpr int S = C::S;
    size_t el = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    bool live = el < n;
    size_t ec = live ? el : n - 1;
    u32 a[S], m[S];
    jacobi_load_one_lane<C>(a, m, x, ec, nmod);
    // (nothing of a lane's own is kept across the loop, which fills the registers: the element's index is put together again
    // from the wave's first thread, a scalar, and the lane's number)
    const u32 wave_first = __builtin_amdgcn_readfirstlane(threadIdx.x & ~63u);
    if (jacobi_symbol<S>(a, m) != -1) return;
    const u32 lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    el = (size_t)blockIdx.x * BLOCK + wave_first + lane;
    if (el >= n) return;
    Lane<C> ln(nullptr);
    load_elem<C>(a, reread(x + el * C::W), ln);
    load_modulus<C>(m, reread_uniform(nmod), ln);
    borrow_sweep<S>(a, m, a, 0);                 // p - row, row < p
    store_elem<C>(x + el * C::W, a, ln);
}
template <class C>
__global__ void __launch_bounds__(BLOCK, 2)
k_jacobi_fix_lanes(u32* __restrict__ x, size_t n, const u32* __restrict__ nmod) {
    constexpr int L = C::L;
    Lane<C> ln(nullptr);
    size_t el = (size_t)blockIdx.x * C::EPB + ln.eslot;
    bool live = el < n;
    size_t ec = live ? el : n - 1;
    u32 a[L], m[L];
    load_elem<C>(a, x + ec * C::W, ln);
    load_modulus<C>(m, nmod, ln);
    const bool negate = jacobi_symbol_lanes<C>(a, m, ln) == -1;      // (the same on all lanes of the element)
    load_elem<C>(a, reread(x + ec * C::W), ln);
    load_modulus<C>(m, reread(nmod), ln);
    u32 d[L];
    sub_full<C>(d, m, a, ln);                    // every lane of the wave takes part in the cross-lane borrows
    if (live && negate) store_elem<C>(x + el * C::W, d, ln);
}

}  // namespace vmn
