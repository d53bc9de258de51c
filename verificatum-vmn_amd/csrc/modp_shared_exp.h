// modp_shared_exp.h — variants of K1 beside k_modpow: ONE exponent for the whole array (out[i] = x[i]^e, sliding window), for one
// array or for several arrays of one size in one launch (all under one exponent, or each array under its own), and two
// independent exponentiations of small arrays in one launch (k_modpow_jobs, at the end); and the product of several arrays'
// powers under one exponent each with ONE chain of squarings (k_modpow_expprod).
//
// The reference raises whole arrays to a single exponent in the decryption half of the mix-net -- the decryption factors
// f = u^(-x_j / c), a full-length secret exponent per party (elgamal/DistrElGamalSession.java:365-385) -- and in the
// verifiers (B^v, raisedu = u^rho: hvzk/PoSBasicTW.java:1028, mixnet/ShufflerElGamalSession.java:884-896).  With the exponent
// shared, every lane takes the same branch at every step, so the left-to-right SLIDING window is free of divergence: the
// host cuts the exponent into odd windows of at most w bits separated by runs of zeros (a list of "square s times, then
// multiply by x^d", d odd), the per-lane table holds the 2^(w-1) odd powers only, and a b-bit exponent costs about
// b / (w + 1) multiplications instead of the b / w of the fixed window k_modpow uses for per-element exponents (2047 bits,
// w = 7: 256 + 64 table products instead of 342 + 62).
#pragma once
#include "modp_kernels.h"

namespace vmn {

// One step of the schedule: `sq` squarings, then a multiplication by the odd power x^(2 idx + 1) (idx < 0: none -- the
// trailing zeros of the exponent).  The first step has sq = 0: the accumulator starts as that power.
struct SlideStep {
    int sq;
    int idx;
};

// steps s_lo .. s_hi - 1 of the schedule (wave-uniform: every lane walks the same steps).  (A half-open range: with `s <= s_hi`
// the compiler lays the loop of k_modpow_shared<Cfg<19, 1>> out with register copies at its edges, 115 registers instead of 76.)
template <class C>
__device__ __forceinline__ void slide_steps(u32 (&a)[C::L], const SlideStep* __restrict__ steps, int s_lo, int s_hi,
                                            const u32* __restrict__ tb, const Lane<C>& ln, const u32 (&nn)[C::L], u32 n0inv) {
#pragma unroll 1
    for (int s = s_lo; s < s_hi; ++s) {
        const int sq = steps[s].sq, idx = steps[s].idx;
        sqr_times<C>(a, sq, ln, nn, n0inv);
        if (idx >= 0) mul_by_row<C>(a, tb + (size_t)idx * C::W, ln, nn, n0inv);
    }
}

// The arrays of one launch.  A party's decryption factors at width w are w arrays raised to ONE exponent
// (DistrElGamalSession.java:365-389 over a product group): one launch per array would choose its geometry, plan its phases and
// end in a tail w times, and at the reference's own sizes (10^4 elements) each leaves most of the device without a wave.  The
// kernels below therefore walk GLOBAL tiles: tile T belongs to array T / ntiles and is that array's tile T % ntiles (block-uniform:
// the pointers are picked with scalar instructions), and every array keeps its own ragged last tile.  One array is the case k = 1
// of the same body (OneArray: no table, no division).
constexpr int SHARED_ARRAYS = 8;
struct SharedArrays {
    static constexpr bool OWN_SCHEDULES = false;
    const u32* x[SHARED_ARRAYS];
    u32* out[SHARED_ARRAYS];
    // the array of global tile T, and T's index among that array's tiles (the host keeps k * ntiles below 2^32)
    __device__ __forceinline__ u32 array_of(size_t T, u32 ntiles) const { return (u32)T / ntiles; }
    __device__ __forceinline__ size_t tile_of(size_t T, u32 a, u32 ntiles) const { return (u32)T - a * ntiles; }
    __device__ __forceinline__ const u32* x_of(u32 a) const { return x[a]; }
    __device__ __forceinline__ u32* out_of(u32 a) const { return out[a]; }
    // (one schedule for the launch)
    __device__ __forceinline__ const SlideStep* steps_of(u32, const SlideStep* steps) const { return steps; }
    __device__ __forceinline__ int nsteps_of(u32, int nsteps) const { return nsteps; }
};
struct OneArray {
    static constexpr bool OWN_SCHEDULES = false;
    const u32* x;
    u32* out;
    __device__ __forceinline__ u32 array_of(size_t, u32) const { return 0; }
    __device__ __forceinline__ size_t tile_of(size_t T, u32, u32) const { return T; }
    __device__ __forceinline__ const u32* x_of(u32) const { return x; }
    __device__ __forceinline__ u32* out_of(u32) const { return out; }
    __device__ __forceinline__ const SlideStep* steps_of(u32, const SlideStep* steps) const { return steps; }
    __device__ __forceinline__ int nsteps_of(u32, int nsteps) const { return nsteps; }
};
// Arrays that each have an exponent of their OWN.  Under a public key of width kappa a party's decryption factors are
// f_c = u_c^(-x_{c mod kappa} / c_k) (DistrElGamalSession.java:365-389 over (G^kappa)^omega): kappa different exponents over
// kappa omega arrays of one size.  The schedules lie one after the other in the launch's one buffer of steps: array a walks the
// `count[a]` steps from `first[a]` on.  Everything else is the launch's: one window width (the tables of odd powers have one
// size), one phase count.  In the phased body a phase's steps come from the array's own count, so an array with fewer steps
// than the launch has phases passes through phases without a step: it loads its value from out[], stores it and hands over.
struct EachArrays {
    static constexpr bool OWN_SCHEDULES = true;
    const u32* x[SHARED_ARRAYS];
    u32* out[SHARED_ARRAYS];
    u32 first[SHARED_ARRAYS];
    int count[SHARED_ARRAYS];
    __device__ __forceinline__ u32 array_of(size_t T, u32 ntiles) const { return (u32)T / ntiles; }
    __device__ __forceinline__ size_t tile_of(size_t T, u32 a, u32 ntiles) const { return (u32)T - a * ntiles; }
    __device__ __forceinline__ const u32* x_of(u32 a) const { return x[a]; }
    __device__ __forceinline__ u32* out_of(u32 a) const { return out[a]; }
    __device__ __forceinline__ const SlideStep* steps_of(u32 a, const SlideStep* steps) const { return steps + first[a]; }
    __device__ __forceinline__ int nsteps_of(u32 a, int) const { return count[a]; }
};

// `total` global tiles, `ntiles` of them per array of n elements; a table per lane slot in `tab`
template <class C, class A>
__device__ __forceinline__ void modpow_shared_tiles(const A& arrs, u32 ntiles, size_t total, const SlideStep* __restrict__ steps, int nsteps,
                                                    int tsize, size_t n, const u32* __restrict__ nmod, u32 n0inv, u32* __restrict__ tab, u32* lds) {
    constexpr int W = C::W;
    Lane<C> ln(lds);
    u32 nn[C::L];
    load_modulus<C>(nn, nmod, ln);
    u32* mytab = tab + ((size_t)blockIdx.x * C::EPB + ln.eslot) * (size_t)tsize * W;
    for (size_t T = blockIdx.x; T < total; T += gridDim.x) {
        const u32 arr = arrs.array_of(T, ntiles);
        const size_t t = arrs.tile_of(T, arr, ntiles);
        const u32* __restrict__ x = arrs.x_of(arr);
        u32* __restrict__ out = arrs.out_of(arr);
        const SlideStep* __restrict__ st = arrs.steps_of(arr, steps);
        size_t el = t * C::EPB + ln.eslot;
        bool live = el < n;
        size_t ec = live ? el : n - 1;
        u32 a[C::L];
        odd_power_table<C>(a, mytab, tsize, x + ec * W, ln, nn, n0inv);
        load_elem<C>(a, mytab + (size_t)st[0].idx * W, ln);
        slide_steps<C>(a, st, 1, arrs.nsteps_of(arr, nsteps), mytab, ln, nn, n0inv);
        canonicalize<C>(a, nn, ln);
        if (live) store_elem<C>(out + el * W, a, ln);
    }
}

// The same for more than one round of tiles: the schedule's steps in phases from a queue of (phase, global tile) units
// (UnitQueue, modp_kernels.h); a tile's table of odd powers lives in a table of its own, indexed by the GLOBAL element
// T * EPB + slot.  The decryption factors of a party -- one full-length secret exponent over every ciphertext -- are this
// kernel's large case.
template <class C, class A>
__device__ __forceinline__ void modpow_shared_units(const A& arrs, u32 ntiles, u32 total, const SlideStep* __restrict__ steps, int nsteps,
                                                    int tsize, size_t n, const u32* __restrict__ nmod, u32 n0inv, u32* __restrict__ tab,
                                                    int phases, u32* __restrict__ queue, u32* __restrict__ done, u32* s_unit, u32* lds) {
    constexpr int W = C::W;
    Lane<C> ln(lds);
    u32 nn[C::L];
    load_modulus<C>(nn, nmod, ln);
    const int M_launch = nsteps - 1;                     // steps of the main loop (step 0 is the first table read)
    UnitQueue q(queue, done, s_unit, total, phases);
    while (q.take()) {
        const int ph = q.ph;
        const u32 arr = arrs.array_of(q.t, ntiles);
        const size_t t = arrs.tile_of(q.t, arr, ntiles);
        const u32* __restrict__ x = arrs.x_of(arr);
        u32* __restrict__ out = arrs.out_of(arr);
        const SlideStep* __restrict__ st = arrs.steps_of(arr, steps);
        int M = M_launch;                                    // (one schedule for the launch: computed once, before the queue)
        if constexpr (A::OWN_SCHEDULES) M = arrs.nsteps_of(arr, nsteps) - 1;
        size_t el = t * C::EPB + ln.eslot;
        bool live = el < n;
        size_t ec = live ? el : n - 1;
        u32* mytab = tab + ((size_t)q.t * C::EPB + ln.eslot) * (size_t)tsize * W;
        u32 a[C::L];
        if (ph == 0) {
            odd_power_table<C>(a, mytab, tsize, x + ec * W, ln, nn, n0inv);
            load_elem<C>(a, mytab + (size_t)st[0].idx * W, ln);
        } else {
            load_elem<C>(a, out + ec * W, ln);
        }
        // the steps of this phase: 1 + M ph / P  up to  M (ph + 1) / P (s_hi: one past it; none where M < P leaves the phase empty)
        const int s_lo = 1 + (int)((long)M * ph / phases), s_hi = 1 + (int)((long)M * (ph + 1) / phases);
        slide_steps<C>(a, st, s_lo, s_hi, mytab, ln, nn, n0inv);
        if (q.last()) canonicalize<C>(a, nn, ln);
        if (live) store_elem<C>(out + el * W, a, ln);
        q.hand_over();
    }
}

template <class C>
__global__ void __launch_bounds__(BLOCK, C::MINW)
k_modpow_shared(u32* __restrict__ out, const u32* __restrict__ x, const SlideStep* __restrict__ steps, int nsteps, int tsize, size_t n,
                const u32* __restrict__ nmod, u32 n0inv, u32* __restrict__ tab) {
    extern __shared__ u32 lds[];
    modpow_shared_tiles<C>(OneArray{x, out}, 0, (n + C::EPB - 1) / C::EPB, steps, nsteps, tsize, n, nmod, n0inv, tab, lds);
}
template <class C>
__global__ void __launch_bounds__(BLOCK, C::MINW)
k_modpow_shared_phased(u32* __restrict__ out, const u32* __restrict__ x, const SlideStep* __restrict__ steps, int nsteps, int tsize,
                       size_t n, const u32* __restrict__ nmod, u32 n0inv, u32* __restrict__ tab, int phases, u32* __restrict__ queue,
                       u32* __restrict__ done) {
    extern __shared__ u32 lds[];
    __shared__ u32 s_unit;
    modpow_shared_units<C>(OneArray{x, out}, 0, (u32)((n + C::EPB - 1) / C::EPB), steps, nsteps, tsize, n, nmod, n0inv, tab, phases, queue,
                           done, &s_unit, lds);
}
// several arrays of n elements each (ntiles tiles each, `total` = arrays x ntiles)
template <class C>
__global__ void __launch_bounds__(BLOCK, C::MINW)
k_modpow_shared_multi(SharedArrays arrs, u32 ntiles, u32 total, const SlideStep* __restrict__ steps, int nsteps, int tsize, size_t n,
                      const u32* __restrict__ nmod, u32 n0inv, u32* __restrict__ tab) {
    extern __shared__ u32 lds[];
    modpow_shared_tiles<C>(arrs, ntiles, total, steps, nsteps, tsize, n, nmod, n0inv, tab, lds);
}
template <class C>
__global__ void __launch_bounds__(BLOCK, C::MINW)
k_modpow_shared_multi_phased(SharedArrays arrs, u32 ntiles, u32 total, const SlideStep* __restrict__ steps, int nsteps, int tsize, size_t n,
                             const u32* __restrict__ nmod, u32 n0inv, u32* __restrict__ tab, int phases, u32* __restrict__ queue,
                             u32* __restrict__ done) {
    extern __shared__ u32 lds[];
    __shared__ u32 s_unit;
    modpow_shared_units<C>(arrs, ntiles, total, steps, nsteps, tsize, n, nmod, n0inv, tab, phases, queue, done, &s_unit, lds);
}

// several arrays of n elements each, array a under the schedule steps[arrs.first[a]] .. of arrs.count[a] steps
template <class C>
__global__ void __launch_bounds__(BLOCK, C::MINW)
k_modpow_shared_each(EachArrays arrs, u32 ntiles, u32 total, const SlideStep* __restrict__ steps, int tsize, size_t n,
                     const u32* __restrict__ nmod, u32 n0inv, u32* __restrict__ tab) {
    extern __shared__ u32 lds[];
    modpow_shared_tiles<C>(arrs, ntiles, total, steps, 0, tsize, n, nmod, n0inv, tab, lds);
}
template <class C>
__global__ void __launch_bounds__(BLOCK, C::MINW)
k_modpow_shared_each_phased(EachArrays arrs, u32 ntiles, u32 total, const SlideStep* __restrict__ steps, int tsize, size_t n,
                            const u32* __restrict__ nmod, u32 n0inv, u32* __restrict__ tab, int phases, u32* __restrict__ queue,
                            u32* __restrict__ done) {
    extern __shared__ u32 lds[];
    __shared__ u32 s_unit;
    modpow_shared_units<C>(arrs, ntiles, total, steps, 0, tsize, n, nmod, n0inv, tab, phases, queue, done, &s_unit, lds);
}

// K3' over arrays: out[i] = prod_j x_j[i]^(c_j), the c_j the same for every element (pGroup.expProd(bases[], integers[],
// bitLength), elgamal/DistrElGamalSessionBasic.java:465-503).  ONE chain of squarings for all bases (Straus): the bases of a
// product are cut into groups of up to EXPPROD_GROUP, a lane's table holds for every group the 2^g - 1 products of its subsets
// (row (mask - 1) of the group's EXPPROD_GROUP_ROWS rows = the product of the bases whose bit is set in `mask`; one product per
// row: the row without the lowest base, times that base), and the host's schedule is a list of SlideStep as above -- `sq`
// squarings, then the product by the table row `idx` that a column of exponent bits selects (expprod_schedule.h).
//
// A launch computes up to two products over the SAME input arrays, the positive and the negative part of a signed exponent
// vector, as the tiles of two "arrays" with a schedule each, exactly as EachArrays does: global tile T belongs to product
// T / ntiles.  (Two accumulators in one lane do not fit: the one-lane 2048-bit kernels already sit at ~245 VGPRs.)  The host
// inverts the negative product with the batched inversion and multiplies.
//
// EXPPROD_BASES, the bases of one launch: two groups of four = 30 table rows per lane slot, half of the 64 rows the sliding
// window of a 2048-bit exponent takes (w = 7), so the launch never asks for more scratch than k_modpow_shared does; every further
// group adds up to one product per exponent bit, the same as a launch of its own would, while a launch of its own has the
// squarings and the tail again -- which for the few-bit Lagrange integers this serves costs less than a 45-row table per slot
// costs every tile.  Beyond the limit the host multiplies the launches' results.
constexpr int EXPPROD_GROUP = 4;
constexpr int EXPPROD_GROUP_ROWS = (1 << EXPPROD_GROUP) - 1;
constexpr int EXPPROD_BASES = 8;
constexpr int EXPPROD_ROWS = EXPPROD_BASES / EXPPROD_GROUP * EXPPROD_GROUP_ROWS;
struct ExpProdArrays {
    const u32* x[EXPPROD_BASES];              // the launch's input arrays
    u32* out[2];                              // the two products
    u32 first[2];                             // product s walks count[s] steps from steps[first[s]] on
    int count[2];
    int nb[2];                                // bases of product s: x[base[s][0 .. nb[s] - 1]], in groups of EXPPROD_GROUP
    unsigned char base[2][EXPPROD_BASES];
    int trows;                                // table rows per lane slot: EXPPROD_GROUP_ROWS per group of the longer product
};
// the joint table of product s of the element at index ec, into tb (a: work registers)
template <class C>
__device__ __forceinline__ void subset_product_table(u32 (&a)[C::L], u32* tb, const ExpProdArrays& arrs, u32 s, size_t ec, const Lane<C>& ln,
                                                     const u32 (&nn)[C::L], u32 n0inv) {
    constexpr int W = C::W;
    const int nb = arrs.nb[s];
#pragma unroll 1
    for (int g0 = 0; g0 < nb; g0 += EXPPROD_GROUP) {
        u32* gt = tb + (size_t)(g0 / EXPPROD_GROUP * EXPPROD_GROUP_ROWS) * W;
        const int gs = nb - g0 < EXPPROD_GROUP ? nb - g0 : EXPPROD_GROUP;
#pragma unroll 1
        for (u32 mask = 1; mask < (1u << gs); ++mask) {
            const u32 low = mask & (0u - mask), rest = mask ^ low;
            if (rest == 0) {
                load_elem<C>(a, arrs.x[arrs.base[s][g0 + (__ffs(low) - 1)]] + ec * W, ln);
            } else {
                load_elem<C>(a, gt + (size_t)(rest - 1) * W, ln);
                mul_by_row<C>(a, gt + (size_t)(low - 1) * W, ln, nn, n0inv);
            }
            store_elem<C>(gt + (size_t)(mask - 1) * W, a, ln);
        }
    }
}
// `total` global tiles, `ntiles` per product of n elements; a table of arrs.trows rows per lane slot in `tab`
template <class C>
__global__ void __launch_bounds__(BLOCK, C::MINW)
k_modpow_expprod(ExpProdArrays arrs, u32 ntiles, u32 total, const SlideStep* __restrict__ steps, u32 n32, const u32* __restrict__ nmod,
                 u32 n0inv, u32* tab) {
    extern __shared__ u32 lds[];
    constexpr int W = C::W;
    Lane<C> ln(lds);
    u32 nn[C::L];
    load_modulus<C>(nn, nmod, ln);
    u32* mytab = tab + ((size_t)blockIdx.x * C::EPB + ln.eslot) * (size_t)arrs.trows * W;
    // 32-bit tile and element indices (n32 elements per product): the host keeps n below 2^31, hence `total` below 2^29, so
    // T + gridDim.x and a ragged tile's indices cannot wrap.  In Cfg<74, 1> the 74 limbs of the modulus live in scalar registers,
    // and every scalar held across the loop of steps is one they need: 64-bit counters, a division for the product's number and
    // an output pointer looked up in front of the loop cost 8 spilled SGPRs, this form none.
    for (u32 T = blockIdx.x; T < total; T += gridDim.x) {
        const u32 s = T >= ntiles ? 1u : 0u;                   // (block-uniform; a launch has at most two products)
        const u32 t = s ? T - ntiles : T;
        const SlideStep* __restrict__ st = steps + arrs.first[s];
        const u32 el = t * C::EPB + ln.eslot;
        const size_t ec = el < n32 ? el : n32 - 1;
        u32 a[C::L];
        subset_product_table<C>(a, mytab, arrs, s, ec, ln, nn, n0inv);
        load_elem<C>(a, mytab + (size_t)st[0].idx * W, ln);
        slide_steps<C>(a, st, 1, arrs.count[s], mytab, ln, nn, n0inv);
        canonicalize<C>(a, nn, ln);
        // (the output pointer and the ragged edge are looked up HERE, behind the loop of steps, for the same reason)
        if (el < n32) store_elem<C>(arrs.out[s] + (size_t)el * W, a, ln);
    }
}

// Two independent exponentiations in ONE launch (small arrays): job 0 = out0[i] = x0[i]^e0 (one exponent for all), job 1 =
// out1[i] = x1[i]^e1[i] (per-element exponents).  A verifier's check (B) in its separate form needs B^v and B_shift^(k_E): at the
// reference's demo size (10^4 ciphertexts) each of the two kernels alone leaves 40 % of the SIMDs without a wave, and they
// used to run one after the other; as one grid (the first `tiles0` blocks work on job 0) they run side by side.  Fixed window
// `wbits` for both, one tile per block, per-lane tables in `tab` (gridDim.x * EPB * 2^wbits rows).
struct ModpowJob {
    u32* out;
    const u32* x;
    const u32* e;
    int ewords;
    size_t estride;        // words between the exponents of consecutive elements; 0 = one shared exponent
    int ebits;
    size_t n;
};
// one tile (C::EPB elements) of a job; `blocktab`: this block's table rows
template <class C>
__device__ __forceinline__ void modpow_job_tile(const ModpowJob& J, size_t t, int wbits, const u32* __restrict__ nmod, u32 n0inv,
                                                const u32* __restrict__ one_m, u32* __restrict__ blocktab, u32* lds) {
    constexpr int W = C::W;
    Lane<C> ln(lds);
    u32 nn[C::L];
    load_modulus<C>(nn, nmod, ln);
    const int tsize = 1 << wbits;
    u32* mytab = blocktab + (size_t)ln.eslot * (size_t)tsize * W;
    const int nwin = (J.ebits + wbits - 1) / wbits;
    size_t el = t * C::EPB + ln.eslot;
    bool live = el < J.n;
    size_t ec = live ? el : J.n - 1;
    const u32* ep = J.e + ec * J.estride;
    u32 a[C::L];
    window_table<C>(a, mytab, tsize, J.x + ec * W, one_m, ln, nn, n0inv);
    load_elem<C>(a, mytab + (size_t)exp_digit(ep, J.ewords, (nwin - 1) * wbits, wbits) * W, ln);      // the top window
    fixed_windows<C>(a, ep, J.ewords, wbits, nwin - 2, 0, mytab, ln, nn, n0inv);
    canonicalize<C>(a, nn, ln);
    if (live) store_elem<C>(J.out + el * W, a, ln);
}
template <class C>
__global__ void __launch_bounds__(BLOCK, C::MINW)
k_modpow_jobs(ModpowJob j0, ModpowJob j1, unsigned tiles0, int wbits, const u32* __restrict__ nmod, u32 n0inv,
              const u32* __restrict__ one_m, u32* __restrict__ tab) {
    extern __shared__ u32 lds[];
    const bool second = blockIdx.x >= tiles0;                        // (block-uniform)
    u32* blocktab = tab + (size_t)blockIdx.x * C::EPB * ((size_t)1 << wbits) * C::W;
    if (second) modpow_job_tile<C>(j1, blockIdx.x - tiles0, wbits, nmod, n0inv, one_m, blocktab, lds);
    else modpow_job_tile<C>(j0, blockIdx.x, wbits, nmod, n0inv, one_m, blocktab, lds);
}
// The same with the two jobs in DIFFERENT geometries of the same rows: the long job eight lanes per element, the short one
// four.  At 10^4 elements each the long chain (766 dependent products at 613 bits) sets the time of the launch; with eight
// lanes a product of that chain takes two thirds of the time, and the short job's four-lane tiles still fit beside it.
template <class CA, class CB>
__global__ void __launch_bounds__(BLOCK, (CA::MINW < CB::MINW ? CA::MINW : CB::MINW))
k_modpow_jobs_mixed(ModpowJob j0, ModpowJob j1, unsigned tiles0, int wbits, const u32* __restrict__ nmod, u32 n0inv,
                    const u32* __restrict__ one_m, u32* __restrict__ tab) {
    static_assert(CA::W == CB::W, "the two geometries read the same rows");
    extern __shared__ u32 lds[];
    constexpr int EPBMAX = CA::EPB > CB::EPB ? CA::EPB : CB::EPB;
    const bool second = blockIdx.x >= tiles0;                        // (block-uniform)
    u32* blocktab = tab + (size_t)blockIdx.x * EPBMAX * ((size_t)1 << wbits) * CA::W;
    if (second) modpow_job_tile<CB>(j1, blockIdx.x - tiles0, wbits, nmod, n0inv, one_m, blocktab, lds);
    else modpow_job_tile<CA>(j0, blockIdx.x, wbits, nmod, n0inv, one_m, blocktab, lds);
}

}  // namespace vmn
