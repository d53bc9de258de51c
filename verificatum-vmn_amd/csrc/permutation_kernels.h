// permutation_kernels.h — the index sort behind vmn_permutation_from_prg / _from_keys (the rule: csrc/permutation_layout.h).
//
// A least-significant-digit radix sort of the u32 INDICES over the key bytes; the keys themselves never move.
//   k_perm_planes    big-endian key rows (k_prg_rows' format, or the caller's) -> digit-major planes, and idx[i] = i
//   per key byte d, least significant first:
//     k_perm_hist    per tile: dig[e] = digit d of key idx[e] (one byte gathered per element, kept for the scatter), and the
//                    tile's histogram hist[g ntiles + tile]
//     (the exclusive scan of the histogram in digit-major order: k_u32_blocksum / k_u32_scan_top / k_u32_scan_apply, light_kernels.h)
//     k_perm_scatter per tile: out[offs[g ntiles + tile] + rank of e among the tile's elements of digit g] = idx[e]
//   k_perm_inverse   inv[pi[j]] = j
// A tile is SORT_TILE consecutive positions, cut into one contiguous piece per wave; a wave walks its piece 64 positions at a
// time.  The rank of a position among the positions of its digit is (elements of the digit in the waves before) + (in the
// earlier rounds of this wave) + (in the lower lanes of this round): the last from __ballot (64-bit on wave64: one ballot per
// digit bit gives the mask of the lanes that hold the same digit), the other two from counters in LDS that only the first lane
// of each such mask writes.  Positions therefore keep their order within a digit (the pass is stable), and nothing is counted
// or placed with an atomic: the output is the order (key, index) bit for bit, whatever the grid and from run to run.
// Per pass and element: 4 + 1 bytes read and 1 written by the histogram, 4 + 1 read and 4 written by the scatter (14 bytes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "permutation_layout.h"

namespace vmn {

namespace permutation {
constexpr int SORT_BLOCK = 256;                              // threads of a block (the launch helpers' BLOCK)
constexpr int SORT_WAVES = SORT_BLOCK / 64;
constexpr int SORT_ITEMS = 16;                               // positions per thread
constexpr int SORT_WAVE_PIECE = 64 * SORT_ITEMS;             // positions of a wave
constexpr int SORT_TILE = SORT_BLOCK * SORT_ITEMS;           // positions of a block: 4096
constexpr int RADIX = 256;                                   // one key byte per pass
static_assert(SORT_BLOCK == RADIX, "thread t of a block owns digit t in the per-digit steps");

// the lanes of this wave, among the valid ones, that hold the same digit as this lane (the value is unused in an invalid lane)
__device__ inline unsigned long long digit_peers(uint32_t g, bool valid) {
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (g >> b) & 1u;
        const unsigned long long m = __ballot(bit);
        peers &= bit ? m : ~m;
    }
    return peers;
}
}  // namespace permutation

// planes[d n + i] = digit d of key i (permutation::plane_at / row_digit), idx[i] = i.  One thread per key.
__global__ void __launch_bounds__(permutation::SORT_BLOCK) k_perm_planes(uint8_t* __restrict__ planes, uint32_t* __restrict__ idx,
                                                                         const uint8_t* __restrict__ rows, size_t nbytes, size_t n) {
    const size_t i = (size_t)blockIdx.x * permutation::SORT_BLOCK + threadIdx.x;
    if (i >= n) return;
    for (size_t d = 0; d < nbytes; ++d) planes[permutation::plane_at(n, d, i)] = permutation::row_digit(rows, nbytes, i, d);
    idx[i] = (uint32_t)i;
}

// One block per tile.  plane = the digits of this pass by key index (n bytes).
__global__ void __launch_bounds__(permutation::SORT_BLOCK) k_perm_hist(uint32_t* __restrict__ hist, uint8_t* __restrict__ dig,
                                                                       const uint32_t* __restrict__ idx, const uint8_t* __restrict__ plane,
                                                                       size_t n, uint32_t ntiles) {
    using namespace permutation;
    __shared__ uint32_t cnt[SORT_WAVES][RADIX];
    const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63u;
#pragma unroll
    for (int k = 0; k < SORT_WAVES; ++k) cnt[k][threadIdx.x] = 0;
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * SORT_TILE + (size_t)w * SORT_WAVE_PIECE + lane;
    for (int r = 0; r < SORT_ITEMS; ++r) {
        const size_t e = base + (size_t)r * 64;
        const bool valid = e < n;
        const uint32_t g = valid ? plane[idx[e]] : 0u;
        if (valid) dig[e] = (uint8_t)g;
        const unsigned long long peers = digit_peers(g, valid);
        // the first lane of each group of equal digits adds the group to the wave's counter; the next round may meet the digit
        // again in another lane, hence the barrier
        if (valid && (peers & ((1ull << lane) - 1)) == 0) cnt[w][g] += (uint32_t)__popcll(peers);
        __syncthreads();
    }
    uint32_t total = 0;
#pragma unroll
    for (int k = 0; k < SORT_WAVES; ++k) total += cnt[k][threadIdx.x];
    hist[(size_t)threadIdx.x * ntiles + blockIdx.x] = total;
}

// One block per tile.  offs = the exclusive prefix sums of hist (digit-major), dig = the digits k_perm_hist left, by position.
__global__ void __launch_bounds__(permutation::SORT_BLOCK) k_perm_scatter(uint32_t* __restrict__ out, const uint32_t* __restrict__ in,
                                                                          const uint8_t* __restrict__ dig, const uint32_t* __restrict__ offs,
                                                                          size_t n, uint32_t ntiles) {
    using namespace permutation;
    __shared__ uint32_t cnt[SORT_WAVES][RADIX];
    const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63u;
#pragma unroll
    for (int k = 0; k < SORT_WAVES; ++k) cnt[k][threadIdx.x] = 0;
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * SORT_TILE + (size_t)w * SORT_WAVE_PIECE + lane;
    uint32_t val[SORT_ITEMS], where[SORT_ITEMS];         // where = digit << 16 | rank within the wave's piece (< 1024)
#pragma unroll
    for (int r = 0; r < SORT_ITEMS; ++r) {
        const size_t e = base + (size_t)r * 64;
        const bool valid = e < n;
        const uint32_t g = valid ? dig[e] : 0u;
        val[r] = valid ? in[e] : 0u;
        const unsigned long long peers = digit_peers(g, valid);
        const unsigned long long below = peers & ((1ull << lane) - 1);
        const uint32_t before = valid ? cnt[w][g] : 0u;           // of this digit in the wave's earlier rounds
        where[r] = (g << 16) | (before + (uint32_t)__popcll(below));
        __syncthreads();                                          // every lane has read the counter
        if (valid && below == 0) cnt[w][g] = before + (uint32_t)__popcll(peers);
        __syncthreads();
    }
    // thread t: where the tile's elements of digit t go, wave by wave
    {
        uint32_t run = offs[(size_t)threadIdx.x * ntiles + blockIdx.x];
#pragma unroll
        for (int k = 0; k < SORT_WAVES; ++k) {
            const uint32_t c = cnt[k][threadIdx.x];
            cnt[k][threadIdx.x] = run;
            run += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < SORT_ITEMS; ++r) {
        const size_t e = base + (size_t)r * 64;
        if (e < n) out[(size_t)cnt[w][where[r] >> 16] + (where[r] & 0xffffu)] = val[r];
    }
}

__global__ void __launch_bounds__(permutation::SORT_BLOCK) k_perm_inverse(uint32_t* __restrict__ inv, const uint32_t* __restrict__ pi, size_t n) {
    const size_t j = (size_t)blockIdx.x * permutation::SORT_BLOCK + threadIdx.x;
    if (j < n) inv[pi[j]] = (uint32_t)j;
}

}  // namespace vmn
