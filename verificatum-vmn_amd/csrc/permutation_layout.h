// permutation_layout.h — a prover's secret permutation from one PRG seed: the rule behind vmn_permutation_from_prg
// (`Permutation.random(size, randomSource, rbitlen)`: mixnet/ShufflerElGamalSession.java:408-409, mixnet/PermutationCommitment.java:209).
// Plain C++, __host__ __device__ under hipcc, no HIP dependency: the tests build it alone (tests/permutation_layout_harness.cpp).
//
// [NOT-IN-REF: VCR Permutation.random; unpinned]  VCR's Permutation is not part of the reference's tree, and a prover's private
// randomness needs no interoperability.  The rule, for a table of n entries (n < 2^32) and 0 <= rbitlen <= 256:
//   kb = rbitlen + 2 ceil(log2(max(n, 2))) key bits, key_bytes = ceil(kb / 8) (at most (256 + 64 + 7) / 8 = 40).
//   key i = the i-th key_bytes bytes of PRG(seed) as a big-endian integer with the superfluous leading bits cleared -- the
//       convention of vmn_rarray_from_prg; a seed of 32 / 48 / 64 bytes selects SHA-256 / 384 / 512 as everywhere else.
//   pi[j] = the index of the element of rank j in the total order (key_i, i): by key, ties broken by ascending index.
//   inv[i] = the rank of i, so inv[pi[j]] = j.  n = 0 gives the empty table, n = 1 gives [0].
// Why this is a draw of the reference's quality: conditioned on no two keys being equal the order of n independent uniform keys
// is exactly uniform over the n! orders.  Some tie occurs with probability at most C(n, 2) / 2^kb < n^2 / 2^(kb + 1), and
// 2^(2 ceil(log2 n)) >= n^2, so that is at most 2^-(rbitlen + 1).  The distribution of pi is therefore within statistical distance
// 2^-(rbitlen + 1) < 2^-rbitlen of uniform, which is what the reference means by rbitlen (ProtocolElGamal.java:277-306).
//
// The sort (csrc/permutation_kernels.h) is a least-significant-digit radix sort of the INDICES over the key bytes.  Digit d of a
// key is its byte key_bytes - 1 - d (digit 0 = the last byte); on the device the keys are kept digit-major ("planes"): digit d of
// key i is the byte planes[d n + i], so that a pass reads one byte of key[idx] and never moves a key.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#if !defined(__HIP_DEVICE_COMPILE__)
#include <algorithm>
#include <vector>
#endif

#if defined(__HIPCC__)
#define VMN_PERM_HD __host__ __device__
#else
#define VMN_PERM_HD
#endif

namespace vmn {
namespace permutation {

constexpr int MAX_RBITLEN = 256;
constexpr uint64_t MAX_N = 0xffffffffull;     // n < 2^32: the tables are uint32_t
constexpr size_t MAX_KEY_BYTES = 64;          // of keys handed in by the caller (vmn_permutation_from_keys); the rule needs <= 40

// ceil(log2(m)) for m >= 1
VMN_PERM_HD inline int ceil_log2(uint64_t m) {
    int b = 0;
    while (b < 64 && ((uint64_t)1 << b) < m) ++b;
    return b;
}
// kb for a table of n entries; 0 when n or rbitlen is out of range
VMN_PERM_HD inline int key_bits(uint64_t n, int rbitlen) {
    if (n > MAX_N || rbitlen < 0 || rbitlen > MAX_RBITLEN) return 0;
    return rbitlen + 2 * ceil_log2(n < 2 ? 2 : n);
}
VMN_PERM_HD inline size_t key_bytes(uint64_t n, int rbitlen) { return ((size_t)key_bits(n, rbitlen) + 7) / 8; }
// the mask of a key's first byte: the superfluous leading bits are cleared
VMN_PERM_HD inline uint8_t top_mask(int kb) { return kb % 8 ? (uint8_t)((1u << (kb % 8)) - 1) : (uint8_t)0xff; }

// digit d (0 = least significant byte) of key i in big-endian rows of nbytes bytes
VMN_PERM_HD inline uint8_t row_digit(const uint8_t* rows, size_t nbytes, size_t i, size_t d) { return rows[i * nbytes + (nbytes - 1 - d)]; }
// where digit d of key i lies in the digit-major planes of n keys
VMN_PERM_HD inline size_t plane_at(size_t n, size_t d, size_t i) { return d * n + i; }

#if !defined(__HIP_DEVICE_COMPILE__)
// The order as the rule states it, on the host: a stable sort of the indices by key (the harness checks it; nothing in the
// library's array paths calls it).  rows: n big-endian keys of nbytes bytes.
inline void reference_order(const uint8_t* rows, size_t nbytes, size_t n, std::vector<uint32_t>& pi) {
    pi.resize(n);
    for (size_t i = 0; i < n; ++i) pi[i] = (uint32_t)i;
    std::stable_sort(pi.begin(), pi.end(), [&](uint32_t a, uint32_t b) {
        return nbytes != 0 && std::memcmp(rows + (size_t)a * nbytes, rows + (size_t)b * nbytes, nbytes) < 0;
    });
}
inline void reference_inverse(const std::vector<uint32_t>& pi, std::vector<uint32_t>& inv) {
    inv.resize(pi.size());
    for (size_t j = 0; j < pi.size(); ++j) inv[pi[j]] = (uint32_t)j;
}
#endif

}  // namespace permutation
}  // namespace vmn
