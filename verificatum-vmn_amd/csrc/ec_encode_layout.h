// ec_encode_layout.h — messages as points of a curve group and back: the rule of the text interface behind a curve session
// (`vmnc -plain -outi native`: ProtocolElGamalInterfaceString.decodePlaintexts, :197-236; demoCiphertexts, :315-428).
// Plain C++, __host__ __device__ under hipcc, no HIP dependency: the tests build it alone (tests/point_encode_layout_harness.cpp).
// record_byte, piece_length, Utf8 and stripped of encode_layout.h serve unchanged.
//
// [NOT-IN-REF: VCR ECqPGroup; unpinned]  encode / decode / getEncodeLength of ECqPGroup are VCR code, which is not part of the
// reference's tree.  The rule built here, on integers, for a curve y^2 = x^3 + a x + b over F_p of cofactor 1 (every named curve
// of the library: a point on the curve is a group element); b = the bit length of p:
//   L = floor((b - 2) / 8) - 5 is the encode length -- one byte less than over a modular group, the byte is the counter
//   (18 / 22 / 24 / 26 / 34 / 42 / 58 / 59 at 192 / 224 / 239 / 256 / 320 / 384 / 512 / 521 bits); the group is supported when L >= 1.
//   encode(m), 0 <= |m| <= L:  T = be32(|m|) || m || 0^(L - |m|), L + 4 bytes; |m| = 0: T[4] = 1 -- the record that
//       encode::record_byte writes at nbytes = L + 4.  x = 256 int(T) + c with c the LEAST counter in 0..255 for which
//       x^3 + a x + b is a NONZERO square mod p; y = the SMALLER of the two roots as integers in [1, p - 1] (the convention of
//       the random points, k_ec_random_points).  0 < x < 2^(8 (L + 5)) <= 2^(b - 2) < p, and c never carries into T.
//   decode(P):  the element is ILL-FORMED, its message empty, when P is the point at infinity, when x >= 2^(8 (L + 5)), or when
//       the length word of T = floor(x / 256) exceeds L; otherwise the message is T[4 : 4 + len].  The counter byte and y are
//       ignored: (x, y) and (x, p - y) decode alike, and so do two points that differ in the counter alone.
//   no counter fits: each x is a nonzero square with chance ~1/2, so all 256 fail with chance 2^-256 per element; the search is
//       bounded all the same, and an exhausted one is a format error of the call (vmn_ec_arrays_from_textlines).
//   ncomp components, the removal of 0x0A / 0x0D and the UTF-8 verdict (judged before the removal, a line that is not
//       well-formed written byte for byte): as stated in encode_layout.h, word for word.
// A point record is a point as the export kernel writes it: x || y, big-endian on `nbytes` bytes each (the wire width of a
// coordinate, > L + 5), the point at infinity all 0xff.
#pragma once
#include "encode_layout.h"

namespace vmn {
namespace encode {

constexpr size_t COUNTER_BYTES = 1;           // the byte behind T that the search counts in
constexpr unsigned COUNTER_ROUNDS = 256;      // the values it takes: the bound of the search loop

// L for a field prime of `bits` bits (0: no message fits)
VMN_ENCODE_HD inline size_t point_encode_length(size_t bits) {
    const size_t modular = encode_length(bits);
    return modular > COUNTER_BYTES ? modular - COUNTER_BYTES : 0;
}

// decode() on a point record: rec = x || y on nbytes bytes each; T (L + 4 bytes) goes to dst and the message length is
// returned, ILL_FORMED -- dst then all zero -- for the point at infinity, for x >= 2^(8 (L + 5)) and for a length word above L.
// Reads 2 nbytes bytes, writes L + 4.  nbytes >= L + 5.
VMN_ENCODE_HD inline uint32_t fold_point_record(uint8_t* dst, const uint8_t* rec, size_t nbytes, size_t L) {
    const size_t tbytes = L + LENGTH_BYTES, pad = nbytes - (tbytes + COUNTER_BYTES);
    uint8_t allff = 0xff, high = 0;
    for (size_t i = 0; i < 2 * nbytes; ++i) allff &= rec[i];
    for (size_t i = 0; i < pad; ++i) high |= rec[i];
    const uint8_t* T = rec + pad;
    const uint32_t len = (uint32_t)T[0] << 24 | (uint32_t)T[1] << 16 | (uint32_t)T[2] << 8 | (uint32_t)T[3];
    const bool ill = allff == 0xff || high != 0 || len > L;
    for (size_t i = 0; i < tbytes; ++i) dst[i] = ill ? 0 : T[i];
    return ill ? ILL_FORMED : len;
}

}  // namespace encode
}  // namespace vmn
