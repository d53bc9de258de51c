// encode_layout.h — messages as group elements and back: the byte-level rules of the text interface behind a session
// (`vmnc -plain -outi native`: ProtocolElGamalInterfaceString.decodePlaintexts, :197-236; demoCiphertexts, :315-428).
// Plain C++, __host__ __device__ under hipcc, no HIP dependency: the tests build it alone (tests/encode_layout_harness.cpp).
//
// [NOT-IN-REF: VCR ModPGroup, safe-prime encoding; unpinned]  pGroup.encode / decode / getEncodeLength are VCR code, which is not
// part of the reference's tree.  The rule, on integers, for a modular group with p = 2q + 1 ("encoding" 1 of
// ProtocolElGamalInterfaceJSONDecode.java:180-188); b = the bit length of p:
//   L = floor((b - 2) / 8) - 4 is the encode length (59 / 123 / 251 / 379 / 507 at 512 / 1024 / 2048 / 3072 / 4096 bits); the group
//   is supported when L >= 1.  Then 2^(8 (L + 4)) <= 2^(b - 2) <= q.
//   encode(m), 0 <= |m| <= L:  T = be32(|m|) || m || 0^(L - |m|), L + 4 bytes; |m| = 0: T[4] = 1, so that the value is not 0;
//       v = T as a big-endian integer, 0 < v < 2^(8 (L + 4)); the element is v if (v / p) = 1, else p - v (-1 is a non-residue
//       since p = 3 mod 4: exactly one of the two is in the group).
//   decode(e):  v = e if e <= q, else p - e; T = v on L + 4 bytes.  The element is ILL-FORMED when v >= 2^(8 (L + 4)) or
//       be32(T[0:4]) > L, and its message is then empty; otherwise the message is T[4 : 4 + len], the bytes behind it are ignored.
//   ncomp components (keywidth * width, flat order): component c encodes the bytes [c L, min((c + 1) L, |m|)) of the message, the
//       later ones the empty message; decoding concatenates the components' messages in order, whatever their lengths.
//   text: a decoded line is the concatenation with every 0x0A and 0x0D byte removed, then \n.  UTF-8 well-formedness (Unicode
//       table 3-7: no overlong forms, no surrogates, nothing above U+10FFFF) is judged on the concatenation BEFORE the removal, as
//       Java decodes before it strips.  A line that is not well-formed is written byte for byte and reported
//       [NOT-IN-REF: Java substitutes U+FFFD].  On the way in a line is its bytes.
// A record is the value of one component of one line as the import / export kernels take it: big-endian on `nbytes` bytes, the
// group's wire width (>= L + 4), T right-aligned in it.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define VMN_ENCODE_HD __host__ __device__
#else
#define VMN_ENCODE_HD
#endif

namespace vmn {
namespace encode {

constexpr size_t LENGTH_BYTES = 4;            // be32(|m|) in front of the message
constexpr size_t MAX_COMPONENTS = 65536;      // the bound of the other text interfaces
constexpr uint32_t ILL_FORMED = 0xffffffffu;  // the length of a record that holds no message

// L for a modulus of `bits` bits (0: no message fits)
VMN_ENCODE_HD inline size_t encode_length(size_t bits) {
    if (bits < 2) return 0;
    const size_t t = (bits - 2) / 8;
    return t > LENGTH_BYTES ? t - LENGTH_BYTES : 0;
}

// the bytes of a message of mlen bytes that component c holds
VMN_ENCODE_HD inline uint64_t piece_length(uint64_t mlen, uint64_t c, uint64_t L) {
    const uint64_t before = c * L;
    if (mlen <= before) return 0;
    return mlen - before < L ? mlen - before : L;
}

// byte k (0 = most significant) of the record of component c for the message msg[0, mlen), mlen <= ncomp L: never reads a
// byte outside msg[c L, c L + piece)
VMN_ENCODE_HD inline uint8_t record_byte(size_t k, size_t nbytes, size_t L, uint64_t c, const uint8_t* msg, uint64_t mlen) {
    const size_t pad = nbytes - (L + LENGTH_BYTES);
    if (k < pad) return 0;
    const size_t t = k - pad;
    const uint64_t piece = piece_length(mlen, c, L);
    if (t < LENGTH_BYTES) return (uint8_t)(piece >> (8 * (LENGTH_BYTES - 1 - t)));
    const size_t j = t - LENGTH_BYTES;
    if (j < piece) return msg[c * L + j];
    return piece == 0 && j == 0 ? 1 : 0;
}

// The fold of decode() on a record, in place: rec (a value below p, big-endian on nbytes bytes) becomes v = min(rec, p - rec) --
// e <= q iff e < p - e, p odd -- and the message length is returned, ILL_FORMED when v >= 2^(8 (L + 4)) or the length word
// exceeds L.  Only the low L + 4 bytes of v are written (the rest of a well-formed v is zero); p_be, q_be: the two primes on nbytes.
VMN_ENCODE_HD inline uint32_t fold_record(uint8_t* rec, size_t nbytes, size_t L, const uint8_t* p_be, const uint8_t* q_be) {
    const size_t pad = nbytes - (L + LENGTH_BYTES);
    size_t k = 0;
    while (k < nbytes && rec[k] == q_be[k]) ++k;
    const bool upper = k < nbytes && rec[k] > q_be[k];             // rec > q: the value is p - rec
    uint8_t high = 0;                                              // OR of the bytes of v above T
    if (upper) {
        int borrow = 0;
        for (size_t i = nbytes; i-- > 0;) {
            const int d = (int)p_be[i] - (int)rec[i] - borrow;
            borrow = d < 0;
            const uint8_t b = (uint8_t)(d & 0xff);
            if (i >= pad) rec[i] = b;
            else high |= b;
        }
    } else {
        for (size_t i = 0; i < pad; ++i) high |= rec[i];
    }
    if (high) return ILL_FORMED;
    const uint32_t len = (uint32_t)rec[pad] << 24 | (uint32_t)rec[pad + 1] << 16 | (uint32_t)rec[pad + 2] << 8 | (uint32_t)rec[pad + 3];
    return len > L ? ILL_FORMED : len;
}

// UTF-8 well-formedness, one byte at a time (Unicode 15 table 3-7).  need: continuation bytes outstanding; lo, hi: the range of
// the next one (the second byte of E0, ED, F0, F4 is narrower than 80..BF: overlong forms, surrogates, above U+10FFFF).
struct Utf8 {
    uint8_t need = 0, lo = 0x80, hi = 0xBF;
    bool bad = false;
    VMN_ENCODE_HD void step(uint8_t b) {
        if (need == 0) {
            lo = 0x80;
            hi = 0xBF;
            if (b < 0x80) return;
            if (b >= 0xC2 && b <= 0xDF) need = 1;
            else if (b >= 0xE0 && b <= 0xEF) {
                need = 2;
                if (b == 0xE0) lo = 0xA0;
                if (b == 0xED) hi = 0x9F;
            } else if (b >= 0xF0 && b <= 0xF4) {
                need = 3;
                if (b == 0xF0) lo = 0x90;
                if (b == 0xF4) hi = 0x8F;
            } else bad = true;                                     // a lone continuation byte, C0, C1, F5..FF
            return;
        }
        if (b < lo || b > hi) {
            bad = true;
            need = 0;
            return;
        }
        --need;
        lo = 0x80;
        hi = 0xBF;
    }
    VMN_ENCODE_HD bool wellformed() const { return !bad && need == 0; }        // (a sequence cut off at the end is none)
};

VMN_ENCODE_HD inline bool stripped(uint8_t b) { return b == 0x0A || b == 0x0D; }

}  // namespace encode
}  // namespace vmn
