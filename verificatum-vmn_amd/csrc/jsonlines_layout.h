// jsonlines_layout.h — the text of one line of the reference's `json` interface (ProtocolElGamalInterfaceJSON,
// ProtocolElGamalInterfaceJSONDecode): one ciphertext per line over a modular group, every number a decimal string.
// Plain C++, __host__ __device__ under hipcc, no HIP dependency: the tests build it alone (tests/jsonlines_layout_harness.cpp).
//
// What is written (exactly what the reference writes, ...JSONDecode.java:216-262, ...JSON.java:55-87):
//   ciphertext, width 1:   {"alpha":"A","beta":"B"}
//   ciphertext, width w:   [{"alpha":"A1","beta":"B1"},...,{"alpha":"Aw","beta":"Bw"}]        pair i = (u_i, v_i)
//   plaintext,  width 1:   "M"                         width w:   ["M1",...,"Mw"]
//   decimals as BigInteger.toString(10) gives them (no sign, no leading zero), no spaces, every line ended by \n.
// What is read: the written ciphertext form, and what Java's reader demonstrably accepts --
//   lines ended as readLine ends them (\n, \r, \r\n counted once; see light_kernels.h);
//   the two keys of a pair in either order;
//   spaces and tabs BETWEEN tokens (json.dumps writes ": " and ", ");
//   leading zeros in a number (new BigInteger("007", 10) is 7): the digit run of a number is not bounded by the modulus.
// [NOT-IN-REF] Everything else is a format defect of its line: a missing, duplicate, unknown or extra key; an empty number
//   string; a sign; a non-digit inside a number string; a backslash or a byte >= 0x80 anywhere (no token holds one); a pair
//   count different from the width; [...] at width 1 or a bare map at width > 1; anything -- white space too -- in front of the
//   first token or behind the closing bracket; a blank line.  The reference parses a line with VCR's SimpleJSON, which is not
//   part of its tree, and rejects the whole file without naming the line; here the smallest defective line is named.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define VMN_JSONLINES_HD __host__ __device__
#define VMN_JSONLINES_NO_UNROLL _Pragma("unroll 1")
#else
#define VMN_JSONLINES_HD
#define VMN_JSONLINES_NO_UNROLL
#endif

namespace vmn {
namespace jsonlines {

constexpr size_t PAIR_FRAMING = 22;           // {"alpha":"  ","beta":"  "}  = 10 + 10 + 2
constexpr size_t MAX_WIDTH = 65536;

// the longest line the writer produces over a modulus of dmax decimal digits, newline included
VMN_JSONLINES_HD inline size_t max_ciphertext_line(size_t dmax, size_t width) {
    const size_t pairs = width * (PAIR_FRAMING + 2 * dmax);
    return width == 1 ? pairs + 1 : 2 + pairs + (width - 1) + 1;
}
VMN_JSONLINES_HD inline size_t max_plaintext_line(size_t dmax, size_t width) {
    const size_t items = width * (2 + dmax);
    return width == 1 ? items + 1 : 2 + items + (width - 1) + 1;
}

// ---- the reader: one line, text[start, end), never a byte outside of it ---------------------------------------------------
VMN_JSONLINES_HD inline void skip_blanks(const uint8_t* text, uint64_t& at, uint64_t end) {
    while (at < end && (text[at] == ' ' || text[at] == '\t')) ++at;
}
VMN_JSONLINES_HD inline bool eat(const uint8_t* text, uint64_t& at, uint64_t end, uint8_t c) {
    if (at < end && text[at] == c) {
        ++at;
        return true;
    }
    return false;
}
// "alpha": 0, "beta": 1, anything else: -1
VMN_JSONLINES_HD inline int key(const uint8_t* text, uint64_t& at, uint64_t end) {
    const uint8_t* t = text + at;
    if (end - at >= 7 && t[0] == '"' && t[1] == 'a' && t[2] == 'l' && t[3] == 'p' && t[4] == 'h' && t[5] == 'a' && t[6] == '"') {
        at += 7;
        return 0;
    }
    if (end - at >= 6 && t[0] == '"' && t[1] == 'b' && t[2] == 'e' && t[3] == 't' && t[4] == 'a' && t[5] == '"') {
        at += 6;
        return 1;
    }
    return -1;
}
// every byte of v is one of '0'..'9': the high nibble is 3 and the low nibble + 6 does not reach 16
VMN_JSONLINES_HD inline bool eight_digits(uint64_t v) {
    return (v & 0xf0f0f0f0f0f0f0f0ull) == 0x3030303030303030ull && (((v & 0x0f0f0f0f0f0f0f0full) + 0x0606060606060606ull) & 0xf0f0f0f0f0f0f0f0ull) == 0;
}
// "digits": emit(comp, where the significant digits begin, how many there are) -- leading zeros stripped, "0" has none
template <class Emit>
VMN_JSONLINES_HD inline bool number(const uint8_t* text, uint64_t& at, uint64_t end, uint32_t comp, Emit& emit) {
    if (!eat(text, at, end, '"')) return false;
    const uint64_t first = at;
    while (at < end && text[at] == '0') ++at;
    const uint64_t sig = at;
    while (end - at >= 8) {                                   // eight digits at a time while all eight are digits
        uint64_t v;
        __builtin_memcpy(&v, text + at, 8);
        if (!eight_digits(v)) break;
        at += 8;
    }
    while (at < end && (uint8_t)(text[at] - '0') < 10) ++at;
    if (at == first) return false;                            // empty, a sign, a non-digit at once
    const uint64_t stop = at;
    if (!eat(text, at, end, '"')) return false;               // a non-digit inside, or the line ends in the number
    emit(comp, sig, stop - sig);
    return true;
}
// { "key" : "digits" , "key" : "digits" } with the two keys distinct (one loop over the two members: the kernel holds one copy)
template <class Emit>
VMN_JSONLINES_HD inline bool pair_map(const uint8_t* text, uint64_t& at, uint64_t end, uint32_t pair, uint32_t width, Emit& emit) {
    if (!eat(text, at, end, '{')) return false;
    int first = -1;
    VMN_JSONLINES_NO_UNROLL
    for (int m = 0; m < 2; ++m) {
        skip_blanks(text, at, end);
        if (m == 1) {
            if (!eat(text, at, end, ',')) return false;
            skip_blanks(text, at, end);
        }
        const int k = key(text, at, end);
        if (k < 0 || k == first) return false;
        first = k;
        skip_blanks(text, at, end);
        if (!eat(text, at, end, ':')) return false;
        skip_blanks(text, at, end);
        if (!number(text, at, end, k ? width + pair : pair, emit)) return false;
    }
    skip_blanks(text, at, end);
    return eat(text, at, end, '}');
}

// A ciphertext line of `width` >= 1: true when it is well formed; emit(c, begin, count) has then been called once for each of the
// 2 width components c (u_1..u_w at 0..w-1, v_1..v_w at w..2w-1), begin inside [start, end) and begin + count <= end.  On a
// defective line emit may have been called for some components (always with c < 2 width and a span inside the line).
template <class Emit>
VMN_JSONLINES_HD inline bool scan_ciphertext_line(const uint8_t* text, uint64_t start, uint64_t end, uint32_t width, Emit&& emit) {
    uint64_t at = start;
    const bool list = width > 1;                              // [pair,...,pair]; a bare pair at width 1
    if (list) {
        if (!eat(text, at, end, '[')) return false;
        skip_blanks(text, at, end);
    }
    uint32_t pairs = 0;
    for (;;) {
        if (pairs == width) return false;                     // one pair too many
        if (!pair_map(text, at, end, pairs, width, emit)) return false;
        ++pairs;
        if (!list) break;
        skip_blanks(text, at, end);
        if (!eat(text, at, end, ',')) break;
        skip_blanks(text, at, end);
    }
    if (list && !eat(text, at, end, ']')) return false;
    return pairs == width && at == end;
}

}  // namespace jsonlines
}  // namespace vmn
