// hexlines_layout.h — the byte layout of one line of the reference's `native` ciphertext interface
// (ProtocolElGamalInterfaceNative / ...SeqHex, CiphertextReaderLine, CiphertextWriterLine): one ciphertext per line, the
// line being the hexadecimal form of that ciphertext's byte tree.  Host-only, plain C++, no HIP: the tests build it alone.
//
// A ciphertext of width w is node(u, v); at w = 1 u and v are element trees, at w > 1 each is node(w element trees).
//   element tree over a ModPGroup:  leaf(elem_bytes)                E = 5 + elem_bytes
//   element tree over a curve:      node(leaf(x), leaf(y))          E = 15 + 2 * coord_bytes   (infinity: two leaves of 0xff)
//   bytes per line:                 B = 5 + (w > 1 ? 10 : 0) + 2 w E,   hex digits per line H = 2 B
// (framing as in SURVEY.md App. D: node = 00 | uint32_be(children), leaf = 01 | uint32_be(bytes)).
// The widths are the group's wire widths, so a group at the reference's widths gives the reference's lines.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace vmn {
namespace hexlines {

enum : uint8_t {
    PAYLOAD = 0,      // a byte of a value
    OUTER = 1,        // framing of node(u, v) and, at w > 1, of the two inner nodes: written by k_hexlines_encode
    ELEMENT = 2       // framing inside an element tree (leaf headers, the node of a curve point): written by the export kernels
};

struct Layout {
    size_t B = 0;                      // bytes per line
    size_t E = 0;                      // bytes per element tree
    std::vector<uint8_t> tmpl;         // B bytes: the framing bytes in place, payload bytes 0
    std::vector<uint8_t> mask;         // B bytes: PAYLOAD / OUTER / ELEMENT
    std::vector<size_t> offset;        // 2 w byte offsets of the element trees, in the order u_1..u_w, v_1..v_w
};

inline size_t element_bytes(bool curve, size_t value_bytes) { return curve ? 15 + 2 * value_bytes : 5 + value_bytes; }
inline size_t line_bytes(bool curve, size_t value_bytes, size_t width) {
    return 5 + (width > 1 ? 10 : 0) + 2 * width * element_bytes(curve, value_bytes);
}

// value_bytes: the width of one leaf (a residue, resp. ONE coordinate of a point); width >= 1
inline Layout make_layout(bool curve, size_t value_bytes, size_t width) {
    Layout L;
    L.E = element_bytes(curve, value_bytes);
    L.B = line_bytes(curve, value_bytes, width);
    L.tmpl.assign(L.B, 0);
    L.mask.assign(L.B, PAYLOAD);
    size_t at = 0;
    auto header = [&](uint8_t tag, size_t count, uint8_t owner) {
        const uint8_t h[5] = {tag, (uint8_t)(count >> 24), (uint8_t)(count >> 16), (uint8_t)(count >> 8), (uint8_t)count};
        for (int k = 0; k < 5; ++k) {
            L.tmpl[at] = h[k];
            L.mask[at] = owner;
            ++at;
        }
    };
    header(0, 2, OUTER);                                       // node(u, v)
    for (int half = 0; half < 2; ++half) {
        if (width > 1) header(0, width, OUTER);                // node(w element trees)
        for (size_t c = 0; c < width; ++c) {
            L.offset.push_back(at);
            if (curve) {
                header(0, 2, ELEMENT);
                header(1, value_bytes, ELEMENT);
                at += value_bytes;
                header(1, value_bytes, ELEMENT);
                at += value_bytes;
            } else {
                header(1, value_bytes, ELEMENT);
                at += value_bytes;
            }
        }
    }
    return L;
}

}  // namespace hexlines
}  // namespace vmn
