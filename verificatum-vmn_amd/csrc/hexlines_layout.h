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
//
// Under a public key of width kappa the plaintext group is G^kappa and a ciphertext of width w lives in ((G^kappa)^w)^2
// [NOT-IN-REF: PPGroupElement.toByteTree is VCR code; the rule of SURVEY.md App. D, a product element is the node of its
// factors' trees, applied once more]: each half is [w > 1: node(w; ...)] over [kappa > 1: node(kappa; ...)] over element trees,
//   B = 5 + 2 ((w > 1 ? 5 : 0) + w ((kappa > 1 ? 5 : 0) + kappa E)),
// and the 2 kappa w element trees are numbered u_0.., v_0.. with c = l kappa + j the key j of plaintext component l.
// kappa = 1 is the layout above; w = 1 is the layout above at width kappa: only kappa > 1 with w > 1 adds a level.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace vmn {
namespace hexlines {

enum : uint8_t {
    PAYLOAD = 0,      // a byte of a value
    OUTER = 1,        // framing of node(u, v) and of the nodes inside a half, down to the element trees: written by k_hexlines_encode
    ELEMENT = 2       // framing inside an element tree (leaf headers, the node of a curve point): written by the export kernels
};

struct Layout {
    size_t B = 0;                      // bytes per line
    size_t E = 0;                      // bytes per element tree
    std::vector<uint8_t> tmpl;         // B bytes: the framing bytes in place, payload bytes 0
    std::vector<uint8_t> mask;         // B bytes: PAYLOAD / OUTER / ELEMENT
    std::vector<size_t> offset;        // 2 kappa w byte offsets of the element trees, the u half first, c = l kappa + j inside a half
};

inline size_t element_bytes(bool curve, size_t value_bytes) { return curve ? 15 + 2 * value_bytes : 5 + value_bytes; }
inline size_t line_bytes(bool curve, size_t value_bytes, size_t keywidth, size_t width) {
    const size_t inner = (keywidth > 1 ? 5 : 0) + keywidth * element_bytes(curve, value_bytes);
    return 5 + 2 * ((width > 1 ? 5 : 0) + width * inner);
}
inline size_t line_bytes(bool curve, size_t value_bytes, size_t width) { return line_bytes(curve, value_bytes, 1, width); }

// value_bytes: the width of one leaf (a residue, resp. ONE coordinate of a point); keywidth >= 1, width >= 1
inline Layout make_layout(bool curve, size_t value_bytes, size_t keywidth, size_t width) {
    Layout L;
    L.E = element_bytes(curve, value_bytes);
    L.B = line_bytes(curve, value_bytes, keywidth, width);
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
        if (width > 1) header(0, width, OUTER);                // node(w elements of G^kappa)
        for (size_t l = 0; l < width; ++l) {
            if (keywidth > 1) header(0, keywidth, OUTER);      // node(kappa element trees)
            for (size_t j = 0; j < keywidth; ++j) {
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
    }
    return L;
}
inline Layout make_layout(bool curve, size_t value_bytes, size_t width) { return make_layout(curve, value_bytes, 1, width); }

}  // namespace hexlines
}  // namespace vmn
