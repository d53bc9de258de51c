// Stand-alone program over csrc/hexlines_layout.h at a key width (host code only; built with -fsanitize=address,undefined by
// tests/test_keyed_layout_host.py):  keyed_layout_harness KIND VALUE_BYTES KEYWIDTH WIDTH, KIND = modp | curve.
// Prints B, E, the template and the mask in hex and the 2 * KEYWIDTH * WIDTH offsets, one item per line.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../verificatum-vmn_amd/csrc/hexlines_layout.h"

int main(int argc, char** argv) {
    if (argc != 5 || (strcmp(argv[1], "modp") != 0 && strcmp(argv[1], "curve") != 0)) {
        fprintf(stderr, "usage: %s modp|curve VALUE_BYTES KEYWIDTH WIDTH\n", argv[0]);
        return 2;
    }
    const bool curve = strcmp(argv[1], "curve") == 0;
    const size_t value_bytes = (size_t)strtoull(argv[2], nullptr, 10), keywidth = (size_t)strtoull(argv[3], nullptr, 10),
                 width = (size_t)strtoull(argv[4], nullptr, 10);
    if (value_bytes == 0 || keywidth == 0 || width == 0) return 2;
    const vmn::hexlines::Layout L = vmn::hexlines::make_layout(curve, value_bytes, keywidth, width);
    if (L.tmpl.size() != L.B || L.mask.size() != L.B || L.offset.size() != 2 * keywidth * width) return 1;
    if (L.B != vmn::hexlines::line_bytes(curve, value_bytes, keywidth, width) || L.E != vmn::hexlines::element_bytes(curve, value_bytes)) return 1;
    printf("B %zu\nE %zu\ntemplate ", L.B, L.E);
    for (size_t i = 0; i < L.B; ++i) printf("%02x", L.tmpl[i]);
    printf("\nmask ");
    for (size_t i = 0; i < L.B; ++i) printf("%02x", L.mask[i]);
    printf("\noffsets");
    for (size_t c = 0; c < L.offset.size(); ++c) printf(" %zu", L.offset[c]);
    printf("\n");
    return 0;
}
