// Stand-alone host program over csrc/permutation_layout.h (tests/test_permutation_layout_host.py builds it with
// -fsanitize=address,undefined and compares its output with tests/permutation_cases.py).
//   permutation_layout_harness width N RBITLEN         -> "key_bits key_bytes top_mask"
//   permutation_layout_harness order NBYTES FILE       -> per key of FILE (one hex row per line): "pi[j] inv[j]"
// `order` computes the table twice: with the header's reference (std::stable_sort on the keys) and with a least-significant-digit
// counting sort of the indices that reads the keys only through plane_at / row_digit, pass by pass as the kernels do; the two
// must agree, or the program fails.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "../verificatum-vmn_amd/csrc/permutation_layout.h"

namespace pm = vmn::permutation;

static int hexval(char c) {
    if (c >= '0' && c <= '9') return c - '0';
    if (c >= 'a' && c <= 'f') return c - 'a' + 10;
    return -1;
}

int main(int argc, char** argv) {
    if (argc == 4 && std::string(argv[1]) == "width") {
        const uint64_t n = strtoull(argv[2], nullptr, 10);
        const int rbitlen = atoi(argv[3]);
        const int kb = pm::key_bits(n, rbitlen);
        printf("%d %zu %u\n", kb, pm::key_bytes(n, rbitlen), kb ? (unsigned)pm::top_mask(kb) : 0u);
        return 0;
    }
    if (argc == 4 && std::string(argv[1]) == "order") {
        const size_t nbytes = strtoull(argv[2], nullptr, 10);
        if (nbytes < 1 || nbytes > pm::MAX_KEY_BYTES) return 2;
        std::ifstream in(argv[3]);
        std::vector<uint8_t> rows;
        std::string line;
        size_t n = 0;
        while (std::getline(in, line)) {
            if (line.size() != 2 * nbytes) return 3;
            for (size_t k = 0; k < nbytes; ++k) {
                const int hi = hexval(line[2 * k]), lo = hexval(line[2 * k + 1]);
                if (hi < 0 || lo < 0) return 3;
                rows.push_back((uint8_t)(hi * 16 + lo));
            }
            ++n;
        }
        std::vector<uint32_t> pi, inv;
        pm::reference_order(rows.data(), nbytes, n, pi);
        pm::reference_inverse(pi, inv);
        // the kernels' view: digit-major planes, one stable counting pass per digit over the indices
        std::vector<uint8_t> planes(n * nbytes);
        for (size_t i = 0; i < n; ++i)
            for (size_t d = 0; d < nbytes; ++d) planes[pm::plane_at(n, d, i)] = pm::row_digit(rows.data(), nbytes, i, d);
        std::vector<uint32_t> cur(n), nxt(n);
        for (size_t i = 0; i < n; ++i) cur[i] = (uint32_t)i;
        for (size_t d = 0; d < nbytes; ++d) {
            size_t count[257] = {0};
            for (size_t e = 0; e < n; ++e) ++count[planes[pm::plane_at(n, d, cur[e])] + 1];
            for (int g = 0; g < 256; ++g) count[g + 1] += count[g];
            for (size_t e = 0; e < n; ++e) nxt[count[planes[pm::plane_at(n, d, cur[e])]]++] = cur[e];
            cur.swap(nxt);
        }
        if (cur != pi) {
            fprintf(stderr, "the digit passes and the reference order differ\n");
            return 4;
        }
        for (size_t j = 0; j < n; ++j) printf("%u %u\n", pi[j], inv[j]);
        return 0;
    }
    fprintf(stderr, "usage: width N RBITLEN | order NBYTES FILE\n");
    return 1;
}
