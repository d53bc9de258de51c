// Stand-alone host program around csrc/encode_layout.h for tests/test_encode_layout_host.py (built with ASan + UBSan).  Every FILE
// holds one hexadecimal string per line (an empty line is the empty string).
//   encode_layout_harness length BITS                     the encode length of a modulus of BITS bits
//   encode_layout_harness records NBYTES L NCOMP FILE     per message: the NCOMP records (hex, separated by spaces), byte by byte
//                                                         through record_byte as k_textlines_records does
//   encode_layout_harness fold NBYTES L P Q FILE          per record: "ill", or the message length and the low L + 4 bytes of the
//                                                         folded value (hex), through fold_record as k_textlines_fold does
//   encode_layout_harness utf8 FILE                       per string: the verdict of Utf8 (1 / 0) and the bytes that are not stripped
// Each message and each record is held in a heap block of exactly its size: a read or write outside of it is a report of the
// sanitizer.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../verificatum-vmn_amd/csrc/encode_layout.h"

using Bytes = std::vector<uint8_t>;

static bool unhex(const std::string& s, Bytes& out) {
    if (s.size() % 2) return false;
    out.clear();
    for (size_t i = 0; i < s.size(); i += 2) {
        unsigned v;
        if (sscanf(s.c_str() + i, "%2x", &v) != 1) return false;
        out.push_back((uint8_t)v);
    }
    out.shrink_to_fit();
    return true;
}
static void hex(const uint8_t* p, size_t n) {
    for (size_t i = 0; i < n; ++i) printf("%02x", p[i]);
}
static bool read_lines(const char* path, std::vector<Bytes>& out) {
    FILE* f = fopen(path, "r");
    if (!f) return false;
    std::string cur;
    for (int c; (c = fgetc(f)) != EOF;) {
        if (c != '\n') {
            cur.push_back((char)c);
            continue;
        }
        Bytes b;
        if (!unhex(cur, b)) return false;
        out.push_back(b);
        cur.clear();
    }
    fclose(f);
    return cur.empty();
}

int main(int argc, char** argv) {
    using namespace vmn::encode;
    if (argc < 3) return 2;
    const std::string mode = argv[1];
    if (mode == "length" && argc == 3) {
        printf("%zu\n", encode_length((size_t)atol(argv[2])));
        return 0;
    }
    std::vector<Bytes> items;
    if (!read_lines(argv[argc - 1], items)) return 2;
    if (mode == "records" && argc == 6) {
        const size_t nbytes = (size_t)atol(argv[2]), L = (size_t)atol(argv[3]), ncomp = (size_t)atol(argv[4]);
        if (L < 1 || nbytes < L + LENGTH_BYTES || ncomp < 1) return 2;
        for (const Bytes& msg : items) {
            if (msg.size() > ncomp * L) return 3;
            for (size_t c = 0; c < ncomp; ++c) {
                Bytes rec(nbytes);
                rec.shrink_to_fit();
                for (size_t k = 0; k < nbytes; ++k) rec[k] = record_byte(k, nbytes, L, c, msg.data(), msg.size());
                if (c) printf(" ");
                hex(rec.data(), nbytes);
            }
            printf("\n");
        }
        return 0;
    }
    if (mode == "fold" && argc == 7) {
        const size_t nbytes = (size_t)atol(argv[2]), L = (size_t)atol(argv[3]);
        Bytes p, q;
        if (!unhex(argv[4], p) || !unhex(argv[5], q) || p.size() != nbytes || q.size() != nbytes || nbytes < L + LENGTH_BYTES) return 2;
        for (Bytes rec : items) {
            if (rec.size() != nbytes) return 3;
            const uint32_t len = fold_record(rec.data(), nbytes, L, p.data(), q.data());
            if (len == ILL_FORMED) {
                printf("ill\n");
                continue;
            }
            printf("%u ", len);
            hex(rec.data() + (nbytes - L - LENGTH_BYTES), L + LENGTH_BYTES);
            printf("\n");
        }
        return 0;
    }
    if (mode == "utf8" && argc == 3) {
        for (const Bytes& s : items) {
            Utf8 u;
            Bytes kept;
            for (uint8_t b : s) {
                u.step(b);
                if (!stripped(b)) kept.push_back(b);
            }
            printf("%d ", u.wellformed() ? 1 : 0);
            hex(kept.data(), kept.size());
            printf("\n");
        }
        return 0;
    }
    return 2;
}
