// Stand-alone host program around csrc/ec_encode_layout.h for tests/test_point_encode_layout_host.py (built with ASan + UBSan).
// Every FILE holds one hexadecimal string per line (an empty line is the empty string).
//   point_encode_layout_harness length BITS               the encode length over a curve whose field prime has BITS bits
//   point_encode_layout_harness records L NCOMP FILE      per message: the NCOMP records T of L + 4 bytes (hex, separated by
//                                                         spaces), byte by byte through record_byte at nbytes = L + 4, as
//                                                         k_textlines_records writes them for the curve interface
//   point_encode_layout_harness fold NBYTES L FILE        per point record x || y of 2 NBYTES bytes: "ill", or the message length
//                                                         and T (hex), through fold_point_record as k_ec_textlines_fold does;
//                                                         an ill-formed record's T must be all zero
// Each message and each record is held in a heap block of exactly its size: a read or write outside of it is a report of the
// sanitizer.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../verificatum-vmn_amd/csrc/ec_encode_layout.h"

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
        printf("%zu\n", point_encode_length((size_t)atol(argv[2])));
        return 0;
    }
    std::vector<Bytes> items;
    if (!read_lines(argv[argc - 1], items)) return 2;
    if (mode == "records" && argc == 5) {
        const size_t L = (size_t)atol(argv[2]), ncomp = (size_t)atol(argv[3]), tbytes = L + LENGTH_BYTES;
        if (L < 1 || ncomp < 1) return 2;
        for (const Bytes& msg : items) {
            if (msg.size() > ncomp * L) return 3;
            for (size_t c = 0; c < ncomp; ++c) {
                Bytes rec(tbytes);
                rec.shrink_to_fit();
                for (size_t k = 0; k < tbytes; ++k) rec[k] = record_byte(k, tbytes, L, c, msg.data(), msg.size());
                if (c) printf(" ");
                hex(rec.data(), tbytes);
            }
            printf("\n");
        }
        return 0;
    }
    if (mode == "fold" && argc == 5) {
        const size_t nbytes = (size_t)atol(argv[2]), L = (size_t)atol(argv[3]), tbytes = L + LENGTH_BYTES;
        if (L < 1 || nbytes < tbytes + COUNTER_BYTES) return 2;
        for (const Bytes& rec : items) {
            if (rec.size() != 2 * nbytes) return 3;
            Bytes T(tbytes, 0xa5);
            T.shrink_to_fit();
            const uint32_t len = fold_point_record(T.data(), rec.data(), nbytes, L);
            if (len == ILL_FORMED) {
                for (uint8_t b : T)
                    if (b) return 4;
                printf("ill\n");
                continue;
            }
            printf("%u ", len);
            hex(T.data(), tbytes);
            printf("\n");
        }
        return 0;
    }
    return 2;
}
