// Stand-alone host program around csrc/jsonlines_layout.h for tests/test_jsonlines_layout_host.py (built with ASan + UBSan).
//   jsonlines_layout_harness lines WIDTH FILE    one output line per line of FILE: "bad", or "ok" and c:begin:count per component
//   jsonlines_layout_harness sizes DMAX WIDTH    the longest ciphertext line and the longest plaintext line
// The text is held in a heap block of exactly its size, and every line is handed over as [start, end) of that block, as the
// kernel gets it: a read outside the text is a report of the sanitizer.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../verificatum-vmn_amd/csrc/jsonlines_layout.h"

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    if (!strcmp(argv[1], "sizes")) {
        const long dmax = atol(argv[2]), width = atol(argv[3]);
        if (dmax < 1 || width < 1) return 2;
        printf("%zu %zu\n", vmn::jsonlines::max_ciphertext_line((size_t)dmax, (size_t)width),
               vmn::jsonlines::max_plaintext_line((size_t)dmax, (size_t)width));
        return 0;
    }
    if (strcmp(argv[1], "lines")) return 2;
    const long width = atol(argv[2]);
    if (width < 1 || width > (long)vmn::jsonlines::MAX_WIDTH) return 2;
    FILE* f = fopen(argv[3], "rb");
    if (!f) return 2;
    std::vector<uint8_t> text;
    for (int c; (c = fgetc(f)) != EOF;) text.push_back((uint8_t)c);
    fclose(f);
    text.shrink_to_fit();
    const uint8_t* t = text.data();
    const uint64_t len = text.size();
    // readLine: \n, \r, or \r\n counted once; text behind the last terminator is a line if it is not empty
    uint64_t start = 0;
    for (uint64_t i = 0; i <= len; ++i) {
        uint64_t end;
        if (i == len) {
            if (start == len) break;
            end = len;
        } else if (t[i] == '\n' || t[i] == '\r') {
            end = i;
        } else {
            continue;
        }
        std::vector<uint64_t> spans;
        bool inside = true;
        const bool ok = vmn::jsonlines::scan_ciphertext_line(t, start, end, (uint32_t)width, [&](uint32_t c, uint64_t begin, uint64_t count) {
            inside = inside && c < 2 * (uint32_t)width && begin >= start && begin + count <= end;
            spans.push_back(c);
            spans.push_back(begin);
            spans.push_back(count);
        });
        if (!inside) return 3;                                    // a span outside its line, on a good or a defective line
        if (!ok) {
            printf("bad\n");
        } else {
            printf("ok");
            for (size_t k = 0; k < spans.size(); k += 3) printf(" %llu:%llu:%llu", (unsigned long long)spans[k], (unsigned long long)spans[k + 1], (unsigned long long)spans[k + 2]);
            printf("\n");
        }
        if (i < len && t[i] == '\r' && i + 1 < len && t[i + 1] == '\n') ++i;
        start = i + 1;
    }
    return 0;
}
