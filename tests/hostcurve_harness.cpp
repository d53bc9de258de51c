// Test harness for the general-a doubling of verificatum-vmn_amd/csrc/hostcurve.h (HostCurve with `a` set): reads
// "p a gx gy k" as hex from argv and prints, as hex lines of the x || y encoding (all ff = infinity), k G, 2 (k G) and
// k G + G.  Built and run by tests/test_named_curves.py against libcrypto and the Python scalars.
#include <stdio.h>
#include <string.h>

#include <string>

#include "../verificatum-vmn_amd/csrc/hostcurve.h"

using namespace vmn::num64;

static Bytes from_hex(const char* s, size_t nbytes) {
    std::string h(s);
    while (h.size() < 2 * nbytes) h = "0" + h;
    Bytes out;
    for (size_t i = 0; i < h.size(); i += 2) out.push_back((uint8_t)strtoul(h.substr(i, 2).c_str(), nullptr, 16));
    return out;
}
static void print_bytes(const Bytes& b) {
    for (uint8_t c : b) printf("%02x", c);
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc != 6) {
        fprintf(stderr, "usage: %s p a gx gy k (hex)\n", argv[0]);
        return 2;
    }
    size_t cb = (strlen(argv[1]) + 1) / 2;
    Bytes pb = from_hex(argv[1], cb);
    size_t fl = (cb + 7) / 8;
    Mod F(from_be(pb.data(), cb, fl));
    HostCurve C;
    C.F = &F;
    C.cb = cb;
    C.fl = fl;
    Bytes ab = from_hex(argv[2], cb);
    C.a = F.to_m(from_be(ab.data(), cb, fl));
    Bytes g = from_hex(argv[3], cb), gy = from_hex(argv[4], cb);
    g.insert(g.end(), gy.begin(), gy.end());
    std::string k(argv[5]);
    if (k.size() % 2) k = "0" + k;
    Bytes kb = from_hex(k.c_str(), k.size() / 2);
    Bytes kg = C.exp(g, kb.data(), kb.size());
    print_bytes(kg);
    print_bytes(C.add(kg, kg));
    print_bytes(C.add(kg, g));
    return 0;
}
