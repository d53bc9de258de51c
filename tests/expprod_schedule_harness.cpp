// Stand-alone driver of the host's schedule builder for products of powers (csrc/expprod_schedule.h), built with
// -fsanitize=address,undefined by tests/test_expprod_schedule_host.py.
//   expprod_schedule_harness <bits> <group> <hex exponent> ...
// builds the schedule, walks it over a table of subset products of fixed bases modulo the prime 2^61 - 1, compares the result
// with the product of the plain square-and-multiply powers, and prints "ok <steps> <mults> <squarings>".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../verificatum-vmn_amd/csrc/expprod_schedule.h"

using vmn::hostbig::Big;
typedef unsigned long long u64;
static const u64 P61 = (1ULL << 61) - 1;
static u64 mulm(u64 a, u64 b) { return (u64)((unsigned __int128)a * b % P61); }

struct Step {
    int sq, idx;
};

static Big from_hex(const char* s) {
    const size_t len = strlen(s);
    Big r((len + 7) / 8 + 1, 0);
    for (size_t i = 0; i < len; ++i) {
        const char ch = s[len - 1 - i];
        const unsigned v = ch <= '9' ? ch - '0' : (ch | 32) - 'a' + 10;
        r[i / 8] |= v << (4 * (i % 8));
    }
    return r;
}

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const int bits = atoi(argv[1]), group = atoi(argv[2]), rows = (1 << group) - 1;
    std::vector<Big> es;
    for (int i = 3; i < argc; ++i) es.push_back(from_hex(argv[i]));
    const size_t nb = es.size();
    std::vector<Step> steps;
    long mults = 0, squarings = 0;
    const size_t count = vmn::expprod_schedule(es.data(), nb, bits, group, rows, steps, mults, squarings);
    if (count != steps.size()) return 3;
    // the table the kernels build: per group, row (mask - 1) = the row without the lowest base, times that base
    std::vector<u64> base(nb), tab(((nb + group - 1) / group) * rows, 0);
    for (size_t j = 0; j < nb; ++j) base[j] = 1000003ULL * (j + 2) + 7;
    for (size_t g0 = 0; g0 < nb; g0 += group) {
        const size_t gs = nb - g0 < (size_t)group ? nb - g0 : (size_t)group, off = g0 / group * rows;
        for (unsigned mask = 1; mask < (1u << gs); ++mask) {
            const unsigned low = mask & (0u - mask), rest = mask ^ low;
            const u64 b = base[g0 + __builtin_ctz(low)];
            tab[off + mask - 1] = rest ? mulm(tab[off + rest - 1], b) : b;
        }
    }
    u64 want = 1;
    bool allzero = true;
    for (size_t j = 0; j < nb; ++j) {
        u64 acc = 1;
        for (int i = vmn::hostbig::bit_length(es[j]) - 1; i >= 0; --i) {
            acc = mulm(acc, acc);
            if (vmn::hostbig::get_bit(es[j], i)) acc = mulm(acc, base[j]);
        }
        if (!vmn::hostbig::is_zero(es[j])) allzero = false;
        want = mulm(want, acc);
    }
    if (allzero != (count == 0)) return 4;
    u64 got = 1;
    long m = 0, s = 0;
    for (size_t t = 0; t < steps.size(); ++t) {
        if (t == 0 && (steps[t].sq != 0 || steps[t].idx < 0)) return 5;
        if (steps[t].idx >= (int)tab.size() || (steps[t].idx >= 0 && tab[steps[t].idx] == 0)) return 6;      // a row the table has
        if (steps[t].idx < 0 && t + 1 != steps.size()) return 7;
        for (int d = 0; d < steps[t].sq; ++d) got = mulm(got, got);
        if (steps[t].idx >= 0) got = t ? mulm(got, tab[steps[t].idx]) : tab[steps[t].idx];
        if (t) {
            s += steps[t].sq;
            m += steps[t].idx >= 0;
        }
    }
    if (got != want || m != mults || s != squarings) return 8;
    if (s > bits) return 9;                                  // one chain of squarings, whatever the number of bases
    printf("ok %zu %ld %ld\n", steps.size(), mults, squarings);
    return 0;
}
