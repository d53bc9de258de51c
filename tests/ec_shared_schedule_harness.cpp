// Stand-alone driver of the host's schedule builder for curve powers under one scalar (csrc/ec_shared_schedule.h), built with
// -fsanitize=address,undefined by tests/test_ec_shared_schedule_host.py.
//   ec_shared_schedule_harness <window, or 0 for the chosen one> <hex order q> <hex scalar> ...
// Reduces every scalar modulo q, picks ONE window for all of them as a launch does, appends their schedules to one buffer, and
// per scalar checks the digits of the recoding, walks the schedule over plain integers (table row r = 2 r + 1, a doubling = times
// two) and compares with the reduced scalar.  Prints "ok <w>" and per scalar "<hex e mod q> <steps> <adds> <dbls> <min digit>
// <max digit>"; any failed check ends the program with a status of its own.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../verificatum-vmn_amd/csrc/ec_shared_schedule.h"

using vmn::hostbig::Big;

struct Step {
    int sq, op;
};

static Big from_hex(const char* s, size_t words) {
    const size_t len = strlen(s);
    Big r(words > (len + 7) / 8 + 1 ? words : (len + 7) / 8 + 1, 0);
    for (size_t i = 0; i < len; ++i) {
        const char ch = s[len - 1 - i];
        const unsigned v = ch <= '9' ? ch - '0' : (ch | 32) - 'a' + 10;
        r[i / 8] |= v << (4 * (i % 8));
    }
    return r;
}
// plain integers of the walk: little-endian words with room above the order
static void times_two(Big& a) {
    uint32_t top = 0;
    for (size_t i = 0; i < a.size(); ++i) {
        const uint32_t nt = a[i] >> 31;
        a[i] = (a[i] << 1) | top;
        top = nt;
    }
    if (top) exit(20);
}
static void add_small(Big& a, uint32_t v) {
    uint64_t c = v;
    for (size_t i = 0; i < a.size() && c; ++i) {
        c += a[i];
        a[i] = (uint32_t)c;
        c >>= 32;
    }
    if (c) exit(21);
}
static void sub_small(Big& a, uint32_t v) {
    uint64_t b = v;
    for (size_t i = 0; i < a.size() && b; ++i) {
        const uint64_t d = (uint64_t)a[i] - b;
        a[i] = (uint32_t)d;
        b = (d >> 63) & 1;
    }
    if (b) exit(22);                                       // the walk never goes below zero: the top digit is positive
}

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const int forced = atoi(argv[1]);
    const Big q0 = from_hex(argv[2], 0);
    std::vector<Big> es;
    size_t words = q0.size();
    for (int i = 3; i < argc; ++i) words = std::max(words, from_hex(argv[i], 0).size());
    const Big q = from_hex(argv[2], words);
    for (int i = 3; i < argc; ++i) {
        Big rem;
        vmn::hostbig::div(from_hex(argv[i], words), q, &rem);
        es.push_back(rem);
    }
    const int w = vmn::ec_shared_window(es.data(), es.size(), 6.9, 15.4, forced);
    if (w < 2 || w > 6 || (forced >= 2 && forced <= 6 && w != forced)) return 3;
    // every schedule into ONE buffer, as the launch uploads them
    std::vector<Step> steps;
    std::vector<size_t> first(es.size()), count(es.size());
    std::vector<long> adds(es.size()), dbls(es.size());
    for (size_t c = 0; c < es.size(); ++c) {
        first[c] = steps.size();
        count[c] = vmn::ec_shared_schedule(es[c], w, steps, adds[c], dbls[c]);
        if (first[c] + count[c] != steps.size()) return 4;
    }
    printf("ok %d\n", w);
    for (size_t c = 0; c < es.size(); ++c) {
        const Big& e = es[c];
        const int bits = vmn::hostbig::bit_length(e);
        if ((count[c] == 0) != vmn::hostbig::is_zero(e)) return 5;
        // the digits
        std::vector<int> d;
        vmn::ec_shared_digits(e, w, d);
        if ((int)d.size() > bits + 1) return 6;
        if (d.empty() != (bits == 0) || (!d.empty() && d.back() <= 0)) return 7;
        int dmin = 0, dmax = 0, last = -w;
        for (int i = 0; i < (int)d.size(); ++i) {
            if (d[i] == 0) continue;
            if ((d[i] & 1) == 0 || d[i] >= (1 << (w - 1)) || -d[i] >= (1 << (w - 1))) return 8;
            if (i - last < w) return 9;                     // at most one non-zero digit among w consecutive positions
            last = i;
            dmin = d[i] < dmin ? d[i] : dmin;
            dmax = d[i] > dmax ? d[i] : dmax;
        }
        {                                                   // sum d[i] 2^i = e, from the top (Horner)
            Big v(words + 1, 0);
            for (int i = (int)d.size() - 1; i >= 0; --i) {
                times_two(v);
                if (d[i] > 0) add_small(v, (uint32_t)d[i]);
                if (d[i] < 0) sub_small(v, (uint32_t)-d[i]);
            }
            if (v.back() != 0) return 10;
            v.resize(words);
            if (vmn::hostbig::cmp(v, e) != 0) return 10;
        }
        // the schedule, found at first / count in the shared buffer
        Big got(words + 1, 0);
        long a = 0, s = 0;
        for (size_t t = 0; t < count[c]; ++t) {
            const Step& st = steps[first[c] + t];
            if (t == 0 && (st.sq != 0 || st.op < 0 || (st.op & 1))) return 11;       // the first step loads a row
            if (st.op < -1 || (st.op >= 0 && (st.op >> 1) >= vmn::ec_shared_rows(w))) return 12;
            if (st.op < 0 && (t + 1 != count[c] || st.sq <= 0)) return 13;           // only the trailing zeros go without a row
            for (int k = 0; k < st.sq; ++k) times_two(got);
            if (st.op >= 0) {
                const uint32_t row = 2 * (uint32_t)(st.op >> 1) + 1;
                if (st.op & 1) sub_small(got, row);
                else add_small(got, row);
            }
            if (t) {
                s += st.sq;
                a += st.op >= 0;
            }
        }
        if (got.back() != 0) return 14;
        got.resize(words);
        if (vmn::hostbig::cmp(got, e) != 0) return 14;
        if (a != adds[c] || s != dbls[c]) return 15;
        if (s > bits) return 16;
        for (size_t i = words; i-- > 0;) printf("%08x", e[i]);
        printf(" %zu %ld %ld %d %d\n", count[c], adds[c], dbls[c], dmin, dmax);
    }
    return 0;
}
