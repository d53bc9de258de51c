// ec_shared_schedule.h — the host's schedule of a scalar multiplication e * P with ONE scalar for a whole array of points, read by
// k_ec_mulshared (ec_kernels.h).  Negation is free on a curve, so the scalar is recoded into SIGNED odd digits (width-w
// non-adjacent form): the per-lane table holds the 2^(w-2) odd multiples P, 3P, ... only, and a b-bit scalar costs about
// b / (w + 1) additions.  Host code only, no device header: the step type is a template parameter (ECSharedStep in the library),
// so that the builder compiles alone under a sanitizer (tests/ec_shared_schedule_harness.cpp).
#pragma once
#include <stddef.h>
#include <vector>

#include "hostbig.h"

namespace vmn {

constexpr int EC_SHARED_WMIN = 2, EC_SHARED_WMAX = 6;

// e = sum d[i] 2^i with every non-zero d[i] odd, |d[i]| < 2^(w-1), at most one non-zero digit among any w consecutive positions
// and a positive top digit; d.size() <= bit_length(e) + 1, empty for e = 0.  One pass over the bits from the right with a carry:
// where bit + carry is odd, the w bits from here (plus the carry) are the window's value v; v >= 2^(w-1) becomes the digit
// v - 2^w and a carry into the position behind the window.  No subtraction of big numbers.
inline void ec_shared_digits(const hostbig::Big& e, int w, std::vector<int>& d) {
    d.clear();
    const int bits = hostbig::bit_length(e);
    auto bit = [&](int i) { return i < bits ? hostbig::get_bit(e, i) : 0; };
    int carry = 0;
    for (int i = 0; i < bits || carry;) {
        if (((bit(i) + carry) & 1) == 0) {             // 0 + 0 or 1 + 1: the digit is zero, the carry stays as it is
            d.push_back(0);
            ++i;
            continue;
        }
        int v = carry;
        for (int b = 0; b < w; ++b) v += bit(i + b) << b;
        carry = v >= (1 << (w - 1));
        d.push_back(carry ? v - (1 << w) : v);
        for (int b = 1; b < w; ++b) d.push_back(0);
        i += w;
    }
    while (!d.empty() && d.back() == 0) d.pop_back();  // (the zeros behind the top window)
}

// The schedule of e under windows of w bits, read left to right: a step is {sq, op} = `sq` doublings, then the addition
// (op = 2 r) or the subtraction (op = 2 r + 1) of table row r = (2 r + 1) P; op = -1: no addition (the trailing zero positions, a
// last step).  The first step has sq = 0 and an even op: the accumulator starts as that row.  Appends to `steps` and returns the
// number of steps appended, 0 for e = 0.  `adds` / `dbls`: the additions and doublings behind the first step.
template <class Step>
inline size_t ec_shared_schedule(const hostbig::Big& e, int w, std::vector<Step>& steps, long& adds, long& dbls) {
    const size_t first = steps.size();
    std::vector<int> d;
    ec_shared_digits(e, w, d);
    adds = dbls = 0;
    int pending = 0;
    for (int i = (int)d.size() - 1; i >= 0; --i) {
        if (d[i] != 0) {
            const int mag = d[i] < 0 ? -d[i] : d[i];
            steps.push_back(Step{pending, (mag - 1) / 2 * 2 + (d[i] < 0 ? 1 : 0)});
            if (steps.size() > first + 1) ++adds;
            dbls += pending;
            pending = 0;
        }
        ++pending;
    }
    if (--pending > 0) {                               // (the loop counted one position below digit 0)
        steps.push_back(Step{pending, -1});
        dbls += pending;
    }
    return steps.size() - first;
}

// rows of the table of odd multiples under windows of w bits
inline int ec_shared_rows(int w) { return 1 << (w - 2); }

// What a point costs under the schedule's counts: the main loop, the table's additions and the one doubling (2 P) every table
// of more than one row starts with.  `c_dbl` / `c_add`: a doubling and an addition in the caller's unit.
inline double ec_shared_cost(int w, long adds, long dbls, double c_dbl, double c_add) {
    return c_dbl * (double)dbls + c_add * (double)(adds + ec_shared_rows(w) - 1) + (w > 2 ? c_dbl : 0.0);
}

// The window of a launch over the k scalars es[]: the cheapest of 2 ... 6 by the sum of the costs on the actual recodings (ONE
// width per launch: the tables have one size); `forced` in 2 ... 6 overrides.
inline int ec_shared_window(const hostbig::Big* es, size_t k, double c_dbl, double c_add, int forced = 0) {
    if (forced >= EC_SHARED_WMIN && forced <= EC_SHARED_WMAX) return forced;
    struct Probe {
        int sq, op;
    };
    int best = EC_SHARED_WMIN;
    double best_cost = -1;
    for (int w = EC_SHARED_WMIN; w <= EC_SHARED_WMAX; ++w) {
        double cost = 0;
        for (size_t c = 0; c < k; ++c) {
            std::vector<Probe> st;
            long adds = 0, dbls = 0;
            if (ec_shared_schedule(es[c], w, st, adds, dbls)) cost += ec_shared_cost(w, adds, dbls, c_dbl, c_add);
        }
        if (best_cost < 0 || cost < best_cost) {
            best_cost = cost;
            best = w;
        }
    }
    return best;
}

}  // namespace vmn
