// expprod_schedule.h — the host's schedule of a product of powers prod_j x_j^(e_j) under ONE chain of squarings (Straus), read
// by k_modpow_expprod (modp_shared_exp.h) and k_ec_expprod (ec_kernels.h).  Host code only, no device header: the step type is a
// template parameter (SlideStep in the library), so that the builder compiles alone under a sanitizer
// (tests/expprod_schedule_harness.cpp).
#pragma once
#include <stddef.h>
#include <vector>

#include "hostbig.h"

namespace vmn {

// The bases are cut into groups of `group` in their order; group G's subset products are the table rows G * group_rows + mask - 1,
// bit b of mask = base G * group + b.  Walks the bit columns from `bits` - 1 down: a step is {sq, idx} = `sq` squarings, then the
// product by row `idx`.  The first step carries sq = 0 and is the accumulator's first value; all-zero columns merge into the `sq`
// of the next step; every further group with a bit in a column adds one step with sq = 0; squarings left after the last product
// form a step with idx = -1.  Appends to `steps` and returns the number of steps appended: 0 when every exponent is zero (the
// product is then the identity and there is nothing to launch).  `mults` / `squarings`: the products and squarings behind the
// first step.  An exponent may be shorter than `bits`, and shorter than the others by any amount.
template <class Step>
inline size_t expprod_schedule(const hostbig::Big* es, size_t nb, int bits, int group, int group_rows, std::vector<Step>& steps,
                               long& mults, long& squarings) {
    const size_t first = steps.size();
    auto bit = [&](size_t j, int i) { return (size_t)i / 32 < es[j].size() ? (unsigned)hostbig::get_bit(es[j], i) : 0u; };
    mults = squarings = 0;
    int pending = 0;
    bool started = false;
    for (int i = bits - 1; i >= 0; --i) {
        if (started) ++pending;
        for (size_t g0 = 0; g0 < nb; g0 += (size_t)group) {
            unsigned mask = 0;
            for (size_t b = 0; b < (size_t)group && g0 + b < nb; ++b) mask |= bit(g0 + b, i) << b;
            if (!mask) continue;
            const int row = (int)(g0 / (size_t)group) * group_rows + (int)mask - 1;
            if (started) {
                squarings += pending;
                ++mults;
            }
            steps.push_back(Step{started ? pending : 0, row});
            pending = 0;
            started = true;
        }
    }
    if (pending) {
        squarings += pending;
        steps.push_back(Step{pending, -1});
    }
    return steps.size() - first;
}

}  // namespace vmn
