// light_kernels.h — the kernels that are not templates over an execution geometry: row movement (gather, compare), the
// counting sort and task bookkeeping of the multi-exponentiation, small helpers.  Included by vmnhip.hip only (the
// instantiation units csrc/inst_*.hip include modp_kernels.h, which holds templates only, so that nothing is defined twice).
#pragma once
#include "modp_kernels.h"

namespace vmn {

// t = row * per + c, per a small count of 16-byte chunks per row.  A 64-bit division costs ~100 instructions, more than the
// 16-byte copy it addresses: the 32-bit form is used whenever the index fits (it always does up to 2^32 chunks = 64 GB).
__device__ __forceinline__ void split_chunk(size_t t, int per, size_t& row, int& c) {
    if (t <= 0xffffffffull) {
        const u32 tt = (u32)t, pp = (u32)per;
        const u32 r = tt / pp;
        row = r;
        c = (int)(tt - r * pp);
    } else {
        row = t / (size_t)per;
        c = (int)(t % (size_t)per);
    }
}

// ---- clearing and uploading SMALL things as kernels ------------------------------------------------
// hipMemsetAsync / hipMemcpyAsync go through the runtime's blit path; between kernels of the same stream each of them cost
// 55-70 us of idle device in the small-size timelines (profiles/r04_timeline_p256_n10000_after.txt) where a kernel launch
// costs 7.  A flag word, a histogram of a few thousand counters, a seed or a scalar in a pinned slot are moved by these two
// instead (pinned host memory is mapped into the device's address space: the upload kernel reads it in place).
__global__ void __launch_bounds__(BLOCK) k_zero_words(u32* __restrict__ p, size_t n) {
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * BLOCK) p[i] = 0;
}
__global__ void __launch_bounds__(BLOCK) k_copy_bytes(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, size_t n) {
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * BLOCK) dst[i] = src[i];
}

// ---- generic exclusive scan of a u32 array (three tiny kernels; n up to a few million) ----------
constexpr int SCAN_ITEMS = 16;                         // items per thread

// out[0] = max over the n integers (nw packed little-endian words each) of their bit length.  One thread per
// integer; serves the verifier, which must use every bit of an exponent array it was sent (a reply's k_E) and
// still wants the short path when the entries are as short as an honest prover's.
__global__ void __launch_bounds__(BLOCK) k_words_maxbits(const u32* __restrict__ w, size_t n, int nw, u32* __restrict__ out) {
    size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    u32 bits = 0;
    if (i < n) {
        const u32* p = w + i * (size_t)nw;
        for (int k = nw - 1; k >= 0; --k) {
            u32 v = p[k];
            if (v) {
                bits = 32u * (u32)k + (32u - (u32)__builtin_clz(v));
                break;
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) bits = max(bits, (u32)__shfl_xor((int)bits, o));
    if ((threadIdx.x & 63) == 0 && bits) atomicMax(out, bits);
}

// ---------------------------------------------------------------------------------------------
// K6: flags[0] |= 1 if x != y anywhere.  One thread per 16-byte chunk (HBM-bound, coalesced).
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BLOCK) k_compare(const uint4* __restrict__ x, const uint4* __restrict__ y,
                                                   size_t nchunks, u32* __restrict__ flags) {
    size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    bool diff = false;
    for (; i < nchunks; i += (size_t)gridDim.x * BLOCK) {
        uint4 a = x[i], b = y[i];
        diff |= (a.x != b.x) | (a.y != b.y) | (a.z != b.z) | (a.w != b.w);
    }
    if (__any(diff) && (threadIdx.x & 63) == 0) atomicOr(flags, 1u);
}

// ---------------------------------------------------------------------------------------------
// K7: out[i] = in[idx[i]]  (idx[i] == 0xffffffff: out[i] = fill).  One thread per 16-byte chunk of
// a row: rows are contiguous W-word records, so a gather moves whole aligned rows.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BLOCK) k_gather(uint4* __restrict__ out, const uint4* __restrict__ in,
                                                  const u32* __restrict__ idx, const uint4* __restrict__ fill,
                                                  size_t n_out, int chunks_per_row) {
    size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    size_t total = n_out * (size_t)chunks_per_row;
    for (; t < total; t += (size_t)gridDim.x * BLOCK) {
        size_t row;
        int c;
        split_chunk(t, chunks_per_row, row, c);
        u32 src = idx[row];
        out[t] = src == 0xffffffffu ? fill[c] : in[(size_t)src * chunks_per_row + c];
    }
}

// out[i] = fill for every row i < n_out (the array of ones resp. of infinity): one thread per 16-byte chunk, as k_gather
__global__ void __launch_bounds__(BLOCK) k_fill_rows(uint4* __restrict__ out, const uint4* __restrict__ fill, size_t n_out,
                                                     int chunks_per_row) {
    size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    size_t total = n_out * (size_t)chunks_per_row;
    for (; t < total; t += (size_t)gridDim.x * BLOCK) {
        size_t row;
        int c;
        split_chunk(t, chunks_per_row, row, c);
        out[t] = fill[c];
    }
}

// out = the rows of several arrays, one segment after the other (pGroup.toElementArray(PGroupElementArray[]) and copyOfRange in
// one).  Segment k begins at output row seg[k].first and is read from seg[k].src, the source's row from[k]; the table holds the
// non-empty segments only, so `first` rises strictly and seg[0].first = 0.  One thread per 16-byte chunk of an output row, as
// k_gather: consecutive lanes write consecutive chunks, and read consecutive chunks too wherever they share a segment.  The
// segment of a row is found by binary search (lanes of a wave that straddles a boundary take different branches THERE, over
// a table that sits in cache); the copy itself is one load and one store issued by the whole wave after the search.
struct RowSegment {
    u64 first;               // first output row of the segment
    const uint4* src;        // row from[k] of its source
};
static_assert(sizeof(RowSegment) == 16, "a table entry is one 16-byte load");
__global__ void __launch_bounds__(BLOCK) k_rows_segments(uint4* __restrict__ out, const RowSegment* __restrict__ seg, u32 nseg,
                                                         size_t n_out, int chunks_per_row) {
    size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    size_t total = n_out * (size_t)chunks_per_row;
    for (; t < total; t += (size_t)gridDim.x * BLOCK) {
        size_t row;
        int c;
        split_chunk(t, chunks_per_row, row, c);
        u32 lo = 0, hi = nseg;                       // seg[lo].first <= row < seg[hi].first (seg[nseg].first = n_out, not stored)
        while (hi - lo > 1) {
            const u32 mid = lo + ((hi - lo) >> 1);
            if (seg[mid].first <= (u64)row) lo = mid;
            else hi = mid;
        }
        const RowSegment s = seg[lo];
        // (a pointer read from memory is a generic one to the compiler: said to be global, the load is global_load_dwordx4, not flat_)
        typedef u32 chunk_t __attribute__((ext_vector_type(4)));
        const auto* src = (const __attribute__((address_space(1))) chunk_t*)s.src;
        const chunk_t v = src[(row - (size_t)s.first) * (size_t)chunks_per_row + c];
        out[t] = make_uint4(v.x, v.y, v.z, v.w);
    }
}

// ---------------------------------------------------------------------------------------------
// K2 fixed base.  Table T[k][d] = base^(d * 2^(w*k)), k < nwin, d < 2^w, rows of W words at
// (k*2^w + d)*W.  The host supplies sq[j] = base^(2^j) (the sequential squaring chain); level l
// fills d in (2^l, 2^(l+1)):  T[k][d] = T[k][d - 2^l] * T[k][2^l].
// ---------------------------------------------------------------------------------------------
// one thread per (k, l) plus the d = 0 rows; plain row copies (W words, constants are in row layout)
__global__ void __launch_bounds__(BLOCK) k_fixed_seed(u32* __restrict__ T, const u32* __restrict__ sq, int w, int nwin,
                                                      const u32* __restrict__ one_row, int W) {
    size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    size_t total = (size_t)nwin * (w + 1);
    if (t >= total) return;
    int k = (int)(t / (w + 1)), l = (int)(t % (w + 1));
    u32* dst;
    const u32* src;
    if (l == w) {                          // d = 0: the Montgomery one
        dst = T + ((size_t)k << w) * W;
        src = one_row;
    } else {
        dst = T + (((size_t)k << w) + ((size_t)1 << l)) * W;
        src = sq + ((size_t)k * w + l) * W;
    }
    for (int j = 0; j < W; ++j) dst[j] = src[j];
}

// ---------------------------------------------------------------------------------------------
// K3 multi-exponentiation (Pippenger): counting sort of (window, digit), then a product tree per bucket.
// ---------------------------------------------------------------------------------------------
// counts[win][d] += 1 for every element; one thread per (element, window).
// (grid = gx blocks per window: the window of a block is blockIdx.x / gx -- one scalar division per block instead of two
// 64-bit divisions per item, which were most of this kernel's instructions)
// A NARROW window -- the top one when c does not divide the exponent length: 1 bit at c = 15 for 256-bit exponents, all 10^6
// elements on two counters -- is counted in LDS first and reaches the global counters once per block and digit
// (NARROW_BITS; with global atomics alone that one window took longer than all the others together).  The signed windows
// of the curves have 2^12 buckets at 10^6 points: every window of theirs goes this way (2 x 16 KB of LDS in the scatter), and
// the sort of a P-256 multi-exponentiation takes 2.3 ms instead of 5.2 ms.
constexpr int NARROW_BITS = 12;
__device__ __forceinline__ int window_bits(int w, int c, int ebits) {
    const int left = ebits - w * c;
    return left < c ? (left < 1 ? 1 : left) : c;
}
// SIGNED windows (curves, where a negation is free): the c-bit digits are recoded to d' in (-2^(c-1), 2^(c-1)] -- a digit
// above 2^(c-1) becomes d - 2^c and carries one into the next window -- so that a window needs 2^(c-1) buckets instead of 2^c
// (index |d'| - 1; zero digits are not inserted at all) and one more bit per window costs the same aggregation.  The carry into
// window w is decided by the digits below it: the nearest one that is not exactly 2^(c-1) settles it.  ebits covers the
// exponents' storage, so the top window takes the last carry without overflowing.
__device__ __forceinline__ int signed_digit(const u32* __restrict__ ep, int ewords, int w, int c) {
    const u32 half = 1u << (c - 1);
    int carry = 0;
    for (int v = w - 1; v >= 0; --v) {
        const u32 dv = exp_digit(ep, ewords, v * c, c);
        if (dv != half) {
            carry = dv > half;
            break;
        }
    }
    int d = (int)exp_digit(ep, ewords, w * c, c) + carry;
    return d > (int)half ? d - (1 << c) : d;
}
// digit of element i in window w as (bucket index inside the window, negative?), or false for "nothing to insert";
// cb = bucket bits of a window (c, or c - 1 in the signed form)
template <bool SIGNED>
__device__ __forceinline__ bool bucket_of(const u32* __restrict__ ep, int ewords, int w, int c, u32& bucket, u32& neg) {
    if constexpr (SIGNED) {
        const int d = signed_digit(ep, ewords, w, c);
        if (d == 0) return false;
        neg = d < 0;
        bucket = (u32)(d < 0 ? -d : d) - 1u;
        return true;
    } else {
        bucket = exp_digit(ep, ewords, w * c, c);
        neg = 0;
        return true;
    }
}
// distinct bucket indices a window can hold, as a bit count (for the LDS-privatised path)
template <bool SIGNED>
__device__ __forceinline__ int bucket_index_bits(int w, int c, int ebits) {
    if constexpr (SIGNED) {
        const int left = ebits - w * c;
        return left <= 0 ? 0 : (left < c - 1 ? left : c - 1);
    } else {
        return window_bits(w, c, ebits);
    }
}
template <bool SIGNED>
__global__ void __launch_bounds__(BLOCK) k_bucket_hist(u32* __restrict__ counts, const u32* __restrict__ e, int ewords,
                                                       size_t n, int c, int nwin, u32 gx, int ebits) {
    __shared__ u32 h[1 << NARROW_BITS];
    const u32 w = blockIdx.x / gx, bx = blockIdx.x % gx;
    if ((int)w >= nwin) return;
    const int cb = SIGNED ? c - 1 : c;
    u32* __restrict__ cw = counts + ((size_t)w << cb);
    const int bw = bucket_index_bits<SIGNED>((int)w, c, ebits);
    if (bw <= NARROW_BITS) {
        const u32 nd = 1u << bw;
        for (u32 k = threadIdx.x; k < nd; k += BLOCK) h[k] = 0;
        __syncthreads();
        for (size_t i = (size_t)bx * BLOCK + threadIdx.x; i < n; i += (size_t)gx * BLOCK) {
            u32 d, neg;
            if (!bucket_of<SIGNED>(e + i * ewords, ewords, (int)w, c, d, neg)) continue;
            if (d < nd) atomicAdd(&h[d], 1u);
            else atomicAdd(&cw[d], 1u);                // (an exponent wider than the caller declared: still its own bucket)
        }
        __syncthreads();
        for (u32 k = threadIdx.x; k < nd; k += BLOCK)
            if (h[k]) atomicAdd(&cw[k], h[k]);
        return;
    }
    for (size_t i = (size_t)bx * BLOCK + threadIdx.x; i < n; i += (size_t)gx * BLOCK) {
        u32 d, neg;
        if (bucket_of<SIGNED>(e + i * ewords, ewords, (int)w, c, d, neg)) atomicAdd(&cw[d], 1u);
    }
}

__global__ void __launch_bounds__(BLOCK) k_u32_blocksum(u32* __restrict__ bsum, const u32* __restrict__ in, size_t n) {
    __shared__ u32 part[BLOCK];
    size_t base = ((size_t)blockIdx.x * BLOCK + threadIdx.x) * SCAN_ITEMS;
    u32 s = 0;
    for (int k = 0; k < SCAN_ITEMS; ++k) s += base + k < n ? in[base + k] : 0u;
    part[threadIdx.x] = s;
    __syncthreads();
    for (int st = BLOCK / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) part[threadIdx.x] += part[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) bsum[blockIdx.x] = part[0];
}

__global__ void k_u32_scan_top(u32* __restrict__ bsum, size_t nblocks, u32* __restrict__ total) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        u32 run = 0;
        for (size_t i = 0; i < nblocks; ++i) {
            u32 v = bsum[i];
            bsum[i] = run;
            run += v;
        }
        *total = run;
    }
}

// out[i] = exclusive prefix; out2 (optional) receives a copy (the scatter cursors); out[n] = total
__global__ void __launch_bounds__(BLOCK) k_u32_scan_apply(u32* __restrict__ out, u32* __restrict__ out2,
                                                          const u32* __restrict__ in, const u32* __restrict__ bsum, size_t n) {
    __shared__ u32 part[BLOCK];
    size_t base = ((size_t)blockIdx.x * BLOCK + threadIdx.x) * SCAN_ITEMS;
    u32 v[SCAN_ITEMS];
    u32 s = 0;
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        v[k] = base + k < n ? in[base + k] : 0u;
        s += v[k];
    }
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 run = bsum[blockIdx.x];
        for (int i = 0; i < BLOCK; ++i) {
            u32 t = part[i];
            part[i] = run;
            run += t;
        }
    }
    __syncthreads();
    u32 run = part[threadIdx.x];
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        if (base + k < n) {
            out[base + k] = run;
            if (out2) out2[base + k] = run;
        }
        run += v[k];
        if (base + k + 1 == n) out[n] = run;
    }
}

// sorted[cursor[bucket]++] = element index; one thread per (element, window); bucket = w*2^c + digit.  A narrow window (see
// k_bucket_hist) is placed in two passes over the block's items: count in LDS, reserve one range per digit with a single
// global atomic, then hand out the positions inside the ranges with LDS atomics.
// (SIGNED: the entry carries the digit's sign in bit 31 -- the first tree level negates the point, ec_kernels.h)
template <bool SIGNED>
__global__ void __launch_bounds__(BLOCK) k_bucket_scatter(u32* __restrict__ sorted, u32* __restrict__ cursor,
                                                          const u32* __restrict__ e, int ewords, size_t n, int c, int nwin, u32 gx,
                                                          int ebits) {
    __shared__ u32 h[1 << NARROW_BITS];
    __shared__ u32 base[1 << NARROW_BITS];
    const u32 w = blockIdx.x / gx, bx = blockIdx.x % gx;
    if ((int)w >= nwin) return;
    const int cb = SIGNED ? c - 1 : c;
    u32* __restrict__ cw = cursor + ((size_t)w << cb);
    const int bw = bucket_index_bits<SIGNED>((int)w, c, ebits);
    if (bw <= NARROW_BITS) {
        const u32 nd = 1u << bw;
        for (u32 k = threadIdx.x; k < nd; k += BLOCK) h[k] = 0;
        __syncthreads();
        for (size_t i = (size_t)bx * BLOCK + threadIdx.x; i < n; i += (size_t)gx * BLOCK) {
            u32 d, neg;
            if (bucket_of<SIGNED>(e + i * ewords, ewords, (int)w, c, d, neg) && d < nd) atomicAdd(&h[d], 1u);
        }
        __syncthreads();
        for (u32 k = threadIdx.x; k < nd; k += BLOCK) {
            base[k] = h[k] ? atomicAdd(&cw[k], h[k]) : 0u;
            h[k] = 0;
        }
        __syncthreads();
        for (size_t i = (size_t)bx * BLOCK + threadIdx.x; i < n; i += (size_t)gx * BLOCK) {
            u32 d, neg;
            if (!bucket_of<SIGNED>(e + i * ewords, ewords, (int)w, c, d, neg)) continue;
            u32 pos = d < nd ? base[d] + atomicAdd(&h[d], 1u) : atomicAdd(&cw[d], 1u);
            sorted[pos] = (u32)i | (neg << 31);
        }
        return;
    }
    for (size_t i = (size_t)bx * BLOCK + threadIdx.x; i < n; i += (size_t)gx * BLOCK) {
        u32 d, neg;
        if (!bucket_of<SIGNED>(e + i * ewords, ewords, (int)w, c, d, neg)) continue;
        u32 pos = atomicAdd(&cw[d], 1u);
        sorted[pos] = (u32)i | (neg << 31);
    }
}

// digit 0 contributes nothing: drop those buckets' items
__global__ void __launch_bounds__(BLOCK) k_bucket_drop_zero(u32* __restrict__ counts, int c, int nwin) {
    size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t < (size_t)nwin) counts[t << c] = 0;
}

// cnt_out[b] = ceil(cnt_in[b] / F); maxcnt = max over b
__global__ void __launch_bounds__(BLOCK) k_task_counts(u32* __restrict__ cnt_out, const u32* __restrict__ cnt_in,
                                                       size_t nbuckets, u32 F, u32* __restrict__ maxcnt) {
    size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    u32 v = 0;
    if (t < nbuckets) {
        v = (cnt_in[t] + F - 1) / F;
        cnt_out[t] = v;
    }
    for (int o = 32; o > 0; o >>= 1) v = max(v, (u32)__shfl_xor((int)v, o));
    if ((threadIdx.x & 63) == 0 && v) atomicMax(maxcnt, v);
}

// B[b] = the bucket's single remaining item, or one if it is empty (row copies, 16-byte chunks)
__global__ void __launch_bounds__(BLOCK) k_bucket_finalize(uint4* __restrict__ B, const uint4* __restrict__ items,
                                                           const u32* __restrict__ off_in, const u32* __restrict__ cnt_in,
                                                           size_t nbuckets, const uint4* __restrict__ one_row, int cpr) {
    size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    size_t total = nbuckets * cpr;
    for (; t < total; t += (size_t)gridDim.x * BLOCK) {
        size_t b;
        int ch;
        split_chunk(t, cpr, b, ch);
        B[t] = cnt_in[b] ? items[(size_t)off_in[b] * cpr + ch] : one_row[ch];
    }
}

// overwrite element 0 of every segment with `one` (the d = 0 slot of the suffix products)
__global__ void __launch_bounds__(BLOCK) k_set_segment_heads(uint4* __restrict__ a, size_t seglen, size_t nseg,
                                                             const uint4* __restrict__ one_row, int cpr) {
    size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= nseg * cpr) return;
    size_t s;
    int ch;
    split_chunk(t, cpr, s, ch);
    a[s * seglen * cpr + ch] = one_row[ch];
}

// ---------------------------------------------------------------------------------------------
// The `native` ciphertext interface (csrc/hexlines_layout.h): a text of one ciphertext per line, each line the hex digits of
// that ciphertext's byte tree, <-> records of B bytes, one per line, on which the import / export kernels work component by
// component (be = rec + offset, stride = B, leaf headers on).
// Lines end as Java's readLine ends them: at \n, at \r, or at \r\n, which counts once; text behind the last terminator is a
// line only if it is not empty.  Terminators are mixed freely, so line k does not start at k (H + 1): the starts are found
// -- a count of the terminators per chunk of the text, the u32 scan above over the counts, a second walk that writes where
// every line begins and ends.  Offsets are 64-bit (10^6 lines of an 8192-bit group pass 4 GB), the line count is below 2^32.
// The text buffer is padded by 48 bytes: a thread reads its 16 bytes whole and the byte behind them.
// ---------------------------------------------------------------------------------------------
constexpr int HEXLINES_SEG = 16;                              // bytes of text per thread
constexpr int HEXLINES_CHUNK = BLOCK * HEXLINES_SEG;          // bytes of text per workgroup
constexpr int HEXLINES_LANES = 32;                            // lanes per line in the two conversions
constexpr int HEXLINES_PAD = 48;

// bit k: a line ends with the byte at base + k (a \n, or a \r that no \n follows); base is a multiple of 16
__device__ __forceinline__ u32 hexlines_term_mask(const uint8_t* __restrict__ text, size_t len, size_t base) {
    if (base >= len) return 0;
    const uint4 v = *reinterpret_cast<const uint4*>(text + base);
    const u32 w[5] = {v.x, v.y, v.z, v.w, (u32)text[base + HEXLINES_SEG]};
    u32 m = 0;
#pragma unroll
    for (int k = 0; k < HEXLINES_SEG; ++k) {
        const u32 c = (w[k >> 2] >> (8 * (k & 3))) & 0xffu;
        const u32 nx = (w[(k + 1) >> 2] >> (8 * ((k + 1) & 3))) & 0xffu;
        const bool lf_follows = base + k + 1 < len && nx == '\n';
        if (base + k < len && (c == '\n' || (c == '\r' && !lf_follows))) m |= 1u << k;
    }
    return m;
}

// counts[chunk] = terminators of the chunk; *total += the same (64-bit: a text of 2^32 lines or more is refused by the host)
__global__ void __launch_bounds__(BLOCK) k_hexlines_count(u32* __restrict__ counts, unsigned long long* __restrict__ total,
                                                          const uint8_t* __restrict__ text, size_t len) {
    __shared__ u32 sum;
    if (threadIdx.x == 0) sum = 0;
    __syncthreads();
    const size_t base = ((size_t)blockIdx.x * BLOCK + threadIdx.x) * HEXLINES_SEG;
    u32 c = (u32)__builtin_popcount(hexlines_term_mask(text, len, base));
    for (int o = 32; o > 0; o >>= 1) c += (u32)__shfl_xor((int)c, o);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&sum, c);
    __syncthreads();
    if (threadIdx.x == 0) {
        counts[blockIdx.x] = sum;
        if (sum) atomicAdd(total, (unsigned long long)sum);
    }
}

// start[k], end[k] = where the digits of line k begin and end (end exclusive: the terminator is not part of the line), k < nlines;
// first[chunk] = terminators in front of the chunk (the scan of the counts)
__global__ void __launch_bounds__(BLOCK) k_hexlines_walk(u64* __restrict__ start, u64* __restrict__ end, const uint8_t* __restrict__ text,
                                                         size_t len, const u32* __restrict__ first, u32 nlines) {
    __shared__ u32 wave_total[BLOCK / 64];
    const size_t base = ((size_t)blockIdx.x * BLOCK + threadIdx.x) * HEXLINES_SEG;
    const u32 terms = hexlines_term_mask(text, len, base);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u32 mine = (u32)__builtin_popcount(terms);
    u32 inc = mine;
    for (int o = 1; o < 64; o <<= 1) {
        const u32 below = (u32)__shfl_up((int)inc, o);
        if (lane >= o) inc += below;
    }
    if (lane == 63) wave_total[wave] = inc;
    __syncthreads();
    u32 rank = first[blockIdx.x] + inc - mine;
    for (int k = 0; k < wave; ++k) rank += wave_total[k];
    if (base == 0 && nlines) start[0] = 0;
    for (u32 m = terms; m; m &= m - 1) {
        const size_t j = base + (size_t)__builtin_ctz(m);
        const bool crlf = text[j] == '\n' && j > 0 && text[j - 1] == '\r';
        if (rank < nlines) end[rank] = crlf ? j - 1 : j;
        if (j + 1 < len && rank + 1 < nlines) start[rank + 1] = j + 1;
        ++rank;
    }
    // text behind the last terminator: a line that the end of the text closes
    if (len && nlines && len - 1 >= base && len - 1 - base < (size_t)HEXLINES_SEG && !((terms >> (len - 1 - base)) & 1u)) end[nlines - 1] = len;
}

__device__ __forceinline__ u32 hex_nibble(u32 c, u32& err) {          // 0-9 a-f A-F, nothing else
    const u32 d = c - '0', a = (c | 0x20u) - 'a';
    err |= (u32)!(d < 10u || a < 6u);
    return d < 10u ? d : (a + 10u) & 15u;
}
__device__ __forceinline__ u32 hex_digit(u32 n) { return n + '0' + (n > 9u ? (u32)('a' - '0' - 10) : 0u); }
// which bytes of a record are framing, eight at a time, as 0xff / 0x00 from the mask's 0 / 1 / 2 (hexlines_layout.h)
__device__ __forceinline__ u64 hexlines_any_framing(u64 m) { return ((m | (m >> 1)) & 0x0101010101010101ull) * 0xffull; }
__device__ __forceinline__ u64 hexlines_outer_framing(u64 m) { return (m & 0x0101010101010101ull) * 0xffull; }

// rec + line * B = the B bytes that the H = 2 B digits of line `line` spell; HEXLINES_LANES lanes per line, 16 digits -> 8 bytes per
// step.  A line whose length is not H, a character that is no hex digit, a framing byte that differs from the template:
// *first_bad = min(*first_bad, line).  The digits are read only when the line has H of them inside the text, so nothing that the
// text says becomes an address.  The leaf headers are compared here too -- the line is to be named -- and again by the import kernels.
__global__ void __launch_bounds__(BLOCK) k_hexlines_decode(uint8_t* __restrict__ rec, const uint8_t* __restrict__ text, size_t len,
                                                           const u64* __restrict__ start, const u64* __restrict__ end, u32 nlines, u32 B,
                                                           const uint8_t* __restrict__ tmpl, const uint8_t* __restrict__ mask,
                                                           u32* __restrict__ first_bad) {
    const size_t line = ((size_t)blockIdx.x * BLOCK + threadIdx.x) / HEXLINES_LANES;
    const u32 sub = threadIdx.x % HEXLINES_LANES;
    if (line >= nlines) return;
    const u64 s = start[line], e = end[line];
    u32 bad = !(s <= e && e <= (u64)len && e - s == 2ull * B);
    if (!bad) {
        const uint8_t* __restrict__ src = text + s;
        uint8_t* __restrict__ dst = rec + line * B;
        for (u32 c = sub * 8; c < B; c += HEXLINES_LANES * 8) {
            if (c + 8 <= B) {
                uint4 d;
                __builtin_memcpy(&d, src + 2 * (size_t)c, 16);
                const u32 w[4] = {d.x, d.y, d.z, d.w};
                u64 out = 0;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const u32 pair = w[k >> 1] >> (16 * (k & 1));
                    const u32 byte = (hex_nibble(pair & 0xffu, bad) << 4) | hex_nibble((pair >> 8) & 0xffu, bad);
                    out |= (u64)byte << (8 * k);
                }
                u64 t, m;
                __builtin_memcpy(&t, tmpl + c, 8);
                __builtin_memcpy(&m, mask + c, 8);
                bad |= (u32)(((out ^ t) & hexlines_any_framing(m)) != 0);
                __builtin_memcpy(dst + c, &out, 8);
            } else {
                for (u32 k = c; k < B; ++k) {
                    const u32 byte = (hex_nibble(src[2 * (size_t)k], bad) << 4) | hex_nibble(src[2 * (size_t)k + 1], bad);
                    bad |= (u32)(mask[k] != 0 && byte != tmpl[k]);
                    dst[k] = (uint8_t)byte;
                }
            }
        }
    }
    if (bad) atomicMin(first_bad, (u32)line);
}

// The reverse: line `line` of the text = the 2 B lowercase digits of the record at rec + line * B and a \n.  The export kernels have
// written the components with their leaf headers into the records; the framing of the outer nodes comes from the template.
__global__ void __launch_bounds__(BLOCK) k_hexlines_encode(uint8_t* __restrict__ text, const uint8_t* __restrict__ rec, u32 nlines, u32 B,
                                                           const uint8_t* __restrict__ tmpl, const uint8_t* __restrict__ mask) {
    const size_t line = ((size_t)blockIdx.x * BLOCK + threadIdx.x) / HEXLINES_LANES;
    const u32 sub = threadIdx.x % HEXLINES_LANES;
    if (line >= nlines) return;
    const uint8_t* __restrict__ src = rec + line * B;
    uint8_t* __restrict__ dst = text + line * (2 * (size_t)B + 1);
    for (u32 c = sub * 8; c < B; c += HEXLINES_LANES * 8) {
        if (c + 8 <= B) {
            u64 r, t, m;
            __builtin_memcpy(&r, src + c, 8);
            __builtin_memcpy(&t, tmpl + c, 8);
            __builtin_memcpy(&m, mask + c, 8);
            const u64 outer = hexlines_outer_framing(m);
            r = (r & ~outer) | (t & outer);
            u32 w[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const u32 b0 = (u32)(r >> (16 * k)) & 0xffu, b1 = (u32)(r >> (16 * k + 8)) & 0xffu;
                w[k] = hex_digit(b0 >> 4) | (hex_digit(b0 & 15u) << 8) | (hex_digit(b1 >> 4) << 16) | (hex_digit(b1 & 15u) << 24);
            }
            const uint4 o = make_uint4(w[0], w[1], w[2], w[3]);
            __builtin_memcpy(dst + 2 * (size_t)c, &o, 16);
        } else {
            for (u32 k = c; k < B; ++k) {
                const u32 byte = mask[k] == 1 ? tmpl[k] : src[k];
                dst[2 * (size_t)k] = (uint8_t)hex_digit(byte >> 4);
                dst[2 * (size_t)k + 1] = (uint8_t)hex_digit(byte & 15u);
            }
        }
    }
    if (sub == 0) dst[2 * (size_t)B] = '\n';
}

}  // namespace vmn
