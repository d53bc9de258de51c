// decimal_kernels.h — the `json` ciphertext interface (csrc/jsonlines_layout.h): lines of decimal strings <-> big-endian records of
// nbytes per value, on which the import / export kernels of the byte trees work component by component.  Included by vmnhip.hip
// only, behind light_kernels.h, whose line discovery (k_hexlines_count, the u32 scan, k_hexlines_walk) finds the lines here too.
//
// Reading:   k_jsonlines_scan   grammar of every line; where the significant digits of its 2w numbers are
//            k_dec_to_rows      decimal -> binary: value = sum_j chunk_j 10^(9j), chunks of 9 digits from the least significant end
// Writing:   k_rows_to_dec      binary -> decimal: base-10^9 chunk k = sum_h half_h (2^(16h))_k, then one carry pass
//            k_jsonlines_lengths / k_jsonlines_offsets / k_jsonlines_emit
//                               line lengths from the digit counts, their 64-bit exclusive scan (10^6 lines at width 3 pass 4 GB),
//                               the text with its fixed framing
// The tables of powers (10^(9j) in 32-bit words, 2^(16h) in base 10^9) are built once per group on the host (vmnhip.hip).
// Both conversions give a wave to a value: a lane owns output words (chunks) lane, lane + 64, ... and accumulates its column of
// the product lazily, so there is no carry chain inside the quadratic part and the table reads are coalesced; one lane then
// resolves the carries of the value in LDS, a pass as long as one column.
#pragma once
#include "jsonlines_layout.h"
#include "light_kernels.h"

namespace vmn {

constexpr u32 DEC_BASE = 1000000000u;                  // 10^9 < 2^30
constexpr int DEC_DIGITS = 9;
constexpr int DEC_LANES = 64;                          // lanes per value in the two conversions: one wave
constexpr int DEC_VPB = BLOCK / DEC_LANES;             // values per workgroup
// The limits of the LDS of the two conversions; the host refuses a modulus beyond them (VMN_ERR_UNSUPPORTED).  A 16 384-bit
// modulus has 4933 digits = 549 chunks, and 10^(9 * 549) has 513 words.
constexpr int DEC_MAX_CHUNKS = 552;
constexpr int DEC_MAX_WORDS = 516;
constexpr int JSONLINES_LANES = 32;                    // lanes per line in k_jsonlines_emit

// ---- reading -----------------------------------------------------------------------------------------------------------------
// One lane per line walks the grammar (jsonlines::scan_ciphertext_line): span_at / span_len [line * 2w + c] = where the significant
// digits of component c begin in the text and how many there are (leading zeros stripped; none for "0"; saturated at 2^32 - 1).
// A defective line: *first_bad = min(*first_bad, line).  The walk reads inside [start, end) of its own line only and a span lies
// inside it: nothing that the text says becomes an address.
__global__ void __launch_bounds__(BLOCK) k_jsonlines_scan(u64* __restrict__ span_at, u32* __restrict__ span_len,
                                                          const uint8_t* __restrict__ text, size_t len, const u64* __restrict__ start,
                                                          const u64* __restrict__ end, u32 nlines, u32 width, u32* __restrict__ first_bad) {
    const size_t line = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (line >= nlines) return;
    const u64 s = start[line], e = end[line];
    bool ok = s <= e && e <= (u64)len;
    if (ok) {
        u64* __restrict__ at = span_at + line * 2 * (size_t)width;
        u32* __restrict__ ln = span_len + line * 2 * (size_t)width;
        ok = jsonlines::scan_ciphertext_line(text, s, e, width, [&](u32 c, u64 begin, u64 count) {
            at[c] = begin;
            ln[c] = count > 0xffffffffull ? 0xffffffffu : (u32)count;
        });
    }
    if (!ok) atomicMin(first_bad, (u32)line);
}

// rows + v * nbytes = the value of number v as nbytes big-endian bytes, v = c * nlines + line (component by component, so that the
// import kernel runs once per component at stride nbytes).  A number of more than dmax significant digits, or one that does not
// fit 8 nbytes bits, is nbytes bytes of 0xff: no prime is 2^(8n) - 1, so the import kernel reports it by itself.
// pow10[j * nwa + i] = word i of 10^(9j), j < ceil(dmax / 9) <= DEC_MAX_CHUNKS, nwa = the words of 10^(9 ceil(dmax / 9)) <=
// DEC_MAX_WORDS: every value of at most dmax digits fits them.  Word i of 10^(9j) is zero while 30 j <= 32 i: the column starts
// at j = 32 i / 30.
// Accumulator: a chunk is below 10^9 < 2^30 and a table word below 2^32, so a term is below 2^62; a column has at most
// DEC_MAX_CHUNKS = 552 terms, below 2^72 together: 64 bits and a 32-bit count of their overflows hold it.
__global__ void __launch_bounds__(BLOCK) k_dec_to_rows(uint8_t* __restrict__ rows, u32 nbytes, const uint8_t* __restrict__ text,
                                                       const u64* __restrict__ span_at, const u32* __restrict__ span_len, u32 nlines,
                                                       u32 ncomp, u32 dmax, u32 nwa, const u32* __restrict__ pow10) {
    __shared__ u32 chunk[DEC_VPB][DEC_MAX_CHUNKS];
    __shared__ u32 part[DEC_VPB][3][DEC_MAX_WORDS + 2];          // part[p][i]: bits 32p .. 32p + 31 of column i - p
    __shared__ u32 over[DEC_VPB];
    const u32 slot = threadIdx.x / DEC_LANES, lane = threadIdx.x % DEC_LANES;
    const size_t total = (size_t)nlines * ncomp;
    const size_t v = (size_t)blockIdx.x * DEC_VPB + slot;
    const bool live = v < total;
    u32 count = 0;
    u64 at = 0;
    if (live) {
        const size_t c = v / nlines, line = v - c * nlines;
        at = span_at[line * ncomp + c];
        count = span_len[line * ncomp + c];
    }
    const bool too_long = count > dmax;
    const u32 nc = too_long ? 0u : (count + DEC_DIGITS - 1) / DEC_DIGITS;
    for (u32 j = lane; j < nc; j += DEC_LANES) {
        const u32 hi = count - DEC_DIGITS * j, lo = hi >= (u32)DEC_DIGITS ? hi - DEC_DIGITS : 0u;
        u32 val = 0;
        for (u32 k = lo; k < hi; ++k) val = val * 10u + (u32)(text[at + k] - '0');
        chunk[slot][j] = val;
    }
    if (lane == 0) part[slot][1][0] = part[slot][2][0] = part[slot][2][1] = 0;
    __syncthreads();
    for (u32 i = lane; i < nwa; i += DEC_LANES) {
        u64 lo = 0;
        u32 hi = 0;
        const u32* __restrict__ col = pow10 + i;
        for (u32 j = (32u * i) / 30u; j < nc; ++j) {
            const u64 term = (u64)chunk[slot][j] * col[(size_t)j * nwa];
            lo += term;
            hi += (u32)(lo < term);
        }
        part[slot][0][i] = (u32)lo;
        part[slot][1][i + 1] = (u32)(lo >> 32);
        part[slot][2][i + 2] = hi;
    }
    __syncthreads();
    if (lane == 0) {                                              // the carries of the value: word i = the three parts that meet there
        const u32 whole = nbytes / 4, rest = nbytes % 4;
        u64 carry = 0;
        u32 beyond = 0;
        for (u32 i = 0; i < nwa; ++i) {
            const u64 s = (u64)part[slot][0][i] + part[slot][1][i] + part[slot][2][i] + carry;
            const u32 w = (u32)s;
            carry = s >> 32;
            part[slot][0][i] = w;
            if (i > whole) beyond |= w;
            else if (i == whole) beyond |= rest ? w >> (8 * rest) : w;
        }
        over[slot] = beyond | (u32)carry;                         // (the carry out of the last word: zero by the bound on nwa)
    }
    __syncthreads();
    if (!live) return;
    const bool ff = too_long || over[slot] != 0;
    uint8_t* __restrict__ dst = rows + v * nbytes;
    for (u32 b = lane; b < nbytes; b += DEC_LANES) {
        const u32 k = nbytes - 1 - b;                             // the byte's weight: 2^(8k)
        const u32 w = k / 4 < nwa ? part[slot][0][k / 4] : 0u;
        dst[b] = ff ? (uint8_t)0xff : (uint8_t)(w >> (8 * (k % 4)));
    }
}

// ---- writing -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ u32 dec_digits_of(u32 chunk) {         // decimal digits of a chunk below 10^9; 0 has none
    u32 d = 0;
    for (u32 p = 1; d < (u32)DEC_DIGITS && chunk >= p; p *= 10u) ++d;          // (p stays below 10^9 < 2^32)
    return d;
}

// digits + v * dmax = the dmax decimal digits of the value at rows + v * nbytes (big-endian, below the modulus, as the export
// kernel writes it), zero-padded in front; counts[v] = its digits without the padding, 1 for zero -- from the conversion itself,
// not from the bit length.  nw = the words of the modulus; pow2[h * nc + k] = chunk k (base 10^9) of 2^(16h), h < 2 nw, nc =
// ceil(dmax / 9) chunks.  Chunk k of 2^(16h) is zero while 2^(16h) < 10^(9k): the column starts at h = 1868 k / 1000 (9 log2(10) /
// 16 = 1.8686...).
// Accumulator: a half word is below 2^16 and a table chunk below 2^30, so a term is below 2^46; a column has at most 2 nw <=
// 2 DEC_MAX_WORDS = 1032 terms, below 2^57 together; with the carry of the chunk below (< 2^28) it stays in 64 bits.
__global__ void __launch_bounds__(BLOCK) k_rows_to_dec(uint8_t* __restrict__ digits, u32* __restrict__ counts, const uint8_t* __restrict__ rows,
                                                       u32 nbytes, size_t total, u32 dmax, u32 nc, u32 nw, const u32* __restrict__ pow2) {
    __shared__ u32 half[DEC_VPB][2 * DEC_MAX_WORDS];
    __shared__ u64 acc[DEC_VPB][DEC_MAX_CHUNKS];
    const u32 slot = threadIdx.x / DEC_LANES, lane = threadIdx.x % DEC_LANES;
    const size_t v = (size_t)blockIdx.x * DEC_VPB + slot;
    const bool live = v < total;
    const uint8_t* __restrict__ src = rows + (live ? v : 0) * nbytes;
    for (u32 h = lane; h < 2 * nw; h += DEC_LANES) {              // half word h: the bytes of weight 2^(16h) and 2^(16h + 8)
        const u32 k = 2 * h;
        const u32 b0 = live && k < nbytes ? src[nbytes - 1 - k] : 0u, b1 = live && k + 1 < nbytes ? src[nbytes - 2 - k] : 0u;
        half[slot][h] = b0 | (b1 << 8);
    }
    __syncthreads();
    for (u32 k = lane; k < nc; k += DEC_LANES) {
        u64 a = 0;
        const u32* __restrict__ col = pow2 + k;
        for (u32 h = (1868u * k) / 1000u; h < 2 * nw; ++h) a += (u64)half[slot][h] * col[(size_t)h * nc];
        acc[slot][k] = a;
    }
    __syncthreads();
    if (lane == 0) {                                              // the carries, in base 10^9; the exact digit count
        u64 carry = 0;
        u32 top = 0, top_chunk = 0;
        for (u32 k = 0; k < nc; ++k) {
            const u64 s = acc[slot][k] + carry;
            carry = s / DEC_BASE;
            const u32 c = (u32)(s - carry * DEC_BASE);
            acc[slot][k] = c;
            if (c) {
                top = k;
                top_chunk = c;
            }
        }
        if (live) counts[v] = top_chunk ? DEC_DIGITS * top + dec_digits_of(top_chunk) : 1u;
    }
    __syncthreads();
    if (!live) return;
    uint8_t* __restrict__ dst = digits + v * dmax;
    for (u32 k = lane; k < nc; k += DEC_LANES) {
        u32 c = (u32)acc[slot][k];
        for (u32 d = 0; d < (u32)DEC_DIGITS; ++d) {
            const u32 pos = DEC_DIGITS * k + d;                   // the digit's weight: 10^pos
            const u32 q = c / 10u;
            if (pos < dmax) dst[dmax - 1 - pos] = (uint8_t)('0' + (c - q * 10u));
            c = q;
        }
    }
}

// the framing of a line around its digits (jsonlines_layout.h)
__device__ __forceinline__ u32 jsonlines_framing(u32 width, int plain) {
    const u32 per = plain ? 2u : (u32)jsonlines::PAIR_FRAMING;
    return width == 1 ? per + 1 : 2 + width * per + (width - 1) + 1;
}

// lens[line] = the bytes of line `line`, newline included (below 2^30: the host bounds the width); bsum[block] = the sum over the
// BLOCK lines of the workgroup, 64-bit.  counts[c * nlines + line], c < ncomp = (plain ? width : 2 width).
__global__ void __launch_bounds__(BLOCK) k_jsonlines_lengths(u32* __restrict__ lens, u64* __restrict__ bsum, const u32* __restrict__ counts,
                                                             u32 nlines, u32 width, int plain) {
    __shared__ u64 wave_total[BLOCK / 64];
    const size_t line = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const u32 ncomp = plain ? width : 2 * width;
    u32 mine = 0;
    if (line < nlines) {
        mine = jsonlines_framing(width, plain);
        for (u32 c = 0; c < ncomp; ++c) mine += counts[(size_t)c * nlines + line];
        lens[line] = mine;
    }
    // (a wave's 64 lines are below 2^36 together: summed in two halves of 32 bits)
    u32 lo = mine & 0xffffu, hi = mine >> 16;
    for (int o = 32; o > 0; o >>= 1) {
        lo += (u32)__shfl_xor((int)lo, o);
        hi += (u32)__shfl_xor((int)hi, o);
    }
    if ((threadIdx.x & 63) == 0) wave_total[threadIdx.x >> 6] = (u64)lo + ((u64)hi << 16);
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 s = 0;
        for (int k = 0; k < BLOCK / 64; ++k) s += wave_total[k];
        bsum[blockIdx.x] = s;
    }
}

// bsum[b] <- the sum of bsum[0 .. b), *total = the sum of all nb of them.  One workgroup: a thread sums a run of the array, thread 0
// scans the BLOCK run sums, every thread writes its run's prefixes.
__global__ void __launch_bounds__(BLOCK) k_jsonlines_offsets(u64* __restrict__ bsum, size_t nb, u64* __restrict__ total) {
    __shared__ u64 run[BLOCK];
    const size_t per = (nb + BLOCK - 1) / BLOCK;
    const size_t lo = (size_t)threadIdx.x * per, hi = lo + per < nb ? lo + per : nb;
    u64 s = 0;
    for (size_t k = lo; k < hi; ++k) s += bsum[k];
    run[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 before = 0;
        for (int t = 0; t < BLOCK; ++t) {
            const u64 r = run[t];
            run[t] = before;
            before += r;
        }
        *total = before;
    }
    __syncthreads();
    u64 before = run[threadIdx.x];
    for (size_t k = lo; k < hi; ++k) {
        const u64 r = bsum[k];
        bsum[k] = before;
        before += r;
    }
}

// Line `line` of the text, JSONLINES_LANES lanes per line: it begins at base[line / BLOCK] + the lengths of the lines of its
// workgroup of k_jsonlines_lengths in front of it.  plain: a line of `width` plaintexts, else of `width` pairs.
__global__ void __launch_bounds__(BLOCK) k_jsonlines_emit(uint8_t* __restrict__ text, const u64* __restrict__ base, const u32* __restrict__ lens,
                                                          const uint8_t* __restrict__ digits, const u32* __restrict__ counts, u32 nlines,
                                                          u32 width, u32 dmax, int plain) {
    const size_t line = ((size_t)blockIdx.x * BLOCK + threadIdx.x) / JSONLINES_LANES;
    const u32 sub = threadIdx.x % JSONLINES_LANES;
    if (line >= nlines) return;
    const size_t group = line / BLOCK, first = group * BLOCK;
    u64 mine = 0;
    for (size_t k = first + sub; k < line; k += JSONLINES_LANES) mine += lens[k];
    u32 lo = (u32)mine, hi = (u32)(mine >> 32);                   // (below 2^38: two words, summed apart)
    u32 lo_lo = lo & 0xffffu, lo_hi = lo >> 16;
    for (int o = JSONLINES_LANES / 2; o > 0; o >>= 1) {
        lo_lo += (u32)__shfl_xor((int)lo_lo, o);
        lo_hi += (u32)__shfl_xor((int)lo_hi, o);
        hi += (u32)__shfl_xor((int)hi, o);
    }
    uint8_t* __restrict__ dst = text + base[group] + (u64)lo_lo + ((u64)lo_hi << 16) + ((u64)hi << 32);
    u64 pos = 0;
    auto put = [&](const char* s, u32 n) {                        // n <= JSONLINES_LANES bytes of framing
        if (sub < n) dst[pos + sub] = (uint8_t)s[sub];
        pos += n;
    };
    auto number = [&](u32 c) {
        const size_t v = (size_t)c * nlines + line;
        const u32 count = counts[v];
        const uint8_t* __restrict__ src = digits + v * dmax + (dmax - count);
        for (u32 t = sub; t < count; t += JSONLINES_LANES) dst[pos + t] = src[t];
        pos += count;
    };
    if (width > 1) put("[", 1);
    for (u32 i = 0; i < width; ++i) {
        if (i) put(",", 1);
        if (plain) {
            put("\"", 1);
            number(i);
            put("\"", 1);
        } else {
            put("{\"alpha\":\"", 10);
            number(i);
            put("\",\"beta\":\"", 10);
            number(width + i);
            put("\"}", 2);
        }
    }
    if (width > 1) put("]", 1);
    put("\n", 1);
}

}  // namespace vmn
