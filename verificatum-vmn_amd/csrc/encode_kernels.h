// encode_kernels.h — the text interface behind a session (csrc/encode_layout.h): lines of text <-> big-endian records of the
// group's wire width, which the import / export kernels of the byte trees take from and bring to the arrays.  The residue fix of
// encode() is k_jacobi_fix / k_jacobi_fix_lanes (modp_kernels.h: the Jacobi loop exists once, beside the membership kernels).
//
// Encoding:  k_textlines_records   the records of all components of all lines, TEXTLINES_LANES lanes per record; the first line
//                                  that has more than ncomp L bytes is named instead
// Decoding:  k_textlines_fold      one lane per record: v = min(e, p - e) in place, the length word read and checked
//            k_textlines_lengths   one lane per line: the UTF-8 verdict over the concatenated payload, the bytes that survive the
//                                  stripping of \n and \r, and the sums of the line lengths per workgroup
//            (k_jsonlines_offsets  the 64-bit exclusive scan of those sums: decimal_kernels.h, unchanged)
//            k_textlines_emit      one lane per line: the scan of its workgroup's lengths, then the surviving bytes and \n
// Records are component-major: record (c, line) at ((size_t)c * nlines + line) * nbytes.
#pragma once
#include "encode_layout.h"
#include "modp_kernels.h"

namespace vmn {

constexpr int TEXTLINES_LANES = 16;                    // lanes per record in k_textlines_records
constexpr u32 TEXTLINES_ILL_FORMED = 1u, TEXTLINES_NOT_UTF8 = 2u;        // the bits OR-ed into the flags word

// rec[(c, line)] = the record of component c of line `line`; *first_long = the smallest line with more than ncomp L bytes
// (atomicMin; 0xffffffff before), whose records are left unwritten.
__global__ void __launch_bounds__(BLOCK) k_textlines_records(uint8_t* __restrict__ rec, const uint8_t* __restrict__ text,
                                                             const u64* __restrict__ starts, const u64* __restrict__ ends, u32 nlines,
                                                             u32 ncomp, u32 nbytes, u32 L, u32* __restrict__ first_long) {
    const size_t idx = ((size_t)blockIdx.x * BLOCK + threadIdx.x) / TEXTLINES_LANES;
    const u32 sub = threadIdx.x % TEXTLINES_LANES;
    if (idx >= (size_t)nlines * ncomp) return;
    const u32 c = (u32)(idx / nlines), line = (u32)(idx % nlines);
    const u64 s = starts[line], mlen = ends[line] - s;
    if (mlen > (u64)ncomp * L) {
        if (c == 0 && sub == 0) atomicMin(first_long, line);
        return;
    }
    uint8_t* __restrict__ dst = rec + idx * nbytes;
    for (u32 k = sub; k < nbytes; k += TEXTLINES_LANES) dst[k] = encode::record_byte(k, nbytes, L, c, text + s, mlen);
}

// plen[r] = the message length of record r after the fold (encode::ILL_FORMED: none, reported in flags); p_be, q_be on nbytes bytes
__global__ void __launch_bounds__(BLOCK) k_textlines_fold(uint8_t* __restrict__ rec, u32* __restrict__ plen, size_t total, u32 nbytes, u32 L,
                                                          const uint8_t* __restrict__ p_be, const uint8_t* __restrict__ q_be,
                                                          u32* __restrict__ flags) {
    const size_t r = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (r >= total) return;
    const u32 len = encode::fold_record(rec + r * nbytes, nbytes, L, p_be, q_be);
    plen[r] = len;
    if (len == encode::ILL_FORMED) atomicOr(flags, TEXTLINES_ILL_FORMED);
}

// the payload of record (c, line): where it begins and how many bytes it has (none when ill-formed)
__device__ __forceinline__ const uint8_t* textlines_piece(const uint8_t* __restrict__ rec, const u32* __restrict__ plen, u32 c, u32 line,
                                                          u32 nlines, u32 nbytes, u32 L, u32& count) {
    const size_t r = (size_t)c * nlines + line;
    const u32 len = plen[r];
    count = len == encode::ILL_FORMED ? 0u : len;
    return rec + r * nbytes + (nbytes - L);
}

// lens[line] = surviving bytes + 1; bsum[workgroup] = the sum of its lines' lengths (as k_jsonlines_lengths)
__global__ void __launch_bounds__(BLOCK) k_textlines_lengths(u32* __restrict__ lens, u64* __restrict__ bsum, const uint8_t* __restrict__ rec,
                                                             const u32* __restrict__ plen, u32 nlines, u32 ncomp, u32 nbytes, u32 L,
                                                             u32* __restrict__ flags) {
    __shared__ u64 wave_total[BLOCK / 64];
    const size_t line = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    u32 mine = 0;
    if (line < nlines) {
        encode::Utf8 u;
        mine = 1;
        for (u32 c = 0; c < ncomp; ++c) {
            u32 count;
            const uint8_t* __restrict__ src = textlines_piece(rec, plen, c, (u32)line, nlines, nbytes, L, count);
            for (u32 j = 0; j < count; ++j) {
                const uint8_t b = src[j];
                u.step(b);
                mine += encode::stripped(b) ? 0u : 1u;
            }
        }
        lens[line] = mine;
        if (!u.wellformed()) atomicOr(flags, TEXTLINES_NOT_UTF8);
    }
    u32 lo = mine & 0xffffu, hi = mine >> 16;                     // (a wave's 64 lines: summed in two halves of 32 bits)
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

// Line `line` begins at base[line / BLOCK] + the lengths of the lines of its workgroup in front of it (scanned here, in LDS); the
// workgroups are those of k_textlines_lengths.  Writes lens[line] bytes, the last one \n.
__global__ void __launch_bounds__(BLOCK) k_textlines_emit(uint8_t* __restrict__ text, const u64* __restrict__ base, const u32* __restrict__ lens,
                                                          const uint8_t* __restrict__ rec, const u32* __restrict__ plen, u32 nlines,
                                                          u32 ncomp, u32 nbytes, u32 L) {
    __shared__ u64 before[BLOCK];
    const size_t line = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool live = line < nlines;
    const u32 mine = live ? lens[line] : 0u;
    before[threadIdx.x] = mine;
    __syncthreads();
    for (int o = 1; o < BLOCK; o <<= 1) {
        const u64 v = (int)threadIdx.x >= o ? before[threadIdx.x - o] : 0;
        __syncthreads();
        before[threadIdx.x] += v;
        __syncthreads();
    }
    if (!live) return;
    uint8_t* __restrict__ dst = text + base[blockIdx.x] + (before[threadIdx.x] - mine);
    u32 pos = 0;
    for (u32 c = 0; c < ncomp; ++c) {
        u32 count;
        const uint8_t* __restrict__ src = textlines_piece(rec, plen, c, (u32)line, nlines, nbytes, L, count);
        for (u32 j = 0; j < count; ++j) {
            const uint8_t b = src[j];
            if (!encode::stripped(b) && pos + 1 < mine) dst[pos++] = b;     // (pos + 1 < mine always: lens counted these bytes)
        }
    }
    dst[pos] = '\n';
}

}  // namespace vmn
