// One bit per sudoku cell (81 of them) and the masks of the 27 units: shared by the kernels that treat a frame's cells as ballots
// of one wave, a lane owning cells `lane` and `lane + 64` (k9_resolve.hip, k10_propagate.hip).
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace {

struct m81 { uint64_t lo, hi; };  // one bit per cell
__device__ __forceinline__ m81 operator&(m81 a, m81 b) { return {a.lo & b.lo, a.hi & b.hi}; }
__device__ __forceinline__ m81 operator|(m81 a, m81 b) { return {a.lo | b.lo, a.hi | b.hi}; }
__device__ __forceinline__ m81 operator~(m81 a) { return {~a.lo, ~a.hi}; }
__device__ __forceinline__ bool any(m81 a) { return (a.lo | a.hi) != 0; }
__device__ __forceinline__ int pop(m81 a) { return __popcll(a.lo) + __popcll(a.hi); }
__device__ __forceinline__ int first(m81 a) { return a.lo ? __ffsll((long long)a.lo) - 1 : 63 + __ffsll((long long)a.hi); }
__device__ __forceinline__ m81 shl(m81 a, int s)   // 0 <= s < 128
{
    if (s >= 64) return {0, a.lo << (s - 64)};
    return {a.lo << s, (a.hi << s) | (s ? a.lo >> (64 - s) : 0)};
}
__device__ __forceinline__ m81 row_mask(int r) { return shl({0x1FFull, 0}, 9 * r); }
__device__ __forceinline__ m81 col_mask(int c) { return shl({0x8040201008040201ull, 0x100ull}, c); }               // bits 0, 9, .., 72
__device__ __forceinline__ m81 box_mask(int b) { return shl({0x1C0E07ull, 0}, 27 * (b / 3) + 3 * (b % 3)); }       // bits 0-2, 9-11, 18-20
__device__ __forceinline__ int box_of(int x) { return (x / 27) * 3 + (x % 9) / 3; }
// units in validate_predictions' order: rows 0-8, columns 9-17, boxes 18-26
__device__ __forceinline__ m81 unit_mask(int u) { return u < 9 ? row_mask(u) : u < 18 ? col_mask(u - 9) : box_mask(u - 18); }

}  // namespace
