// wave_primitives.h — wave64 cross-lane building blocks for gfx950 (CDNA4): the wave and its four 16-lane DPP rows.
//
// Everything here is wave-wide (64 lanes) or row-wide (16) and uses DPP row operations directly
// (`__builtin_amdgcn_update_dpp`), not LDS and not 32-wide shuffle idioms.  At the end: how a launch that strides sizes its grid.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace inq {

constexpr int kWave = 64;
constexpr int kRowLanes = 16;  // lanes of one DPP row: one read stream of the row walk, one record or pair of the side kernels

// DPP control words (GFX9 encoding)
constexpr int DPP_ROW_SHR1 = 0x111;
constexpr int DPP_ROW_SHR2 = 0x112;
constexpr int DPP_ROW_SHR4 = 0x114;
constexpr int DPP_ROW_SHR8 = 0x118;
constexpr int DPP_ROW_BCAST15 = 0x142;  // lane 15 of each row -> every lane of the next row
constexpr int DPP_ROW_BCAST31 = 0x143;  // lane 31 -> every lane of rows 2 and 3

__device__ __forceinline__ int lane_id() { return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

// x + (x shifted right by N lanes inside a 16-lane row, 0 shifted in)
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_shr_zero(uint32_t x) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xf, 0xf, true);
}
// ... of a 64-bit value: two 32-bit DPP moves
template <int CTRL>
__device__ __forceinline__ uint64_t dpp_shr_zero_u64(uint64_t x) {
    return (uint64_t)dpp_shr_zero<CTRL>((uint32_t)x) | (uint64_t)dpp_shr_zero<CTRL>((uint32_t)(x >> 32)) << 32;
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_bcast(uint32_t x) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, ROW_MASK, 0xf, false);
}

// Inclusive prefix sum inside each row, wrapping arithmetic.  4 DPP adds (8 moves for u64).
__device__ __forceinline__ uint32_t row_inclusive_scan_u32(uint32_t x) {
    x += dpp_shr_zero<DPP_ROW_SHR1>(x);
    x += dpp_shr_zero<DPP_ROW_SHR2>(x);
    x += dpp_shr_zero<DPP_ROW_SHR4>(x);
    x += dpp_shr_zero<DPP_ROW_SHR8>(x);
    return x;
}
__device__ __forceinline__ uint64_t row_inclusive_scan_u64(uint64_t x) {
    x += dpp_shr_zero_u64<DPP_ROW_SHR1>(x);
    x += dpp_shr_zero_u64<DPP_ROW_SHR2>(x);
    x += dpp_shr_zero_u64<DPP_ROW_SHR4>(x);
    x += dpp_shr_zero_u64<DPP_ROW_SHR8>(x);
    return x;
}
// Lane 15 of each row to every lane of the row: ds_swizzle in bit-mask mode reads lane
// ((l & 0x10) | 0x0f) of its 32-lane half.
__device__ __forceinline__ uint32_t row_last(uint32_t x) { return (uint32_t)__builtin_amdgcn_ds_swizzle((int)x, 0x10 | (0x0f << 5)); }
__device__ __forceinline__ uint64_t row_last_u64(uint64_t x) { return (uint64_t)row_last((uint32_t)x) | (uint64_t)row_last((uint32_t)(x >> 32)) << 32; }
// The value of lane (l ^ J), J a power of two: ds_swizzle in bit-mask mode (and 0x1f, or 0, xor J) inside a 32-lane half,
// ds_bpermute between the halves.  Every lane of the wave must be active.
template <int J>
__device__ __forceinline__ uint32_t lane_xor(uint32_t x, int lane) {
    static_assert(J == 1 || J == 2 || J == 4 || J == 8 || J == 16 || J == 32, "one lane bit");
    if constexpr (J < 32)
        return (uint32_t)__builtin_amdgcn_ds_swizzle((int)x, 0x1f | (J << 10));
    else
        return (uint32_t)__builtin_amdgcn_ds_bpermute((lane ^ 32) << 2, (int)x);
}
// Lane 15 of the row holds the OR / the maximum of its lanes
__device__ __forceinline__ uint32_t row_or(uint32_t x) {
    x |= dpp_shr_zero<DPP_ROW_SHR1>(x);
    x |= dpp_shr_zero<DPP_ROW_SHR2>(x);
    x |= dpp_shr_zero<DPP_ROW_SHR4>(x);
    x |= dpp_shr_zero<DPP_ROW_SHR8>(x);
    return x;
}
__device__ __forceinline__ uint64_t row_max_u64(uint64_t x) {
    const auto larger = [](uint64_t o, uint64_t v) { return o > v ? o : v; };
    x = larger(dpp_shr_zero_u64<DPP_ROW_SHR1>(x), x);
    x = larger(dpp_shr_zero_u64<DPP_ROW_SHR2>(x), x);
    x = larger(dpp_shr_zero_u64<DPP_ROW_SHR4>(x), x);
    x = larger(dpp_shr_zero_u64<DPP_ROW_SHR8>(x), x);
    return x;
}

// Inclusive prefix sum over the 64 lanes, wrapping u32 arithmetic.  6 DPP adds.
__device__ __forceinline__ uint32_t wave_inclusive_scan_u32(uint32_t x) {
    x = row_inclusive_scan_u32(x);
    x += dpp_bcast<DPP_ROW_BCAST15, 0xa>(x);  // row0 total -> row1, row2 total -> row3
    x += dpp_bcast<DPP_ROW_BCAST31, 0xc>(x);  // rows0-1 total -> rows 2,3
    return x;
}

__device__ __forceinline__ uint32_t readlane_u32(uint32_t v, int l) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, l);
}
__device__ __forceinline__ int64_t readlane_i64(int64_t v, int l) {
    uint32_t lo = readlane_u32((uint32_t)v, l);
    uint32_t hi = readlane_u32((uint32_t)((uint64_t)v >> 32), l);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
// v_writelane_b32 through the LLVM intrinsic (this clang has no __builtin_amdgcn_writelane): the value and the
// lane select are wave-uniform, register allocation and M0 are the compiler's business
extern "C" __device__ int inq_llvm_writelane_i32(int value, int lane, int old) __asm("llvm.amdgcn.writelane.i32");
__device__ __forceinline__ uint32_t writelane_u32(uint32_t old, uint32_t value, int l) {
    return (uint32_t)inq_llvm_writelane_i32((int)value, l, (int)old);
}
__device__ __forceinline__ uint64_t ballot64(bool p) { return __builtin_amdgcn_ballot_w64(p); }

// The sum over the 64 lanes, in every lane
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t x) { return readlane_u32(wave_inclusive_scan_u32(x), kWave - 1); }
__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t x) {
    for (int d = 1; d < kWave; d *= 2) x += __shfl_xor((unsigned long long)x, d, kWave);
    return x;
}

// A launch whose workgroups stride over their tiles: one workgroup per tile up to `cap` of them, the rest by stride
constexpr uint32_t kGridCap = 1u << 16;
inline uint32_t capped_grid(uint64_t tiles, uint32_t cap = kGridCap) { return (uint32_t)(tiles < cap ? tiles : cap); }
// ... of a side kernel: the context option "grid_side" lowers the launcher's own cap (0, the default, leaves it)
inline uint32_t side_grid(uint64_t tiles, uint32_t grid_side, uint32_t cap = kGridCap) {
    return capped_grid(tiles, grid_side && grid_side < cap ? grid_side : cap);
}

}  // namespace inq
