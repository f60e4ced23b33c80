// wave.h — what one 64-lane wavefront does the same way in every device query (changes / past
// kernels): a sum, an inclusive scan, and the bitmap tile that turns "selected history positions"
// into history order; and the DPP control words of the two merge kernels' own VALU-only scans.
// Device only.  Nothing here holds a barrier: the call sites keep theirs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// DPP lane moves (gfx9 encodings) for __builtin_amdgcn_update_dpp: lanes without a source read 0
#define DPP_ROW_SHR(n) (0x110 + (n))
#define DPP_WAVE_SHR1 0x138
#define DPP_ROW_BCAST15 0x142
#define DPP_ROW_BCAST31 0x143

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (uint32_t d = 32; d; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// inclusive prefix sum over the wave's lanes (lane 63 holds the total)
template <typename T>
__device__ __forceinline__ T wave_incl_scan(T v, uint32_t lane) {
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const T up = __shfl_up(v, d);
        if (lane >= d) v += up;
    }
    return v;
}

// TILE history positions as an LDS bitmap, one 32-bit word per lane, used by one wave:
//   clear | barrier | mark the selected positions of the tile | barrier | rank | barrier | slot
// (position p belongs to tile p / TILE; the caller asks only about positions of the current tile)
template <uint32_t TILE>
struct HistTile {
    static_assert(TILE % 64u == 0u && TILE / 32u <= 64u, "a tile's bitmap words fit one per lane");
    uint32_t bits[64], pre[64];

    __device__ __forceinline__ void clear(uint32_t lane) { bits[lane] = 0u; }
    __device__ __forceinline__ void mark(uint32_t p) { atomicOr(&bits[(p % TILE) >> 5], 1u << (p & 31u)); }
    // popcount prefix over the words; returns the positions marked in the tile
    __device__ __forceinline__ uint32_t rank(uint32_t lane) {
        const uint32_t c1 = (uint32_t)__popc(bits[lane]);
        const uint32_t incl = wave_incl_scan(c1, lane);
        pre[lane] = incl - c1;
        return __shfl(incl, 63);
    }
    // is p marked?  k = the marked positions of the tile below it
    __device__ __forceinline__ bool slot(uint32_t p, uint32_t &k) const {
        const uint32_t b = p % TILE, wd = bits[b >> 5], bit = 1u << (b & 31u);
        k = pre[b >> 5] + (uint32_t)__popc(wd & (bit - 1u));
        return (wd & bit) != 0u;
    }
};
