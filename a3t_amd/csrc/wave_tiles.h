// wave_tiles.h -- the tile contract of the waveform kernels (pwg_fused.hip, pwg_fused_f16.hip, hifigan.hip,
// hifigan_f16.hip, melgan.hip, stylemelgan.hip; wave_conv.h: the fp32 convolution loop and the output convolution that the
// last three share), device and host side, and the small functions that more than one of them uses.
//
// A [B][Tw] batch of samples is cut into tiles of 256.  Dense form (tiles == NULL): the grid is all B * ceil(Tw / 256) tiles and
// every row is Tw samples long.  Ragged form: the grid is a host-built device list, int32 [ntiles][4] = {row b, first sample t0
// (a multiple of 256), valid samples W_b of row b, 0}, one entry per tile with t0 < W_b (0 <= b < B, W_b <= Tw: the caller's to
// guarantee, the kernels trust the list; a3t_amd/vocoder.py::pwg_tile_list builds it).  Row b is computed as if it were alone:
// a tap beyond W_b is zero like one beyond the utterance, and rows behind W_b are neither loaded, computed nor stored.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <type_traits>
#include "../../include/a3t_hip.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

struct WaveTile { int b, t0, Wb; };      // row, first sample, valid samples of the row

__device__ __forceinline__ WaveTile wave_tile_of(int4 e) { return {e.x, e.y, e.z}; }

// Tile idx of the grid: the list's entry (one uniform 16-byte load), or row-major over the dense B x tiles_t tiles.  Index: int
// for a persistent loop's counter, unsigned for blockIdx.x (the division keeps the caller's signedness).
template <bool RAGGED, typename Index>
__device__ __forceinline__ WaveTile wave_tile(const int4* tiles, Index idx, int tiles_t, int Tw) {
    if (RAGGED) return wave_tile_of(tiles[idx]);
    WaveTile w;
    w.b = idx / tiles_t, w.t0 = (idx - w.b * tiles_t) * 256, w.Wb = Tw;
    return w;
}

// Row of register r of a 32 x 32 fp32 MFMA accumulator in the lanes of half lk (= lane >> 5), counted from row0; the column is
// lane & 31.  (row0 is summed in here, left to right: hipcc does not reassociate the sum, and the kernels' address arithmetic was
// measured with row0 in front.)
__device__ __forceinline__ int acc32_row(int r, int lk, int row0 = 0) { return row0 + (r & 3) + 8 * (r >> 2) + 4 * lk; }

// tanh(ya) * sigmoid(yb) with tanh(y) = 1 - 2 / (1 + e^{2y}): two v_exp_f32 + two v_rcp_f32 per output (abs error ~1e-7)
__device__ __forceinline__ float pwg_gate(float ya, float yb) {
    const float th = 1.f - 2.f * __frcp_rn(1.f + __expf(2.f * ya));
    return th * __frcp_rn(1.f + __expf(-yb));
}

__device__ __forceinline__ float leaky(float v, float slope) { return v > 0.f ? v : v * slope; }
__device__ __forceinline__ float4 leaky(float4 v, float slope) {
    return make_float4(leaky(v.x, slope), leaky(v.y, slope), leaky(v.z, slope), leaky(v.w, slope));
}

// h() = round to nearest even to fp16, saturated to +-65504, of eight consecutive values
__device__ __forceinline__ float sat16(float v) { return fminf(fmaxf(v, -65504.f), 65504.f); }
__device__ __forceinline__ f16x8 pack_f16_sat(float4 v0, float4 v1) {
    f16x8 q;
    q[0] = (_Float16)sat16(v0.x), q[1] = (_Float16)sat16(v0.y), q[2] = (_Float16)sat16(v0.z), q[3] = (_Float16)sat16(v0.w);
    q[4] = (_Float16)sat16(v1.x), q[5] = (_Float16)sat16(v1.y), q[6] = (_Float16)sat16(v1.z), q[7] = (_Float16)sat16(v1.w);
    return q;
}

inline int wave_tiles_t(int Tw) { return (int)(((int64_t)Tw + 255) / 256); }

// The grid of an entry point: A3T_EINVAL (< 0) for arguments outside the contract, 0 for an empty list (nothing to launch,
// success), else the number of tiles.
inline int wave_grid(const int32_t* tiles, int ntiles, int B, int Tw) {
    if (B <= 0 || Tw <= 0 || ntiles < 0 || (!tiles && ntiles) || ((uintptr_t)tiles & 15)) return A3T_EINVAL;
    if (tiles) return ntiles;
    const int64_t n = (int64_t)B * wave_tiles_t(Tw);
    return n > INT_MAX ? A3T_EINVAL : (int)n;
}

// The dense / ragged choice of an entry point: f(std::true_type) with a tile list, f(std::false_type) without, for a generic
// lambda that launches kernel<..., decltype(ragged)::value>.
template <typename F>
inline auto wave_ragged(const void* tiles, F&& f) { return tiles ? f(std::true_type{}) : f(std::false_type{}); }

// Dynamic LDS beyond 64 KiB has to be granted per kernel and per device.  Cached like device_cus(): the largest size granted
// to KERNEL so far on each device (a kernel's size may depend on its arguments); the HIP status of a refusal is the caller's
// to return.
template <auto KERNEL>
inline hipError_t wave_lds_opt_in(int bytes) {
    static int granted[64] = {};
    int dev = 0;
    const bool known = hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64;
    if (known && bytes <= granted[dev]) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess && known) granted[dev] = bytes;
    return e;
}
