// stylemelgan.hip -- StyleMelGAN generator kernels (espnet2/gan_tts/style_melgan/style_melgan.py:28-232,
// tade_res_block.py:15-185) for gfx950, fp32 channels-last [B*T][C] tensors on the tile contract of wave_tiles.h.
//
//   a3t_smg_conv    one convolution of a TADEResBlock in one launch, three epilogues on the accumulators:
//                       v[t] = bias + sum_{tap,c} W[tap][c][:] * x[(t + (tap - (k-1)/2) * dil) / up][c]
//                       PLAIN  y[t][c] = v[t][c]                                                              (Cout = 64)
//                       TADE   y[t][c] = v[t][c] * ((m[t / ux][c] - mean[b][c]) * rstd[b][c]) + v[t][64 + c]  (Cout = 128)
//                       GATE   y[t][c] = g(v[t][:64])[c] * tanh(v[t][64 + c]) (+ R[t / ur][c])                (Cout = 128)
//                   g = softmax over the 64 channels (maximum subtracted) or sigmoid.
//   a3t_smg_stats   mean and rstd = 1 / sqrt(var + eps) of every (row, channel) over the row's own W_b samples (InstanceNorm1d:
//                   biased variance), C = 64.
//
// a3t_smg_conv is the implicit-im2col GEMM of wave_conv.h (wave_conv_mainloop), as hfg_conv_kernel (hifigan.hip): one
// 256-sample tile and all Cout columns per workgroup, K = taps * Cin tap-major in chunks of 16, the activations staged as they
// are.  48.5 KiB of LDS at Cout = 128, 128 accumulator registers per wave; two workgroups share a CU (186 registers, no
// scratch; three at Cout = 64).
// Nearest-neighbour upsampling is an index map: the input holds ceil(Tw / up) rows per batch row and a tap at ts in [0, W_b)
// reads row ts / up; m and R likewise with ux and ur.  Samples sit on the accumulator's rows and channels on its 32 columns =
// the 32 lanes of a half wave, so column c (block j) and column 64 + c (block j + 2) are registers of the same lane -- the two
// halves of TADE and GATE pair without a permutation -- and the softmax's maximum and sum over the 64 channels are a butterfly
// over the 32 lanes of a half (5 x __shfl_xor, masks 1 .. 16) on top of the lane's own two columns.  A butterfly adds in the
// same order in every lane, whatever the tile, the row's place in the batch or the other rows.
//
// a3t_smg_stats is two launches.  The first gives every tile its (mean, M2 = sum (x - mean)^2) per channel, two passes over
// registers: 4 groups of 64 threads hold 64 rows each, group sums are added in group order.  The second merges a row's tiles
// with Chan's update (n, mean, M2) in a fixed order that depends on the row's number of tiles alone: 16 contiguous segments of
// tiles, each merged in tile order by one group of 64 threads, then the 16 segments in order.  No atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/a3t_hip.h"
#include "wave_conv.h"

enum { SMG_PLAIN = 0, SMG_TADE = 1, SMG_GATE = 2 };

struct SmgArgs {
    const float* x;       // [B * ceil(Tw / up)][Cin] conv input
    const float* wt;      // [taps*Cin][N] k-major: row = tap * Cin + in channel, column = out channel
    const float* bias;    // [N] or nullptr
    const float* m;       // TADE: [B * ceil(Tw / ux)][64] the tensor that is normalised and modulated
    const float* stats;   // TADE: [B][2][64] mean | rstd (a3t_smg_stats)
    const float* R;       // GATE: [B * ceil(Tw / ur)][64] residual or nullptr
    float* y;             // [B*Tw][64]
    int B, Tw, Cin, taps, dil, up, ux, ur, sigmoid, tiles_t;
    const int4* tiles;    // RAGGED: [ntiles] tile list (wave_tiles.h)
};

__device__ __forceinline__ float half_max(float v) {
#pragma unroll
    for (int m = 1; m < 32; m <<= 1) v = fmaxf(v, __shfl_xor(v, m));
    return v;
}
__device__ __forceinline__ float half_sum(float v) {
#pragma unroll
    for (int m = 1; m < 32; m <<= 1) v += __shfl_xor(v, m);
    return v;
}

template <int N, int MODE, bool RAGGED>
__global__ __launch_bounds__(256, 2) void smg_conv_kernel(SmgArgs a) {
    constexpr int NJ = N / 32;
    const int tid = threadIdx.x, lane = tid & 63, wm = (tid >> 6) * 64, lr = lane & 31, lk = lane >> 5;
    const WaveTile at = wave_tile<RAGGED>(a.tiles, blockIdx.x, a.tiles_t, a.Tw);
    const int b = at.b, t0 = at.t0, Wb = at.Wb;
    const int Cin = a.Cin, CPT = Cin / 16, half = (a.taps - 1) / 2;      // CPT: chunks per tap
    const int t = t0 + tid;                                  // the row this thread stages
    const float* xb = a.x + (int64_t)b * ((a.Tw + a.up - 1) / a.up) * Cin;

    f32x16 acc[2][NJ];
    wave_conv_mainloop<N>(
        acc, a.wt, a.taps * CPT,
        [&](int kc) -> const float4* {
            const int tap = kc / CPT, c0 = (kc - tap * CPT) * 16;
            const int64_t ts = (int64_t)t + (int64_t)(tap - half) * a.dil;
            return t < Wb && ts >= 0 && ts < Wb ? (const float4*)(xb + (ts / a.up) * Cin + c0) : nullptr;
        },
        [](float v) { return v; });

    float bj[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) bj[j] = a.bias ? a.bias[j * 32 + lr] : 0.f;

    if constexpr (MODE == SMG_PLAIN) {
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int tt = acc32_row(r, lk, t0 + wm + i * 32);
                    if (tt < Wb) a.y[((int64_t)b * a.Tw + tt) * N + j * 32 + lr] = acc[i][j][r] + bj[j];
                }
    }
    if constexpr (MODE == SMG_TADE) {       // columns j*32 + lr (scale) and 64 + j*32 + lr (shift) of the same lane
        const float* mb = a.m + (int64_t)b * ((a.Tw + a.ux - 1) / a.ux) * 64;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = j * 32 + lr;
            const float mean = a.stats[(int64_t)b * 128 + col], rstd = a.stats[(int64_t)b * 128 + 64 + col];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int tt = acc32_row(r, lk, t0 + wm + i * 32);
                    if (tt >= Wb) continue;
                    const float xn = (mb[(int64_t)(tt / a.ux) * 64 + col] - mean) * rstd;
                    a.y[((int64_t)b * a.Tw + tt) * 64 + col] = (acc[i][j][r] + bj[j]) * xn + (acc[i][j + 2][r] + bj[j + 2]);
                }
        }
    }
    if constexpr (MODE == SMG_GATE) {
        const float* Rb = a.R ? a.R + (int64_t)b * ((a.Tw + a.ur - 1) / a.ur) * 64 : nullptr;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {      // one sample: its 64 gate channels are two registers in each of 32 lanes
                const int tt = acc32_row(r, lk, t0 + wm + i * 32);
                const float v0 = acc[i][0][r] + bj[0], v1 = acc[i][1][r] + bj[1];
                float g0, g1;
                if (a.sigmoid) {
                    g0 = 1.f / (1.f + expf(-v0)), g1 = 1.f / (1.f + expf(-v1));
                } else {      // (every lane takes part in the butterflies, also for rows behind W_b: their v is the bias)
                    const float mx = half_max(fmaxf(v0, v1));
                    const float e0 = expf(v0 - mx), e1 = expf(v1 - mx);
                    const float s = half_sum(e0 + e1);
                    g0 = e0 / s, g1 = e1 / s;
                }
                if (tt >= Wb) continue;
                float y0 = g0 * tanhf(acc[i][2][r] + bj[2]), y1 = g1 * tanhf(acc[i][3][r] + bj[3]);
                if (Rb) {
                    const float* rr = Rb + (int64_t)(tt / a.ur) * 64;
                    y0 += rr[lr], y1 += rr[32 + lr];
                }
                float* yr = a.y + ((int64_t)b * a.Tw + tt) * 64;
                yr[lr] = y0, yr[32 + lr] = y1;
            }
    }
}

template <int N, int MODE>
static int smg_conv_launch(const SmgArgs& a, int ntiles, void* stream) {
    return wave_ragged(a.tiles, [&](auto ragged) {
        hipLaunchKernelGGL((smg_conv_kernel<N, MODE, decltype(ragged)::value>), dim3(ntiles), dim3(256), 0, (hipStream_t)stream, a);
        return (int)hipGetLastError();
    });
}

extern "C" int a3t_smg_conv(const float* x, const float* wt, const float* bias, const float* m, const float* stats,
                            const float* R, float* y, int mode, int sigmoid, const int32_t* tiles, int ntiles, int B, int Tw,
                            int Cin, int Cout, int taps, int dil, int up, int ux, int ur, void* stream) {
    if (!x || !wt || !y || Cin < 16 || (Cin & 15) || taps < 1 || taps > 9 || !(taps & 1) || dil < 1 || up < 1 || ux < 1 || ur < 1)
        return A3T_EINVAL;
    if (mode == SMG_PLAIN ? Cout != 64 : Cout != 128) return A3T_EINVAL;
    if (mode != SMG_PLAIN && mode != SMG_TADE && mode != SMG_GATE) return A3T_EINVAL;
    if (mode == SMG_TADE && (!m || !stats)) return A3T_EINVAL;
    if (x == y || (mode == SMG_TADE && m == y)) return A3T_EINVAL;      // other tiles read x[t +- halo] and m[t / ux]
    if (((uintptr_t)x | (uintptr_t)wt) & 15) return A3T_EINVAL;
    const int n = wave_grid(tiles, ntiles, B, Tw);
    if (n <= 0) return n;
    SmgArgs a;
    a.x = x, a.wt = wt, a.bias = bias, a.m = m, a.stats = stats, a.R = mode == SMG_GATE ? R : nullptr, a.y = y;
    a.B = B, a.Tw = Tw, a.Cin = Cin, a.taps = taps, a.dil = dil, a.up = up, a.ux = ux, a.ur = ur, a.sigmoid = sigmoid;
    a.tiles_t = wave_tiles_t(Tw), a.tiles = (const int4*)tiles;
    if (mode == SMG_PLAIN) return smg_conv_launch<64, SMG_PLAIN>(a, n, stream);
    if (mode == SMG_TADE) return smg_conv_launch<128, SMG_TADE>(a, n, stream);
    return smg_conv_launch<128, SMG_GATE>(a, n, stream);
}

// ------------------------------------------------------------------------------------------ InstanceNorm statistics, C = 64
// part [ntiles][2][64]: mean | M2 of the tile's min(256, W_b - t0) valid rows.
template <bool RAGGED>
__global__ __launch_bounds__(256) void smg_stats_tile_kernel(const float* __restrict__ x, float* __restrict__ part, int Tw,
                                                            int tiles_t, const int4* __restrict__ tiles) {
    __shared__ float red[4][64];
    const int tid = threadIdx.x, c = tid & 63, q = tid >> 6;
    const auto [b, t0, Wb] = wave_tile<RAGGED>(tiles, blockIdx.x, tiles_t, Tw);
    const int n = min(256, Wb - t0);
    const float* xb = x + ((int64_t)b * Tw + t0) * 64 + c;
    float v[64], s = 0.f;
#pragma unroll
    for (int i = 0; i < 64; ++i) {      // rows q, q + 4, ...: a group of 64 threads reads one 256-byte row at a time
        const int r = q + 4 * i;
        v[i] = r < n ? xb[(int64_t)r * 64] : 0.f;
        s += v[i];
    }
    red[q][c] = s;
    __syncthreads();
    const float mean = (((red[0][c] + red[1][c]) + red[2][c]) + red[3][c]) / (float)n;
    __syncthreads();
    // (the valid rows counted, not "q + 4 i < n" again: the compiler keeps the first loop's 64 lane masks for a second use and
    // spills SGPRs)
    const int cnt = (n - q + 3) >> 2;
    float m2 = 0.f;
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        const float d = i < cnt ? v[i] - mean : 0.f;
        m2 += d * d;
    }
    red[q][c] = m2;
    __syncthreads();
    if (q == 0) {
        part[(int64_t)blockIdx.x * 128 + c] = mean;
        part[(int64_t)blockIdx.x * 128 + 64 + c] = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
    }
}

struct SmgMoments { float n, mean, m2; };

// Chan's update: b appended to a (either may be empty)
__device__ __forceinline__ SmgMoments smg_merge(SmgMoments a, SmgMoments b) {
    if (b.n == 0.f) return a;
    if (a.n == 0.f) return b;
    SmgMoments o;
    const float d = b.mean - a.mean;
    o.n = a.n + b.n;
    o.mean = a.mean + d * (b.n / o.n);
    o.m2 = (a.m2 + b.m2) + (d * d) * (a.n * (b.n / o.n));
    return o;
}

// One workgroup per row: stats [B][2][64] = mean | rstd.  A row without a tile (W_b = 0) gets mean 0, rstd 0.
template <bool RAGGED>
__global__ __launch_bounds__(1024) void smg_stats_merge_kernel(const float* __restrict__ part, float* __restrict__ stats, int Tw,
                                                              int tiles_t, const int4* __restrict__ tiles, int ntiles, float eps) {
    __shared__ SmgMoments seg[16][64];
    const int tid = threadIdx.x, c = tid & 63, q = tid >> 6, b = blockIdx.x;
    int first, cnt, Wb;
    if (RAGGED) {      // the list is sorted by row: the first entry of row >= b and of row >= b + 1
        int lo = 0, hi = ntiles;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (tiles[mid].x < b) lo = mid + 1; else hi = mid; }
        first = lo, hi = ntiles;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (tiles[mid].x <= b) lo = mid + 1; else hi = mid; }
        cnt = lo - first;
        Wb = cnt ? tiles[first].z : 0;
    } else {
        first = b * tiles_t, cnt = tiles_t, Wb = Tw;
    }
    const int per = (cnt + 15) / 16, i0 = min(cnt, q * per), i1 = min(cnt, i0 + per);
    SmgMoments acc = {0.f, 0.f, 0.f};
    for (int i = i0; i < i1; ++i) {
        const float* p = part + (int64_t)(first + i) * 128;
        acc = smg_merge(acc, SmgMoments{(float)min(256, Wb - i * 256), p[c], p[64 + c]});
    }
    seg[q][c] = acc;
    __syncthreads();
    if (q) return;
    for (int s = 1; s < 16; ++s) acc = smg_merge(acc, seg[s][c]);
    stats[(int64_t)b * 128 + c] = acc.mean;
    stats[(int64_t)b * 128 + 64 + c] = acc.n > 0.f ? 1.f / sqrtf(acc.m2 / acc.n + eps) : 0.f;
}

extern "C" int a3t_smg_stats(const float* x, float* part, float* stats, float eps, const int32_t* tiles, int ntiles, int B,
                             int Tw, int C, void* stream) {
    if (!x || !part || !stats || C != 64 || !(eps >= 0.f)) return A3T_EINVAL;
    const int n = wave_grid(tiles, ntiles, B, Tw);
    if (n < 0) return n;
    const int tiles_t = wave_tiles_t(Tw);
    if (n)
        wave_ragged(tiles, [&](auto ragged) {
            constexpr bool R = decltype(ragged)::value;
            hipLaunchKernelGGL(smg_stats_tile_kernel<R>, dim3(n), dim3(256), 0, (hipStream_t)stream, x, part, Tw, tiles_t,
                               (const int4*)tiles);
            hipLaunchKernelGGL(smg_stats_merge_kernel<R>, dim3(B), dim3(1024), 0, (hipStream_t)stream, part, stats, Tw, tiles_t,
                               (const int4*)tiles, n, eps);
        });
    return (int)hipGetLastError();
}
