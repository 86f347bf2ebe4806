// hifigan.hip -- HiFi-GAN generator kernels (espnet2/gan_tts/hifigan/hifigan.py:25-221, residual_block.py:17-99) for gfx950,
// fp32 channels-last [B*T][C] tensors.
//
//   a3t_hfg_conv    one residual-unit convolution of the narrow stages (C = 32 / 64) in one launch:
//                       v[t] = bias + sum_{tap,c} W[tap][c][:] * leaky(x[t + (tap - (k-1)/2) * dil][c]) (+ R[t])
//                       y[t] = v[t]  and / or  acc[t] (+)= alpha * v[t]            (acc: the MRF sum / mean of the stage)
//   a3t_hfg_out     tanh(bias + conv_K(leaky(x))), C -> 1
//   a3t_leaky_relu  element-wise, for the layer-by-layer path and the wide stages
//
// a3t_hfg_conv is an implicit-im2col GEMM on v_mfma_f32_32x32x2f32 (exact fp32 products): a workgroup owns one 256-sample
// tile and all C output channels, K = k * C runs tap-major in chunks of 16 (one tap, 16 input channels).  A chunk's
// activations are read at the tap's shifted rows -- so the halo (k-1)/2 * dil may be of any size: nothing but the 256 x 16
// chunk is ever staged -- pass through LeakyReLU on their way into a k-major LDS slab, and the chunk's 16 x C weights are
// staged beside them.  Both are double-buffered: the loads of chunk s+1 are in flight while the MFMAs of chunk s run.
// LDS budget: 2 x (16 x 260 + 16 x C) floats = 40 KiB at C = 64 (36 KiB at C = 32); the workgroups that share a CU (two at
// C = 64 by registers) are expected to cover a workgroup's barrier.  Keeping a whole weight set resident instead (44 KiB at C = 32, k = 11) would
// fit, but not at C = 64 (176 KiB at k = 11 > 160 KiB): the weights are streamed at both widths, one path.  A streamed
// weight chunk is 1/8 (C = 32) or 1/4 (C = 64) of the activation chunk's bytes and is expected to come from L2.
// The bias, the residual and the MRF accumulation happen on the accumulators.
// Arithmetic per output sample is the same whatever its tile, its row's position in the batch or the other rows: the sum runs
// over k in the same order, and taps outside the row add exact zeros (leaky(0) = 0).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/a3t_hip.h"
#include "wave_tiles.h"

__device__ __forceinline__ float leaky(float v, float slope) { return v > 0.f ? v : v * slope; }

struct HfgArgs {
    const float* x;       // [B*Tw][C] conv input (read through LeakyReLU)
    const float* wt;      // [taps*C][C] k-major: row = tap * C + in channel, column = out channel
    const float* bias;    // [C] or nullptr
    const float* R;       // [B*Tw][C] residual or nullptr (may alias y)
    float* y;             // [B*Tw][C] or nullptr
    float* acc;           // [B*Tw][C] or nullptr
    float slope, alpha;
    int acc_add;          // acc += alpha * v, else acc = alpha * v
    int B, Tw, taps, dil, tiles_t;
    const int4* tiles;    // RAGGED: [ntiles] tile list (wave_tiles.h)
};

// RAGGED: the tile contract of wave_tiles.h, the grid is the host-built list of the tiles that hold valid samples.
template <int C, bool RAGGED>
__global__ __launch_bounds__(256) void hfg_conv_kernel(HfgArgs a) {
    // 4 waves, each 64 samples x C channels: 2 x C/32 accumulator blocks, every A value feeds C/32 MFMAs, every B value two
    constexpr int BK = 16, TILE = 256, LD = TILE + 4, NJ = C / 32, CPT = C / BK;   // CPT: chunks per tap
    __shared__ __attribute__((aligned(16))) float As[2][BK][LD];
    __shared__ __attribute__((aligned(16))) float Ws[2][BK * C];

    const int tid = threadIdx.x, lane = tid & 63, wm = (tid >> 6) * 64, lr = lane & 31, lk = lane >> 5;
    const WaveTile at = wave_tile<RAGGED>(a.tiles, blockIdx.x, a.tiles_t, a.Tw);
    const int b = at.b, t0 = at.t0, Wb = at.Wb;      // (named: the lambdas below capture them)
    const int nch = a.taps * CPT, half = (a.taps - 1) / 2;
    const int t = t0 + tid;                                  // the row this thread stages
    const float* xb = a.x + (int64_t)b * a.Tw * C;

    float4 P[4], Q;
    auto load_chunk = [&](int kc) {
        const int tap = kc / CPT, c0 = (kc - tap * CPT) * BK;
        const int64_t ts = (int64_t)t + (int64_t)(tap - half) * a.dil;
        if (t < Wb && ts >= 0 && ts < Wb) {
            const float4* s = (const float4*)(xb + ts * C + c0);
#pragma unroll
            for (int i = 0; i < 4; ++i) P[i] = s[i];
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) P[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        if (tid < 4 * C) Q = ((const float4*)(a.wt + (int64_t)kc * BK * C))[tid];
    };
    auto store_chunk = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            As[buf][4 * i + 0][tid] = leaky(P[i].x, a.slope);
            As[buf][4 * i + 1][tid] = leaky(P[i].y, a.slope);
            As[buf][4 * i + 2][tid] = leaky(P[i].z, a.slope);
            As[buf][4 * i + 3][tid] = leaky(P[i].w, a.slope);
        }
        if (tid < 4 * C) ((float4*)Ws[buf])[tid] = Q;
    };

    f32x16 acc[2][NJ];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    load_chunk(0);
    store_chunk(0);
    __syncthreads();
    int buf = 0;
    for (int kc = 0; kc < nch; ++kc) {
        const bool more = kc + 1 < nch;
        if (more) load_chunk(kc + 1);
#pragma unroll
        for (int kk = 0; kk < BK / 2; ++kk) {
            const int k = kk * 2 + lk;
            const float a0 = As[buf][k][wm + lr], a1 = As[buf][k][wm + 32 + lr];
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const float bj = Ws[buf][k * C + j * 32 + lr];
                acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bj, acc[0][j], 0, 0, 0);
                acc[1][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bj, acc[1][j], 0, 0, 0);
            }
        }
        // the other buffer was last read before the barrier that ended the previous chunk
        if (more) store_chunk(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }

    // bias / residual / store / MRF accumulation straight from the accumulators
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int col = j * 32 + lr;
        const float bj = a.bias ? a.bias[col] : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int tt = acc32_row(r, lk, t0 + wm + i * 32);
                if (tt >= Wb) continue;
                const int64_t idx = ((int64_t)b * a.Tw + tt) * C + col;
                float v = acc[i][j][r] + bj;
                if (a.R) v += a.R[idx];
                if (a.y) a.y[idx] = v;
                if (a.acc) a.acc[idx] = a.acc_add ? a.acc[idx] + a.alpha * v : a.alpha * v;
            }
    }
}

template <int C, bool RAGGED>
static int hfg_conv_launch(const HfgArgs& a, int ntiles, void* stream) {
    hipLaunchKernelGGL((hfg_conv_kernel<C, RAGGED>), dim3(ntiles), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

extern "C" int a3t_hfg_conv(const float* x, const float* wt, const float* bias, const float* R, float* y, float* acc,
                            float alpha, int acc_add, float slope, const int32_t* tiles, int ntiles, int B, int Tw, int C,
                            int taps, int dil, void* stream) {
    if (!x || !wt || (!y && !acc) || (C != 32 && C != 64) || taps < 1 || taps > 11 || !(taps & 1) || dil < 1) return A3T_EINVAL;
    if (x == y || x == acc || (y && y == acc)) return A3T_EINVAL;      // other tiles read x[t +- halo]
    if (((uintptr_t)x | (uintptr_t)wt) & 15) return A3T_EINVAL;
    const int n = wave_grid(tiles, ntiles, B, Tw);
    if (n <= 0) return n;
    HfgArgs a;
    a.x = x, a.wt = wt, a.bias = bias, a.R = R, a.y = y, a.acc = acc, a.slope = slope, a.alpha = alpha, a.acc_add = acc_add;
    a.B = B, a.Tw = Tw, a.taps = taps, a.dil = dil, a.tiles_t = wave_tiles_t(Tw), a.tiles = (const int4*)tiles;
    if (tiles) return C == 32 ? hfg_conv_launch<32, true>(a, n, stream) : hfg_conv_launch<64, true>(a, n, stream);
    return C == 32 ? hfg_conv_launch<32, false>(a, n, stream) : hfg_conv_launch<64, false>(a, n, stream);
}

// ---------------------------------------------------------------- output convolution: C -> 1, LeakyReLU in front, tanh behind
// One workgroup per 256-sample tile: the tile's rows with their (K-1)/2 halo pass through LeakyReLU into LDS (row stride C + 1:
// thread t reads row t + tap, an odd stride keeps the 32 lanes of a group on 32 banks), one output sample per thread, four
// partial sums over c % 4.
template <bool RAGGED>
__global__ __launch_bounds__(256) void hfg_out_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                      const float* __restrict__ bias, float* __restrict__ y, float slope, int C,
                                                      int K, int Tw, int tiles_t, const int4* __restrict__ tiles) {
    constexpr int TILE = 256;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int rows = TILE + K - 1, ld = C + 1, half = (K - 1) / 2;
    float* Xs = lds;                   // [rows][C + 1]
    float* Wk = lds + rows * ld;       // [K][C]
    const int tid = threadIdx.x;
    const auto [b, t0, Wb] = wave_tile<RAGGED>(tiles, blockIdx.x, tiles_t, Tw);
    const float* xb = x + (int64_t)b * Tw * C;
    for (int i = tid; i < rows * C; i += 256) {
        const int r = i / C, c = i - r * C, ts = t0 - half + r;
        Xs[r * ld + c] = (ts >= 0 && ts < Wb) ? leaky(xb[(int64_t)ts * C + c], slope) : 0.f;
    }
    for (int i = tid; i < K * C; i += 256) Wk[i] = w[i];
    __syncthreads();
    const int t = t0 + tid;
    if (t >= Wb) return;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    for (int tap = 0; tap < K; ++tap) {
        const float* xr = Xs + (tid + tap) * ld;
        const float* wr = Wk + tap * C;
        for (int c = 0; c < C; c += 4) {
            s0 = fmaf(xr[c], wr[c], s0);
            s1 = fmaf(xr[c + 1], wr[c + 1], s1);
            s2 = fmaf(xr[c + 2], wr[c + 2], s2);
            s3 = fmaf(xr[c + 3], wr[c + 3], s3);
        }
    }
    y[(int64_t)b * Tw + t] = tanhf((s0 + s1) + (s2 + s3) + (bias ? bias[0] : 0.f));
}

extern "C" int a3t_hfg_out(const float* x, const float* w, const float* bias, float* y, float slope, const int32_t* tiles,
                           int ntiles, int B, int Tw, int C, int K, void* stream) {
    if (!x || !w || !y || C < 4 || C > 64 || (C & 3) || K < 1 || K > 11 || !(K & 1)) return A3T_EINVAL;
    const int n = wave_grid(tiles, ntiles, B, Tw);
    if (n <= 0) return n;
    const int lds = ((256 + K - 1) * (C + 1) + K * C) * 4, tiles_t = wave_tiles_t(Tw);      // more than 64 KiB at C = 64
    const hipError_t e = tiles ? wave_lds_opt_in<hfg_out_kernel<true>>(lds) : wave_lds_opt_in<hfg_out_kernel<false>>(lds);
    if (e != hipSuccess) return (int)e;
    if (tiles)
        hipLaunchKernelGGL(hfg_out_kernel<true>, dim3(n), dim3(256), lds, (hipStream_t)stream, x, w, bias, y, slope, C, K, Tw,
                           tiles_t, (const int4*)tiles);
    else
        hipLaunchKernelGGL(hfg_out_kernel<false>, dim3(n), dim3(256), lds, (hipStream_t)stream, x, w, bias, y, slope, C, K, Tw,
                           tiles_t, (const int4*)nullptr);
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------- element-wise LeakyReLU, 16 bytes per lane
__global__ void leaky_relu_kernel(const float* x, float* y, int64_t n, int64_t nv, float slope) {
    const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = i0; i < nv; i += step) {
        float4 v = ((const float4*)x)[i];
        v.x = leaky(v.x, slope), v.y = leaky(v.y, slope), v.z = leaky(v.z, slope), v.w = leaky(v.w, slope);
        ((float4*)y)[i] = v;
    }
    for (int64_t i = nv * 4 + i0; i < n; i += step) y[i] = leaky(x[i], slope);      // the tail, or all of it when unaligned
}

extern "C" int a3t_leaky_relu(const float* x, float* y, int64_t n, float slope, void* stream) {
    if (n < 0 || (n && (!x || !y))) return A3T_EINVAL;
    if (!n) return 0;
    const int64_t nv = (((uintptr_t)x | (uintptr_t)y) & 15) ? 0 : n / 4;
    int64_t blocks = ((nv ? nv : n) + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(leaky_relu_kernel, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream, x, y, n, nv, slope);
    return (int)hipGetLastError();
}
