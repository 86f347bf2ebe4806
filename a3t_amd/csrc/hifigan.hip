// hifigan.hip -- HiFi-GAN generator kernels (espnet2/gan_tts/hifigan/hifigan.py:25-221, residual_block.py:17-99) for gfx950,
// fp32 channels-last [B*T][C] tensors.
//
//   a3t_hfg_conv    one residual-unit convolution of the narrow stages (C = 32 / 64) in one launch:
//                       v[t] = bias + sum_{tap,c} W[tap][c][:] * leaky(x[t + (tap - (k-1)/2) * dil][c]) (+ R[t])
//                       y[t] = v[t]  and / or  acc[t] (+)= alpha * v[t]            (acc: the MRF sum / mean of the stage)
//   a3t_hfg_out     tanh(bias + conv_K(leaky(x))), C -> 1
//   a3t_leaky_relu  element-wise, for the layer-by-layer path and the wide stages
//
// a3t_hfg_conv is the implicit-im2col GEMM of wave_conv.h (wave_conv_mainloop: one 256-sample tile and all C output channels
// per workgroup, v_mfma_f32_32x32x2f32, activations and weights double-buffered in LDS) with K = k * C tap-major in chunks of
// 16 = one tap, 16 input channels.  A chunk's activations are read at the tap's shifted rows -- so the halo (k-1)/2 * dil may
// be of any size -- and pass through LeakyReLU on their way into LDS.  LDS: 40 KiB at C = 64 (36 KiB at C = 32); the
// workgroups that share a CU (two at C = 64 by registers) are expected to cover a workgroup's barrier.  Keeping a whole weight
// set resident instead (44 KiB at C = 32, k = 11) would fit, but not at C = 64 (176 KiB at k = 11 > 160 KiB): the weights are
// streamed at both widths, one path.  A streamed weight chunk is 1/8 (C = 32) or 1/4 (C = 64) of the activation chunk's
// bytes and is expected to come from L2.
// The bias, the residual and the MRF accumulation happen on the accumulators.
// Arithmetic per output sample is the same whatever its tile, its row's position in the batch or the other rows: the sum runs
// over k in the same order, and taps outside the row add exact zeros (leaky(0) = 0).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/a3t_hip.h"
#include "wave_conv.h"

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
    constexpr int NJ = C / 32, CPT = C / 16;   // CPT: chunks per tap
    const int tid = threadIdx.x, lane = tid & 63, wm = (tid >> 6) * 64, lr = lane & 31, lk = lane >> 5;
    const WaveTile at = wave_tile<RAGGED>(a.tiles, blockIdx.x, a.tiles_t, a.Tw);
    const int b = at.b, t0 = at.t0, Wb = at.Wb;      // (named: the lambdas below capture them)
    const int half = (a.taps - 1) / 2;
    const int t = t0 + tid;                                  // the row this thread stages
    const float* xb = a.x + (int64_t)b * a.Tw * C;

    f32x16 acc[2][NJ];
    wave_conv_mainloop<C>(
        acc, a.wt, a.taps * CPT,
        [&](int kc) -> const float4* {
            const int tap = kc / CPT, c0 = (kc - tap * CPT) * 16;
            const int64_t ts = (int64_t)t + (int64_t)(tap - half) * a.dil;
            return t < Wb && ts >= 0 && ts < Wb ? (const float4*)(xb + ts * C + c0) : nullptr;
        },
        [&](float v) { return leaky(v, a.slope); });

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

template <int C>
static int hfg_conv_launch(const HfgArgs& a, int ntiles, void* stream) {
    return wave_ragged(a.tiles, [&](auto ragged) {
        hipLaunchKernelGGL((hfg_conv_kernel<C, decltype(ragged)::value>), dim3(ntiles), dim3(256), 0, (hipStream_t)stream, a);
        return (int)hipGetLastError();
    });
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
    return C == 32 ? hfg_conv_launch<32>(a, n, stream) : hfg_conv_launch<64>(a, n, stream);
}

// Output convolution, C -> 1, LeakyReLU in front, tanh behind: wave_out_kernel (wave_conv.h) with zero padding and four
// partial sums over c % 4.
extern "C" int a3t_hfg_out(const float* x, const float* w, const float* bias, float* y, float slope, const int32_t* tiles,
                           int ntiles, int B, int Tw, int C, int K, void* stream) {
    if (!x || !w || !y || C < 4 || C > 64 || (C & 3) || K < 1 || K > 11 || !(K & 1)) return A3T_EINVAL;
    const int n = wave_grid(tiles, ntiles, B, Tw);
    if (n <= 0) return n;
    return wave_out_launch<false, 4, 1>(x, w, bias, y, slope, 1, tiles, n, Tw, C, 1, K, stream);
}

// ---------------------------------------------------------------- element-wise LeakyReLU, 16 bytes per lane
__global__ void leaky_relu_kernel(const float* x, float* y, int64_t n, int64_t nv, float slope) {
    const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = i0; i < nv; i += step) ((float4*)y)[i] = leaky(((const float4*)x)[i], slope);
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
