// wave_conv.h -- what the fp32 convolution kernels of the waveform generators share (hifigan.hip, melgan.hip, stylemelgan.hip):
// the implicit-im2col main loop of hfg_conv_kernel / smg_conv_kernel and the output convolution C -> 1..4 of both families.
#pragma once
#include "wave_tiles.h"

// ReflectionPad1d's index for a row of W samples, clamped so that an index outside the contract (|ts| beyond one reflection)
// still stays inside the row
__device__ __forceinline__ int64_t refl(int64_t ts, int64_t W) {
    if (ts < 0) ts = -ts;
    if (ts >= W) ts = 2 * (W - 1) - ts;
    return ts < 0 ? 0 : (ts >= W ? W - 1 : ts);
}

// ---------------------------------------------------------------- main loop: acc [256 samples][N] = act(X) [256][16 nch] . wt
// An implicit-im2col GEMM on v_mfma_f32_32x32x2f32 (exact fp32 products).  A workgroup of 4 waves owns one 256-sample tile and
// all N output columns, a wave 64 samples: 2 x N/32 accumulator blocks, every A value feeds N/32 MFMAs, every B value two.
// K runs in nch chunks of 16.  Thread tid stages sample tid of the tile: src(kc) is where its 16 consecutive values of chunk kc
// lie (16-byte aligned; nullptr: zeros -- so a tap may read any row, nothing but the 256 x 16 chunk is ever staged), they pass
// through act on their way into a k-major LDS slab, and the chunk's 16 x N weights (wt [16 nch][N] k-major, 16-byte aligned)
// are staged beside them.  Both are double-buffered: the loads of chunk s+1 are in flight while the MFMAs of chunk s run, one
// barrier per chunk.  LDS: 2 x (16 x 260 + 16 x N) floats = 36 / 40 / 48.5 KiB at N = 32 / 64 / 128.
// The prefetch is unconditional: the last iteration loads its own chunk again and drops it.  Conditionally written prefetch
// registers go to scratch in smg_conv_kernel, and in hfg_conv_kernel the compiler copies them behind the loads (a vmcnt wait
// in front of the MFMAs: no prefetch at all) or splits the loads around a branch (the C = 32 stage 4 % slower); the repeated
// load was measured within the noise of both.  Keep the load one `if (s) ... else ...` over all four registers.
// The accumulators are zeroed here and left to the caller's epilogue: register r of acc[i][j] is sample
// acc32_row(r, lk, wm + 32 i) of the tile, column 32 j + lr (wm = 64 * wave, lr = lane & 31, lk = lane >> 5).
template <int N, typename Src, typename Act>
__device__ __forceinline__ void wave_conv_mainloop(f32x16 (&acc)[2][N / 32], const float* wt, int nch, Src src, Act act) {
    constexpr int BK = 16, TILE = 256, LD = TILE + 4, NJ = N / 32, WV = (4 * N + 255) / 256;   // WV: weight float4 per thread
    __shared__ __attribute__((aligned(16))) float As[2][BK][LD];
    __shared__ __attribute__((aligned(16))) float Ws[2][BK * N];
    const int tid = threadIdx.x, lane = tid & 63, wm = (tid >> 6) * 64, lr = lane & 31, lk = lane >> 5;

    float4 P[4], Q[WV];
    auto mine = [&](int i) { return 256 * (i + 1) <= 4 * N || tid + 256 * i < 4 * N; };      // (false only at N = 32)
    auto load_chunk = [&](int kc) {
        const float4* s = src(kc);
        if (s) {
#pragma unroll
            for (int i = 0; i < 4; ++i) P[i] = s[i];
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) P[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        const float4* wsrc = (const float4*)(wt + (int64_t)kc * BK * N);
#pragma unroll
        for (int i = 0; i < WV; ++i)
            if (mine(i)) Q[i] = wsrc[tid + 256 * i];
    };
    auto store_chunk = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            As[buf][4 * i + 0][tid] = act(P[i].x);
            As[buf][4 * i + 1][tid] = act(P[i].y);
            As[buf][4 * i + 2][tid] = act(P[i].z);
            As[buf][4 * i + 3][tid] = act(P[i].w);
        }
#pragma unroll
        for (int i = 0; i < WV; ++i)
            if (mine(i)) ((float4*)Ws[buf])[tid + 256 * i] = Q[i];
    };

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
        load_chunk(more ? kc + 1 : kc);
#pragma unroll
        for (int kk = 0; kk < BK / 2; ++kk) {
            const int k = kk * 2 + lk;
            const float a0 = As[buf][k][wm + lr], a1 = As[buf][k][wm + 32 + lr];
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const float bj = Ws[buf][k * N + j * 32 + lr];
                acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bj, acc[0][j], 0, 0, 0);
                acc[1][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bj, acc[1][j], 0, 0, 0);
            }
        }
        // the other buffer was last read before the barrier that ended the previous chunk
        if (more) store_chunk(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }
}

// ---------------------------------------------------------------- output convolution: C -> O <= OMAX, LeakyReLU in front
// y[t][o] = act(bias[o] + conv_K(leaky(x))[o]), act = tanh or nothing.  One workgroup per 256-sample tile: the tile's rows with
// their (K-1)/2 halo pass through LeakyReLU into LDS (row stride C + 1: thread t reads row t + tap, an odd stride keeps the 32
// lanes of a group on 32 banks), one output sample per thread.  A tap outside the row's own [0, W_b) is zero, or with REFLECT
// the row's reflected sample (the caller guarantees (K-1)/2 < W_b).  NS partial sums per output channel over c % NS, added as
// s0 + s1 (NS = 2) or (s0 + s1) + (s2 + s3) (NS = 4); C is a multiple of NS.  w: [O][K][C].
template <bool RAGGED, bool REFLECT, int NS, int OMAX>
__global__ __launch_bounds__(256) void wave_out_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                       const float* __restrict__ bias, float* __restrict__ y, float slope, int C,
                                                       int O, int K, int act_tanh, int Tw, int tiles_t,
                                                       const int4* __restrict__ tiles) {
    static_assert(NS == 2 || NS == 4, "the two summation orders of the entry points");
    constexpr int TILE = 256;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int rows = TILE + K - 1, ld = C + 1, half = (K - 1) / 2;
    float* Xs = lds;                   // [rows][C + 1]
    float* Wk = lds + rows * ld;       // [O][K][C]
    const int tid = threadIdx.x;
    const auto [b, t0, Wb] = wave_tile<RAGGED>(tiles, blockIdx.x, tiles_t, Tw);
    const float* xb = x + (int64_t)b * Tw * C;
    for (int i = tid; i < rows * C; i += 256) {
        const int r = i / C, c = i - r * C;
        const int64_t ts = (int64_t)t0 - half + r;
        if (REFLECT) Xs[r * ld + c] = leaky(xb[refl(ts, Wb) * C + c], slope);
        else Xs[r * ld + c] = (ts >= 0 && ts < Wb) ? leaky(xb[ts * C + c], slope) : 0.f;
    }
    for (int i = tid; i < O * K * C; i += 256) Wk[i] = w[i];
    __syncthreads();
    const int t = t0 + tid;
    if (t >= Wb) return;
    float s[OMAX][NS] = {};
    for (int tap = 0; tap < K; ++tap) {
        const float* xr = Xs + (tid + tap) * ld;
        for (int c = 0; c < C; c += NS)
#pragma unroll
            for (int o = 0; o < OMAX; ++o)
                if (OMAX == 1 || o < O) {
                    const float* wr = Wk + (o * K + tap) * C + c;
#pragma unroll
                    for (int i = 0; i < NS; ++i) s[o][i] = fmaf(xr[c + i], wr[i], s[o][i]);
                }
    }
#pragma unroll
    for (int o = 0; o < OMAX; ++o)
        if (OMAX == 1 || o < O) {
            float sum = s[o][0] + s[o][1];
            if constexpr (NS == 4) sum += s[o][2] + s[o][3];
            const float v = sum + (bias ? bias[o] : 0.f);
            y[((int64_t)b * Tw + t) * O + o] = act_tanh ? tanhf(v) : v;
        }
}

// The launch behind a3t_hfg_out and a3t_mgan_out (arguments checked there; n = wave_grid() > 0).
template <bool REFLECT, int NS, int OMAX>
inline int wave_out_launch(const float* x, const float* w, const float* bias, float* y, float slope, int act_tanh,
                           const int32_t* tiles, int n, int Tw, int C, int O, int K, void* stream) {
    const int lds = ((256 + K - 1) * (C + 1) + O * K * C) * 4;      // more than 64 KiB at C = 64
    return wave_ragged(tiles, [&](auto ragged) {
        constexpr auto kernel = wave_out_kernel<decltype(ragged)::value, REFLECT, NS, OMAX>;
        const hipError_t e = wave_lds_opt_in<kernel>(lds);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(kernel, dim3(n), dim3(256), lds, (hipStream_t)stream, x, w, bias, y, slope, C, O, K, act_tanh, Tw,
                           wave_tiles_t(Tw), (const int4*)tiles);
        return (int)hipGetLastError();
    });
}
