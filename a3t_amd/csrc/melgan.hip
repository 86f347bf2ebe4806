// melgan.hip -- MelGAN / multi-band MelGAN generator kernels (espnet2/gan_tts/melgan/melgan.py:22-199, residual_stack.py:16-71,
// pqmf.py:56-160) for gfx950, fp32 channels-last [B*T][C] tensors on the tile contract of wave_tiles.h.
//
//   a3t_mgan_stack        one ResidualStack in one launch:
//                             h[t] = leaky(b1 + sum_{tap,c} W1[tap][c][:] * leaky(x[refl(t + (tap - 1) * dil)][c]))
//                             y[t] = (bs + b2) + Ws x[t] + W2 h[t]
//   a3t_mgan_out          y[t][o] = act(bias[o] + conv_K(leaky(x))[o]) with reflection, C -> 1..4 channels
//   a3t_pqmf_synthesis    the PQMF synthesis filter bank, S sub-bands [B*Ts][S] -> [B*Ts*S] samples
//   a3t_reflect_pad_rows  x [B][T][C] -> y [B][T + 2 pad][C] (+ _ragged), for the layer-by-layer path
//
// Reflection (torch.nn.ReflectionPad1d) is an index map on the tap's row: refl(ts) = -ts for ts < 0, 2 (W - 1) - ts for ts >= W,
// with W the row's OWN length at the layer's rate, so a ragged row is the row run alone.
//
// a3t_mgan_stack computes the transposed products on v_mfma_f32_32x32x2f32 (exact fp32 products): M = output channels (the
// weights are the A operand), N = samples.  A workgroup owns 128 samples (half a tile of the contract, grid = 2 x tiles), a wave 32
// of them and ALL channels, so the wave that holds h[:, its 32 samples] in its accumulators is the wave that needs it as the B
// operand of the second product -- and the accumulator layout IS a B layout: register r of block j holds, in lane (n, lk), channel
// 32 j + (r & 3) + 8 (r >> 2) + 4 lk of sample n, i.e. the two k of one MFMA step in the two lane halves.  The packer orders the rows
// of W2 to match, and h never leaves the registers: no LDS, no HBM.  K runs in chunks of 16 through one double-buffered stream
// of 3 C/16 chunks of the dilated convolution (activations staged k-major through LeakyReLU, as in hifigan.hip, read at the tap's
// reflected rows: the halo is free), C/16 chunks of the skip product (x as it is) and Cp/16 chunks of W2 (weights only).
// C = 48 runs with Cp = 64 output columns whose weights and biases are zero (leaky(0) = 0 feeds zero rows of W2).
// LDS: 2 x (16 x 132 + 16 x Cp) floats = 41 KiB at C = 192.  Registers: 2 x Cp/32 accumulator blocks = 192 at C = 192.
// A sample's arithmetic does not depend on its tile, its row's position or the other rows: one k order, no position-dependent path.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/a3t_hip.h"
#include "wave_conv.h"

namespace {

struct MgsArgs {
    const float* x;       // [B*Tw][C]
    const float* w;       // [(4 C + Cp)][Cp]: W1 tap-major | Ws | W2 in accumulator order (vocoder.pack_melgan_stack)
    const float* bias;    // [2][Cp]: b1 | bs + b2
    float* y;             // [B*Tw][C]
    float slope;
    int B, Tw, dil, tiles_t;
    const int4* tiles;
};

template <int C, bool RAGGED>
__global__ __launch_bounds__(256) void mgan_stack_kernel(MgsArgs a) {
    constexpr int BK = 16, SUB = 128, LD = SUB + 4, CP = (C + 31) / 32 * 32, NJ = CP / 32, CPT = C / BK, HCH = CP / BK;
    constexpr int NQ = (4 * CP + 255) / 256;      // float4 of a weight chunk per thread
    __shared__ __attribute__((aligned(16))) float As[2][BK][LD];
    __shared__ __attribute__((aligned(16))) float Ws[2][BK * CP];

    const int tid = threadIdx.x, lane = tid & 63, wn = (tid >> 6) * 32, lr = lane & 31, lk = lane >> 5;
    const WaveTile at = wave_tile<RAGGED>(a.tiles, blockIdx.x >> 1, a.tiles_t, a.Tw);
    const int b = at.b, t0 = at.t0 + SUB * (blockIdx.x & 1), Wb = at.Wb;
    if (t0 >= Wb) return;                                    // (uniform: the second half of a tile that ends in its first)
    const int row = tid & (SUB - 1), part = tid >> 7;        // the sample and the 8 channels of a chunk this thread stages
    const int t = t0 + row;
    const float* xb = a.x + (int64_t)b * a.Tw * C;

    float4 P[2], Q[NQ];
    auto load_chunk = [&](int kc) {
        if (kc < 4 * CPT) {
            const int tap = kc < 3 * CPT ? kc / CPT : 1, c0 = (kc % CPT) * BK + 8 * part;
            if (t < Wb) {
                const int64_t ts = refl((int64_t)t + (int64_t)(tap - 1) * a.dil, Wb);
                const float4* s = (const float4*)(xb + ts * C + c0);
                P[0] = s[0], P[1] = s[1];
            } else {
                P[0] = P[1] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
        const float4* wq = (const float4*)(a.w + (int64_t)kc * BK * CP);
#pragma unroll
        for (int i = 0; i < NQ; ++i) Q[i] = tid + 256 * i < 4 * CP ? wq[tid + 256 * i] : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    auto store_chunk = [&](int buf, int kc) {
        if (kc < 4 * CPT) {
            const float sl = kc < 3 * CPT ? a.slope : 1.f;      // (the skip product reads x as it is)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                As[buf][8 * part + 4 * i + 0][row] = leaky(P[i].x, sl);
                As[buf][8 * part + 4 * i + 1][row] = leaky(P[i].y, sl);
                As[buf][8 * part + 4 * i + 2][row] = leaky(P[i].z, sl);
                As[buf][8 * part + 4 * i + 3][row] = leaky(P[i].w, sl);
            }
        }
#pragma unroll
        for (int i = 0; i < NQ; ++i)
            if (tid + 256 * i < 4 * CP) ((float4*)Ws[buf])[tid + 256 * i] = Q[i];
    };

    f32x16 acc1[NJ], acc2[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc1[j][r] = 0.f, acc2[j][r] = 0.f;

    // one chunk of a product whose B operand comes from the staged activations
    auto mma_x = [&](f32x16(&acc)[NJ], int buf) {
#pragma unroll
        for (int kk = 0; kk < BK / 2; ++kk) {
            const int k = kk * 2 + lk;
            const float bv = As[buf][k][wn + lr];
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(Ws[buf][k * CP + j * 32 + lr], bv, acc[j], 0, 0, 0);
        }
    };

    load_chunk(0);
    store_chunk(0, 0);
    __syncthreads();
    int buf = 0, kc = 0;
    // ---- the dilated convolution: h^T = W1^T leaky(x)^T
    for (; kc < 3 * CPT; ++kc) {
        load_chunk(kc + 1);
        mma_x(acc1, buf);
        store_chunk(buf ^ 1, kc + 1);      // (the other buffer was last read before the barrier that ended the previous chunk)
        __syncthreads();
        buf ^= 1;
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc1[j][r] = leaky(acc1[j][r] + a.bias[acc32_row(r, lk, j * 32)], a.slope);
    // ---- the skip product on x
    for (; kc < 4 * CPT; ++kc) {
        load_chunk(kc + 1);
        mma_x(acc2, buf);
        store_chunk(buf ^ 1, kc + 1);
        __syncthreads();
        buf ^= 1;
    }
    // ---- W2 on h, straight from the accumulators: step kk of chunk q is register r = 8 (q & 1) + kk of block q >> 1
#pragma unroll
    for (int q = 0; q < HCH; ++q) {
        if (q + 1 < HCH) load_chunk(4 * CPT + q + 1);
#pragma unroll
        for (int kk = 0; kk < BK / 2; ++kk) {
            const int k = kk * 2 + lk;
            const float bv = acc1[q >> 1][8 * (q & 1) + kk];
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                acc2[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(Ws[buf][k * CP + j * 32 + lr], bv, acc2[j], 0, 0, 0);
        }
        if (q + 1 < HCH) store_chunk(buf ^ 1, 4 * CPT + q + 1);
        __syncthreads();
        buf ^= 1;
    }

    // ---- bias and store: a lane holds 4 consecutive channels of its sample per register group
    const int ts = t0 + wn + lr;
    if (ts >= Wb) return;
    float* yr = a.y + ((int64_t)b * a.Tw + ts) * C;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int c0 = j * 32 + 8 * g + 4 * lk;
            if (c0 >= C) continue;
            const float4 bb = *(const float4*)(a.bias + CP + c0);
            float4 v;
            v.x = acc2[j][4 * g + 0] + bb.x, v.y = acc2[j][4 * g + 1] + bb.y;
            v.z = acc2[j][4 * g + 2] + bb.z, v.w = acc2[j][4 * g + 3] + bb.w;
            *(float4*)(yr + c0) = v;
        }
}

template <int C>
int mgan_stack_launch(const MgsArgs& a, int ntiles, void* stream) {
    return wave_ragged(a.tiles, [&](auto ragged) {
        hipLaunchKernelGGL((mgan_stack_kernel<C, decltype(ragged)::value>), dim3(2 * ntiles), dim3(256), 0, (hipStream_t)stream, a);
        return (int)hipGetLastError();
    });
}

}  // namespace

extern "C" int a3t_mgan_stack(const float* x, const float* w, const float* bias, float* y, float slope, const int32_t* tiles,
                              int ntiles, int wmin, int B, int Tw, int C, int dil, void* stream) {
    if (!x || !w || !bias || !y || x == y || (C != 48 && C != 96 && C != 192) || dil < 1) return A3T_EINVAL;
    if (((uintptr_t)x | (uintptr_t)w | (uintptr_t)bias | (uintptr_t)y) & 15) return A3T_EINVAL;
    const int n = wave_grid(tiles, ntiles, B, Tw);
    if (n <= 0) return n;
    if (n > INT_MAX / 2 || dil >= (tiles ? wmin : Tw)) return A3T_EINVAL;      // the reflection needs dil < W_b
    MgsArgs a;
    a.x = x, a.w = w, a.bias = bias, a.y = y, a.slope = slope, a.B = B, a.Tw = Tw, a.dil = dil, a.tiles_t = wave_tiles_t(Tw);
    a.tiles = (const int4*)tiles;
    return C == 48 ? mgan_stack_launch<48>(a, n, stream) : C == 96 ? mgan_stack_launch<96>(a, n, stream)
                                                                   : mgan_stack_launch<192>(a, n, stream);
}

// Output convolution, C -> O <= 4, LeakyReLU in front: wave_out_kernel (wave_conv.h) with the halo reflected at the row's own
// ends and two partial sums per output channel over c % 2.
extern "C" int a3t_mgan_out(const float* x, const float* w, const float* bias, float* y, float slope, int act_tanh,
                            const int32_t* tiles, int ntiles, int wmin, int B, int Tw, int C, int O, int K, void* stream) {
    if (!x || !w || !y || C < 2 || C > 64 || (C & 1) || O < 1 || O > 4 || K < 1 || K > 11 || !(K & 1)) return A3T_EINVAL;
    const int n = wave_grid(tiles, ntiles, B, Tw);
    if (n <= 0) return n;
    if ((K - 1) / 2 >= (tiles ? wmin : Tw)) return A3T_EINVAL;      // the reflection needs (K-1)/2 < W_b
    return wave_out_launch<true, 2, 4>(x, w, bias, y, slope, act_tanh, tiles, n, Tw, C, O, K, stream);
}

// ---------------------------------------------------------------- PQMF synthesis
// y[n] = S * sum_q sum_k h[k][S q - n + taps/2] * x[q][k] over 0 <= q < W_b / S and a filter index in [0, taps]: the reference's
// zero-stuffing transposed convolution, zero padding and convolution (pqmf.py:144-160) with the products of the stuffed zeros
// left out.  One workgroup per 256 output samples: the (256 + taps) / S sub-band rows the tile reaches and the filter go to
// LDS (16-byte loads where S = 4), a thread sums its ~ (taps + 1) / S rows in ascending q, k.  Memory-bound: 4 bytes in and out
// per sample.
namespace {
template <bool RAGGED>
__global__ __launch_bounds__(256) void pqmf_synthesis_kernel(const float* __restrict__ x, const float* __restrict__ h,
                                                             float* __restrict__ y, int S, int taps, int Tw, int tiles_t,
                                                             const int4* __restrict__ tiles) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int half = taps / 2, nf = taps + 1, nrows = (255 + taps) / S + 2;
    float* Xs = lds;                    // [nrows][S]
    float* Hs = lds + nrows * S;        // [S][taps + 1]
    const int tid = threadIdx.x;
    const auto [b, t0, Wb] = wave_tile<RAGGED>(tiles, blockIdx.x, tiles_t, Tw);
    const int Ts = Tw / S, Wq = Wb / S, K0 = half / S + 1;
    const int qlo = (t0 - half + S * K0) / S - K0;      // floor((t0 - half) / S)
    const float* xb = x + (int64_t)b * Ts * S;
    if (S == 4) {
        for (int r = tid; r < nrows; r += 256) {
            const int q = qlo + r;
            ((float4*)Xs)[r] = (q >= 0 && q < Wq) ? ((const float4*)xb)[q] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    } else {
        for (int i = tid; i < nrows * S; i += 256) {
            const int q = qlo + i / S;
            Xs[i] = (q >= 0 && q < Wq) ? xb[(int64_t)q * S + i % S] : 0.f;
        }
    }
    for (int i = tid; i < S * nf; i += 256) Hs[i] = h[i];
    __syncthreads();
    const int n = t0 + tid;
    if (n >= Wb) return;
    const int qa = (n - half + S * K0 + S - 1) / S - K0, qb = (n + half) / S;      // ceil((n - half) / S) .. floor((n + half) / S)
    float s = 0.f;
    for (int q = qa; q <= qb; ++q) {
        const int i = S * q - n + half;
        const float* xr = Xs + (q - qlo) * S;
        for (int k = 0; k < S; ++k) s = fmaf(Hs[k * nf + i], xr[k], s);
    }
    y[(int64_t)b * Tw + n] = (float)S * s;
}
}  // namespace

extern "C" int a3t_pqmf_synthesis(const float* x, const float* h, float* y, const int32_t* tiles, int ntiles, int B, int Ts,
                                  int S, int taps, void* stream) {
    if (!x || !h || !y || S < 1 || S > 8 || taps < 2 || taps > 254 || (taps & 1) || Ts <= 0 || (int64_t)Ts * S > INT_MAX)
        return A3T_EINVAL;
    if (S == 4 && ((uintptr_t)x & 15)) return A3T_EINVAL;
    const int Tw = Ts * S;
    const int n = wave_grid(tiles, ntiles, B, Tw);
    if (n <= 0) return n;
    const int lds = (((255 + taps) / S + 2) * S + S * (taps + 1)) * 4, tiles_t = wave_tiles_t(Tw);
    return wave_ragged(tiles, [&](auto ragged) {
        hipLaunchKernelGGL(pqmf_synthesis_kernel<decltype(ragged)::value>, dim3(n), dim3(256), lds, (hipStream_t)stream, x, h, y,
                           S, taps, Tw, tiles_t, (const int4*)tiles);
        return (int)hipGetLastError();
    });
}

// ---------------------------------------------------------------- reflection padding of rows, the twin of a3t_replicate_pad
// y[b][u] = x[b][refl(u - pad)] over the row's own length L (RAGGED: lens[b] * mul; zero for an empty row).  Positions that one
// reflection does not reach (L <= pad, or behind a short row's reflected end) are clamped into the row.
namespace {
template <bool RAGGED>
__global__ void reflect_pad_rows_kernel(const float* x, float* y, const int32_t* __restrict__ lens, int mul, int64_t B, int64_t T,
                                        int C, int pad) {
    const int64_t Tp = T + 2 * pad, n = B * Tp * C;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t ta = i / C;
        const int c = (int)(i - ta * C);
        const int64_t b = ta / Tp;
        int64_t L = RAGGED ? (int64_t)lens[b] * mul : T;
        L = L > T ? T : L;
        y[i] = L > 0 ? x[(b * T + refl(ta - b * Tp - pad, L)) * C + c] : 0.f;
    }
}
template <bool RAGGED>
int reflect_pad_rows(const float* x, float* y, const int32_t* lens, int mul, int64_t B, int64_t T, int C, int pad, void* stream) {
    if (!x || !y || B <= 0 || T <= 0 || C <= 0 || pad < 0 || mul <= 0 || (!RAGGED && pad >= T)) return A3T_EINVAL;
    const int64_t n = B * (T + 2 * pad) * C;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(reflect_pad_rows_kernel<RAGGED>, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream, x, y, lens, mul, B, T,
                       C, pad);
    return (int)hipGetLastError();
}
}  // namespace

extern "C" int a3t_reflect_pad_rows(const float* x, float* y, int64_t B, int64_t T, int C, int pad, void* stream) {
    return reflect_pad_rows<false>(x, y, nullptr, 1, B, T, C, pad, stream);
}
extern "C" int a3t_reflect_pad_rows_ragged(const float* x, float* y, const int32_t* lens, int mul, int64_t B, int64_t T, int C,
                                           int pad, void* stream) {
    if (!lens) return A3T_EINVAL;
    return reflect_pad_rows<true>(x, y, lens, mul, B, T, C, pad, stream);
}
