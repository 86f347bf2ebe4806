// pwg_fused_f16.hip -- ParallelWaveGAN residual block (espnet2/gan_tts/wavenet/residual_block.py:114-169) in ONE launch on
// the 16-bit MFMA of gfx950 (v_mfma_f32_32x32x16_f16, fp32 accumulate), channels-last [T][C] tensors.
//
//   y = dilated Conv1d_k3(h(x))[t] + Conv1x1_aux(cu16)[t] + b0;   g = tanh(ya) * sigmoid(yb)                (128 gate channels)
//   o = Conv1x1_out(h(g)) + b1;   x_out[t] = (o[:64] + x[t]) * sqrt(1/2);   skips[t] += o[64:]
//
// h() = round to nearest even to fp16, saturated to +-65504.  It is applied to the conv input x, to cu (once per call, by
// a3t_cast_f16_sat), to g and to the three weight matrices (on the host); accumulation, biases, tanh / sigmoid, the residual
// stream and skips stay fp32.
//
// TRANSPOSED formulation: the weights are the MFMA's A operand and the samples its columns,
//   Y^T [128 n'][32 t] = W0^T [n'][272 k] . act^T [k][t],      O^T [128 m][32 t] = W1^T [m][64 c] . G^T [c][t].
// * A B fragment is 8 consecutive channels of one sample = 32 contiguous bytes of x (16 of cu16): the activations go from
//   global memory to registers and are converted there.  No LDS staging, so no barrier inside the persistent loop: a wave
//   owns 32 samples from its loads to its stores.  (The alternative, a 128-sample x 272 fp16 LDS tile, costs 68 KiB and two
//   barriers per tile to feed the same MFMAs; with 84 KiB of weights resident it would also leave no room for a second
//   buffer.  The direct form was chosen for that reason and has not been measured against a staged one.)
// * The accumulator tile of Y^T has the sample on the lane and the gate channel in the registers, and so has G^T: rounded
//   to fp16 it IS the B operand of the second product, which sums over its row (register) index.  g, y and o never leave
//   the registers.  Element j of lane half h of k-step s is row 16 s + 8 (j >> 2) + 4 h + (j & 3) of the tile; the W1
//   fragments are laid out in that k order.
// * With the host's column permutation a wave's M-tiles 2i and 2i + 1 hold the tanh and the sigmoid pre-activation of
//   the same 32 channels in the same lane and register: the gate needs no exchange.
// * Output row i of M-tile mt is channel 16 (2 mt + (i >> 4)) + 8 ((i >> 2) & 1) + 4 ((i >> 3) & 1) + (i & 3): a lane then
//   finishes exactly the 32 channels of x whose fp32 values it loaded for the centre tap (the residual needs no second
//   read) and stores 32 contiguous bytes per sample and k-step.
//
// LDS: W0 as [4 M-tiles][17 k-steps][64 lanes] fragments = 68 KiB, W1 as [4][4][64] = 16 KiB, biases 1 KiB: 85 KiB, one
// persistent workgroup of 8 waves (two per SIMD) per CU.  Every fragment read is one ds_read_b128 of consecutive lanes.
// A sample is one MFMA column and its K order is fixed, so its bits do not depend on its tile or on the rest of the batch.
// x_out must not alias x_in: a tile reads x[t +- dil] of tiles that another workgroup may already have finished.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/a3t_hip.h"
#include "device_cus.h"
#include "wave_tiles.h"

struct PwgF16Args {
    const float* x_in;       // [B*Tw][64]
    float* x_out;            // [B*Tw][64], != x_in
    const _Float16* cu;      // [B*Tw][80]
    const _Float16* w0;      // [272][128] k-major, permuted columns
    const float* b0;         // [128] permuted the same way
    const _Float16* w1;      // [64][128] = conv1x1_out.weight^T
    const float* b1;         // [128]
    float* skips;            // [B*Tw][64]
    const int4* tiles;       // RAGGED: [ntiles] tile list (wave_tiles.h)
    int ntiles, B, Tw, dil, tiles_t;
};

// channel of output row i (0..31) of M-tile mt (0..1) of the second product
__device__ __forceinline__ int out_channel(int mt, int i) {
    return 16 * (2 * mt + (i >> 4)) + 8 * ((i >> 2) & 1) + 4 * ((i >> 3) & 1) + (i & 3);
}

template <bool RAGGED>
__global__ __launch_bounds__(512) void pwg_f16_kernel(PwgF16Args a) {
    constexpr int KS0 = 17, KS1 = 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    f16x8* W0f = (f16x8*)smem;                 // [4][KS0][64]
    f16x8* W1f = W0f + 4 * KS0 * 64;           // [4][KS1][64]
    float* B0s = (float*)(W1f + 4 * KS1 * 64); // [128] row order of Y^T
    float* B1s = B0s + 128;                    // [128] row order of O^T

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
    for (int f = tid; f < 4 * KS0 * 64; f += 512) {
        const int l = f & 63, ms = f >> 6, mt = ms / KS0, s = ms - mt * KS0;
        const _Float16* src = a.w0 + (16 * s + 8 * (l >> 5)) * 128 + 32 * mt + (l & 31);
        f16x8 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = src[j * 128];
        W0f[f] = v;
    }
    for (int f = tid; f < 4 * KS1 * 64; f += 512) {
        const int l = f & 63, ms = f >> 6, mt = ms >> 2, ks = ms & 3;
        const int m = 64 * (mt >> 1) + out_channel(mt & 1, l & 31);
        f16x8 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = a.w1[(16 * ks + 8 * (j >> 2) + 4 * (l >> 5) + (j & 3)) * 128 + m];
        W1f[f] = v;
    }
    if (tid < 128) {
        B0s[tid] = a.b0[tid];
        B1s[tid] = a.b1[64 * (tid >> 6) + out_channel((tid >> 5) & 1, tid & 31)];
    }
    __syncthreads();

    const int ntiles = RAGGED ? a.ntiles : a.B * a.tiles_t;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const auto [b, t0, Wb] = wave_tile<RAGGED>(a.tiles, tile, a.tiles_t, a.Tw);
        if (t0 + w * 32 >= Wb) continue;        // (wave-uniform; no barrier below)
        const int t = t0 + w * 32 + r;
        const bool valid = t < Wb;
        const int64_t base = (int64_t)b * a.Tw;
        const int64_t row = base + (valid ? t : 0);

        // ---- loads: three taps of x (fp32, 8 channels per k-step), cu16, the skips this lane will update
        float4 xc[4][2];
        f16x8 bf[KS0];
#pragma unroll
        for (int tap = 0; tap < 3; ++tap) {
            const int ts = t + (tap - 1) * a.dil;
            const bool ok = valid && ts >= 0 && ts < Wb;
            const float* src = a.x_in + (base + (ok ? ts : 0)) * 64 + 8 * h;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0;
                if (ok) v0 = *(const float4*)(src + 16 * s), v1 = *(const float4*)(src + 16 * s + 4);
                if (tap == 1) xc[s][0] = v0, xc[s][1] = v1;
                bf[tap * 4 + s] = pack_f16_sat(v0, v1);
            }
        }
#pragma unroll
        for (int s = 0; s < 5; ++s) {
            f16x8 q = {0, 0, 0, 0, 0, 0, 0, 0};
            if (valid) q = *(const f16x8*)(a.cu + row * 80 + 16 * s + 8 * h);
            bf[12 + s] = q;
        }
        float4 sk[4][2];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            sk[s][0] = sk[s][1] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (valid) {
                const float* src = a.skips + row * 64 + 16 * s + 8 * h;
                sk[s][0] = *(const float4*)src, sk[s][1] = *(const float4*)(src + 4);
            }
        }

        // ---- Y^T = W0^T act^T
        f32x16 acc[4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[mt][i] = 0.f;
#pragma unroll
        for (int s = 0; s < KS0; ++s)
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
                acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(W0f[(mt * KS0 + s) * 64 + lane], bf[s], acc[mt], 0, 0, 0);

        // ---- gate on the accumulators; G^T rounded to fp16 is the next B operand
        f16x8 gf[4];
#pragma unroll
        for (int gt = 0; gt < 2; ++gt)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 ba = *(const float4*)(B0s + 64 * gt + 8 * q + 4 * h);
                const float4 bb = *(const float4*)(B0s + 64 * gt + 32 + 8 * q + 4 * h);
                const float bav[4] = {ba.x, ba.y, ba.z, ba.w}, bbv[4] = {bb.x, bb.y, bb.z, bb.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int i = 4 * q + e;
                    const float ya = acc[2 * gt][i] + bav[e], yb = acc[2 * gt + 1][i] + bbv[e];
                    gf[2 * gt + (q >> 1)][4 * (q & 1) + e] = (_Float16)pwg_gate(ya, yb);
                }
            }

        // ---- O^T = W1^T G^T
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[mt][i] = 0.f;
#pragma unroll
            for (int ks = 0; ks < KS1; ++ks)
                acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(W1f[(mt * KS1 + ks) * 64 + lane], gf[ks], acc[mt], 0, 0, 0);
        }

        // ---- residual and skip, fp32: register group q of M-tile mt = channels 16 (2 mt + (q >> 1)) + 8 h + 4 (q & 1) .. + 3
        if (valid) {
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int s = 2 * mt + (q >> 1), ch = 16 * s + 8 * h + 4 * (q & 1);
                    const float4 b1x = *(const float4*)(B1s + 32 * mt + 8 * q + 4 * h);
                    const float4 b1s = *(const float4*)(B1s + 64 + 32 * mt + 8 * q + 4 * h);
                    const float4 xo = xc[s][q & 1], so = sk[s][q & 1];
                    float4 xn, sn;
                    xn.x = (acc[mt][4 * q + 0] + b1x.x + xo.x) * 0.70710678118654752440f;
                    xn.y = (acc[mt][4 * q + 1] + b1x.y + xo.y) * 0.70710678118654752440f;
                    xn.z = (acc[mt][4 * q + 2] + b1x.z + xo.z) * 0.70710678118654752440f;
                    xn.w = (acc[mt][4 * q + 3] + b1x.w + xo.w) * 0.70710678118654752440f;
                    sn.x = so.x + (acc[2 + mt][4 * q + 0] + b1s.x);
                    sn.y = so.y + (acc[2 + mt][4 * q + 1] + b1s.y);
                    sn.z = so.z + (acc[2 + mt][4 * q + 2] + b1s.z);
                    sn.w = so.w + (acc[2 + mt][4 * q + 3] + b1s.w);
                    *(float4*)(a.x_out + row * 64 + ch) = xn;
                    *(float4*)(a.skips + row * 64 + ch) = sn;
                }
        }
    }
}

// One residual block on the 16-bit MFMA.  x_in -> x_out (two different buffers: the caller swaps them per layer), skips updated
// in place.  cu16 [B*Tw][80] fp16 (a3t_cast_f16_sat of the upsampled mel); w0h [272][128] fp16, rows and columns as wt0 of
// a3t_pwg_block; w1h [64][128] fp16 = conv1x1_out.weight^T; b0 / b1 fp32 as there.  tiles: the contract of wave_tiles.h.
extern "C" int a3t_pwg_block_f16(const float* x_in, float* x_out, const void* cu16, const void* w0h, const float* b0,
                                 const void* w1h, const float* b1, float* skips, const int32_t* tiles, int ntiles, int B, int Tw,
                                 int dil, void* stream) {
    const int n = wave_grid(tiles, ntiles, B, Tw);
    if (n < 0 || dil <= 0 || !x_in || !x_out || !cu16 || !w0h || !b0 || !w1h || !b1 || !skips) return A3T_EINVAL;
    if ((((uintptr_t)x_in | (uintptr_t)x_out | (uintptr_t)cu16 | (uintptr_t)skips) & 15) ||
        (((uintptr_t)w0h | (uintptr_t)w1h) & 1) || (((uintptr_t)b0 | (uintptr_t)b1) & 3))
        return A3T_EINVAL;
    const uintptr_t bytes = (uintptr_t)B * (uintptr_t)Tw * 64 * sizeof(float), xi = (uintptr_t)x_in, xo = (uintptr_t)x_out;
    if (xi < xo + bytes && xo < xi + bytes) return A3T_EINVAL;      // x_out overlaps x_in
    if (!n) return 0;
    PwgF16Args a;
    a.x_in = x_in, a.x_out = x_out, a.cu = (const _Float16*)cu16, a.w0 = (const _Float16*)w0h, a.b0 = b0;
    a.w1 = (const _Float16*)w1h, a.b1 = b1, a.skips = skips;
    a.B = B, a.Tw = Tw, a.dil = dil, a.tiles_t = wave_tiles_t(Tw);
    a.tiles = (const int4*)tiles, a.ntiles = ntiles;
    return wave_ragged(tiles, [&](auto ragged) {
        constexpr auto kernel = pwg_f16_kernel<decltype(ragged)::value>;
        constexpr int lds = (4 * 17 + 4 * 4) * 64 * 16 + 256 * 4;      // 87 040 B
        const hipError_t e = wave_lds_opt_in<kernel>(lds);
        if (e != hipSuccess) return (int)e;
        const int cus = device_cus();
        hipLaunchKernelGGL(kernel, dim3(n < cus ? n : cus), dim3(512), lds, (hipStream_t)stream, a);
        return (int)hipGetLastError();
    });
}

__global__ void cast_f16_sat_kernel(const float* __restrict__ src, _Float16* __restrict__ dst, int64_t n) {
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 8;
    if (i + 8 <= n) {
        *(f16x8*)(dst + i) = pack_f16_sat(*(const float4*)(src + i), *(const float4*)(src + i + 4));
    } else {
        for (int64_t j = i; j < n; ++j) dst[j] = (_Float16)sat16(src[j]);
    }
}

// dst[i] = fp16(src[i]): round to nearest even, saturated to +-65504 (a NaN becomes a finite number).  src 16-byte, dst
// 16-byte aligned.
extern "C" int a3t_cast_f16_sat(const float* src, void* dst, int64_t n, void* stream) {
    if (n < 0 || !src || !dst || (((uintptr_t)src | (uintptr_t)dst) & 15)) return A3T_EINVAL;
    if (n == 0) return 0;
    const int64_t groups = (n + 7) / 8;
    hipLaunchKernelGGL(cast_f16_sat_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src,
                       (_Float16*)dst, n);
    return (int)hipGetLastError();
}
