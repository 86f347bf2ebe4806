// hifigan_f16.hip -- the HiFi-GAN residual-unit convolution (a3t_hfg_conv of hifigan.hip) on the 16-bit MFMA of gfx950
// (v_mfma_f32_32x32x16_f16, fp32 accumulate), for every stage width of the v1 plan: C = 32 / 64 / 128 / 256.
//
//   v[t] = bias + sum_{tap,c} h(W[tap][c][:]) * h(leaky(x[t + (tap - (k-1)/2) * dil][c])) (+ R[t])
//   y[t] = v[t]  and / or  acc[t] (+)= alpha * v[t]
//
// h() = round to nearest even to fp16, saturated to +-65504.  leaky() is computed in fp32 and rounded on its way into the MFMA;
// the weight is rounded once on the host (vocoder.pack_hifigan_conv_f16).  Products are fp16 x fp16, exact in the fp32
// accumulator; bias, residual, the MRF accumulation and every tensor in memory stay fp32.
//
// TRANSPOSED product, as pwg_fused_f16.hip:  V^T [C out][32 t] = W^T [C out][k * C] . act^T [k * C][32 t].
// * The samples are the MFMA's columns.  A B fragment is 8 consecutive channels of one sample at one tap = 32 contiguous bytes
//   of the fp32 x: global memory -> registers -> leaky -> fp16.  No activation tile in LDS, so the halo (k-1)/2 * dil may be of
//   any size: a tap's row is addressed, never staged.
// * A workgroup is one 256-sample tile of wave_tiles.h, 8 waves of 32 samples x all C output channels: C / 32 accumulator
//   blocks per wave (16 / 32 / 64 / 128 registers).
// * K runs tap-major, channels ascending, in k-steps of 16 input channels.  The weights are the A operand.  The host lays them
//   out in fragment order, [k-step][C / 32 M-tiles][64 lanes][8 halves] = 1 KiB per fragment, and the kernel streams them through
//   LDS in double-buffered chunks of KSC k-steps (KSC x C/32 KiB: 4 / 8 / 16 / 16 KiB at C = 32 / 64 / 128 / 256): chunk c + 1 travels global -> registers -> LDS
//   while the MFMAs of chunk c run, one barrier per chunk.  The copy is linear and every fragment read is one ds_read_b128 of
//   64 consecutive lanes (conflict-free).  The activations of chunk c + 1 are loaded under the MFMAs of chunk c as well.
//   The last chunk of a convolution may be partial (k-steps = taps * C / 16 is no multiple of KSC = 4 at C = 32): its missing
//   k-steps are zero weights times zero activations, exact zeros on the accumulator.
// * A staged chunk of KSC x C/32 KiB feeds 8 waves x KSC x C/32 MFMAs: 128 B of L2 -> LDS traffic per MFMA.  A wave
//   reads each fragment once from LDS: 1 KiB per 32-cycle MFMA and wave, 4 SIMDs -> 128 B / cycle, the LDS peak.  The kernel
//   is therefore LDS-paced at C >= 128 (a second 32-sample column block per wave would halve that and needs 256 accumulator
//   registers at C = 256) and paced by the activation loads (k reads of every x value through L1 / L2) at C = 32 / 64.
//
// A sample is one MFMA column and its K order is fixed: its bits depend neither on its tile, nor on its row's place in the
// batch, nor on the other rows; taps outside the row are exact zeros (leaky(0) = 0).
//
// LDS: 2 buffers x KSC x C/32 KiB, static.  Compiler's report for gfx950 (-O3), no scratch, no spills:
//   C     KSC   VGPRs   AGPRs   LDS      waves / SIMD by registers   workgroups (2 waves / SIMD each) per CU
//   32    4     96      0       8 KiB    5                           2
//   64    4     112     0       16 KiB   4                           2
//   128   4     147     0       32 KiB   3                           1
//   256   2     184     0       32 KiB   2                           1
// The registers beside the accumulators (16 C / 32) are the next chunk's activations in flight: KSC x 8 fp32 + KSC x 4 packed.
// At C = 32 / 64 the kernel waits for memory, not for the MFMA: KSC = 4 and the launch bound keep it under 128 VGPRs for a
// second resident workgroup (measured against KSC = 8 with one workgroup per CU, 8 x 1000 frames of the v1 plan: the C = 32
// stage 6.3 ms against 8.0 ms, the C = 64 stage 5.2 ms against 6.1 ms).
// HBM model per sample and convolution: x read once 4 C (its other k - 1 reads are expected from L1 / L2), y or acc written
// 4 C, + 4 C for R, + 4 C for acc_add's read: 8 C - 16 C bytes; a residual unit of two convolutions 20 C.  Weights: 2 k C^2 bytes
// per workgroup from L2.
// x must not alias y or acc: a tile reads x[t +- halo] of tiles that another workgroup may already have finished.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/a3t_hip.h"
#include "wave_tiles.h"

struct HfgF16Args {
    const float* x;       // [B*Tw][C] conv input (read through LeakyReLU)
    const uint4* wf;      // [taps*C/16][C/32][64] fragments of 8 halves
    const float* bias;    // [C] or nullptr
    const float* R;       // [B*Tw][C] residual or nullptr (may alias y)
    float* y;             // [B*Tw][C] or nullptr
    float* acc;           // [B*Tw][C] or nullptr
    float slope, alpha;
    int acc_add;          // acc += alpha * v, else acc = alpha * v
    int B, Tw, taps, dil, tiles_t;
    const int4* tiles;    // RAGGED: [ntiles] tile list (wave_tiles.h)
};

template <int C, bool RAGGED>
__global__ __launch_bounds__(512, C <= 64 ? 2 : 1) void hfg_conv_f16_kernel(HfgF16Args a) {
    // MT M-tiles of 32 output channels, KPT k-steps per tap, KSC k-steps per chunk, FR fragments (1 KiB) per chunk, NQ 16-byte
    // pieces of a chunk per thread
    constexpr int MT = C / 32, KPT = C / 16, KSC = C >= 256 ? 2 : 4, FR = KSC * MT, NQ = (FR + 7) / 8;
    __shared__ __attribute__((aligned(16))) uint4 Ws[2][FR * 64];

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
    const WaveTile at = wave_tile<RAGGED>(a.tiles, blockIdx.x, a.tiles_t, a.Tw);
    const int b = at.b, Wb = at.Wb, t = at.t0 + w * 32 + r;      // (named: the lambdas below capture them)
    const bool valid = t < Wb;
    const int nks = a.taps * KPT, nch = (nks + KSC - 1) / KSC, half = (a.taps - 1) / 2, npieces = nks * MT * 64;
    const float* xb = a.x + (int64_t)b * a.Tw * C + 8 * h;

    uint4 Q[NQ];
    float4 P[KSC][2];
    f16x8 bf[KSC];
    auto load_chunk = [&](int ch) {
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            const int idx = ch * (FR * 64) + i * 512 + tid;
            Q[i] = (FR >= 8 || tid < FR * 64) && idx < npieces ? a.wf[idx] : make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (int s = 0; s < KSC; ++s) {
            const int ks = ch * KSC + s, tap = ks / KPT, c0 = (ks - tap * KPT) * 16;
            const int64_t ts = (int64_t)t + (int64_t)(tap - half) * a.dil;
            P[s][0] = P[s][1] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (valid && ks < nks && ts >= 0 && ts < Wb) {
                const float4* src = (const float4*)(xb + ts * C + c0);
                P[s][0] = src[0], P[s][1] = src[1];
            }
        }
    };
    auto store_chunk = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NQ; ++i)
            if (FR >= 8 || tid < FR * 64) Ws[buf][i * 512 + tid] = Q[i];
#pragma unroll
        for (int s = 0; s < KSC; ++s) bf[s] = pack_f16_sat(leaky(P[s][0], a.slope), leaky(P[s][1], a.slope));      // h(leaky())
    };

    f32x16 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[mt][i] = 0.f;

    load_chunk(0);
    store_chunk(0);
    __syncthreads();
    int buf = 0;
    for (int ch = 0; ch < nch; ++ch) {
        const bool more = ch + 1 < nch;
        if (more) load_chunk(ch + 1);
        const f16x8* Wf = (const f16x8*)Ws[buf];
#pragma unroll
        for (int s = 0; s < KSC; ++s)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
                acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Wf[(s * MT + mt) * 64 + lane], bf[s], acc[mt], 0, 0, 0);
        // the other buffer was last read before the barrier that ended the previous chunk
        if (more) store_chunk(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }

    // bias / residual / store / MRF accumulation straight from the accumulators: registers 4 q .. 4 q + 3 of M-tile mt are
    // channels 32 mt + 8 q + 4 h .. + 3 of sample t (acc32_row)
    if (!valid) return;
    const int64_t row = ((int64_t)b * a.Tw + t) * C;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t idx = row + acc32_row(4 * q, h, 32 * mt);
            float4 v = make_float4(acc[mt][4 * q], acc[mt][4 * q + 1], acc[mt][4 * q + 2], acc[mt][4 * q + 3]);
            if (a.bias) {
                const float4 bj = *(const float4*)(a.bias + acc32_row(4 * q, h, 32 * mt));
                v.x += bj.x, v.y += bj.y, v.z += bj.z, v.w += bj.w;
            }
            if (a.R) {
                const float4 rj = *(const float4*)(a.R + idx);
                v.x += rj.x, v.y += rj.y, v.z += rj.z, v.w += rj.w;
            }
            if (a.y) *(float4*)(a.y + idx) = v;
            if (a.acc) {
                float4 o = make_float4(a.alpha * v.x, a.alpha * v.y, a.alpha * v.z, a.alpha * v.w);
                if (a.acc_add) {
                    const float4 p = *(const float4*)(a.acc + idx);
                    o.x = p.x + o.x, o.y = p.y + o.y, o.z = p.z + o.z, o.w = p.w + o.w;
                }
                *(float4*)(a.acc + idx) = o;
            }
        }
}

template <int C>
static int hfg_conv_f16_launch(const HfgF16Args& a, int ntiles, void* stream) {
    return wave_ragged(a.tiles, [&](auto ragged) {
        hipLaunchKernelGGL((hfg_conv_f16_kernel<C, decltype(ragged)::value>), dim3(ntiles), dim3(512), 0, (hipStream_t)stream, a);
        return (int)hipGetLastError();
    });
}

// a3t_hfg_conv with fp16 operands.  wf: the fp16 fragments of vocoder.pack_hifigan_conv_f16, [taps*C/16][C/32][64][8]:
// wf[ks][mt][l][j] = fp16(W[out 32 mt + (l & 31)][in 16 (ks % (C/16)) + 8 (l >> 5) + j][tap ks / (C/16)]).
extern "C" int a3t_hfg_conv_f16(const float* x, const void* wf, const float* bias, const float* R, float* y, float* acc,
                                float alpha, int acc_add, float slope, const int32_t* tiles, int ntiles, int B, int Tw, int C,
                                int taps, int dil, void* stream) {
    if (!x || !wf || (!y && !acc) || (C != 32 && C != 64 && C != 128 && C != 256) || taps < 1 || taps > 11 || !(taps & 1) || dil < 1)
        return A3T_EINVAL;
    if (x == y || x == acc || (y && y == acc)) return A3T_EINVAL;      // other tiles read x[t +- halo]
    if (((uintptr_t)x | (uintptr_t)wf | (uintptr_t)bias | (uintptr_t)R | (uintptr_t)y | (uintptr_t)acc) & 15) return A3T_EINVAL;
    const int n = wave_grid(tiles, ntiles, B, Tw);
    if (n <= 0) return n;
    HfgF16Args a;
    a.x = x, a.wf = (const uint4*)wf, a.bias = bias, a.R = R, a.y = y, a.acc = acc, a.slope = slope, a.alpha = alpha;
    a.acc_add = acc_add, a.B = B, a.Tw = Tw, a.taps = taps, a.dil = dil, a.tiles_t = wave_tiles_t(Tw), a.tiles = (const int4*)tiles;
    switch (C) {
        case 32: return hfg_conv_f16_launch<32>(a, n, stream);
        case 64: return hfg_conv_f16_launch<64>(a, n, stream);
        case 128: return hfg_conv_f16_launch<128>(a, n, stream);
        default: return hfg_conv_f16_launch<256>(a, n, stream);
    }
}
