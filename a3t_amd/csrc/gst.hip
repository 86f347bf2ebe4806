// gst.hip -- the GST style encoder of a gst+xvector FastSpeech2 for gfx950 (espnet2/tts/gst/style_encoder.py), as the
// duration path of the speech editor runs it (sedit_inference.py:413-418): fp32, eval mode, forward only.
//   a3t_gst_conv_bn_relu : one Conv2d(k x k, stride s, no bias) + BatchNorm2d (running statistics, folded to scale / shift)
//                          + ReLU layer of the ReferenceEncoder, channels-last, with per-row lengths;
//   a3t_gst_gru_stl      : the GRU recurrence over a row's own steps and the style-token attention, one workgroup per prompt;
//   a3t_gst_add_style    : hs[b][t][:] += style[row of b][:].
// A batch of prompts is padded to the longest; every row gets what it would get alone (the "ragged" rule of the header).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/a3t_hip.h"

#define GST_MAXH 128      // gru_units: one W_hh gate row per thread, held in GST_MAXH VGPRs
#define GST_MAXD 1024     // gst_token_dim (= adim)
#define GST_MAXS 512      // gst_heads * gst_tokens

// One thread per output element (b, t', f', co), co fastest: the weight reads w[kt][kf][ci][co] are coalesced over co and
// the input reads x[b][t][f][ci] are the same address for all co of a position (one broadcast load).
// Row b reads zeros at t >= n = lens[b] and stores 0 at t' >= n' = (n + 2p - k) / s + 1; what x holds behind n is never read.
__global__ __launch_bounds__(256) void gst_conv_bn_relu_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                               const float* __restrict__ scale,
                                                               const float* __restrict__ shift, float* __restrict__ y,
                                                               const int32_t* __restrict__ lens, int B, int Tin, int Fin,
                                                               int Cin, int Tout, int Fout, int Cout, int k, int s) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t total = (int64_t)B * Tout * Fout * Cout;
    if (idx >= total) return;
    const int co = (int)(idx % Cout);
    int64_t r = idx / Cout;
    const int fo = (int)(r % Fout);
    r /= Fout;
    const int to = (int)(r % Tout);
    const int b = (int)(r / Tout);
    const int p = (k - 1) / 2;
    int n = Tin;
    if (lens) n = min(max(lens[b], 0), Tin);
    const int nout = (n + 2 * p - k >= 0) ? (n + 2 * p - k) / s + 1 : 0;
    if (to >= nout) {
        y[idx] = 0.f;
        return;
    }
    const float* xb = x + (int64_t)b * Tin * Fin * Cin;
    float acc = 0.f;
    for (int kt = 0; kt < k; ++kt) {
        const int t = to * s - p + kt;
        if (t < 0 || t >= n) continue;
        for (int kf = 0; kf < k; ++kf) {
            const int f = fo * s - p + kf;
            if (f < 0 || f >= Fin) continue;
            const float* xp = xb + ((int64_t)t * Fin + f) * Cin;
            const float* wp = w + (int64_t)(kt * k + kf) * Cin * Cout + co;
            int ci = 0;
            for (; ci + 4 <= Cin; ci += 4) {
                acc = fmaf(xp[ci], wp[(int64_t)ci * Cout], acc);
                acc = fmaf(xp[ci + 1], wp[(int64_t)(ci + 1) * Cout], acc);
                acc = fmaf(xp[ci + 2], wp[(int64_t)(ci + 2) * Cout], acc);
                acc = fmaf(xp[ci + 3], wp[(int64_t)(ci + 3) * Cout], acc);
            }
            for (; ci < Cin; ++ci) acc = fmaf(xp[ci], wp[(int64_t)ci * Cout], acc);
        }
    }
    y[idx] = fmaxf(fmaf(acc, scale[co], shift[co]), 0.f);
}

extern "C" int a3t_gst_conv_bn_relu(const float* x, const float* w, const float* scale, const float* shift, float* y,
                                    const int32_t* lens, int B, int Tin, int Fin, int Cin, int Cout, int k, int s,
                                    void* stream) {
    if (B <= 0 || Tin <= 0 || Fin <= 0 || Cin <= 0 || Cout <= 0 || k <= 0 || k % 2 == 0 || s <= 0) return A3T_EINVAL;
    const int p = (k - 1) / 2;
    const int Tout = (Tin + 2 * p - k) / s + 1, Fout = (Fin + 2 * p - k) / s + 1;
    const int64_t total = (int64_t)B * Tout * Fout * Cout;
    if ((int64_t)B * Tin * Fin * Cin >= ((int64_t)1 << 40) || (total + 255) / 256 > 0x7fffffff) return A3T_EINVAL;
    hipLaunchKernelGGL(gst_conv_bn_relu_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, w,
                       scale, shift, y, lens, B, Tin, Fin, Cin, Tout, Fout, Cout, k, s);
    return (int)hipGetLastError();
}

__device__ __forceinline__ float gst_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ float gst_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

// out[o] = W[o] . v + bias[o] for o < N (W [N][K] row-major, v [K] in LDS): one wave per output row, lanes over K.
__device__ __forceinline__ void gst_matvec(const float* __restrict__ W, const float* __restrict__ bias, const float* v,
                                           float* out, int N, int K, int wave, int nwaves, int lane) {
    for (int o = wave; o < N; o += nwaves) {
        const float* wr = W + (int64_t)o * K;
        float a = 0.f;
        for (int i = lane; i < K; i += 64) a = fmaf(wr[i], v[i], a);
        a = gst_wave_sum(a);
        if (lane == 0) out[o] = a + bias[o];
    }
}

// Workgroup b: the GRU of row b over its own n = lens[b] steps (PyTorch gate order r, z, n), then the style-token attention.
// 3H threads (rounded up to whole waves); thread j < 3H keeps row j of W_hh in registers, h goes round through LDS.
// gi [B][T][3H] = W_ih x_t + b_ih of every step (a GEMM in front of this launch).
__global__ __launch_bounds__(3 * GST_MAXH) void gst_gru_stl_kernel(
    const float* __restrict__ gi, const float* __restrict__ whh, const float* __restrict__ bhh, const int32_t* __restrict__ lens,
    const float* __restrict__ wq, const float* __restrict__ bq, const float* __restrict__ Kt, const float* __restrict__ Vt,
    const float* __restrict__ wo, const float* __restrict__ bo, float* __restrict__ ref_embs, float* __restrict__ style, int T,
    int H, int d, int heads, int tokens) {
    __shared__ __attribute__((aligned(16))) float sh_h[GST_MAXH];
    __shared__ float sh_g[3 * GST_MAXH];
    __shared__ float sh_q[GST_MAXD];
    __shared__ float sh_c[GST_MAXD];
    __shared__ float sh_p[GST_MAXS];
    const int b = blockIdx.x, j = threadIdx.x, H3 = 3 * H;
    const int lane = j & 63, wave = j >> 6, nwaves = blockDim.x >> 6;
    int n = T;
    if (lens) n = min(max(lens[b], 0), T);

    float wr[GST_MAXH];
#pragma unroll
    for (int i = 0; i < GST_MAXH; ++i) wr[i] = (j < H3 && i < H) ? whh[(int64_t)j * H + i] : 0.f;
    const float bj = (j < H3) ? bhh[j] : 0.f;
    for (int i = j; i < GST_MAXH; i += blockDim.x) sh_h[i] = 0.f;
    __syncthreads();

    const float* gib = gi + (int64_t)b * T * H3;
    for (int t = 0; t < n; ++t) {
        float g_r = 0.f, g_z = 0.f, g_n = 0.f;
        if (j < H) {      // this step's input projection, in flight while the recurrent product runs
            g_r = gib[(int64_t)t * H3 + j];
            g_z = gib[(int64_t)t * H3 + H + j];
            g_n = gib[(int64_t)t * H3 + 2 * H + j];
        }
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
        for (int i = 0; i < GST_MAXH; i += 4) {
            const float4 hv = *reinterpret_cast<const float4*>(&sh_h[i]);
            a0 = fmaf(wr[i], hv.x, a0);
            a1 = fmaf(wr[i + 1], hv.y, a1);
            a2 = fmaf(wr[i + 2], hv.z, a2);
            a3 = fmaf(wr[i + 3], hv.w, a3);
        }
        if (j < H3) sh_g[j] = ((a0 + a1) + (a2 + a3)) + bj;
        __syncthreads();
        if (j < H) {
            const float r = gst_sigmoid(g_r + sh_g[j]);
            const float z = gst_sigmoid(g_z + sh_g[H + j]);
            const float c = tanhf(g_n + r * sh_g[2 * H + j]);
            sh_h[j] = (1.0f - z) * c + z * sh_h[j];
        }
        __syncthreads();
    }
    if (ref_embs && j < H) ref_embs[(int64_t)b * H + j] = sh_h[j];

    // style tokens: q = W_q h + b_q; per head softmax_k(q_h . K[k]_h / sqrt(dk)) . V_h; linear_out
    const int dk = d / heads;
    gst_matvec(wq, bq, sh_h, sh_q, d, H, wave, nwaves, lane);
    __syncthreads();
    const float rs = 1.0f / sqrtf((float)dk);
    for (int e = j; e < heads * tokens; e += blockDim.x) {
        const int hh = e / tokens, kk = e % tokens;
        const float* kr = Kt + (int64_t)kk * d + hh * dk;
        float a = 0.f;
        for (int i = 0; i < dk; ++i) a = fmaf(sh_q[hh * dk + i], kr[i], a);
        sh_p[e] = a * rs;
    }
    __syncthreads();
    for (int hh = j; hh < heads; hh += blockDim.x) {
        float* pr = sh_p + hh * tokens;
        float m = pr[0];
        for (int kk = 1; kk < tokens; ++kk) m = fmaxf(m, pr[kk]);
        float sum = 0.f;
        for (int kk = 0; kk < tokens; ++kk) {
            pr[kk] = expf(pr[kk] - m);
            sum += pr[kk];
        }
        for (int kk = 0; kk < tokens; ++kk) pr[kk] = pr[kk] / sum;
    }
    __syncthreads();
    for (int o = j; o < d; o += blockDim.x) {
        const float* pr = sh_p + (o / dk) * tokens;
        float a = 0.f;
        for (int kk = 0; kk < tokens; ++kk) a = fmaf(pr[kk], Vt[(int64_t)kk * d + o], a);
        sh_c[o] = a;
    }
    __syncthreads();
    gst_matvec(wo, bo, sh_c, style + (int64_t)b * d, d, d, wave, nwaves, lane);
}

extern "C" int a3t_gst_gru_stl(const float* gi, const float* w_hh, const float* b_hh, const int32_t* lens, const float* w_q,
                               const float* b_q, const float* k_tok, const float* v_tok, const float* w_out, const float* b_out,
                               float* ref_embs, float* style, int B, int T, int H, int d, int heads, int tokens, void* stream) {
    if (B <= 0 || T <= 0 || H <= 0 || H > GST_MAXH || d <= 0 || d > GST_MAXD || heads <= 0 || tokens <= 0 || d % heads != 0 ||
        heads * tokens > GST_MAXS)
        return A3T_EINVAL;
    const int threads = (3 * H + 63) / 64 * 64;
    hipLaunchKernelGGL(gst_gru_stl_kernel, dim3(B), dim3(threads), 0, (hipStream_t)stream, gi, w_hh, b_hh, lens, w_q, b_q,
                       k_tok, v_tok, w_out, b_out, ref_embs, style, T, H, d, heads, tokens);
    return (int)hipGetLastError();
}

// hs [B][T][d] += style [S][d] row (rows ? rows[b] : S == 1 ? 0 : b)
__global__ __launch_bounds__(256) void gst_add_style_kernel(float* __restrict__ hs, const float* __restrict__ style,
                                                            const int32_t* __restrict__ rows, int64_t total, int64_t Td, int d,
                                                            int S) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int b = (int)(idx / Td);
    int r = rows ? rows[b] : (S == 1 ? 0 : b);
    r = min(max(r, 0), S - 1);
    hs[idx] += style[(int64_t)r * d + idx % d];
}

extern "C" int a3t_gst_add_style(float* hs, const float* style, const int32_t* rows, int B, int T, int d, int S, void* stream) {
    if (B <= 0 || T <= 0 || d <= 0 || S <= 0 || (!rows && S != 1 && S != B)) return A3T_EINVAL;
    const int64_t total = (int64_t)B * T * d;
    if ((total + 255) / 256 > 0x7fffffff) return A3T_EINVAL;
    hipLaunchKernelGGL(gst_add_style_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, hs, style,
                       rows, total, (int64_t)T * d, d, S);
    return (int)hipGetLastError();
}
