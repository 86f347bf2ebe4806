// ragged_rows.hip -- length-aware twins of three row kernels for padded [B][Tmax] batches whose rows have their own lengths
// (lens [B] int32 on the device), fp32, forward only: the batched FastSpeech2 duration model.  Row b is computed exactly as
// if it had been passed alone at length n = lens[b]:
//   * LayerNorm whose rows t >= n are stored as 0 (what the k-tap convolution behind it must read there);
//   * GLU + depthwise Conv1d whose taps read 0 for t >= n (and across the row boundary) and which stores 0 for t >= n;
//   * the rel-pos softmax with the legacy rel_shift (attention.py:145-165) taken at n in the place of T, keys j >= n at
//     probability 0 and query rows i >= n written as 0.
// One wave64 per row as in norm_reduce.hip / convmod_attn.hip; 16-byte accesses where the channel count allows.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/a3t_hip.h"

#define WAVE 64

__device__ __forceinline__ float rg_wsum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}
__device__ __forceinline__ float rg_wmax(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, WAVE));
    return v;
}
__device__ __forceinline__ int rg_len(const int32_t* __restrict__ lens, int b, int T) {
    const int n = lens[b];
    return n < 0 ? 0 : (n > T ? T : n);      // a length outside 0..T cannot push an index out of the row
}

// ------------------------------------------------------------------------------------------
// LayerNorm.  The arithmetic of ln_fwd_kernel / ln_fwd_vec_kernel (norm_reduce.hip), operation for operation, so a valid row
// has the bits the plain kernel gives it.
// ------------------------------------------------------------------------------------------
#define RG_LN_MAXV 24  // D <= 1536

template <int V>
__global__ __launch_bounds__(256) void ln_fwd_ragged_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                            const float* __restrict__ b, float* __restrict__ y,
                                                            float* __restrict__ mean, float* __restrict__ rstd,
                                                            const int32_t* __restrict__ lens, int M, int T, int D,
                                                            float eps) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int row = blockIdx.x * 4 + wv;
    if (row >= M) return;
    const int bb = row / T, t = row - bb * T;
    float* yr = y + (int64_t)row * D;
    if (t >= rg_len(lens, bb, T)) {      // (wave-uniform)
        for (int c = lane; c < D; c += 64) yr[c] = 0.f;
        if (lane == 0 && mean) mean[row] = 0.f, rstd[row] = 0.f;
        return;
    }
    const float* xr = x + (int64_t)row * D;
    float v[V];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < V; ++i) {
        int c = lane + i * 64;
        v[i] = (c < D) ? xr[c] : 0.f;
        s += v[i];
    }
    const float mu = rg_wsum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < V; ++i) {
        int c = lane + i * 64;
        float dlt = (c < D) ? (v[i] - mu) : 0.f;
        q += dlt * dlt;
    }
    const float var = rg_wsum(q) / (float)D;
    const float rs = 1.0f / sqrtf(var + eps);
#pragma unroll
    for (int i = 0; i < V; ++i) {
        int c = lane + i * 64;
        if (c < D) yr[c] = (v[i] - mu) * rs * g[c] + b[c];
    }
    if (lane == 0 && mean) mean[row] = mu, rstd[row] = rs;
}

// D % 128 == 0: half a wave per row, NQ float4 per lane (D = 128 * NQ)
template <int NQ>
__global__ __launch_bounds__(256) void ln_fwd_ragged_vec_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                                const float* __restrict__ b, float* __restrict__ y,
                                                                float* __restrict__ mean, float* __restrict__ rstd,
                                                                const int32_t* __restrict__ lens, int M, int T, int D,
                                                                float eps) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, hl = lane & 31, half = lane >> 5;
    const int row = (blockIdx.x * 4 + wv) * 2 + half;
    const bool ok = row < M;
    const int rr = ok ? row : 0;
    const int bb = rr / T, t = rr - bb * T;
    const bool live = t < rg_len(lens, bb, T);
    const int64_t ro = (int64_t)rr * D;
    float4 v[NQ];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        v[i] = live ? *(const float4*)(x + ro + (hl + 32 * i) * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        s += v[i].x + v[i].y + v[i].z + v[i].w;
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) s += __shfl_xor(s, o, WAVE);
    const float mu = s / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        const float a = v[i].x - mu, c = v[i].y - mu, d = v[i].z - mu, e = v[i].w - mu;
        q += a * a + c * c + d * d + e * e;
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) q += __shfl_xor(q, o, WAVE);
    const float rs = 1.0f / sqrtf(q / (float)D + eps);
    if (!ok) return;
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        const int c = (hl + 32 * i) * 4;
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (live) {
            const float4 gg = *(const float4*)(g + c), bv = *(const float4*)(b + c);
            o = make_float4((v[i].x - mu) * rs * gg.x + bv.x, (v[i].y - mu) * rs * gg.y + bv.y,
                            (v[i].z - mu) * rs * gg.z + bv.z, (v[i].w - mu) * rs * gg.w + bv.w);
        }
        *(float4*)(y + ro + c) = o;
    }
    if (hl == 0 && mean) {
        mean[row] = live ? mu : 0.f;
        rstd[row] = live ? rs : 0.f;
    }
}

static inline bool rg_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

extern "C" int a3t_layernorm_fwd_ragged(const float* x, const float* gamma, const float* beta, float* y, float* mean,
                                        float* rstd, const int32_t* lens, int B, int T, int D, float eps, void* stream) {
    if (B <= 0 || T <= 0 || D <= 0 || D > 64 * RG_LN_MAXV || !lens || (mean == nullptr) != (rstd == nullptr) ||
        (int64_t)B * T > 0x7fffffff)
        return A3T_EINVAL;
    const int M = B * T;
    if (D % 128 == 0 && D <= 512 && rg_al16(x) && rg_al16(y) && rg_al16(gamma) && rg_al16(beta)) {
#define VCALL(NQ)                                                                                                      \
    hipLaunchKernelGGL(ln_fwd_ragged_vec_kernel<NQ>, dim3((M + 7) / 8), dim3(256), 0, (hipStream_t)stream, x, gamma, \
                       beta, y, mean, rstd, lens, M, T, D, eps)
        if (D == 128) VCALL(1);
        else if (D == 256) VCALL(2);
        else if (D == 384) VCALL(3);
        else VCALL(4);
#undef VCALL
        return (int)hipGetLastError();
    }
#define CALL(V)                                                                                                     \
    hipLaunchKernelGGL(ln_fwd_ragged_kernel<V>, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, x, gamma, beta, \
                       y, mean, rstd, lens, M, T, D, eps)
    if (D <= 64) CALL(1);
    else if (D <= 128) CALL(2);
    else if (D <= 256) CALL(4);
    else if (D <= 384) CALL(6);
    else if (D <= 512) CALL(8);
    else CALL(RG_LN_MAXV);
#undef CALL
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// GLU + depthwise conv: glu_dwconv_fwd_kernel (convmod_attn.hip) with the row's own length in the place of Tseq for what a tap
// may read; block = 64 channels x 4 row lanes, time tile of 64 rows, the GLU'd window in LDS.  A tile that lies behind the
// row's length only stores zeros.
// ------------------------------------------------------------------------------------------
#define RG_TT 64
#define RG_KMAX 31

__device__ __forceinline__ float rg_sigm(float v) { return 1.f / (1.f + __expf(-v)); }

template <int KT>
__global__ __launch_bounds__(256) void glu_dwconv_fwd_ragged_kernel(const float* __restrict__ g,
                                                                    const float* __restrict__ wdw,
                                                                    const float* __restrict__ bdw, float* __restrict__ glu,
                                                                    float* __restrict__ z, const int32_t* __restrict__ lens,
                                                                    int C, int K, int Tseq, int tiles_t) {
    __shared__ float win[RG_TT + RG_KMAX - 1][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + tx;
    const int b = blockIdx.y / tiles_t, t0 = (blockIdx.y % tiles_t) * RG_TT;
    const int n = rg_len(lens, b, Tseq);
    const int pad = (K - 1) / 2;
    const int64_t mbase = (int64_t)b * Tseq;
    if (t0 >= n) {      // (block-uniform) nothing valid in this tile
        if (c < C)
            for (int r = ty; r < RG_TT && t0 + r < Tseq; r += 4) {
                glu[(mbase + t0 + r) * (int64_t)C + c] = 0.f;
                z[(mbase + t0 + r) * (int64_t)C + c] = 0.f;
            }
        return;
    }
    const int rows = RG_TT + K - 1;
    for (int rb = ty; rb < rows; rb += 32) {
        float ga[8], gb[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int r = rb + 4 * u, t = t0 - pad + r;
            const bool ok = (c < C) && (r < rows) && (t >= 0) && (t < n);
            const int64_t gi = ok ? (mbase + t) * (int64_t)(2 * C) + c : 0;
            ga[u] = ok ? g[gi] : 0.f;
            gb[u] = ok ? g[gi + C] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int r = rb + 4 * u, t = t0 - pad + r;
            const bool ok = (c < C) && (r < rows) && (t >= 0) && (t < n);
            const float v = ok ? ga[u] * rg_sigm(gb[u]) : 0.f;
            if ((c < C) && r >= pad && r < pad + RG_TT && t < Tseq) glu[(mbase + t) * (int64_t)C + c] = v;
            if (r < rows) win[r][tx] = v;
        }
    }
    __syncthreads();
    if (c >= C) return;
    float w[KT];
#pragma unroll
    for (int k = 0; k < KT; ++k) w[k] = (k < K) ? wdw[(int64_t)c * K + k] : 0.f;
    const float bias = bdw[c];
    if (K == KT) {   // register-blocked: 4 consecutive time steps share one (KT+3)-value window
        for (int r0 = ty * 4; r0 < RG_TT; r0 += 16) {
            float v[KT + 3];
#pragma unroll
            for (int j = 0; j < KT + 3; ++j) v[j] = win[r0 + j][tx];
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) {
                float acc = bias;
#pragma unroll
                for (int k = 0; k < KT; ++k) acc += w[k] * v[tt + k];
                int t = t0 + r0 + tt;
                if (t < Tseq) z[(mbase + t) * (int64_t)C + c] = t < n ? acc : 0.f;
            }
        }
        return;
    }
    for (int r = ty; r < RG_TT; r += 4) {
        int t = t0 + r;
        if (t >= Tseq) break;
        float acc = bias;
#pragma unroll
        for (int k = 0; k < KT; ++k)
            if (k < K) acc += w[k] * win[r + k][tx];
        z[(mbase + t) * (int64_t)C + c] = t < n ? acc : 0.f;
    }
}

extern "C" int a3t_glu_dwconv_fwd_ragged(const float* g, const float* wdw, const float* bdw, float* glu, float* z,
                                         const int32_t* lens, int B, int Tseq, int C, int K, void* stream) {
    if (K > RG_KMAX || K <= 0 || (K & 1) == 0 || Tseq <= 0 || B <= 0 || C <= 0 || !lens) return A3T_EINVAL;
    const int tiles_t = (Tseq + RG_TT - 1) / RG_TT;
    if ((int64_t)B * tiles_t > 65535) return A3T_EINVAL;      // grid.y
    dim3 grid((C + 63) / 64, B * tiles_t);
#define CALL(KT)                                                                                                       \
    hipLaunchKernelGGL(glu_dwconv_fwd_ragged_kernel<KT>, grid, dim3(256), 0, (hipStream_t)stream, g, wdw, bdw, glu, z, \
                       lens, C, K, Tseq, tiles_t)
    if (K <= 7) CALL(7);
    else if (K <= 15) CALL(15);
    else CALL(RG_KMAX);
#undef CALL
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// Rel-pos softmax.  One wave per (z, i) row of the padded [T][T] score block; bd is the compact (q+v) P^T matrix of the padded
// launch (row stride T).  For i, j < n the row alone would read  j <= i : bd[i][n-1-i+j],  j == i+1 : 0,
// j > i+1 : bd[i+1][j-i-2]  (i + 1 < n there, since j < n).  NV > 0: the row lives in NV registers per lane (T <= 64 * NV);
// NV == 0: three passes for very long rows.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ float rg_score(const float* __restrict__ ar, const float* __restrict__ bz, int T, int n, int i,
                                          int j, float scale) {
    float s = ar[j];
    if (j <= i) s += bz[(int64_t)i * T + (n - 1 - i + j)];
    else if (j > i + 1) s += bz[(int64_t)(i + 1) * T + (j - i - 2)];
    return s * scale;
}

template <int NV>
__global__ __launch_bounds__(256) void relpos_softmax_fwd_ragged_kernel(const float* __restrict__ ac,
                                                                        const float* __restrict__ bd,
                                                                        const int32_t* __restrict__ lens,
                                                                        float* __restrict__ probs, int H, int T,
                                                                        int64_t ac_bs, int64_t bd_bs, int64_t p_bs,
                                                                        float scale, int64_t nrows) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= nrows) return;
    const int64_t zz = row / T;
    const int i = (int)(row - zz * T);
    const int n = rg_len(lens, (int)(zz / H), T);
    float* pr = probs + zz * p_bs + (int64_t)i * T;
    if (i >= n) {      // (wave-uniform) a padded query row: probs @ V must read zeros there
        for (int j = lane; j < T; j += 64) pr[j] = 0.f;
        return;
    }
    const float* ar = ac + zz * ac_bs + (int64_t)i * T;
    const float* bz = bd + zz * bd_bs;
    const float NEG = -3.4028235e38f;
    if (NV > 0) {
        float v[NV > 0 ? NV : 1];
        float mx = NEG;
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            const int j = lane + q * 64;
            v[q] = (j < n) ? rg_score(ar, bz, T, n, i, j, scale) : NEG;
            mx = fmaxf(mx, v[q]);
        }
        mx = rg_wmax(mx);
        float s = 0.f;
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            const int j = lane + q * 64;
            v[q] = (j < n) ? expf(v[q] - mx) : 0.f;
            s += v[q];
        }
        s = rg_wsum(s);
        const float inv_s = s > 0.f ? 1.f / s : 0.f;
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            const int j = lane + q * 64;
            if (j < T) pr[j] = v[q] * inv_s;
        }
        return;
    }
    float mx = NEG;
    for (int j = lane; j < n; j += 64) mx = fmaxf(mx, rg_score(ar, bz, T, n, i, j, scale));
    mx = rg_wmax(mx);
    float s = 0.f;
    for (int j = lane; j < n; j += 64) s += expf(rg_score(ar, bz, T, n, i, j, scale) - mx);
    s = rg_wsum(s);
    const float inv_s = s > 0.f ? 1.f / s : 0.f;
    for (int j = lane; j < T; j += 64) pr[j] = (j < n) ? expf(rg_score(ar, bz, T, n, i, j, scale) - mx) * inv_s : 0.f;
}

extern "C" int a3t_relpos_softmax_fwd_ragged(const void* ac, const void* bd, int scores_dtype, const int32_t* lens,
                                             void* probs, int probs_dtype, int B, int H, int T, int64_t ac_bs,
                                             int64_t bd_bs, int64_t p_bs, float scale, void* stream) {
    if (scores_dtype != A3T_F32 || probs_dtype != A3T_F32 || !lens || B <= 0 || H <= 0 || T <= 0) return A3T_EINVAL;
    const int64_t tt = (int64_t)T * T;
    if (ac_bs < tt || bd_bs < tt || p_bs < tt) return A3T_EINVAL;
    const int64_t nrows = (int64_t)B * H * T;
    if ((nrows + 3) / 4 > 0x7fffffff) return A3T_EINVAL;
#define CALL(NV)                                                                                                     \
    hipLaunchKernelGGL(relpos_softmax_fwd_ragged_kernel<NV>, dim3((unsigned)((nrows + 3) / 4)), dim3(256), 0,        \
                       (hipStream_t)stream, (const float*)ac, (const float*)bd, lens, (float*)probs, H, T, ac_bs, bd_bs, \
                       p_bs, scale, nrows)
    if (T <= 128) CALL(2);
    else if (T <= 256) CALL(4);
    else if (T <= 512) CALL(8);
    else if (T <= 1152) CALL(18);
    else if (T <= 2048) CALL(32);
    else CALL(0);
#undef CALL
    return (int)hipGetLastError();
}
