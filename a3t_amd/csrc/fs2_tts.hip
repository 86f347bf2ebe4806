// fs2_tts.hip -- what FastSpeech2's text-to-mel inference needs behind the duration predictor, for gfx950
// (espnet2/tts/fastspeech2/fastspeech2.py:662-699, espnet/nets/pytorch_backend/fastspeech/length_regulator.py,
// espnet2/layers/global_mvn.py): the pitch / energy embeddings added to the encoder output, the length regulator as an
// offset scan and a gather, and the last step of the mel (postnet residual, GlobalMVN inverse).  fp32, forward only.
// All of them take padded [B][T] rows with per-row lengths (int32 on the device, NULL: every row is full) and compute
// row b as if it had been passed alone; nothing behind a row's length is read.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/a3t_hip.h"

#define WAVE 64
#define FS2_MAXK 9
#define FS2_MAXDUR (1 << 18)  // per-token saturation of the offset scan: 5000 tokens of it still fit an int32
#define FS2_TILE 64           // output frames per workgroup of length_expand

__device__ __forceinline__ int fs2_row_len(const int32_t* lens, int b, int T) {
    if (!lens) return T;
    const int n = lens[b];
    return n < 0 ? 0 : (n > T ? T : n);
}

// hs[b][t][:] += bp + be + sum_j pitch[b][t + j - (kp-1)/2] wp[j][:] + sum_j energy[b][t + j - (ke-1)/2] we[j][:], t < n_b.
// One lane per four channels of one row; wp / we are [k][d] (taps outermost) so that a tap is one 16-byte load.
__global__ __launch_bounds__(256) void variance_embed_kernel(float* __restrict__ hs, const float* __restrict__ pitch,
                                                             const float* __restrict__ energy,
                                                             const float* __restrict__ wp, const float* __restrict__ bp,
                                                             const float* __restrict__ we, const float* __restrict__ be,
                                                             const int32_t* __restrict__ lens, int B, int T, int d4,
                                                             int kp, int ke) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = i / d4;
    if (row >= (int64_t)B * T) return;
    const int c = (int)(i - row * d4);
    const int b = (int)(row / T), t = (int)(row - (int64_t)b * T);
    const int n = fs2_row_len(lens, b, T);
    if (t >= n) return;
    const float4* wp4 = reinterpret_cast<const float4*>(wp);
    const float4* we4 = reinterpret_cast<const float4*>(we);
    float4 acc = reinterpret_cast<const float4*>(be)[c];
    const float* er = energy + (int64_t)b * T;
    for (int j = 0; j < ke; ++j) {
        const int tt = t + j - (ke - 1) / 2;
        if (tt < 0 || tt >= n) continue;
        const float v = er[tt];
        const float4 w = we4[(int64_t)j * d4 + c];
        acc.x += v * w.x, acc.y += v * w.y, acc.z += v * w.z, acc.w += v * w.w;
    }
    float4 accp = reinterpret_cast<const float4*>(bp)[c];
    const float* pr = pitch + (int64_t)b * T;
    for (int j = 0; j < kp; ++j) {
        const int tt = t + j - (kp - 1) / 2;
        if (tt < 0 || tt >= n) continue;
        const float v = pr[tt];
        const float4 w = wp4[(int64_t)j * d4 + c];
        accp.x += v * w.x, accp.y += v * w.y, accp.z += v * w.z, accp.w += v * w.w;
    }
    float4* h4 = reinterpret_cast<float4*>(hs) + row * d4 + c;
    float4 h = *h4;   // (hs + e_embs) + p_embs, the reference's order
    h.x = (h.x + acc.x) + accp.x, h.y = (h.y + acc.y) + accp.y, h.z = (h.z + acc.z) + accp.z, h.w = (h.w + acc.w) + accp.w;
    *h4 = h;
}

extern "C" int a3t_fs2_variance_embed(float* hs, const float* pitch, const float* energy, const float* wp, const float* bp,
                                      const float* we, const float* be, const int32_t* lens, int B, int T, int d, int kp,
                                      int ke, void* stream) {
    if (B <= 0 || T <= 0 || d <= 0 || d % 4 || kp < 1 || ke < 1 || kp > FS2_MAXK || ke > FS2_MAXK || kp % 2 == 0 ||
        ke % 2 == 0)
        return A3T_EINVAL;
    const int d4 = d / 4;
    const int64_t total = (int64_t)B * T * d4;
    hipLaunchKernelGGL(variance_embed_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, hs,
                       pitch, energy, wp, bp, we, be, lens, B, T, d4, kp, ke);
    return (int)hipGetLastError();
}

// One wave per row: exclusive offsets of the (alpha-scaled) durations, 64 entries per step, the running total carried in a
// register.  Entries behind the row's length count as 0, so offsets[n .. T] all hold the row's frame count.
__global__ __launch_bounds__(WAVE) void length_offsets_kernel(const int64_t* __restrict__ frames,
                                                              const int32_t* __restrict__ lens, float alpha,
                                                              int32_t* __restrict__ offsets, int32_t* __restrict__ frame_lens,
                                                              int64_t* __restrict__ scaled, int T) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int n = fs2_row_len(lens, b, T);
    const int64_t* fr = frames + (int64_t)b * T;
    int32_t* off = offsets + (int64_t)b * (T + 1);
    int carry = 0;
    for (int t0 = 0; t0 < T; t0 += WAVE) {
        const int t = t0 + lane;
        int64_t d64 = (t < n) ? fr[t] : 0;
        d64 = d64 < 0 ? 0 : (d64 > FS2_MAXDUR ? FS2_MAXDUR : d64);
        int d = (int)d64;
        if (alpha != 1.0f)   // torch.round(ds.float() * alpha): one fp32 product, half to even
            d = (int)fminf(fmaxf(rintf((float)d * alpha), 0.f), (float)FS2_MAXDUR);
        int incl = d;
#pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) {
            const int v = __shfl_up(incl, o, WAVE);
            if (lane >= o) incl += v;
        }
        if (t < T) {
            off[t] = carry + incl - d;
            if (scaled) scaled[(int64_t)b * T + t] = (int64_t)d;
        }
        carry += __shfl(incl, WAVE - 1, WAVE);
    }
    if (lane == 0) {
        off[T] = carry;
        frame_lens[b] = carry;
    }
}

extern "C" int a3t_length_offsets(const int64_t* frames, const int32_t* lens, float alpha, int32_t* offsets,
                                  int32_t* frame_lens, int64_t* scaled, int B, int T, void* stream) {
    if (B <= 0 || T <= 0 || !(alpha > 0.f)) return A3T_EINVAL;
    hipLaunchKernelGGL(length_offsets_kernel, dim3(B), dim3(WAVE), 0, (hipStream_t)stream, frames, lens, alpha, offsets,
                       frame_lens, scaled, T);
    return (int)hipGetLastError();
}

// out[b][f][:] = scale * hs[b][tok(f)][:] for f < frame_lens[b], 0 for frame_lens[b] <= f < Fp.  One workgroup per
// FS2_TILE output frames of one row: the row's offsets [n + 1] are staged in LDS, one lane per frame finds the first
// j with offsets[j] > f (tok = j - 1: a token of duration 0 has offsets[t] == offsets[t + 1] and is never found), then all
// lanes copy, four channels each.
__global__ __launch_bounds__(256) void length_expand_kernel(const float* __restrict__ hs, const int32_t* __restrict__ offsets,
                                                            const int32_t* __restrict__ lens,
                                                            const int32_t* __restrict__ frame_lens, float* __restrict__ out,
                                                            int T, int Fp, int d4, float scale) {
    extern __shared__ int32_t fs2_lds[];
    int32_t* off = fs2_lds;            // [T + 1]
    int32_t* tok = fs2_lds + (T + 1);  // [FS2_TILE]
    const int b = blockIdx.y, f0 = blockIdx.x * FS2_TILE, tid = threadIdx.x;
    const int n = fs2_row_len(lens, b, T);
    int F = frame_lens[b];
    F = F < 0 ? 0 : (F > Fp ? Fp : F);
    const int nf = min(FS2_TILE, Fp - f0);
    if (f0 < F) {
        for (int i = tid; i <= n; i += 256) off[i] = offsets[(int64_t)b * (T + 1) + i];
        __syncthreads();
        if (tid < nf && f0 + tid < F) {
            const int f = f0 + tid;
            int lo = 0, hi = n;   // the answer lies in (0, n]: offsets[0] = 0 <= f < F <= offsets[n]
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (off[mid] > f) hi = mid; else lo = mid + 1;
            }
            tok[tid] = max(lo - 1, 0);
        }
        __syncthreads();
    }
    const float4* h4 = reinterpret_cast<const float4*>(hs) + (int64_t)b * T * d4;
    float4* o4 = reinterpret_cast<float4*>(out) + ((int64_t)b * Fp + f0) * d4;
    for (int i = tid; i < nf * d4; i += 256) {
        const int r = i / d4, c = i - r * d4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (f0 + r < F) {
            v = h4[(int64_t)tok[r] * d4 + c];
            v.x *= scale, v.y *= scale, v.z *= scale, v.w *= scale;
        }
        o4[i] = v;
    }
}

extern "C" int a3t_length_expand(const float* hs, const int32_t* offsets, const int32_t* lens, const int32_t* frame_lens,
                                 float* out, int B, int T, int Fp, int d, float scale, void* stream) {
    if (B <= 0 || T <= 0 || Fp <= 0 || d <= 0 || d % 4 || T > 12000) return A3T_EINVAL;
    const size_t lds = (size_t)(T + 1 + FS2_TILE) * sizeof(int32_t);
    hipLaunchKernelGGL(length_expand_kernel, dim3((Fp + FS2_TILE - 1) / FS2_TILE, B), dim3(256), lds, (hipStream_t)stream, hs,
                       offsets, lens, frame_lens, out, T, Fp, d / 4, scale);
    return (int)hipGetLastError();
}

// after = before + post (post NULL: after = before); denorm = after * std + mean (each NULL: that step is left out; denorm
// NULL: not written).  Rows f >= lens[b] of [B][F][C] are written as 0 and not read.
template <typename V>
__device__ __forceinline__ V fs2_fma(V a, V s, V m, bool has_s, bool has_m);
template <>
__device__ __forceinline__ float fs2_fma<float>(float a, float s, float m, bool has_s, bool has_m) {
    if (has_s) a *= s;
    if (has_m) a += m;
    return a;
}
template <>
__device__ __forceinline__ float4 fs2_fma<float4>(float4 a, float4 s, float4 m, bool has_s, bool has_m) {
    if (has_s) a.x *= s.x, a.y *= s.y, a.z *= s.z, a.w *= s.w;
    if (has_m) a.x += m.x, a.y += m.y, a.z += m.z, a.w += m.w;
    return a;
}
__device__ __forceinline__ float fs2_add(float a, float b) { return a + b; }
__device__ __forceinline__ float4 fs2_add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ void fs2_zero(float& a) { a = 0.f; }
__device__ __forceinline__ void fs2_zero(float4& a) { a = make_float4(0.f, 0.f, 0.f, 0.f); }

template <typename V>
__global__ __launch_bounds__(256) void fs2_finish_kernel(const V* __restrict__ before, const V* __restrict__ post,
                                                         const V* __restrict__ mean, const V* __restrict__ std_,
                                                         V* __restrict__ after, V* __restrict__ denorm,
                                                         const int32_t* __restrict__ lens, int B, int F, int Cv) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = i / Cv;
    if (row >= (int64_t)B * F) return;
    const int c = (int)(i - row * Cv);
    const int b = (int)(row / F), f = (int)(row - (int64_t)b * F);
    V a, dn;
    if (f < fs2_row_len(lens, b, F)) {
        a = before[i];
        if (post) a = fs2_add(a, post[i]);
        dn = fs2_fma<V>(a, std_ ? std_[c] : a, mean ? mean[c] : a, std_ != nullptr, mean != nullptr);
    } else {
        fs2_zero(a);
        fs2_zero(dn);
    }
    after[i] = a;
    if (denorm) denorm[i] = dn;
}

extern "C" int a3t_fs2_finish(const float* before, const float* post, const float* mean, const float* std_, float* after,
                              float* denorm, const int32_t* lens, int B, int F, int C, void* stream) {
    if (B <= 0 || F <= 0 || C <= 0) return A3T_EINVAL;
    if (C % 4 == 0) {
        const int64_t total = (int64_t)B * F * (C / 4);
        hipLaunchKernelGGL(fs2_finish_kernel<float4>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                           (const float4*)before, (const float4*)post, (const float4*)mean, (const float4*)std_,
                           (float4*)after, (float4*)denorm, lens, B, F, C / 4);
    } else {
        const int64_t total = (int64_t)B * F * C;
        hipLaunchKernelGGL(fs2_finish_kernel<float>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                           before, post, mean, std_, after, denorm, lens, B, F, C);
    }
    return (int)hipGetLastError();
}

// GlobalMVN forward of a prompt's log-mel: y[m][c] = (x[m][c] - mean[c]) / std[c] (each NULL: that step is left out).
__global__ __launch_bounds__(256) void fs2_mvn_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                      const float* __restrict__ std_, float* __restrict__ y, int64_t total,
                                                      int C) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C);
    float v = x[i];
    if (mean) v -= mean[c];
    if (std_) v /= std_[c];
    y[i] = v;
}

extern "C" int a3t_fs2_mvn(const float* x, const float* mean, const float* std_, float* y, int64_t M, int C, void* stream) {
    if (M <= 0 || C <= 0) return A3T_EINVAL;
    const int64_t total = M * C;
    hipLaunchKernelGGL(fs2_mvn_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, mean, std_,
                       y, total, C);
    return (int)hipGetLastError();
}
