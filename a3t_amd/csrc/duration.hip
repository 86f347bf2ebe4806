// duration.hip -- the FastSpeech2 duration head for gfx950 (espnet/nets/pytorch_backend/fastspeech/duration_predictor.py):
// the last LayerNorm of the predictor, Linear(C -> 1) and the inference transform in one launch, one wave64 per row
// (the idiom of norm_reduce.hip's ln_fwd_kernel); and the row L2 normalisation of the x-vector (F.normalize,
// espnet2/tts/fastspeech2/fastspeech2.py:784-808).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/a3t_hip.h"

#define WAVE 64
#define DUR_MAXV 8  // C <= 512

__device__ __forceinline__ float dur_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}

// Row m of z [M][C]: y = LayerNorm(z[m]) (biased variance), x = y . w + bias, logd[m] = x,
// frames[m] = max(rint(exp(x) - offset), 0)  (torch.round: half to even; rintf in the default rounding mode).
template <int V>
__global__ __launch_bounds__(256) void duration_head_kernel(const float* __restrict__ z, const float* __restrict__ g,
                                                            const float* __restrict__ b, const float* __restrict__ w,
                                                            const float* __restrict__ bias, float* __restrict__ logd,
                                                            int64_t* __restrict__ frames, int M, int C, float eps,
                                                            float offset) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int row = blockIdx.x * 4 + wv;
    if (row >= M) return;
    const float* zr = z + (int64_t)row * C;
    float v[V];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const int c = lane + i * 64;
        v[i] = (c < C) ? zr[c] : 0.f;
        s += v[i];
    }
    const float mu = dur_wave_sum(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const int c = lane + i * 64;
        const float d = (c < C) ? (v[i] - mu) : 0.f;
        q += d * d;
    }
    const float rs = 1.0f / sqrtf(dur_wave_sum(q) / (float)C + eps);
    float dot = 0.f;
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const int c = lane + i * 64;
        if (c < C) dot += ((v[i] - mu) * rs * g[c] + b[c]) * w[c];
    }
    const float x = dur_wave_sum(dot) + bias[0];
    if (lane == 0) {
        logd[row] = x;
        const float f = rintf(expf(x) - offset);
        frames[row] = (int64_t)fmaxf(f, 0.f);
    }
}

extern "C" int a3t_duration_head(const float* z, const float* gamma, const float* beta, const float* w,
                                 const float* bias, float* logd, int64_t* frames, int M, int C, float eps, float offset,
                                 void* stream) {
    if (M <= 0 || C <= 0 || C > 64 * DUR_MAXV) return A3T_EINVAL;
    const int V = (C + 63) / 64;
#define CALL(NV)                                                                                                       \
    hipLaunchKernelGGL(duration_head_kernel<NV>, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, z, gamma, beta, \
                       w, bias, logd, frames, M, C, eps, offset)
    switch (V) {
        case 1: CALL(1); break;
        case 2: CALL(2); break;
        case 3: CALL(3); break;
        case 4: CALL(4); break;
        case 5: CALL(5); break;
        case 6: CALL(6); break;
        case 7: CALL(7); break;
        default: CALL(8); break;
    }
#undef CALL
    return (int)hipGetLastError();
}

// y[r] = x[r] / max(||x[r]||_2, eps): one wave per row, any n.
__global__ __launch_bounds__(256) void l2_normalize_kernel(const float* __restrict__ x, float* __restrict__ y, int B,
                                                           int n, float eps) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int row = blockIdx.x * 4 + wv;
    if (row >= B) return;
    const float* xr = x + (int64_t)row * n;
    float q = 0.f;
    for (int c = lane; c < n; c += 64) q += xr[c] * xr[c];
    const float nrm = fmaxf(sqrtf(dur_wave_sum(q)), eps);
    for (int c = lane; c < n; c += 64) y[(int64_t)row * n + c] = xr[c] / nrm;
}

extern "C" int a3t_l2_normalize(const float* x, float* y, int B, int n, float eps, void* stream) {
    if (B <= 0 || n <= 0) return A3T_EINVAL;
    hipLaunchKernelGGL(l2_normalize_kernel, dim3((B + 3) / 4), dim3(256), 0, (hipStream_t)stream, x, y, B, n, eps);
    return (int)hipGetLastError();
}
