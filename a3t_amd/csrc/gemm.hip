// gemm.hip -- the one dense-contraction kernel family of the A3T path (gfx950 / MI355X).
//
// Covers torch.nn.Linear, Conv1d-as-implicit-im2col (FFN k=3, postnet k=5, PWG dilated k=3),
// the attention bmm's and every data / weight gradient of those (NT, NN, TN operand layouts).
// Three arithmetic modes:
//   * A3T_F32  : v_mfma_f32_32x32x2_f32  -- exact fp32 (bitwise an fmaf chain), the parity path
//   * A3T_BF16 : v_mfma_f32_32x32x16_bf16 -- bf16 operands staged through LDS, fp32 accumulate
//   * A3T_BF16X3 : fp32 operands split into (hi, lo) bf16 pairs in the loader, three bf16 MFMAs per product
// Tiling is wave64-native: 256 threads = 4 waves in a 2x2 arrangement, each wave owns a 64x64
// output sub-tile = 2x2 MFMA 32x32 accumulators (64 AGPR-class registers), block tile 128x128.
// Operands are register-staged (global -> VGPR -> LDS) so the loader can do the im2col row
// shift / utterance-boundary zeroing, the fp32->bf16 conversion and the transposing store for
// reduction-strided operands; LDS is double buffered, one barrier per K-tile.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/a3t_hip.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

#include "gemm_common.h"

#include <stdio.h>
#include <stdlib.h>
static thread_local char g_last_kernel[128] = "";
void a3t_note_kernel(const char* name) { snprintf(g_last_kernel, sizeof(g_last_kernel), "%s", name); }
extern "C" const char* a3t_gemm_last_kernel(void) { return g_last_kernel; }

// =============================================================================================
// fp32 MFMA kernel: LDS tiles are k-major ([BK][BM+4]) so a lane's single-float fragment read is
// conflict free (lanes 0-31 -> 32 consecutive rows, lanes 32-63 -> next k).
// =============================================================================================
template <bool AK, bool BKC, bool VEC>
__global__ __launch_bounds__(256) void gemm_f32_kernel(GP p) {
    constexpr int BM = 128, BN = 128, BK = 16, LD = 132;
    __shared__ __attribute__((aligned(16))) float smem[4 * BK * LD];
    float(*As)[BK][LD] = (float(*)[BK][LD])smem;
    float(*Bs)[BK][LD] = (float(*)[BK][LD])(smem + 2 * BK * LD);

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int tn = blockIdx.x % p.tiles_n, tm = blockIdx.x / p.tiles_n;
    const int ks = blockIdx.y % p.splitk, bz = blockIdx.y / p.splitk;
    const int z0 = bz / p.batch_inner, z1 = bz % p.batch_inner;
    const float* A = (const float*)p.A + z0 * p.a_bs0 + z1 * p.a_bs1;
    const float* B = (const float*)p.B + z0 * p.b_bs0 + z1 * p.b_bs1;
    const int64_t zoff = z0 * p.c_bs0 + z1 * p.c_bs1;

    const int ktiles = (p.K + BK - 1) / BK;
    const int per = (ktiles + p.splitk - 1) / p.splitk;
    const int kt0 = ks * per, kt1 = min(ktiles, kt0 + per);
    if (kt0 >= kt1) return;

    float4 ra[2], rb[2];
    int a_t[2];
    if (AK) {
        for (int ps = 0; ps < 2; ++ps) {
            int m = tm * BM + (tid >> 2) + ps * 64;
            a_t[ps] = (p.taps > 1) ? (m % p.Tseq) : 0;
        }
    }

    auto load_tiles = [&](int k0) {
        if (AK) {
            const int r = tid >> 2, kq = tid & 3;
#pragma unroll
            for (int ps = 0; ps < 2; ++ps) {
                int m = tm * BM + r + ps * 64, kg = k0 + kq * 4;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (m < p.M) {
                    if (VEC) {
                        if (kg < p.K) {
                            const float* q = a_ptr_k(p, A, m, a_t[ps], kg);
                            if (q) v = *(const float4*)q;
                        }
                    } else {
                        float t[4];
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            t[i] = 0.f;
                            if (kg + i < p.K) {
                                const float* q = a_ptr_k(p, A, m, a_t[ps], kg + i);
                                if (q) t[i] = *q;
                            }
                        }
                        v = make_float4(t[0], t[1], t[2], t[3]);
                    }
                }
                ra[ps] = v;
            }
        } else {
            const int kr = tid >> 5, mq = tid & 31;
#pragma unroll
            for (int ps = 0; ps < 2; ++ps) {
                int k = k0 + kr + ps * 8, m0 = tm * BM + mq * 4;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (k < p.K) {
                    const float* q = A + (int64_t)k * p.a_cs + m0;
                    if (VEC && m0 + 3 < p.M) {
                        v = *(const float4*)q;
                    } else {
                        if (m0 + 0 < p.M) v.x = q[0];
                        if (m0 + 1 < p.M) v.y = q[1];
                        if (m0 + 2 < p.M) v.z = q[2];
                        if (m0 + 3 < p.M) v.w = q[3];
                    }
                }
                ra[ps] = v;
            }
        }
        if (BKC) {
            const int r = tid >> 2, kq = tid & 3;
#pragma unroll
            for (int ps = 0; ps < 2; ++ps) {
                int n = tn * BN + r + ps * 64, kg = k0 + kq * 4;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (n < p.N) {
                    if (VEC) {
                        if (kg < p.K) {
                            int64_t koff;
                            if (b_koff(p, kg, koff)) v = *(const float4*)(B + (int64_t)n * p.b_rs + koff);
                        }
                    } else {
                        float t[4];
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            t[i] = 0.f;
                            int64_t koff;
                            if (kg + i < p.K && b_koff(p, kg + i, koff)) t[i] = B[(int64_t)n * p.b_rs + koff];
                        }
                        v = make_float4(t[0], t[1], t[2], t[3]);
                    }
                }
                rb[ps] = v;
            }
        } else {
            const int kr = tid >> 5, nq = tid & 31;
#pragma unroll
            for (int ps = 0; ps < 2; ++ps) {
                int k = k0 + kr + ps * 8, n0 = tn * BN + nq * 4;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                int64_t koff;
                if (k < p.K && b_koff(p, k, koff)) {
                    const float* q = B + koff + n0;
                    if (VEC && n0 + 3 < p.N) {
                        v = *(const float4*)q;
                    } else {
                        if (n0 + 0 < p.N) v.x = q[0];
                        if (n0 + 1 < p.N) v.y = q[1];
                        if (n0 + 2 < p.N) v.z = q[2];
                        if (n0 + 3 < p.N) v.w = q[3];
                    }
                }
                rb[ps] = v;
            }
        }
    };
    auto store_tiles = [&](int buf) {
        if (AK) {
            const int r = tid >> 2, kq = tid & 3;
#pragma unroll
            for (int ps = 0; ps < 2; ++ps) {
                As[buf][kq * 4 + 0][r + ps * 64] = ra[ps].x;
                As[buf][kq * 4 + 1][r + ps * 64] = ra[ps].y;
                As[buf][kq * 4 + 2][r + ps * 64] = ra[ps].z;
                As[buf][kq * 4 + 3][r + ps * 64] = ra[ps].w;
            }
        } else {
            const int kr = tid >> 5, mq = tid & 31;
#pragma unroll
            for (int ps = 0; ps < 2; ++ps) *(float4*)&As[buf][kr + ps * 8][mq * 4] = ra[ps];
        }
        if (BKC) {
            const int r = tid >> 2, kq = tid & 3;
#pragma unroll
            for (int ps = 0; ps < 2; ++ps) {
                Bs[buf][kq * 4 + 0][r + ps * 64] = rb[ps].x;
                Bs[buf][kq * 4 + 1][r + ps * 64] = rb[ps].y;
                Bs[buf][kq * 4 + 2][r + ps * 64] = rb[ps].z;
                Bs[buf][kq * 4 + 3][r + ps * 64] = rb[ps].w;
            }
        } else {
            const int kr = tid >> 5, nq = tid & 31;
#pragma unroll
            for (int ps = 0; ps < 2; ++ps) *(float4*)&Bs[buf][kr + ps * 8][nq * 4] = rb[ps];
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int wm = (w >> 1) * 64, wn = (w & 1) * 64, lr = lane & 31, lk = lane >> 5;
    load_tiles(kt0 * BK);
    store_tiles(0);
    __syncthreads();
    int buf = 0;
    for (int kt = kt0; kt < kt1; ++kt) {
        const bool more = (kt + 1 < kt1);
        if (more) load_tiles((kt + 1) * BK);
#pragma unroll
        for (int kk = 0; kk < BK / 2; ++kk) {
            float a0 = As[buf][kk * 2 + lk][wm + lr], a1 = As[buf][kk * 2 + lk][wm + 32 + lr];
            float b0 = Bs[buf][kk * 2 + lk][wn + lr], b1 = Bs[buf][kk * 2 + lk][wn + 32 + lr];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        if (more) store_tiles(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                int row = tm * BM + wm + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
                int col = tn * BN + wn + j * 32 + lr;
                epilogue_store(p, zoff, row, col, acc[i][j][r], ks);
            }
}

// =============================================================================================
// bf16 MFMA kernel: LDS tiles are row-major bf16 [128][BK+8] (k contiguous, 80-byte rows ->
// conflict-free ds_read_b128 fragment reads); sources may be fp32 (converted in the loader) or bf16.
// =============================================================================================
template <typename TA, typename TB, bool AK, bool BKC>
__global__ __launch_bounds__(256) void gemm_bf16_kernel(GP p) {
    constexpr int BM = 128, BN = 128, BK = 32, LD = 40;
    __shared__ __attribute__((aligned(16))) unsigned short smem[4 * BM * LD];
    unsigned short(*As)[BM][LD] = (unsigned short(*)[BM][LD])smem;
    unsigned short(*Bs)[BN][LD] = (unsigned short(*)[BN][LD])(smem + 2 * BM * LD);

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int tn = blockIdx.x % p.tiles_n, tm = blockIdx.x / p.tiles_n;
    const int ks = blockIdx.y % p.splitk, bz = blockIdx.y / p.splitk;
    const int z0 = bz / p.batch_inner, z1 = bz % p.batch_inner;
    const TA* A = (const TA*)p.A + z0 * p.a_bs0 + z1 * p.a_bs1;
    const TB* B = (const TB*)p.B + z0 * p.b_bs0 + z1 * p.b_bs1;
    const int64_t zoff = z0 * p.c_bs0 + z1 * p.c_bs1;

    const int ktiles = (p.K + BK - 1) / BK;
    const int per = (ktiles + p.splitk - 1) / p.splitk;
    const int kt0 = ks * per, kt1 = min(ktiles, kt0 + per);
    if (kt0 >= kt1) return;

    // staged registers: k-contig: 2 chunks of 8 bf16 (uint4); row-contig: 4x4 micro tile -> 4 x uint2
    uint4 sa[2], sb[2];
    int a_t[2];
    if (AK) {
        for (int ps = 0; ps < 2; ++ps) {
            int m = tm * BM + (tid >> 2) + ps * 64;
            a_t[ps] = (p.taps > 1) ? (m % p.Tseq) : 0;
        }
    }
    auto pack8 = [](const float* f) {
        uint4 u;
        u.x = io_pack2(f[0], f[1]);
        u.y = io_pack2(f[2], f[3]);
        u.z = io_pack2(f[4], f[5]);
        u.w = io_pack2(f[6], f[7]);
        return u;
    };
    auto load8 = [&](const float* q) {  // 8 consecutive fp32 -> 8 bf16
        float4 v0 = *(const float4*)q, v1 = *(const float4*)(q + 4);
        float f[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
        return pack8(f);
    };
    auto load8h = [&](const unsigned short* q) { return *(const uint4*)q; };

    auto load_k = [&](auto* base, bool isA, int row, int kg, int tpos, uint4& out) {
        out = make_uint4(0, 0, 0, 0);
        if (isA) {
            if (row < p.M && kg < p.K) {
                auto* q = a_ptr_k(p, base, row, tpos, kg);
                if (q) {
                    if constexpr (sizeof(*base) == 4)
                        out = load8((const float*)q);
                    else
                        out = load8h((const unsigned short*)q);
                }
            }
        } else {
            int64_t koff;
            if (row < p.N && kg < p.K && b_koff(p, kg, koff)) {
                auto* q = base + (int64_t)row * p.b_rs + koff;
                if constexpr (sizeof(*base) == 4)
                    out = load8((const float*)q);
                else
                    out = load8h((const unsigned short*)q);
            }
        }
    };
    // row-contiguous operand: 4 rows x 4 k micro tile, transposed in registers
    auto load_r = [&](auto* base, bool isA, int r0, int rmax, int k0, uint4& o01, uint4& o23) {
        float v[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int k = k0 + i;
            v[i][0] = v[i][1] = v[i][2] = v[i][3] = 0.f;
            int64_t koff;
            bool ok = k < p.K;
            if (isA)
                koff = (int64_t)k * p.a_cs;
            else
                ok = ok && b_koff(p, k, koff);
            if (ok && r0 < rmax) {
                auto* q = base + koff + r0;
                if (r0 + 3 < rmax) {
                    if constexpr (sizeof(*base) == 4) {
                        float4 t = *(const float4*)q;
                        v[i][0] = t.x, v[i][1] = t.y, v[i][2] = t.z, v[i][3] = t.w;
                    } else {
                        uint2 t = *(const uint2*)q;
                        v[i][0] = bf2f(t.x & 0xffff), v[i][1] = bf2f(t.x >> 16);
                        v[i][2] = bf2f(t.y & 0xffff), v[i][3] = bf2f(t.y >> 16);
                    }
                } else {
                    for (int j = 0; j < 4; ++j)
                        if (r0 + j < rmax) v[i][j] = ldf(q + j);
                }
            }
        }
        // row j gets (v[0][j], v[1][j], v[2][j], v[3][j]) = 4 consecutive k
        o01.x = io_pack2(v[0][0], v[1][0]);
        o01.y = io_pack2(v[2][0], v[3][0]);
        o01.z = io_pack2(v[0][1], v[1][1]);
        o01.w = io_pack2(v[2][1], v[3][1]);
        o23.x = io_pack2(v[0][2], v[1][2]);
        o23.y = io_pack2(v[2][2], v[3][2]);
        o23.z = io_pack2(v[0][3], v[1][3]);
        o23.w = io_pack2(v[2][3], v[3][3]);
    };

    auto load_tiles = [&](int k0) {
        if (AK) {
            const int r = tid >> 2, kq = tid & 3;
#pragma unroll
            for (int ps = 0; ps < 2; ++ps) load_k(A, true, tm * BM + r + ps * 64, k0 + kq * 8, a_t[ps], sa[ps]);
        } else {
            load_r(A, true, tm * BM + (tid & 31) * 4, p.M, k0 + (tid >> 5) * 4, sa[0], sa[1]);
        }
        if (BKC) {
            const int r = tid >> 2, kq = tid & 3;
#pragma unroll
            for (int ps = 0; ps < 2; ++ps) load_k(B, false, tn * BN + r + ps * 64, k0 + kq * 8, 0, sb[ps]);
        } else {
            load_r(B, false, tn * BN + (tid & 31) * 4, p.N, k0 + (tid >> 5) * 4, sb[0], sb[1]);
        }
    };
    auto store_tiles = [&](int buf) {
        if (AK) {
            const int r = tid >> 2, kq = tid & 3;
#pragma unroll
            for (int ps = 0; ps < 2; ++ps) *(uint4*)&As[buf][r + ps * 64][kq * 8] = sa[ps];
        } else {
            const int m0 = (tid & 31) * 4, kq = tid >> 5;
            *(uint2*)&As[buf][m0 + 0][kq * 4] = make_uint2(sa[0].x, sa[0].y);
            *(uint2*)&As[buf][m0 + 1][kq * 4] = make_uint2(sa[0].z, sa[0].w);
            *(uint2*)&As[buf][m0 + 2][kq * 4] = make_uint2(sa[1].x, sa[1].y);
            *(uint2*)&As[buf][m0 + 3][kq * 4] = make_uint2(sa[1].z, sa[1].w);
        }
        if (BKC) {
            const int r = tid >> 2, kq = tid & 3;
#pragma unroll
            for (int ps = 0; ps < 2; ++ps) *(uint4*)&Bs[buf][r + ps * 64][kq * 8] = sb[ps];
        } else {
            const int n0 = (tid & 31) * 4, kq = tid >> 5;
            *(uint2*)&Bs[buf][n0 + 0][kq * 4] = make_uint2(sb[0].x, sb[0].y);
            *(uint2*)&Bs[buf][n0 + 1][kq * 4] = make_uint2(sb[0].z, sb[0].w);
            *(uint2*)&Bs[buf][n0 + 2][kq * 4] = make_uint2(sb[1].x, sb[1].y);
            *(uint2*)&Bs[buf][n0 + 3][kq * 4] = make_uint2(sb[1].z, sb[1].w);
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int wm = (w >> 1) * 64, wn = (w & 1) * 64, lr = lane & 31, lk = lane >> 5;
    load_tiles(kt0 * BK);
    store_tiles(0);
    __syncthreads();
    int buf = 0;
    for (int kt = kt0; kt < kt1; ++kt) {
        const bool more = (kt + 1 < kt1);
        if (more) load_tiles((kt + 1) * BK);
#pragma unroll
        for (int kk = 0; kk < BK / 16; ++kk) {
            bf16x8 a0 = *(const bf16x8*)&As[buf][wm + lr][kk * 16 + lk * 8];
            bf16x8 a1 = *(const bf16x8*)&As[buf][wm + 32 + lr][kk * 16 + lk * 8];
            bf16x8 b0 = *(const bf16x8*)&Bs[buf][wn + lr][kk * 16 + lk * 8];
            bf16x8 b1 = *(const bf16x8*)&Bs[buf][wn + 32 + lr][kk * 16 + lk * 8];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc[1][1], 0, 0, 0);
        }
        if (more) store_tiles(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                int row = tm * BM + wm + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
                int col = tn * BN + wn + j * 32 + lr;
                epilogue_store(p, zoff, row, col, acc[i][j][r], ks);
            }
}

// =============================================================================================
// bf16x3 kernel (A3T_BF16X3): fp32 operands, each split on the way to LDS into hi = bf16(x) and lo = bf16(x - hi)
// (round to nearest even, 16 significand bits kept: |x - hi - lo| <= 2^-16 |x|; the split of split_bf16_kernel), and
//     a b ~= lo_a hi_b + hi_a lo_b + hi_a hi_b
// as three v_mfma_f32_32x32x16_bf16 into one fp32 accumulator.  Every product is exact; dropped are lo_a lo_b and the two split
// residuals, each <= 2^-16 |a||b| (bf16 operands: 2^-8).
// Addressing, tiling, split K and epilogue are the bf16 kernel's above; LDS holds a hi and a lo image of both operands in two
// buffers: 2 x 4 x 128 x 40 x 2 B = 80 KiB, dynamic (half a CU's LDS: two workgroups per CU, one barrier per K-tile).
// =============================================================================================
constexpr int X3_LDS = 2 * 4 * 128 * 40 * 2;

// (hi, lo) of two fp32 values, packed like io_pack2.  Where hi is not finite lo is 0 (x - hi would be NaN, or the opposite
// infinity for a finite x that rounds to one).  The outputs such an operand reaches are non-finite as in fp32, but not always
// the same non-finite value: inf x lo_b is NaN where lo_b is 0 and has lo_b's sign elsewhere.
__device__ __forceinline__ void x3_split2(float x0, float x1, unsigned int& hi, unsigned int& lo) {
    hi = io_pack2(x0, x1);
    lo = io_pack2(x0 - __uint_as_float(hi << 16), x1 - __uint_as_float(hi & 0xffff0000u));
    if ((hi & 0x00007f80u) == 0x00007f80u) lo &= 0xffff0000u;
    if ((hi & 0x7f800000u) == 0x7f800000u) lo &= 0x0000ffffu;
}

template <bool AK, bool BKC>
__global__ __launch_bounds__(256) void gemm_bf16x3_kernel(GP p) {
    constexpr int BM = 128, BN = 128, BK = 32, LD = 40;
    extern __shared__ __attribute__((aligned(16))) unsigned char x3_smem[];
    // [buffer][A hi | A lo | B hi | B lo][128][LD]
    unsigned short(*Ts)[4][BM][LD] = (unsigned short(*)[4][BM][LD])x3_smem;

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int tn = blockIdx.x % p.tiles_n, tm = blockIdx.x / p.tiles_n;
    const int ks = blockIdx.y % p.splitk, bz = blockIdx.y / p.splitk;
    const int z0 = bz / p.batch_inner, z1 = bz % p.batch_inner;
    const float* A = (const float*)p.A + z0 * p.a_bs0 + z1 * p.a_bs1;
    const float* B = (const float*)p.B + z0 * p.b_bs0 + z1 * p.b_bs1;
    const int64_t zoff = z0 * p.c_bs0 + z1 * p.c_bs1;

    const int ktiles = (p.K + BK - 1) / BK;
    const int per = (ktiles + p.splitk - 1) / p.splitk;
    const int kt0 = ks * per, kt1 = min(ktiles, kt0 + per);
    if (kt0 >= kt1) return;

    // staged registers, [0] the hi and [1] the lo image: k-contig: 2 chunks of 8 bf16 (uint4); row-contig: 4x4 micro tile -> 4 x uint2
    uint4 sa[2][2], sb[2][2];
    int a_t[2];
    if (AK) {
        for (int ps = 0; ps < 2; ++ps) {
            int m = tm * BM + (tid >> 2) + ps * 64;
            a_t[ps] = (p.taps > 1) ? (m % p.Tseq) : 0;
        }
    }
    auto load8 = [&](const float* q, uint4& h, uint4& l) {  // 8 consecutive fp32 -> 8 (hi, lo)
        const float4 v0 = *(const float4*)q, v1 = *(const float4*)(q + 4);
        x3_split2(v0.x, v0.y, h.x, l.x);
        x3_split2(v0.z, v0.w, h.y, l.y);
        x3_split2(v1.x, v1.y, h.z, l.z);
        x3_split2(v1.z, v1.w, h.w, l.w);
    };
    auto load_k = [&](const float* base, bool isA, int row, int kg, int tpos, uint4& h, uint4& l) {
        h = l = make_uint4(0, 0, 0, 0);
        if (isA) {
            if (row < p.M && kg < p.K) {
                const float* q = a_ptr_k(p, base, row, tpos, kg);
                if (q) load8(q, h, l);
            }
        } else {
            int64_t koff;
            if (row < p.N && kg < p.K && b_koff(p, kg, koff)) load8(base + (int64_t)row * p.b_rs + koff, h, l);
        }
    };
    // row-contiguous operand: 4 rows x 4 k micro tile, transposed in registers
    auto load_r = [&](const float* base, bool isA, int r0, int rmax, int k0, uint4* h, uint4* l) {
        float v[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int k = k0 + i;
            v[i][0] = v[i][1] = v[i][2] = v[i][3] = 0.f;
            int64_t koff;
            bool ok = k < p.K;
            if (isA)
                koff = (int64_t)k * p.a_cs;
            else
                ok = ok && b_koff(p, k, koff);
            if (ok && r0 < rmax) {
                const float* q = base + koff + r0;
                if (r0 + 3 < rmax) {
                    float4 t = *(const float4*)q;
                    v[i][0] = t.x, v[i][1] = t.y, v[i][2] = t.z, v[i][3] = t.w;
                } else {
                    for (int j = 0; j < 4; ++j)
                        if (r0 + j < rmax) v[i][j] = q[j];
                }
            }
        }
        // row j gets (v[0][j], v[1][j], v[2][j], v[3][j]) = 4 consecutive k
        x3_split2(v[0][0], v[1][0], h[0].x, l[0].x);
        x3_split2(v[2][0], v[3][0], h[0].y, l[0].y);
        x3_split2(v[0][1], v[1][1], h[0].z, l[0].z);
        x3_split2(v[2][1], v[3][1], h[0].w, l[0].w);
        x3_split2(v[0][2], v[1][2], h[1].x, l[1].x);
        x3_split2(v[2][2], v[3][2], h[1].y, l[1].y);
        x3_split2(v[0][3], v[1][3], h[1].z, l[1].z);
        x3_split2(v[2][3], v[3][3], h[1].w, l[1].w);
    };

    auto load_tiles = [&](int k0) {
        if (AK) {
            const int r = tid >> 2, kq = tid & 3;
#pragma unroll
            for (int ps = 0; ps < 2; ++ps) load_k(A, true, tm * BM + r + ps * 64, k0 + kq * 8, a_t[ps], sa[0][ps], sa[1][ps]);
        } else {
            load_r(A, true, tm * BM + (tid & 31) * 4, p.M, k0 + (tid >> 5) * 4, sa[0], sa[1]);
        }
        if (BKC) {
            const int r = tid >> 2, kq = tid & 3;
#pragma unroll
            for (int ps = 0; ps < 2; ++ps) load_k(B, false, tn * BN + r + ps * 64, k0 + kq * 8, 0, sb[0][ps], sb[1][ps]);
        } else {
            load_r(B, false, tn * BN + (tid & 31) * 4, p.N, k0 + (tid >> 5) * 4, sb[0], sb[1]);
        }
    };
    // one operand's staged registers -> its hi (img) and lo (img + 1) images
    auto store_op = [&](int buf, int img, bool kcontig, const uint4 (*s)[2]) {
#pragma unroll
        for (int hl = 0; hl < 2; ++hl) {
            unsigned short(*T)[LD] = Ts[buf][img + hl];
            if (kcontig) {
                const int r = tid >> 2, kq = tid & 3;
#pragma unroll
                for (int ps = 0; ps < 2; ++ps) *(uint4*)&T[r + ps * 64][kq * 8] = s[hl][ps];
            } else {
                const int r0 = (tid & 31) * 4, kq = tid >> 5;
                *(uint2*)&T[r0 + 0][kq * 4] = make_uint2(s[hl][0].x, s[hl][0].y);
                *(uint2*)&T[r0 + 1][kq * 4] = make_uint2(s[hl][0].z, s[hl][0].w);
                *(uint2*)&T[r0 + 2][kq * 4] = make_uint2(s[hl][1].x, s[hl][1].y);
                *(uint2*)&T[r0 + 3][kq * 4] = make_uint2(s[hl][1].z, s[hl][1].w);
            }
        }
    };
    auto store_tiles = [&](int buf) {
        store_op(buf, 0, AK, sa);
        store_op(buf, 2, BKC, sb);
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int wm = (w >> 1) * 64, wn = (w & 1) * 64, lr = lane & 31, lk = lane >> 5;
    load_tiles(kt0 * BK);
    store_tiles(0);
    __syncthreads();
    int buf = 0;
    for (int kt = kt0; kt < kt1; ++kt) {
        const bool more = (kt + 1 < kt1);
        if (more) load_tiles((kt + 1) * BK);
#pragma unroll
        for (int kk = 0; kk < BK / 16; ++kk) {
            bf16x8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                ah[i] = *(const bf16x8*)&Ts[buf][0][wm + i * 32 + lr][kk * 16 + lk * 8];
                al[i] = *(const bf16x8*)&Ts[buf][1][wm + i * 32 + lr][kk * 16 + lk * 8];
                bh[i] = *(const bf16x8*)&Ts[buf][2][wn + i * 32 + lr][kk * 16 + lk * 8];
                bl[i] = *(const bf16x8*)&Ts[buf][3][wn + i * 32 + lr][kk * 16 + lk * 8];
            }
            // the two cross terms first, hi x hi last: the small terms are not added to an already large sum
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
        }
        if (more) store_tiles(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                int row = tm * BM + wm + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
                int col = tn * BN + wn + j * 32 + lr;
                epilogue_store(p, zoff, row, col, acc[i][j][r], ks);
            }
}

// =============================================================================================
// host: what the GEMM files share (switches), the plan (route table) and the launch
// =============================================================================================
// Kernel-selection switches, read from the environment on first use.  8P / PN / TT / 8P_TN / 8P_TN3: 0 never, 1 whenever legal,
// 2 (default) the kernel's cost model (PN 3: the cost model for N = 384 only).  STAGES: LDS stages of the 128-row kernel, 1 / 2
// forced (unset: by grid size).  WN3: its 192-column tiles, 0 never, 2 always (unset: where they waste fewer padded columns).
static int sw_mode(const char* e) { return e ? atoi(e) : 2; }
static int sw_stages(const char* e) { return e ? (e[0] == '1' ? 1 : 2) : 0; }
static int sw_wn3(const char* e) { return e ? (e[0] == '0' ? 0 : 2) : 1; }
static const struct {
    const char* env;
    int (*read)(const char*);
} k_switch[] = {{"A3T_GEMM_8P", sw_mode},     {"A3T_GEMM_PN", sw_mode},         {"A3T_GEMM_TT", sw_mode}, {"A3T_GEMM_8P_TN", sw_mode},
                {"A3T_GEMM_8P_TN3", sw_mode}, {"A3T_GEMM_STAGES", sw_stages}, {"A3T_GEMM_WN3", sw_wn3}};
static int g_switch[] = {-1, -1, -1, -1, -1, -1, -1};
int gemm_switch(int s) {
    if (g_switch[s] < 0) g_switch[s] = k_switch[s].read(getenv(k_switch[s].env));
    return g_switch[s];
}
int gemm_switch_set(int s, int v) {
    const int old = gemm_switch(s);
    g_switch[s] = v;
    return old;
}
extern "C" int a3t_gemm_8p_mode(int mode) { return gemm_switch_set(SW_8P, mode); }
extern "C" int a3t_gemm_pn_mode(int mode) { return gemm_switch_set(SW_PN, mode); }
extern "C" int a3t_gemm_tt_mode(int mode) { return gemm_switch_set(SW_TT, mode); }
extern "C" int a3t_gemm_tn3_mode(int mode) { return gemm_switch_set(SW_8P_TN3, mode); }

GP gemm_rep(int M, int N, int K, int taps, int flags, int keep_layout) {
    static float dummy[4] __attribute__((aligned(16)));
    GP p = {};
    p.M = M, p.N = N, p.K = K, p.taps = taps < 1 ? 1 : taps, p.Kc = K / p.taps, p.b_ts = p.Kc;
    p.a_rs = p.Kc, p.a_cs = 1, p.b_rs = K, p.b_cs = 1, p.c_rs = N, p.splitk = 1, p.accumulate = A3T_ACC_STORE;
    p.Tseq = 1, p.colsum_slots = 1, p.c_dtype = (flags & 16) ? A3T_F32 : A3T_BF16;
    if (flags & 1) p.bias = dummy, p.act = A3T_ACT_RELU;
    if (flags & 2) p.drop_inv = 1.25f;
    if (flags & 4) p.keep_out = (unsigned char*)dummy;
    if (flags & 8) p.keep_in = (const unsigned char*)dummy, p.keep_layout = keep_layout;
    if (flags & 32) p.colsum = dummy;
    if (flags & 64) p.S = dummy, p.s_dtype = A3T_BF16;
    return p;
}

static inline bool al(const void* p, int b) { return ((uintptr_t)p % b) == 0; }
static inline bool m4(int64_t v, int m) { return (v % m) == 0; }

// The direct-to-LDS bf16 kernels: their alignment contract, then the routes in order -- 384-column panel, 8-phase (TN: 128 x 384
// or 256 x 256 tiles), streaming, 128-row.  false: none of them takes the descriptor.
static bool glds_routes(GP& p, int batch, bool AK, bool BKC, GemmPlan* pl) {
    const bool aview = (p.a_unaligned & 1) != 0;     // A: a 2-byte aligned strided view (the loaders only do pointer arithmetic)
    bool ok = (aview || al(p.A, 16)) && al(p.B, 16) && m4(p.a_bs0, 8) && m4(p.a_bs1, 8) && m4(p.b_bs0, 8) && m4(p.b_bs1, 8);
    if (AK || BKC) ok = ok && m4(p.Kc, 8);      // (16-byte granules run along k only for k-contiguous operands)
    if (AK)
        ok = ok && (aview || m4(p.a_rs, 8)) && m4(p.K, 8);
    else
        ok = ok && (aview || m4(p.a_cs, 8)) && m4(p.M, 8);
    if (BKC)
        ok = ok && m4(p.b_rs, 8) && m4(p.K, 8) && m4(p.b_ts, 8);
    else
        ok = ok && m4(p.b_cs, 8) && m4(p.b_ts, 8) && m4(p.N, 8);
    if (!AK && p.taps > 1) ok = ok && ((p.N / p.taps) % 128 == 0) && (p.N % p.taps == 0) && p.Tseq > 0;
    if (!ok || (p.colsum && p.accumulate == A3T_ACC_ATOMIC)) return false;
    // vector epilogue contract: 4-column groups never straddle N and every C/R/S/bias access is aligned
    const int epi_vec = (p.N % 4 == 0) && (p.c_rs % 4 == 0) && (p.c_bs0 % 4 == 0) && (p.c_bs1 % 4 == 0) && al(p.C, 16) &&
                        (!p.R || al(p.R, 16)) && (!p.S || al(p.S, 8)) && (!p.bias || al(p.bias, 16));
    if (p.colsum && !epi_vec) return false;
    const bool keep = p.keep_in || p.keep_out;
    const bool keep_rm = p.keep_layout == 1 && keep;      // row-major nibble image: vector epilogue / panel kernel
    if (keep_rm && (!epi_vec || p.c_rs != p.N || batch != 1 || p.splitk != 1 || p.accumulate != A3T_ACC_STORE || p.N % 8 ||
                    (p.keep_out && p.R) || (p.keep_in && p.S)))
        return false;
    if (p.a_signmask && (AK || BKC || p.taps > 1 || p.kshift_mode)) return false;   // (fragment-register pass of the m-contiguous A only)
    p.epi_vec = epi_vec;
    const int ly = (AK && BKC) ? L_NT : (AK ? L_NN : L_TN);
    // N = 384 outputs: one 160-row panel x all columns per workgroup
    if (!(p.keep_out || (p.keep_in && !keep_rm) || p.a_signmask || p.A2 || aview) && pn_plan(p, batch, ly, pl)) return true;
    if (!p.a_signmask && !keep_rm && !p.A2 && !aview) {   // many-tile k-contiguous GEMMs and token reductions: the 8-phase kernels
        if (g8_plan(p, batch, ly, pl)) return true;
        if (keep) return false;                           // (the tile-major keep-bit image exists in the 8-phase kernel only)
    }
    // score-sized A operand x [k][n] slices (attention backward): one streaming workgroup per CU
    if (!BKC && !keep && !aview && tt_plan(p, batch, AK ? L_NN : L_TN, pl)) return true;
    if (p.A2) return false;        // two products in one launch: the streaming kernel only (a3t_gemm_tt_supported)
    glds_plan(p, batch, ly, pl);
    return true;
}

// The register-staged kernels (legacy bf16, bf16x3): k-contiguous operands are read in chunks of 8 elements, row-contiguous in
// chunks of 4
static bool staged_aligned(const GP& p, bool AK, bool BKC) {
    bool ok = al(p.A, 16) && al(p.B, 16);
    if (AK)
        ok = ok && m4(p.a_rs, 8) && m4(p.K, 8) && m4(p.Kc, 8) && m4(p.a_bs0, 8) && m4(p.a_bs1, 8);
    else
        ok = ok && m4(p.a_cs, 4) && m4(p.a_bs0, 4) && m4(p.a_bs1, 4);
    if (BKC)
        ok = ok && m4(p.b_rs, 8) && m4(p.K, 8) && m4(p.Kc, 8) && m4(p.b_ts, 8) && m4(p.b_bs0, 8) && m4(p.b_bs1, 8);
    else
        ok = ok && m4(p.b_cs, 4) && m4(p.b_ts, 4) && m4(p.b_bs0, 4) && m4(p.b_bs1, 4);
    return ok;
}

// Validates the descriptor, fills the kernel argument and walks the routes: fused conv weight gradient, fp32 (and bf16x3 on fp32
// operands), the direct-to-LDS bf16 kernels, the legacy bf16 kernel.  Returns 0 or A3T_EINVAL; launches nothing.
static int gemm_plan(const a3t_gemm_desc* d, GP* gp, GemmPlan* pl) {
    if (!d || !d->A || !d->B || !d->C || d->M <= 0 || d->N <= 0 || d->K <= 0) return A3T_EINVAL;
    GP& p = *gp;
    p = GP{};
    *pl = GemmPlan{};
    p.A = d->A, p.B = d->B, p.C = d->C, p.bias = d->bias, p.R = d->R, p.S = d->S;
    p.M = d->M, p.N = d->N, p.K = d->K;
    p.taps = d->taps < 1 ? 1 : d->taps;
    const bool wgrad_fused = (d->taps > 1 && d->a_cs != 1);   // TN conv weight gradient, columns = (tap, c)
    if (!wgrad_fused && (p.K % p.taps)) return A3T_EINVAL;
    p.Kc = wgrad_fused ? p.K : p.K / p.taps;
    p.a_rs = d->a_rs, p.a_cs = d->a_cs, p.b_rs = d->b_rs, p.b_cs = d->b_cs, p.b_ts = d->b_ts, p.c_rs = d->c_rs;
    int batch = d->batch < 1 ? 1 : d->batch;
    p.batch_inner = d->batch_inner < 1 ? 1 : d->batch_inner;
    p.a_bs0 = d->a_bs0, p.a_bs1 = d->a_bs1, p.b_bs0 = d->b_bs0, p.b_bs1 = d->b_bs1;
    p.c_bs0 = d->c_bs0, p.c_bs1 = d->c_bs1;
    p.pad = d->pad, p.dil = d->dil < 1 ? 1 : d->dil, p.Tseq = d->Tseq, p.kshift = d->kshift;
    p.kshift_mode = (p.taps == 1 && d->Tseq > 0) ? 1 : 0;
    if (p.taps > 1 && p.Tseq <= 0) return A3T_EINVAL;
    p.alpha = d->alpha, p.act = d->act, p.accumulate = d->accumulate;
    p.sole_writer = 0;
    if (p.accumulate == A3T_ACC_SOLE) p.accumulate = A3T_ACC_ATOMIC, p.sole_writer = 1;
    p.splitk = d->splitk < 1 ? 1 : d->splitk;
    if (p.splitk > 1 && p.accumulate != A3T_ACC_ATOMIC) return A3T_EINVAL;
    // every split runs the epilogue on its partial sum: only its linear terms (mask, dropout, alpha) commute with the split
    if (p.splitk > 1 && p.act != A3T_ACT_NONE) return A3T_EINVAL;
    p.c_dtype = d->c_dtype;
    p.s_dtype = d->s_dtype;
    p.colsum = d->colsum, p.colsum_bs1 = d->colsum_bs1, p.colsum_scale = d->colsum_scale;
    p.colsum_slots = d->colsum_slots > 1 ? d->colsum_slots : 1, p.colsum_ss = d->colsum_ss;
    if (d->drop_p < 0.f || d->drop_p >= 1.f) return A3T_EINVAL;
    p.drop_key = d->drop_key;
    p.drop_thr = (unsigned int)((double)d->drop_p * 4294967296.0);
    p.drop_inv = d->drop_p > 0.f ? 1.f / (1.f - d->drop_p) : 0.f;
    p.keep_out = (unsigned char*)d->keep_out, p.keep_in = (const unsigned char*)d->keep_in;
    p.a_signmask = d->a_signmask ? 1 : 0;
    p.A2 = d->A2, p.B2 = d->B2, p.b2_cs = d->b2_cs, p.b2_bs0 = d->b2_bs0, p.b2_bs1 = d->b2_bs1, p.colsum2 = d->colsum2;
    p.a2_rs = d->a2_rs, p.a_unaligned = d->a_unaligned;
    if ((p.A2 == nullptr) != (p.B2 == nullptr) || (!p.A2 && (p.colsum2 || p.a2_rs || (p.a_unaligned & 2))) || (p.a_unaligned & ~3)) return A3T_EINVAL;
    if ((p.a_unaligned & 1) && (d->compute != A3T_BF16 || d->a_dtype != A3T_BF16 || d->b_dtype != A3T_BF16 || p.taps > 1 || d->Tseq > 0 ||
                                ((uintptr_t)p.A & 1)))
        return A3T_EINVAL;
    p.keep_layout = (p.keep_out || p.keep_in) ? d->keep_layout : 0;
    if (p.keep_layout != 0 && p.keep_layout != 1) return A3T_EINVAL;
    const bool keep = p.keep_out || p.keep_in;
    if (keep && (d->compute != A3T_BF16 || d->a_dtype != A3T_BF16 || d->b_dtype != A3T_BF16)) return A3T_EINVAL;
    // bf16 C accumulates only by plain read-modify-write (A3T_ACC_ADD, one launch per element at a time): no bf16 atomics
    if (p.c_dtype == A3T_BF16 && p.accumulate != A3T_ACC_STORE && (p.accumulate != A3T_ACC_ADD || p.splitk > 1)) return A3T_EINVAL;
    const bool AK = (d->a_cs == 1), BKC = (d->b_cs == 1);
    if (!AK && d->a_rs != 1) return A3T_EINVAL;
    if (!BKC && d->b_rs != 1) return A3T_EINVAL;
    p.tiles_n = (p.N + 127) / 128;
    if (p.taps > 1 && !AK) {  // fused conv weight gradient: only the direct-to-LDS bf16 kernels implement it
        if (d->compute != A3T_BF16 || d->a_dtype != A3T_BF16 || d->b_dtype != A3T_BF16 || d->b_cs == 1 || p.a_signmask || p.A2) return A3T_EINVAL;
        return glds_routes(p, batch, false, false, pl) ? 0 : A3T_EINVAL;
    }
    if (!AK && BKC) return A3T_EINVAL;         // (TT layout is never needed on this path)
    const int tiles_m = (p.M + 127) / 128;
    const dim3 grid((unsigned)(p.tiles_n * tiles_m), (unsigned)(batch * p.splitk));

    if (d->compute == A3T_F32 || d->compute == A3T_BF16X3) {
        if (d->a_dtype != A3T_F32 || d->b_dtype != A3T_F32 || d->colsum || p.a_signmask || p.A2) return A3T_EINVAL;
        // bf16x3 takes exactly what fp32 takes: the three-product kernel inside the register-staged loaders' alignment
        // contract, the (more exact) fp32 kernel everywhere else
        if (d->compute == A3T_BF16X3 && staged_aligned(p, AK, BKC)) {
            pl->route = GR_BF16X3, pl->ak = AK, pl->bkc = BKC, pl->grid = grid;
            snprintf(pl->name, sizeof(pl->name), "gemm_bf16x3_kernel<%s, %s>", tf(AK), tf(BKC));
            return 0;
        }
        bool vec = al(p.A, 16) && al(p.B, 16) && m4(p.a_bs0, 4) && m4(p.a_bs1, 4) && m4(p.b_bs0, 4) && m4(p.b_bs1, 4);
        if (AK)
            vec = vec && m4(p.a_rs, 4) && m4(p.K, 4) && m4(p.Kc, 4);
        else
            vec = vec && m4(p.a_cs, 4);
        if (BKC)
            vec = vec && m4(p.b_rs, 4) && m4(p.K, 4) && m4(p.Kc, 4) && m4(p.b_ts, 4);
        else
            vec = vec && m4(p.b_cs, 4) && m4(p.b_ts, 4);
        pl->route = GR_F32, pl->ak = AK, pl->bkc = BKC, pl->vec = vec, pl->grid = grid;
        snprintf(pl->name, sizeof(pl->name), "gemm_f32_kernel<%s, %s, %s>", tf(AK), tf(BKC), tf(vec));
        return 0;
    }
    if (d->compute != A3T_BF16) return A3T_EINVAL;
    if (d->a_dtype == A3T_BF16 && d->b_dtype == A3T_BF16 && glds_routes(p, batch, AK, BKC, pl)) return 0;
    if (keep || p.a_signmask || p.A2 || p.a_unaligned) return A3T_EINVAL;        // keep-bit images only exist in the 8-phase kernel, sign masks in the direct-to-LDS TN kernels
    if (d->colsum) return A3T_EINVAL;   // fused column sums live in the direct-to-LDS kernel's epilogue
    if (!staged_aligned(p, AK, BKC)) return A3T_EINVAL;
    pl->route = GR_BF16_LEGACY, pl->ak = AK, pl->bkc = BKC, pl->grid = grid;
    pl->a_f32 = d->a_dtype == A3T_F32, pl->b_f32 = d->b_dtype == A3T_F32;
    snprintf(pl->name, sizeof(pl->name), "gemm_bf16_kernel<%s, %s, %s, %s>", pl->a_f32 ? "float" : "unsigned short",
             pl->b_f32 ? "float" : "unsigned short", tf(AK), tf(BKC));
    return 0;
}

static int f32_launch(const GP& p, const GemmPlan& pl, hipStream_t stream) {
#define LAUNCH_F32(ak, bk)                                                                          \
    do {                                                                                            \
        if (pl.vec)                                                                                 \
            hipLaunchKernelGGL((gemm_f32_kernel<ak, bk, true>), pl.grid, dim3(256), 0, stream, p);  \
        else                                                                                        \
            hipLaunchKernelGGL((gemm_f32_kernel<ak, bk, false>), pl.grid, dim3(256), 0, stream, p); \
    } while (0)
    if (pl.ak && pl.bkc)
        LAUNCH_F32(true, true);
    else if (pl.ak)
        LAUNCH_F32(true, false);
    else
        LAUNCH_F32(false, false);
#undef LAUNCH_F32
    return (int)hipGetLastError();
}

static int legacy_launch(const GP& p, const GemmPlan& pl, hipStream_t stream) {
#define LAUNCH_BF(TA, TB)                                                                                   \
    do {                                                                                                    \
        if (pl.ak && pl.bkc)                                                                                \
            hipLaunchKernelGGL((gemm_bf16_kernel<TA, TB, true, true>), pl.grid, dim3(256), 0, stream, p);   \
        else if (pl.ak)                                                                                     \
            hipLaunchKernelGGL((gemm_bf16_kernel<TA, TB, true, false>), pl.grid, dim3(256), 0, stream, p);  \
        else                                                                                                \
            hipLaunchKernelGGL((gemm_bf16_kernel<TA, TB, false, false>), pl.grid, dim3(256), 0, stream, p); \
    } while (0)
    if (pl.a_f32 && pl.b_f32)
        LAUNCH_BF(float, float);
    else if (pl.a_f32)
        LAUNCH_BF(float, unsigned short);
    else if (pl.b_f32)
        LAUNCH_BF(unsigned short, float);
    else
        LAUNCH_BF(unsigned short, unsigned short);
#undef LAUNCH_BF
    return (int)hipGetLastError();
}

// The 80 KiB are granted per kernel and per device, so at every launch, like the direct-to-LDS kernels' (gemm_bf16.hip): a
// process that drives a second GPU must not launch there without the raised limit.
static int x3_launch(const GP& p, const GemmPlan& pl, hipStream_t stream) {
#define LAUNCH_X3(ak, bk)                                                                                                   \
    do {                                                                                                                    \
        const hipError_t opt_in =                                                                                           \
            hipFuncSetAttribute((const void*)gemm_bf16x3_kernel<ak, bk>, hipFuncAttributeMaxDynamicSharedMemorySize, X3_LDS); \
        if (opt_in != hipSuccess) return (int)opt_in;                                                                       \
        hipLaunchKernelGGL((gemm_bf16x3_kernel<ak, bk>), pl.grid, dim3(256), X3_LDS, stream, p);                            \
    } while (0)
    if (pl.ak && pl.bkc)
        LAUNCH_X3(true, true);
    else if (pl.ak)
        LAUNCH_X3(true, false);
    else
        LAUNCH_X3(false, false);
#undef LAUNCH_X3
    return (int)hipGetLastError();
}

extern "C" int a3t_gemm(const a3t_gemm_desc* d, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GP p;
    GemmPlan pl;
    const int rc = gemm_plan(d, &p, &pl);
    if (rc) return rc;
    int r;
    switch (pl.route) {
        case GR_F32: r = f32_launch(p, pl, stream); break;
        case GR_BF16_LEGACY: r = legacy_launch(p, pl, stream); break;
        case GR_BF16X3: r = x3_launch(p, pl, stream); break;
        case GR_GLDS_128: r = glds_launch(p, pl, stream); break;
        case GR_PN: r = pn_launch(p, pl, stream); break;
        case GR_TT: r = tt_launch(p, pl, stream); break;
        default: r = g8_launch(p, pl, stream); break;   // GR_G8, GR_G8_TN, GR_G8_TN3
    }
    a3t_note_kernel(pl.name);
    return r;
}

extern "C" int a3t_gemm_plan(const a3t_gemm_desc* d, char* name, int len) {
    GP p;
    GemmPlan pl;
    const int rc = gemm_plan(d, &p, &pl);
    if (!rc && name && len > 0) snprintf(name, (size_t)len, "%s", pl.name);
    return rc;
}
