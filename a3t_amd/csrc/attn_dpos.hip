// attn_dpos.hip -- gradient of linear_pos' output in the attention backward (espnet attention.py:190-203 on its way back):
//   dP[r][h dk + n] = sum_b sum_i dbd[b,h][i][r] (q + v)[b T + i][h dk + n]
// as a streaming product + a fold, in the place of the 128-row GEMM with fp32 atomics (32 batch elements per address), the clear of
// its fp32 output and the cast to bf16 that followed.
//
// Kernel A (attn_dpos_stream_kernel) keeps the discipline of gemm_bf16_tt_kernel<ATN = true> (gemm_bf16_tt.hip, whose header explains
// the LDS images and the swizzle): the [k][m] operand in panels of 64 columns read with ds_read_b64_tr_b16, K-tiles of 32 in a ring
// of LDS stages filled by LDS-DMA, every wave issuing the SAME number of 1 KiB pieces per K-tile (DP_Q) so that one counted vmcnt
// wait is right for all of them, one s_barrier per K-tile, pieces past the tile / T / the end of K reading zeros (voffset = OOB;
// the buffer descriptor of a batch element covers exactly that element's extent).  What differs:
//   * a workgroup owns (row tile of r, head, GROUP of batch elements) and walks the K loops of its batch elements back to back
//     into one accumulator set: the ring never drains at the hand-over from b to b + 1, only the descriptor base changes;
//   * the epilogue stores the fp32 accumulators with 16-byte stores into ws[group][T][d]: no atomics, no read-modify-write.
// Kernel B (attn_dpos_fold_kernel): dP16 = bf16(sum_g ws[g]) in ascending g -- the result does not depend on arrival order.
//
// Self-contained on purpose: the loader / fragment code is a restatement of the tt kernel's, not a shared header, so the tt kernels
// stay the objects they were (same code, same registers).
// Geometry (DP_NPA panels of A per stage, DP_STAGES stages) is one compile-time choice: three panels (tiles of <= 192 rows) and six
// stages of 24 KiB.  -DDPOS_NPA / -DDPOS_STAGES build the candidates it was measured against (profiles/attn_dpos.txt,
// tools/experiments/README.md, "linear_pos gradient: tilings"): configs[1] runs 7 tiles of 160 rows x 2 heads x 16 groups of two
// batch elements = 224 workgroups in 70 us (both launches) where the atomic 128-row GEMM + clear + cast took 118.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/a3t_hip.h"
#include "dtype_io.h"
#include "device_cus.h"
#include "mfma_kit.h"

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16;

#ifndef DPOS_NPA
#define DPOS_NPA 3
#endif
#ifndef DPOS_STAGES
#define DPOS_STAGES 6
#endif

namespace {
constexpr int DP_NPA = DPOS_NPA, DP_STAGES = DPOS_STAGES, DP_BK = 32;
constexpr int DP_MAX_ROWS = 64 * DP_NPA;
constexpr int DP_Q = (4 * (DP_NPA + 3) + 7) / 8;        // LDS-DMA pieces per wave and K-tile (4 DP_NPA of A + 12 of B over 8 waves)
constexpr int DP_WA = 4 * DP_NPA / DP_Q;                // waves 0 .. DP_WA-1 request the A pieces, the others the B pieces
constexpr int DP_A_BYTES = DP_NPA * 4096, DP_STAGE = 8 * DP_Q * 1024, DP_LDS = DP_STAGES * DP_STAGE;
static_assert(DP_WA * DP_Q == 4 * DP_NPA && (8 - DP_WA) * DP_Q >= 12, "a wave requests A pieces or B pieces, never both");
static_assert(DP_STAGE - DP_A_BYTES >= 3 * 4096, "three B panels behind the A panels");
static_assert(DP_LDS <= 160 * 1024 && DP_STAGES >= 4 && DP_Q * (DP_STAGES - 1) < 64, "LDS of a CU; the vmcnt field");

struct DposArgs {
    const u16* dbd;
    const u16* qv;
    float* ws;
    int B, H, T, dk, d;
    int64_t a_rs, a_bsb, a_bsh;     // elements
    int TR, ntiles, G;              // rows per tile, row tiles, batch elements per workgroup
};

template <int N>
__device__ __forceinline__ void wait_vm() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

template <int NJ, int NPA, int STAGES>
__global__ __launch_bounds__(512) void attn_dpos_stream_kernel(DposArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int NBI = 2 * NPA;        // 16-row blocks of a wave row at the tallest tile
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = w >> 2, wc = w & 3;
    // workgroup b runs on XCD b % 8: the row tiles of one (group, head) read the same (q + v) rows from one L2
    const int wi = xcd_contiguous(blockIdx.x, gridDim.x);
    const int tm = wi % p.ntiles, zz = wi / p.ntiles;
    const int h = zz % p.H, grp = zz / p.H;
    const int b0 = grp * p.G;
    const int nb = min(p.G, p.B - b0);              // (the last group may be short)
    const int T = p.T, TR = p.TR, dk = p.dk;
    const int m0 = tm * TR;
    const int nbi = TR >> 5;                        // 16-row blocks of a wave row
    const int nkt = (T + DP_BK - 1) / DP_BK;
    const int nkt_all = nb * nkt;

    const bool is_a = w < DP_WA;
    const unsigned a_ld = (unsigned)p.a_rs * 2u, b_ld = (unsigned)p.d * 2u;       // bytes between k-rows
    const unsigned ld = is_a ? a_ld : b_ld;
    const unsigned ext = is_a ? (unsigned)(T - 1) * a_ld + (unsigned)T * 2u : (unsigned)(T - 1) * b_ld + (unsigned)dk * 2u;
    const u16* X0 = is_a ? p.dbd + h * p.a_bsh : p.qv + h * dk;                   // batch element 0 of this head
    const int64_t xbs = is_a ? p.a_bsb : (int64_t)T * p.d;
    const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)LDS_AS(smem));

    // ---- DMA lane geometry ([k][x] image, gemm_bf16_tt.hip): slot s of the wave's operand = panel s >> 2 (64 columns), k-rows
    // 8 (s & 3) .. +7 (128 B each); lane -> k-row 8 (s & 3) + (lane >> 3), position lane & 7 holds source chunk (lane & 7) ^ 2 sw(k-row)
    unsigned voff[DP_Q];
    int kq[DP_Q];
#pragma unroll
    for (int q = 0; q < DP_Q; ++q) {
        const int s = (is_a ? w : w - DP_WA) * DP_Q + q;
        const int r = (s & 3) * 8 + (lane >> 3);
        const int sw = ((r >> 1) & 1) | (((r >> 3) & 1) << 1);
        const int col = (s >> 2) * 64 + (((lane & 7) ^ (sw << 1)) << 3);
        const bool ok = is_a ? (col < TR && m0 + col < T) : (col < dk && col < 64 * NJ);
        voff[q] = ok ? (unsigned)r * ld + (unsigned)((is_a ? m0 : 0) + col) * 2u : OOB;
        kq[q] = r;
    }
    const unsigned kstep = 32u * ld;
    const unsigned dst0 = lds0 + (is_a ? (unsigned)(w * DP_Q) * 1024u : (unsigned)DP_A_BYTES + (unsigned)((w - DP_WA) * DP_Q) * 1024u);
    // issue state: K-tile ik of batch element b0 + ib goes to stage si (all wave-uniform)
    int ik = 0, ib = 0, si = 0;
    auto issue = [&]() __attribute__((always_inline)) {
        const unsigned dst = dst0 + (unsigned)si * (unsigned)DP_STAGE;
        const bool live = ib < nb;       // past the last batch element: zeros (the count of requests stays the same)
        const __amdgpu_buffer_rsrc_t rX = __builtin_amdgcn_make_buffer_rsrc((void*)(X0 + (int64_t)(b0 + (live ? ib : 0)) * xbs), 0, (int)ext, 0x00020000);
        const unsigned so = live ? (unsigned)ik * kstep : 0u;
        const int krem = live ? T - ik * DP_BK : 0;
#pragma unroll
        for (int q = 0; q < DP_Q; ++q) dma16(rX, dst + q * 1024, kq[q] < krem ? voff[q] : OOB, so);
        si = si + 1 == STAGES ? 0 : si + 1;
        if (++ik == nkt) ik = 0, ++ib;
    };

    // ---- fragment geometry: lane (g, pp); k-rows 8 g + (pp >> 2) (+ 4), chunk cb + (pp >> 1 & 1), 8 bytes (pp & 1)
    const int g = lane >> 4, pp = lane & 15;
    const unsigned swr = (unsigned)((((pp >> 3) & 1) | ((g & 1) << 1)) << 1);
    const unsigned kbyte = (unsigned)(g * 8 + (pp >> 2)) * 128u + (unsigned)(pp & 1) * 8u;
    auto frag_rc = [&](const unsigned char* img, const int c0) __attribute__((always_inline)) -> bf16x8 {     // 16 columns from c0
        const unsigned cb = (unsigned)((c0 & 63) >> 3) + (unsigned)((pp >> 1) & 1);
        const unsigned char* a0 = img + (c0 >> 6) * 4096 + kbyte + ((cb ^ swr) << 4);
        s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)LDS_AS(a0));
        s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)LDS_AS(a0 + 512));
        s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        return __builtin_bit_cast(bf16x8, v);
    };

    f32x4 acc[NBI][NJ];
#pragma unroll
    for (int i = 0; i < NBI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll
    for (int s = 0; s < STAGES - 1; ++s) issue();
    const int rb0 = wr * nbi;       // first 16-row block of this wave row
    int sr = 0;                     // the stage K-tile kt lies in
    for (int kt = 0; kt < nkt_all; ++kt) {
        // K-tiles kt .. kt + STAGES - 2 are requested: the oldest has landed when all but (STAGES - 2) DP_Q requests have.  The
        // stage the next request overwrites was read in iteration kt - 1, whose MFMAs every wave has issued before this barrier.
        wait_vm<DP_Q*(STAGES - 2)>();
        BAR();
        issue();
        const unsigned char* sA = smem + sr * DP_STAGE;
        const unsigned char* sB = sA + DP_A_BYTES;
        sr = sr + 1 == STAGES ? 0 : sr + 1;
        bf16x8 fb[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) fb[j] = frag_rc(sB, wc * (16 * NJ) + j * 16);
        // (all NBI blocks, unconditionally: blocks past this wave row's nbi hold the other wave row's rows or the zeros of the pieces
        //  past the tile -- their accumulators are never stored; (rb0 + i) 16 < 64 NPA always)
        bf16x8 fa[NBI];
#pragma unroll
        for (int i = 0; i < NBI; ++i) fa[i] = frag_rc(sA, (rb0 + i) * 16);
        SB();
#pragma unroll
        for (int i = 0; i < NBI; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[j], fa[i], acc[i][j], 0, 0, 0);
    }
    wait_vm<0>();
    __syncthreads();

    // ---- epilogue.  C^T blocks (B fragment first): lane (g, pp) holds, for row (rb0 + i) 16 + pp of the tile, the FOUR consecutive
    // columns wc 16 NJ + j 16 + g 4 .. +3: one 16-byte fp32 store per block into this group's copy.
    const int crow = m0 + rb0 * 16 + pp;
    const int ccol = wc * (16 * NJ) + g * 4;
    float* W = p.ws + (int64_t)grp * T * p.d + h * dk + ccol;
#pragma unroll
    for (int i = 0; i < NBI; ++i) {
        const int row = crow + i * 16;
        const bool rok = i < nbi && row < T;
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            if (rok && ccol + j * 16 < dk) *(f32x4*)(W + (int64_t)row * p.d + j * 16) = acc[i][j];
    }
}

// dP16[i] = bf16(sum_g ws[g][i]), ascending g, eight outputs per thread
__global__ __launch_bounds__(256) void attn_dpos_fold_kernel(const float* __restrict__ ws, u16* __restrict__ dP16, float* __restrict__ dP,
                                                             int groups, int64_t n) {
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8;
    if (i >= n) return;
    float4 a = *(const float4*)(ws + i), b = *(const float4*)(ws + i + 4);
    for (int g = 1; g < groups; ++g) {
        const float4 u = *(const float4*)(ws + g * n + i), v = *(const float4*)(ws + g * n + i + 4);
        a.x += u.x, a.y += u.y, a.z += u.z, a.w += u.w;
        b.x += v.x, b.y += v.y, b.z += v.z, b.w += v.w;
    }
    uint4 o;
    o.x = io_pack2(a.x, a.y), o.y = io_pack2(a.z, a.w), o.z = io_pack2(b.x, b.y), o.w = io_pack2(b.z, b.w);
    *(uint4*)(dP16 + i) = o;
    if (dP) *(float4*)(dP + i) = a, *(float4*)(dP + i + 4) = b;
}

struct DposPlan {
    int rows, tiles, group, grid, groups;
};

// The one place the tiling is decided.  Rows: the fewest row tiles of at most DP_MAX_ROWS rows (a multiple of 32; a last tile with a few
// rows is cheap, its A pieces are zeros).  Group: the fewest batch elements per workgroup that keep (tiles x heads x groups) within ONE
// round of the chip -- a second round pays the first tile's latency and the epilogue again with nothing beside it on the CU
// (tt_tiling, gemm_bf16_tt.hip); more per workgroup than that only idles CUs.
bool dpos_plan(int B, int H, int T, int dk, DposPlan* pl) {
    if (B < 1 || H < 1 || T < 8 || T % 8 || dk < 32 || dk % 32 || dk > 192 || dk == 160) return false;
    const int64_t d = (int64_t)H * dk;
    // one batch element's operands through 32-bit buffer offsets (the wider of the two row strides, T + 1)
    if ((int64_t)(T - 1) * (T + 1) * 2 + (int64_t)T * 2 >= (1ll << 31) || (int64_t)T * d * 2 >= (1ll << 31)) return false;
    const int cus = device_cus();
    // a workgroup streams its rows' share of every batch element of its group: group x (rows + ~64 rows' worth of fill per element)
    int tiles = 0, tr = 0, G = 0;
    long best = 0;
    for (int t = (T + DP_MAX_ROWS - 1) / DP_MAX_ROWS, n = 0; n < 6; ++t, ++n) {
        const int r = (((T + t - 1) / t) + 31) / 32 * 32;
        if (r > DP_MAX_ROWS || (int64_t)r * (t - 1) >= T || (int64_t)t * H > cus) continue;     // (an empty last tile: no tiling of its own)
        const int maxg = cus / (t * H), gg = (B + maxg - 1) / maxg;
        const long cost = (long)gg * (r + 64);
        if (!tiles || cost < best) tiles = t, tr = r, G = gg, best = cost;
    }
    if (!tiles) return false;
    const int64_t units = (int64_t)tiles * H;
    const int groups = (B + G - 1) / G;
    if ((int64_t)groups * T * d >= (1ll << 31)) return false;       // (the workspace size is returned as an int)
    pl->rows = tr, pl->tiles = tiles, pl->group = G, pl->groups = groups, pl->grid = (int)(units * groups);
    return true;
}

template <int NJ>
void launch_stream(const DposArgs& a, int grid, hipStream_t stream) {
    (void)hipFuncSetAttribute((const void*)attn_dpos_stream_kernel<NJ, DP_NPA, DP_STAGES>, hipFuncAttributeMaxDynamicSharedMemorySize, DP_LDS);
    hipLaunchKernelGGL((attn_dpos_stream_kernel<NJ, DP_NPA, DP_STAGES>), dim3(grid), dim3(512), DP_LDS, stream, a);
}
}   // namespace

extern "C" int a3t_attn_bwd_dpos_plan(int B, int H, int T, int dk, int* out) {
    DposPlan pl;
    if (!dpos_plan(B, H, T, dk, &pl)) return 0;
    if (out) out[0] = pl.rows, out[1] = pl.tiles, out[2] = pl.group, out[3] = pl.grid;
    return 1;
}

extern "C" int a3t_attn_bwd_dpos_ws(int B, int H, int T, int dk) {
    DposPlan pl;
    if (!dpos_plan(B, H, T, dk, &pl)) return 0;
    return (int)((int64_t)pl.groups * T * H * dk);
}

extern "C" int a3t_attn_bwd_dpos(const void* dbd, const void* qv, float* ws, void* dP16, float* dP, int B, int H, int T, int dk,
                                 int64_t dbd_rs, int64_t dbd_bsb, int64_t dbd_bsh, void* stream) {
    DposPlan pl;
    if (!dbd || !qv || !ws || !dP16 || !dpos_plan(B, H, T, dk, &pl)) return A3T_EINVAL;
    if (((uintptr_t)dbd & 1) || ((uintptr_t)qv & 15) || ((uintptr_t)ws & 15) || ((uintptr_t)dP16 & 15) || ((uintptr_t)dP & 15)) return A3T_EINVAL;
    if (dbd_rs < T || dbd_bsb < 0 || dbd_bsh < 0 || (dbd_rs * (int64_t)(T - 1) + T) * 2 >= (1ll << 31)) return A3T_EINVAL;
    DposArgs a;
    a.dbd = (const u16*)dbd, a.qv = (const u16*)qv, a.ws = ws;
    a.B = B, a.H = H, a.T = T, a.dk = dk, a.d = H * dk;
    a.a_rs = dbd_rs, a.a_bsb = dbd_bsb, a.a_bsh = dbd_bsh;
    a.TR = pl.rows, a.ntiles = pl.tiles, a.G = pl.group;
    if (dk > 128)
        launch_stream<3>(a, pl.grid, (hipStream_t)stream);
    else
        launch_stream<2>(a, pl.grid, (hipStream_t)stream);
    int rc = (int)hipGetLastError();
    if (rc) return rc;
    const int64_t n = (int64_t)T * a.d;
    hipLaunchKernelGGL(attn_dpos_fold_kernel, dim3((unsigned)((n / 8 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const float*)ws,
                       (u16*)dP16, dP, pl.groups, n);
    return (int)hipGetLastError();
}
