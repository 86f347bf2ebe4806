// gemm_bf16_tn.hip -- the token reductions of the 8-phase family: C[M][N] (+)= alpha * sum_k A[k][m] * B[k][n], both operands
// REDUCTION-strided (token-major activations): the weight gradients of Linear / Conv1d (multi_layer_conv.py:36-63 backward), the
// reduction over the B*T tokens split over workgroups.  Two kernels on the schedule discipline of gemm_bf16_8p.hip (LDS images of
// 128 x 64 halves, DMA issued phases ahead, counted vmcnt waits, two wave groups one barrier apart), one loader (TnFront), one
// fold of the split-K partial tiles, the slab those partials live in, the planners and the grouped entry point.
//
// What the token-major operands change against the k-contiguous kernel:
//   * half-tile image = 64 k-rows x 128 m (256 B per k-row); a wave DMA instruction = 4 k-rows; chunk position p of k-row
//     kr holds source chunk p ^ (((kr & 3) << 2) | (((kr >> 3) & 1) << 1)): the 8 k-rows x 32 B that the 32 lanes of a
//     ds_read_b64_tr_b16 group touch fall on disjoint banks;
//   * fragments by two transposed LDS reads (4 k each) per 16x16x32 operand;
//   * fused conv weight gradient (WG): output columns are (tap, c); a 128-column B half lies inside one tap and reads
//     x[k + (tap - pad) * dil] with zeros across utterance boundaries (buffer range check, as in the forward loader);
//   * one tile x one K split per workgroup; a single split writes C straight from the accumulators (64-byte row segments), K
//     splits leave as partial tiles (slab) that the fold sums in a fixed order.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <map>
#include <mutex>
#include "../../include/a3t_hip.h"
#include "gemm_common.h"
#include "mfma_kit.h"

// -DG8_TIMING (probe build): wall-clock stamps per workgroup and wave row of the 2 x 2 kernel, read with a3t_debug_read
#ifdef G8_TIMING
__device__ unsigned long long g8_stamps[256 * 2 * 16];
#define STAMP(k) do { if (lane == 0 && (w & 3) == 0 && (k) < 16) g8_stamps[(blockIdx.x * 2 + wr) * 16 + (k)] = wall_clock64(); } while (0)
extern "C" int a3t_debug_read(void* dst, size_t bytes) { return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(g8_stamps), bytes); }
#else
#define STAMP(k)
#endif

// Several token reductions over the SAME tokens in one launch (a3t_gemm_tn3_group): problem i owns tiles [tile0, next tile0) of
// every K split.  Passed by value beside GP; n == 0: the single problem described by GP.
struct TN3Prob {
    const void* A;
    const void* B;
    float* C;
    int64_t c_rs;
    int M, N;
    unsigned a_csb, b_csb;      // operand row strides in bytes
    unsigned a_bytes, b_bytes;
    float alpha;
    int accumulate, tile0, tiles_n;
};
struct TN3Group {
    int n;
    TN3Prob q[8];
};

namespace {
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
constexpr int HALF_BYTES = 128 * 64 * 2, TILE_BYTES = 4 * HALF_BYTES;      // LDS: 2 K-tile buffers x 4 half-tile images

// Which (tile, K split) a workgroup works on.  Slice-major, XCD-contiguous: the tiles of one K split (same operand slabs) stay
// inside one XCD's L2.
struct TnSplit {
    int bid, ks;      // tile of the launch, K split
    int per, kt0;     // K-tiles per split, first K-tile of this one
    bool live;        // false: the split has no K-tiles (the host folds only the splits that have some)
};
__device__ __forceinline__ TnSplit tn_split(const GP& p) {
    const int wi = xcd_contiguous(blockIdx.x, gridDim.x);
    TnSplit s;
    s.bid = wi % p.ntiles, s.ks = wi / p.ntiles;
    const int nkt = (p.K + 63) >> 6;              // (tokens past K read zeros through the range check)
    s.per = (nkt + p.splitk - 1) / p.splitk;
    s.per += s.per & 1;                           // whole pairs of K-tiles; tiles past the end read zeros
    s.kt0 = s.ks * s.per;
    s.live = s.kt0 < nkt;
    return s;
}

// transposed fragment read: 8 k-values of one row / column of a 16-wide block -- the MFMA operand layout
__device__ __forceinline__ bf16x8 tn_frag(const unsigned char* img, unsigned off, int s) {
    const unsigned char* a0 = img + off + s * 8192;
    s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)LDS_AS(a0));
    s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)LDS_AS(a0 + 1024));
    s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, v);
}

// What both kernels share in front of and around their phase schedules: the loader (lane geometry, K-tile cursor, DMA issue), the
// fragment reads and the MFMA block of one A half x one B half.  A tile is AH x BH halves of 128 rows / columns; its halves lie in
// a K-tile buffer as images 0 .. AH-1 (A) and AH .. AH+BH-1 (B).  The operand pointers, extents and strides come from the caller
// (the 128 x 384 kernel looks them up in its group); everything else of the problem is read from GP where it is used (a
// reference: copies of K and Tseq in here changed the K loop's code).
template <bool WG, int AH, int BH>
struct TnFront {
    const GP& p;
    int lane, w, wr, wc;
    __amdgpu_buffer_rsrc_t rA, rB;
    unsigned a_csb, b_csb, voffA, voffB, lds0;
    int Mp, Np, tn, krl, sc, mA;
    int shiftB[BH], c0B[BH];
    int c_kt, tpos;             // cursor: K-tile, and (q = 0 | q = 1 << 16) the token position of the lane's rows inside their utterance
    unsigned offA[4], offB[2];
    bf16x8 fa[4][2];

    __device__ __forceinline__ TnFront(const GP& p_, const unsigned char* smem, int kt0, const void* A, const void* B, int M, int N, unsigned a_csb_,
                                       unsigned b_csb_, unsigned a_bytes, unsigned b_bytes, int tm, int tn_)
        : p(p_) {
        const int tid = threadIdx.x;
        lane = tid & 63;
        w = __builtin_amdgcn_readfirstlane(tid >> 6);
        wr = w >> 2, wc = w & 3;
        a_csb = a_csb_, b_csb = b_csb_, Mp = M, Np = N, tn = tn_;
        rA = __builtin_amdgcn_make_buffer_rsrc((void*)A, 0, (int)a_bytes, 0x00020000);
        rB = __builtin_amdgcn_make_buffer_rsrc((void*)B, 0, (int)b_bytes, 0x00020000);

        // ---- DMA lane geometry: instruction (half, q) fills k-rows (q*8 + w)*4 + (lane>>4), chunk position lane&15
        krl = w * 4 + (lane >> 4);                                        // q = 0; q = 1: + 32
        sc = (lane & 15) ^ (((lane >> 4) << 2) | (((w >> 1) & 1) << 1));   // source chunk of this lane (same for q = 0, 1)
        mA = tm * (AH * 128) + sc * 8;                                    // + h*128
        voffA = (unsigned)krl * a_csb + (unsigned)mA * 2u;
        const int cin = WG ? Np / p.taps : Np;
#pragma unroll
        for (int h = 0; h < BH; ++h) {
            const int n0 = tn * (BH * 128) + h * 128;
            const int tap = WG ? n0 / cin : 0;
            shiftB[h] = WG ? (tap - p.pad) * p.dil : 0;
            c0B[h] = n0 - tap * cin;
        }
        voffB = (unsigned)krl * b_csb + (unsigned)(sc * 16);
        tpos = 0;
        if (WG) {
            const int t0 = (kt0 * 64 + krl) % p.Tseq, t1 = (kt0 * 64 + krl + 32) % p.Tseq;
            tpos = t0 | (t1 << 16);
        }
        c_kt = kt0;
        lds0 = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)LDS_AS(smem));

        // ---- transposed fragment reads: lane (g, pp) supplies the address of 4 consecutive m of k-row g*8 + (pp>>2) (+4) and
        // receives column pp of the 16-column block
        const int g = lane >> 4, pp = lane & 15;
        const unsigned swz = (unsigned)(((pp >> 2) << 2) | ((g & 1) << 1));
        const unsigned kbyte = (unsigned)(g * 8 + (pp >> 2)) * 256u + (unsigned)(pp & 1) * 8u;
#pragma unroll
        for (int i = 0; i < 4; ++i) offA[i] = kbyte + ((((unsigned)(wr * 8 + i * 2) + (unsigned)((pp & 3) >> 1)) ^ swz) << 4);
#pragma unroll
        for (int j = 0; j < 2; ++j) offB[j] = kbyte + ((((unsigned)(wc * 4 + j * 2) + (unsigned)((pp & 3) >> 1)) ^ swz) << 4);
    }

    __device__ __forceinline__ void advance() {
        ++c_kt;
        if (WG) {
            int t0 = (tpos & 0xffff) + 64, t1 = (tpos >> 16) + 64;
            if (p.Tseq >= 64) {
                t0 = t0 >= p.Tseq ? t0 - p.Tseq : t0, t1 = t1 >= p.Tseq ? t1 - p.Tseq : t1;
            } else {
                t0 %= p.Tseq, t1 %= p.Tseq;
            }
            tpos = t0 | (t1 << 16);
        }
    }

    // one half-tile image H of K-tile kt (token positions tp) into buffer buf: 2 DMA instructions per lane.  kt / tp are explicit
    // because a schedule may request halves of a K-tile after the cursor has moved on (the caller hands in the values it saved).
    __device__ __forceinline__ void issue(const int H, const int buf, const int kt, const int tp) const {
        int wv = w;
        unsigned acs = a_csb, bcs = b_csb;
        asm volatile("" : "+s"(wv), "+s"(acs), "+s"(bcs));
        const unsigned dst = lds0 + (unsigned)(buf * TILE_BYTES + H * HALF_BYTES) + (unsigned)wv * 1024u;
        const int krem = p.K - kt * 64 - krl;       // > q*32: the lane's token row exists
        if (H < AH) {
            const bool colok = mA + H * 128 < Mp;
            const unsigned so = (unsigned)kt * 64u * acs;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const unsigned vb = voffA + (unsigned)(H * 256) + (unsigned)(q * 32) * acs;
                dma16(rA, dst + q * 8192, (colok && krem > q * 32) ? vb : OOB, so);
            }
        } else {
            const int h = H - AH;
            const bool colok = tn * (BH * 128) + h * 128 + sc * 8 < Np;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int t = q ? (tp >> 16) : (tp & 0xffff);
                const bool ok = colok && (krem > q * 32) && (!WG || ((unsigned)(t + shiftB[h]) < (unsigned)p.Tseq));
                // (the whole token offset lives in voffset: the range check ignores soffset, and the tap shift may be negative)
                const unsigned vb = voffB + (unsigned)(kt * 64 + q * 32 + shiftB[h]) * bcs + (unsigned)(c0B[h] * 2);
                dma16(rB, dst + q * 8192, ok ? vb : OOB, 0u);
            }
        }
    }

    __device__ __forceinline__ void readA(const unsigned char* img, const int i0, const int i1) {
#pragma unroll
        for (int i = i0; i < i1; ++i) fa[i][0] = tn_frag(img, offA[i], 0), fa[i][1] = tn_frag(img, offA[i], 1);
    }
    __device__ __forceinline__ void readB(const unsigned char* img, bf16x8 (&fb)[2][2]) const {
#pragma unroll
        for (int j = 0; j < 2; ++j) fb[j][0] = tn_frag(img, offB[j], 0), fb[j][1] = tn_frag(img, offB[j], 1);
    }
    // 64 x 32 outputs of a wave: the A half in fa x the B half in fb
    __device__ __forceinline__ void mfma(f32x4 (&acc)[4][2], const bf16x8 (&fb)[2][2]) const {
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][s], fb[j][s], acc[i][j], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
    }
};
}   // namespace

// =====================================================================================================================
// 256 x 256 tile = 2 x 2 halves, the four phases per K-tile of gemm_bf16_8p.hip (A0xB0, A0xB1, A1xB1, A1xB0), DMA order B0, A0,
// B1, A1 and ONE counted wait per K-tile.
template <bool WG>
__global__ __launch_bounds__(512, 2) void gemm_bf16_8p_tn_kernel(GP p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    enum { HA0 = 0, HA1 = 1, HB0 = 2, HB1 = 3 };
    const TnSplit sp = tn_split(p);
    const int bid = sp.bid, ks = sp.ks;
    const int tn = bid % p.tiles_n, tm = bid / p.tiles_n;
    if (!sp.live) return;
    TnFront<WG, 2, 2> f(p, smem, sp.kt0, p.A, p.B, p.M, p.N, (unsigned)p.a_cs * 2u, (unsigned)p.b_cs * 2u, p.a_bytes, p.b_bytes, tm, tn);
    const int lane = f.lane, w = f.w, wr = f.wr, wc = f.wc;

    f32x4 acc[2][2][4][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[a][b][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    bf16x8 fb0[2][2], fb1[2][2];
    auto issue = [&](const int H, const int buf) __attribute__((always_inline)) { f.issue(H, buf, f.c_kt, f.tpos); };

    STAMP(0);
    issue(HB0, 0), issue(HA0, 0), issue(HB1, 0), issue(HA1, 0);
    f.advance();
    issue(HB0, 1), issue(HA0, 1), issue(HB1, 1);
    WAIT_VM(6);
    BAR();
    if (wr == 1) BAR();
    STAMP(1);

    auto ktile = [&](const int buf) __attribute__((always_inline)) {
        const unsigned char* cur = smem + buf * TILE_BYTES;
        // phase 1: A0 x B0 (8 + 16 transposed reads; the lgkmcnt field counts to 15: the wait that retires the B0 reads sits
        // after the first half of the A reads)
        f.readB(cur + HB0 * HALF_BYTES, fb0);
        SB();
        f.readA(cur + HA0 * HALF_BYTES, 0, 2);
        WAIT_LGKM(8);
        SB();
        f.readA(cur + HA0 * HALF_BYTES, 2, 4);
        issue(HA1, buf ^ 1);
        f.advance();
        BAR();
        WAIT_LGKM(0);
        SB();
        f.mfma(acc[0][0], fb0);
        BAR();
        f.readB(cur + HB1 * HALF_BYTES, fb1);
        issue(HB0, buf);
        BAR();
        WAIT_LGKM(0);
        SB();
        f.mfma(acc[0][1], fb1);
        BAR();
        f.readA(cur + HA1 * HALF_BYTES, 0, 4);
        issue(HA0, buf);
        BAR();
        WAIT_LGKM(0);
        SB();
        f.mfma(acc[1][1], fb1);
        BAR();
        issue(HB1, buf);
        WAIT_VM(6);
        BAR();
        f.mfma(acc[1][0], fb0);
        BAR();
    };
    for (int u = 0; u < sp.per; u += 2) {
        ktile(0);
        ktile(1);
    }
    STAMP(2);
    if (wr == 0) BAR();
    WAIT_VM(0);

    // ---- epilogue: lane (g, pp) holds rows a*128 + wr*64 + i*16 + g*4 + r, column hb*128 + wc*32 + j*16 + pp
    const int g = lane >> 4, pp = lane & 15;
    if (p.slab) {
        // split-K partial of this (tile, K split): the accumulators go out as they lie in the registers -- 16 bytes per lane and
        // fragment, 1 KiB contiguous per wave instruction -- and gemm_8p_tn_fold_kernel sums the splits of a tile in a fixed
        // order.  (As fp32 atomics straight into C the same 64 values per lane are 64 instructions of 256 scattered bytes each
        // and resolve at the memory side: 48 us for 240 workgroups against 5 us of stores, tools/probes/atomic_epilogue.hip.)
        float* slab = p.slab + ((int64_t)ks * p.ntiles + bid) * 65536 + (w * 64 + lane) * 4;
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            if (tm * 256 + a * 128 >= p.M) continue;
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                if (tn * 256 + b * 128 >= p.N) continue;
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        *(f32x4*)(slab + ((((a * 2 + b) * 4 + i) * 2 + j) * 2048)) = acc[a][b][i][j];
            }
        }
        return;
    }
    float* C = (float*)p.C;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = tm * 256 + a * 128 + wr * 64 + i * 16 + g * 4 + r;
#pragma unroll
                for (int b = 0; b < 2; ++b)
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const int n = tn * 256 + b * 128 + wc * 32 + j * 16 + pp;
                        if (m < p.M && n < p.N) {
                            const float v = p.alpha * acc[a][b][i][j][r];
                            float* c = C + (int64_t)m * p.c_rs + n;
                            if (p.accumulate == A3T_ACC_ATOMIC)
                                atomicAdd(c, v);
                            else if (p.accumulate == A3T_ACC_ADD)
                                *c += v;
                            else
                                *c = v;
                        }
                    }
            }
#ifdef G8_TIMING
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    STAMP(3);
#endif
}

// =====================================================================================================================
// 128 x 384 tile = ONE A half x THREE B halves, three phases per K-tile.
// Every weight gradient of the model has a 384-multiple of input channels per tap (d_model = 384, ff = 1536 = 4 x 384), so
// 128 x 384 tiles cover dW exactly: 1536 x (3 x 384) and 384 x (3 x 1536) are 36 full tiles each, where 256 x 256 tiles fill
// 0.90 / 0.75 of their 30 / 36 tiles; the Linear weight gradients (N = 384) are one tile wide.  The A fragments (64 rows per wave,
// the larger operand) are read once per K-tile and stay in registers for the three B halves: 20 KiB of LDS reads per wave and
// K-tile for 64 x 96 outputs (the 2 x 2 tile: 24 KiB for 128 x 64).
//   phase 1 of K-tile t: read B0 + A0 | DMA B1(t+1),          vmcnt(8)  -> B1(t) landed        | A0 x B0
//   phase 2:             read B1      | DMA B2(t+1), B0(t+2), vmcnt(10) -> B2(t) landed        | A0 x B1
//   phase 3:             read B2      | DMA A0(t+2),          vmcnt(8)  -> B0, A0(t+1) landed  | A0 x B2
//   One counted wait per phase, each retiring exactly the half that is read in the NEXT phase and was requested three (B0: four)
//   phases earlier; four to five half-tiles stay in flight across every barrier.  (A first version waited once per K-tile with
//   vmcnt(4): that wait also retired B1 / B2 of tile t+1, requested one and two phases earlier -- their L2 latency was exposed in
//   every K-tile: 138 us per FFN weight gradient against the figure in DESIGN.md.)
// Restaging distances: B0 one phase after its reads (retired by the lgkmcnt in front of phase 1's first barrier), A0 / B1 / B2
// two phases after theirs -- the rules of the 2 x 2 kernel above.  Epilogue: split-K partial tile by plain stores (slab).
template <bool WG>
__global__ __launch_bounds__(512, 2) void gemm_bf16_8p_tn3_kernel(GP p, TN3Group grp) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    enum { H3A = 0, H3B0 = 1, H3B1 = 2, H3B2 = 3 };
    const TnSplit sp = tn_split(p);
    const int bid = sp.bid, ks = sp.ks;
    // the problem this tile belongs to (uniform): a group member or GP itself
    const void* Ap = p.A;
    const void* Bp = p.B;
    int Mp = p.M, Np = p.N, tiles_n = p.tiles_n, lbid = bid;
    unsigned a_csb = (unsigned)p.a_cs * 2u, b_csb = (unsigned)p.b_cs * 2u, a_bytes = p.a_bytes, b_bytes = p.b_bytes;
    if (grp.n > 0) {
        int k = 0;
        for (int i = 1; i < grp.n; ++i)
            if (bid >= grp.q[i].tile0) k = i;
        Ap = grp.q[k].A, Bp = grp.q[k].B, Mp = grp.q[k].M, Np = grp.q[k].N, tiles_n = grp.q[k].tiles_n;
        a_csb = grp.q[k].a_csb, b_csb = grp.q[k].b_csb, a_bytes = grp.q[k].a_bytes, b_bytes = grp.q[k].b_bytes;
        lbid = bid - grp.q[k].tile0;
    }
    const int tn = lbid % tiles_n, tm = lbid / tiles_n;
    if (!sp.live) return;
    TnFront<WG, 1, 3> f(p, smem, sp.kt0, Ap, Bp, Mp, Np, a_csb, b_csb, a_bytes, b_bytes, tm, tn);
    const int lane = f.lane, w = f.w, wr = f.wr;

    f32x4 acc[3][4][2];
#pragma unroll
    for (int b = 0; b < 3; ++b)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[b][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    bf16x8 fb[2][2][2];        // fb[parity]: the B fragments of a phase are read while the previous phase's are in use

    // K-tile kt0 -> buffer 0 (all four halves), B0 / A0 of K-tile kt0 + 1 -> buffer 1
    f.issue(H3B0, 0, f.c_kt, f.tpos), f.issue(H3A, 0, f.c_kt, f.tpos), f.issue(H3B1, 0, f.c_kt, f.tpos), f.issue(H3B2, 0, f.c_kt, f.tpos);
    f.advance();
    f.issue(H3B0, 1, f.c_kt, f.tpos), f.issue(H3A, 1, f.c_kt, f.tpos);
    WAIT_VM(4);
    BAR();
    if (wr == 1) BAR();

    auto ktile = [&](const int buf) __attribute__((always_inline)) {
        const unsigned char* cur = smem + buf * TILE_BYTES;
        // at entry the cursor (c_kt, tpos) is K-tile t+1, whose B0 / A0 are in flight or landed in buf ^ 1; its B1 / B2 are
        // requested after the cursor has moved on to t+2 for B0
        const int kt1 = f.c_kt, tp1 = f.tpos;
        // phase 1: A0 x B0
        f.readB(cur + H3B0 * HALF_BYTES, fb[0]);
        SB();
        f.readA(cur + H3A * HALF_BYTES, 0, 2);
        WAIT_LGKM(8);                    // the B0 reads (issued first) are retired before the barrier: B0 is restaged in phase 2
        SB();
        f.readA(cur + H3A * HALF_BYTES, 2, 4);
        f.issue(H3B1, buf ^ 1, kt1, tp1);
        WAIT_VM(8);                      // retires B1 of the current tile (requested 3 phases ago, read in phase 2)
        BAR();
        WAIT_LGKM(0);
        SB();
        f.mfma(acc[0], fb[0]);
        BAR();
        // phase 2: A0 x B1
        f.readB(cur + H3B1 * HALF_BYTES, fb[1]);
        f.issue(H3B2, buf ^ 1, kt1, tp1);
        f.advance();
        f.issue(H3B0, buf, f.c_kt, f.tpos);
        WAIT_VM(10);                     // retires B2 of the current tile (requested 3 phases ago, read in phase 3)
        BAR();
        WAIT_LGKM(0);
        SB();
        f.mfma(acc[1], fb[1]);
        BAR();
        // phase 3: A0 x B2
        f.readB(cur + H3B2 * HALF_BYTES, fb[0]);
        f.issue(H3A, buf, f.c_kt, f.tpos);
        WAIT_VM(8);                      // retires B0 / A0 of the next tile (requested 4 / 3 phases ago)
        BAR();
        WAIT_LGKM(0);
        SB();
        f.mfma(acc[2], fb[0]);
        BAR();
    };
    for (int u = 0; u < sp.per; u += 2) {
        ktile(0);
        ktile(1);
    }
    if (wr == 0) BAR();
    WAIT_VM(0);

    // ---- epilogue: lane (g, pp) holds rows wr*64 + i*16 + g*4 + r, column b*128 + wc*32 + j*16 + pp of the tile
    float* slab = p.slab + ((int64_t)ks * p.ntiles + bid) * 49152 + (w * 64 + lane) * 4;
    if (tm * 128 >= Mp) return;
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        if (tn * 384 + b * 128 >= Np) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) *(f32x4*)(slab + (((b * 4 + i) * 2 + j) * 2048)) = acc[b][i][j];
    }
}

// Fold of the split-K partial tiles of a tile of A_HALVES x B_HALVES halves: C (+)= alpha * sum_s slab[s][tile].  One thread per
// 16-byte fragment piece (rows m..m+3 of one column; 4096 pieces per half x half); splits in ascending order, four loads in
// flight at a time -- a fixed order: the result does not depend on the launch.  grp: the members of a grouped launch (n == 0: the
// single problem described by GP).  Writes with atomics unless the caller is the sole writer, then by read-modify-write; stores
// under A3T_ACC_STORE.
template <int A_HALVES, int B_HALVES>
__global__ __launch_bounds__(256) void gemm_8p_tn_fold_kernel(GP p, TN3Group grp) {
    constexpr int PIECE_FLOATS = A_HALVES * B_HALVES * 16384;      // floats of one partial tile
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int bid = blockIdx.y;
    float* Cp = (float*)p.C;
    int64_t c_rs = p.c_rs;
    int Mp = p.M, Np = p.N, tiles_n = p.tiles_n, lbid = bid, accumulate = (p.accumulate == A3T_ACC_ATOMIC && p.sole_writer) ? A3T_ACC_ADD : p.accumulate;
    float alpha = p.alpha;
    if (grp.n > 0) {
        int k = 0;
        for (int i = 1; i < grp.n; ++i)
            if (bid >= grp.q[i].tile0) k = i;
        Cp = grp.q[k].C, c_rs = grp.q[k].c_rs, Mp = grp.q[k].M, Np = grp.q[k].N, tiles_n = grp.q[k].tiles_n;
        accumulate = grp.q[k].accumulate, alpha = grp.q[k].alpha, lbid = bid - grp.q[k].tile0;       // (SOLE arrives as ADD)
    }
    const int tn = lbid % tiles_n, tm = lbid / tiles_n;
    const int lane = t & 63, w = (t >> 6) & 7, q = t >> 9;
    const int j = q & 1, i = (q >> 1) & 3, b = (q >> 3) % B_HALVES, a = q / (8 * B_HALVES);
    const int wr = w >> 2, wc = w & 3, g = lane >> 4, pp = lane & 15;
    const int m = (tm * A_HALVES + a) * 128 + wr * 64 + i * 16 + g * 4;
    const int n = (tn * B_HALVES + b) * 128 + wc * 32 + j * 16 + pp;
    if ((tm * A_HALVES + a) * 128 >= Mp || (tn * B_HALVES + b) * 128 >= Np || n >= Np || m >= Mp) return;      // (halves never written; nothing to store)
    const float* s = p.slab + (int64_t)bid * PIECE_FLOATS + (int64_t)t * 4;
    const int64_t sstride = (int64_t)p.ntiles * PIECE_FLOATS;
    f32x4 v = *(const f32x4*)s;
    int k = 1;
    for (; k + 4 <= p.splitk; k += 4) {
        const f32x4 u0 = *(const f32x4*)(s + (k + 0) * sstride), u1 = *(const f32x4*)(s + (k + 1) * sstride);
        const f32x4 u2 = *(const f32x4*)(s + (k + 2) * sstride), u3 = *(const f32x4*)(s + (k + 3) * sstride);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = (((v[r] + u0[r]) + u1[r]) + u2[r]) + u3[r];
    }
    for (; k < p.splitk; ++k) {
        const f32x4 u = *(const f32x4*)(s + k * sstride);
        v[0] += u[0], v[1] += u[1], v[2] += u[2], v[3] += u[3];
    }
    float* C = Cp + (int64_t)m * c_rs + n;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (m + r >= Mp) break;
        const float x = alpha * v[r];
        if (accumulate == A3T_ACC_ATOMIC)
            atomicAdd(C + (int64_t)r * c_rs, x);
        else if (accumulate == A3T_ACC_ADD)
            C[(int64_t)r * c_rs] += x;
        else
            C[(int64_t)r * c_rs] = x;
    }
}

// Split-K partial workspace: one per (device, stream) -- a launch and its fold are ordered on their stream, launches on
// different streams must not share slabs.  Grow-only per stream (hipMalloc on first use / growth; a few launches during warm-up);
// the device is the STREAM's (a launch on another device's stream gets its slab there), at most G8_MAX_SLABS live at a time (the
// least recently used one is drained and freed), and a3t_release_workspaces() frees them all.
#define G8_MAX_SLABS 16
struct G8Slab {
    float* p;
    size_t bytes;
    unsigned long long used;
};
static std::mutex g8_slab_mu;
static std::map<std::pair<int, hipStream_t>, G8Slab> g8_slabs;
static unsigned long long g8_slab_clock = 0;
static float* g8_slab(hipStream_t stream, size_t bytes) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    if (stream) {
        hipDevice_t sd = 0;
        if (hipStreamGetDevice(stream, &sd) == hipSuccess) dev = (int)sd;
    }
    std::lock_guard<std::mutex> lk(g8_slab_mu);
    const std::pair<int, hipStream_t> key(dev, stream);
    if (!g8_slabs.count(key) && g8_slabs.size() >= G8_MAX_SLABS) {
        auto lru = g8_slabs.begin();
        for (auto it = g8_slabs.begin(); it != g8_slabs.end(); ++it)
            if (it->second.used < lru->second.used) lru = it;
        if (lru->second.p) {
            (void)hipStreamSynchronize(lru->first.second);      // (a destroyed stream: the error is ignored, the memory is idle)
            (void)hipFree(lru->second.p);
        }
        g8_slabs.erase(lru);
    }
    G8Slab& e = g8_slabs[key];
    e.used = ++g8_slab_clock;
    if (e.bytes < bytes) {
        int cur = 0;
        (void)hipGetDevice(&cur);
        if (cur != dev) (void)hipSetDevice(dev);
        if (e.p) {
            (void)hipStreamSynchronize(stream);
            (void)hipFree(e.p);
        }
        e.p = nullptr, e.bytes = 0;
        const hipError_t r = hipMalloc((void**)&e.p, bytes);
        if (cur != dev) (void)hipSetDevice(cur);
        if (r != hipSuccess) {
            e.p = nullptr;
            return nullptr;
        }
        e.bytes = bytes;
    }
    return e.p;
}
// frees every split-K slab (after draining the stream it belongs to) and the attention key-split workspace; the next launch that
// needs one allocates again
void attn_release_split_ws();      // attn_fused.hip
extern "C" int a3t_release_workspaces(void) {
    attn_release_split_ws();
    std::lock_guard<std::mutex> lk(g8_slab_mu);
    for (auto& kv : g8_slabs)
        if (kv.second.p) {
            (void)hipStreamSynchronize(kv.first.second);
            (void)hipFree(kv.second.p);
        }
    g8_slabs.clear();
    (void)hipGetLastError();
    return 0;
}

// K splits of a token-reduction grid of `tiles` output tiles over nkt 64-wide K-tiles: fill the chip, >= 16 K-tiles per workgroup.
// folds: the splits that get K-tiles as the kernels deal them out (an even number each; later splits write nothing) = the fold's splitk.
static void g8_split_k(long tiles, int nkt, int& splits, int& folds) {
    splits = (int)(device_cus() / tiles);
    if (splits < 1) splits = 1;
    if (splits > nkt / 16) splits = nkt / 16 > 0 ? nkt / 16 : 1;
    int per = (nkt + splits - 1) / splits;
    per += per & 1;
    folds = (nkt + per - 1) / per;
}

template <typename Kernel, typename... Args>
static void launch_tn(Kernel kernel, int grid, hipStream_t stream, const Args&... args) {
    (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * TILE_BYTES);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(512), 2 * TILE_BYTES, stream, args...);
}

// What both kernels ask of their operands, on a resolved descriptor (GP) or a caller's (a3t_gemm_desc): fp32 C, plain epilogue,
// token-major bf16 operands of K tokens below 2 GiB, 16-byte aligned rows.
template <typename D>
static bool tn_operands_ok(const D& e, int K) {
    if (e.c_dtype != A3T_F32 || e.M % 8 != 0 || e.N % 8 != 0) return false;
    if (e.a_rs != 1 || e.b_rs != 1 || e.bias || e.R || e.S || e.colsum || e.act != A3T_ACT_NONE) return false;
    if (((uintptr_t)e.A | (uintptr_t)e.B | (uintptr_t)e.C) & 15) return false;
    const int64_t a_bytes = (int64_t)K * e.a_cs * 2, b_bytes = (int64_t)K * e.b_cs * 2;
    return a_bytes < (1ll << 31) && b_bytes < (1ll << 31) && e.a_cs % 8 == 0 && e.b_cs % 8 == 0;
}

// 128 x 384 tiles (gemm_bf16_8p_tn3_kernel), asked by g8_tn_plan under A3T_GEMM_8P_TN3 = 1 (whenever legal) or 2 (default: when
// the tiles fit the output exactly enough and there is enough K per workgroup).
static bool g8_tn3_plan(const GP& p, GemmPlan* pl) {
    const long tm = (p.M + 127) / 128, tn = (p.N + 383) / 384, tiles = tm * tn;
    int splits, folds;
    g8_split_k(tiles, (p.K + 63) / 64, splits, folds);
    if (gemm_switch(SW_8P_TN3) == 2) {
        const double fill = (double)p.M * p.N / ((double)tm * 128 * tn * 384);
        if (fill < 0.85 || tiles * splits < 96) return false;
    }
    pl->route = GR_G8_TN3, pl->cv = p.taps > 1, pl->tiles_n = (int)tn, pl->ntiles = (int)tiles;
    pl->splits = splits, pl->folds = folds, pl->grid = dim3((unsigned)(tiles * splits));
    pl->slab_floats = (size_t)tiles * splits * 49152;
    snprintf(pl->name, sizeof(pl->name), "gemm_bf16_8p_tn3_kernel<%s>", tf(pl->cv));
    return true;
}

// weight gradients: reduction-strided operands, K (tokens) split over workgroups
bool g8_tn_plan(const GP& p, int batch, GemmPlan* pl) {
    // Its K loop runs 1.55 us per K-tile (1.39 PFLOP/s) but the ~240 workgroups of a split-K grid finish together and their
    // 15.7 M fp32 atomics cost 20-35 us with nothing to hide them behind, and a 128-KiB / 496-register workgroup shares its CU
    // with nobody (the 128x128 weight-gradient kernel runs beside the main stream's kernels).  configs[1]'s FFN weight
    // gradients: 153 / 165 us against 170 / 171 us alone, +1 ms per step inside the step; configs[3]'s (K = 28800, 90 K-tiles per
    // workgroup): -1 ms per step.  Hence the margin below.  A3T_GEMM_8P_TN=0 / 1: never / whenever legal.
    const int mode = gemm_switch(SW_8P), tn_on = gemm_switch(SW_8P_TN);
    if (mode == 0 || tn_on == 0) return false;
    if (batch != 1 || p.drop_inv > 0.f || !tn_operands_ok(p, p.K)) return false;
    const bool wg = p.taps > 1;
    if (wg && ((p.N % p.taps) || ((p.N / p.taps) % 128) || p.Tseq <= 0 || p.Tseq >= 32768)) return false;
    if (!wg && p.kshift_mode) return false;
    const long tm = (p.M + 255) / 256, tn = (p.N + 255) / 256, tiles = tm * tn;
    const int nkt = (p.K + 63) / 64;
    int splits, folds;
    g8_split_k(tiles, nkt, splits, folds);
    // Which tile: 256 x 256 (four quadrants per K-tile, 1.55 us: the better K loop) when it covers the output exactly --
    // configs[3]'s 2048 x 1536 / 512 x 6144: 67.97 ms per step against 68.70 on the 128 x 384 tile -- and 128 x 384 (three
    // quadrants, 1.41 us, 176 registers: leaves the CU's other wave slots to the main stream's kernels) where 256 x 256 tiles
    // would be partly empty -- configs[1]'s 1536 x 1152 / 384 x 4608 (fill 0.90 / 0.75): 43.2 ms per step against 44.6.
    const double fill = (double)p.M * p.N / ((double)tm * 256 * tn * 256);
    bool ok22 = true;
    if (mode == 2 && tn_on == 2) {
        const double t8 = (double)((nkt + splits - 1) / splits) * 1.55 + 25.0;      // us: K loop + prologue, partial stores, fold
        const double t128 = 2.0 * p.M * p.N * (double)p.K / 680e6;                 // us at the 128x128 kernel's ~680 TFLOP/s
        ok22 = !(fill < 0.7 || tiles * splits < 160 || nkt / splits < 32 || t8 > 0.7 * t128);
    }
    const int t3 = gemm_switch(SW_8P_TN3);
    if ((t3 == 1 || (t3 == 2 && !(ok22 && fill >= 0.95))) && g8_tn3_plan(p, pl)) return true;
    if (!ok22) return false;
    // K splits always leave through the slab + fold (the fp32-atomic epilogue of rounds 3-4 lost by 21 us per launch and left in
    // round 6; a single split writes C directly in the mode the descriptor asks for)
    pl->route = GR_G8_TN, pl->cv = wg, pl->tiles_n = (int)tn, pl->ntiles = (int)tiles;
    pl->splits = splits, pl->folds = folds, pl->grid = dim3((unsigned)(tiles * splits));
    pl->slab_floats = splits > 1 ? (size_t)tiles * splits * 65536 : 0;
    snprintf(pl->name, sizeof(pl->name), "gemm_bf16_8p_tn_kernel<%s>", tf(wg));
    return true;
}

// K splits leave through the slab and the fold
int g8_tn_launch(const GP& p, const GemmPlan& pl, hipStream_t stream) {
    GP pv = p;
    pv.tiles_n = pl.tiles_n, pv.ntiles = pl.ntiles, pv.splitk = pl.splits;
    pv.a_bytes = (unsigned)((int64_t)p.K * p.a_cs * 2), pv.b_bytes = (unsigned)((int64_t)p.K * p.b_cs * 2);
    pv.slab = nullptr;
    if (pl.slab_floats) {
        pv.slab = g8_slab(stream, pl.slab_floats * sizeof(float));
        if (!pv.slab) return (int)hipErrorOutOfMemory;
    }
    const int grid = (int)pl.grid.x;
    const TN3Group none = {};
    GP pf = pv;
    pf.splitk = pl.folds;
    if (pl.route == GR_G8_TN3) {
        launch_tn(pl.cv ? gemm_bf16_8p_tn3_kernel<true> : gemm_bf16_8p_tn3_kernel<false>, grid, stream, pv, none);
        hipLaunchKernelGGL((gemm_8p_tn_fold_kernel<1, 3>), dim3(48, (unsigned)pl.ntiles), dim3(256), 0, stream, pf, none);
    } else {
        launch_tn(pl.cv ? gemm_bf16_8p_tn_kernel<true> : gemm_bf16_8p_tn_kernel<false>, grid, stream, pv);
        if (pv.slab) hipLaunchKernelGGL((gemm_8p_tn_fold_kernel<2, 2>), dim3(64, (unsigned)pl.ntiles), dim3(256), 0, stream, pf, none);
    }
    return (int)hipGetLastError();
}

// Several Linear weight gradients over the same tokens (dW_i[M_i][N_i] (+)= alpha_i * dy_i^T x_i, K tokens each) in ONE launch of
// the 128 x 384-tile kernel: their tiles share the K splits, so the four small gradients of a Conformer block (linear_out,
// linear_q/k/v, pointwise_conv1/2: 3 + 9 + 3 + 6 tiles) fill the chip with 47 K-tiles per workgroup instead of 16-20 each, and pay
// one prologue / slab / fold instead of four.  Returns -1 when a member does not fit (the caller launches them one by one).
extern "C" int a3t_gemm_tn3_group(const a3t_gemm_desc* d, int n, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!d || n < 1 || n > 8) return A3T_EINVAL;
    if (gemm_switch(SW_8P) == 0 || gemm_switch(SW_8P_TN3) == 0) return -1;
    TN3Group grp = {};
    grp.n = n;
    long tiles = 0;
    const int K = d[0].K;
    for (int i = 0; i < n; ++i) {
        const a3t_gemm_desc& e = d[i];
        if (!e.A || !e.B || !e.C || e.M <= 0 || e.N <= 0 || e.K != K) return A3T_EINVAL;
        if (e.compute != A3T_BF16 || e.a_dtype != A3T_BF16 || e.b_dtype != A3T_BF16) return -1;
        if (e.taps > 1 || e.batch > 1 || e.Tseq > 0 || e.kshift) return -1;
        if (e.drop_p > 0.f || e.keep_in || e.keep_out || !tn_operands_ok(e, K)) return -1;
        const int64_t ab = (int64_t)K * e.a_cs * 2, bb = (int64_t)K * e.b_cs * 2;
        TN3Prob& q = grp.q[i];
        q.A = e.A, q.B = e.B, q.C = (float*)e.C, q.c_rs = e.c_rs, q.M = e.M, q.N = e.N;
        q.a_csb = (unsigned)(e.a_cs * 2), q.b_csb = (unsigned)(e.b_cs * 2), q.a_bytes = (unsigned)ab, q.b_bytes = (unsigned)bb;
        q.alpha = e.alpha, q.accumulate = e.accumulate == A3T_ACC_SOLE ? A3T_ACC_ADD : e.accumulate;
        q.tile0 = (int)tiles, q.tiles_n = (e.N + 383) / 384;
        tiles += (long)((e.M + 127) / 128) * q.tiles_n;
    }
    // A3T_ACC_SOLE members are folded with plain read-modify-writes: two members that write overlapping ranges of one gradient (a
    // tied weight) would race inside the one fold launch -> the caller launches them one by one (ordered on the stream)
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j) {
            const char* ci = (const char*)d[i].C, *cj = (const char*)d[j].C;
            const char* ei = ci + ((int64_t)(d[i].M - 1) * d[i].c_rs + d[i].N) * 4, *ej = cj + ((int64_t)(d[j].M - 1) * d[j].c_rs + d[j].N) * 4;
            if (ci < ej && cj < ei) return -1;
        }
    if (gemm_switch(SW_8P_TN3) == 2) {       // partly empty 384-column tiles (input widths that are no multiple of 384) lose to the single launches
        double out = 0.0;
        for (int i = 0; i < n; ++i) out += (double)d[i].M * d[i].N;
        if (out / ((double)tiles * 128 * 384) < 0.85) return -1;
    }
    int splits, folds;
    g8_split_k(tiles, (K + 63) / 64, splits, folds);
    GP pv = {};
    pv.K = K, pv.taps = 1, pv.Tseq = 1, pv.ntiles = (int)tiles, pv.splitk = splits, pv.tiles_n = 1;
    pv.slab = g8_slab(stream, (size_t)tiles * splits * 49152 * sizeof(float));
    if (!pv.slab) return (int)hipErrorOutOfMemory;
    launch_tn(gemm_bf16_8p_tn3_kernel<false>, (int)(tiles * splits), stream, pv, grp);
    GP pf = pv;
    pf.splitk = folds;
    hipLaunchKernelGGL((gemm_8p_tn_fold_kernel<1, 3>), dim3(48, (unsigned)tiles), dim3(256), 0, stream, pf, grp);
    a3t_note_kernel("gemm_bf16_8p_tn3_kernel<false>");
    return (int)hipGetLastError();
}
