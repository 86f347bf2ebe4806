// mfma_kit.h -- what the hand-scheduled MFMA kernels (gemm_bf16_8p / _tn / _pn / _tt.hip) write their schedules with: fragment
// types, scheduling and wait macros, the 16-byte LDS-DMA as inline asm, the DPP row sum and the XCD-contiguous block order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define LDS_AS(p) ((__attribute__((address_space(3))) void*)(p))
#define SB() __builtin_amdgcn_sched_barrier(0)
#define BAR()                                   \
    do {                                        \
        SB();                                   \
        asm volatile("s_barrier" ::: "memory"); \
        SB();                                   \
    } while (0)
#define WAIT_VM(n) asm volatile("s_waitcnt vmcnt(" #n ")" ::: "memory")
#define WAIT_LGKM(n) asm volatile("s_waitcnt lgkmcnt(" #n ")" ::: "memory")

constexpr unsigned OOB = 0x80000000u;         // voffset beyond every descriptor (host contract: operands < 2 GiB)

// LDS-DMA piece (64 lanes x 16 B -> 1 KiB at the wave-uniform LDS byte address `lds_addr`) as INLINE ASM, for the kernels that read
// their fragments with __builtin_amdgcn_ds_read_tr16_b64: in front of that builtin hipcc waits vmcnt(0) for every LDS-DMA it has
// seen issued through __builtin_amdgcn_raw_ptr_buffer_load_lds (it cannot tell that the transposed read does not alias the tiles
// in flight): one full drain of the DMA queue at the top of every phase -- the counted waits of the schedule never got to wait for
// anything (found in the .s of both token-reduction kernels: 7 "s_waitcnt vmcnt(0)" in the K loop; the k-contiguous kernels, whose
// fragments are plain ds_read_b128, have none).  An asm DMA is invisible to that bookkeeping; the kernels wait for it themselves
// (counted vmcnt + s_barrier, as written).  M0 is set in the same statement that uses it; it cannot be listed as a clobber (hipcc
// rejects reserved registers there), so the kernels that call this use no other M0 consumer.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "buffer_load_dwordx4 ... lds (16-byte LDS-DMA) exists on gfx950 only: build with --offload-arch=gfx950"
#endif
__device__ __forceinline__ void dma16(const __amdgpu_buffer_rsrc_t& r, unsigned lds_addr, unsigned voff, unsigned soff) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" ::"s"(lds_addr), "v"(voff), "s"(r), "s"(soff) : "memory");
}

__device__ __forceinline__ float row16_sum(float v) {   // sum over the 16 lanes of a DPP row, result in every lane
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, true));   // quad_perm [1,0,3,2]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xf, 0xf, true));   // quad_perm [2,3,0,1]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xf, 0xf, true));  // row_half_mirror
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xf, 0xf, true));  // row_mirror
    return v;
}

// Bijective block remap: the hardware deals workgroup b to XCD b % 8; workgroup wi of nwg takes the work item that gives every
// XCD a CONTIGUOUS run of items (neighbouring tiles, the tiles of one K split, the row tiles of one batch element share an L2).
__device__ __forceinline__ int xcd_contiguous(int wi, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, xcd = wi & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (wi >> 3);
}
