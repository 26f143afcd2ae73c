// half16_device.h -- what the half-precision kernels of half16.hip (one vector) and half16_batch.hip (several vectors, one matrix pass)
// share: the binary16 conversions, the 32 chains and their tree, the fused scaleAndAdd epilogue and the streaming rule.  Everything here
// was written in half16.hip and is stated once so that the batched kernel runs, per vector, the instruction sequence of k_f16_mvm.
#pragma once

#include "dot_common.h"

typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ uint16_t f16_bits(float f)
{
    const _Float16 h = (_Float16)f;
    uint16_t b;
    __builtin_memcpy(&b, &h, 2);
    return b;
}

template <bool NT, typename T> __device__ __forceinline__ T ld_stream(const T *p) { return NT ? __builtin_nontemporal_load(p) : *p; }
template <bool NT, typename T> __device__ __forceinline__ void st_stream(T v, T *p)
{
    if (NT) __builtin_nontemporal_store(v, p);
    else *p = v;
}

// ================================================================================================
// the 32 chains and their tree
// ================================================================================================
// A quad of lanes owns one row (or the one dot): lane p = tid & 3 keeps accumulator p of the reference's four __m256 -- chains
// 8p .. 8p + 7 -- in acc[0..7].  A 16-byte load is 8 consecutive elements, i.e. one step of those 8 chains; the quad reads the 64
// contiguous bytes of a 32-element step.
__device__ __forceinline__ void f16_chain_step(const h16x8 a, const h16x8 x, float acc[8])
{
#pragma unroll
    for (int l = 0; l < 8; l++) acc[l] = __builtin_fmaf((float)x[l], (float)a[l], acc[l]);
}
__device__ __forceinline__ void f16_chain_step(const h16x8 a, const f32x4 x0, const f32x4 x1, float acc[8])
{
    acc[0] = __builtin_fmaf(x0.x, (float)a[0], acc[0]);
    acc[1] = __builtin_fmaf(x0.y, (float)a[1], acc[1]);
    acc[2] = __builtin_fmaf(x0.z, (float)a[2], acc[2]);
    acc[3] = __builtin_fmaf(x0.w, (float)a[3], acc[3]);
    acc[4] = __builtin_fmaf(x1.x, (float)a[4], acc[4]);
    acc[5] = __builtin_fmaf(x1.y, (float)a[5], acc[5]);
    acc[6] = __builtin_fmaf(x1.z, (float)a[6], acc[6]);
    acc[7] = __builtin_fmaf(x1.w, (float)a[7], acc[7]);
}

// (acc0 + acc1) + (acc2 + acc3) lane-wise, then _mm256_haddf32_ps (CloverBase.h:149-157): t[i] = s[i + 4] + s[i],
// (t0 + t2) + (t1 + t3).  acc0 + acc1 sits in lanes p, p ^ 1 of the quad, the sum of the two pairs in lanes p, p ^ 2: every lane of
// the quad ends with the value.
__device__ __forceinline__ float f16_chain_tree(const float acc[8])
{
    float s[8];
#pragma unroll
    for (int l = 0; l < 8; l++) {
        const float pair = acc[l] + __shfl_xor(acc[l], 1);
        s[l] = pair + __shfl_xor(pair, 2);
    }
    const float t0 = s[4] + s[0], t1 = s[5] + s[1], t2 = s[6] + s[2], t3 = s[7] + s[3];
    return (t0 + t2) + (t1 + t3);
}

// FUSE... = F16Fuse (clm_f16_mvm_scale_and_add, k_f16_mvm_saa in half16.hip): the CloverVector16::scaleAndAdd that follows this mvm in the IHT / GD loops
// (CloverVector16.h:309-386), done by the lane that stores the row: v = f16(d); r2[row] = f16(fma(f32(v), a, f32(u[row]))) -- the ROUNDED
// v widened again, as two separate calls compute.  A row depends on no other row: no workgroup-wide step.  u[row] is requested before the
// streaming loop.  r (the f16 A x, t of the ABI) may be NULL under FUSE: it is then not stored.
// The flag is a trailing parameter pack, empty or one F16Fuse, and the kernel itself is the shared template: with the body in an inlined
// device function the fp32-vector instantiations came out two instructions longer (another base for the unrolled loads); this way every
// <WAVES, NT, XF32> instantiation keeps its signature and, instruction for instruction, the code it had.
struct F16Fuse {
    const uint16_t *u;
    float a;
    uint16_t *r2;            // may alias u (the in-place form): a lane reads its element of u before it writes it
};
__device__ __forceinline__ uint16_t f16_fuse_load_u(uint64_t) { return 0; }
__device__ __forceinline__ uint16_t f16_fuse_load_u(uint64_t row, const F16Fuse &f) { return f.u[row]; }
__device__ __forceinline__ void f16_fuse_store(void *, uint64_t, float, uint16_t) {}
__device__ __forceinline__ void f16_fuse_store(void *t, uint64_t row, float d, uint16_t ub, const F16Fuse &f)
{
    _Float16 v = (_Float16)d, uh;                                        // _mm256_cvtps_ph(.., 0) of the row block (:302-306)
    uint16_t vb;
    __builtin_memcpy(&vb, &v, 2);
    __builtin_memcpy(&uh, &ub, 2);
    if (t) reinterpret_cast<uint16_t *>(t)[row] = vb;
    // widening, fma and conversion stay the three instructions of k_f16_scale_and_add -- v_cvt_f32_f16, v_fma_f32, v_cvt_f16_f32 (left
    // alone, hipcc folds them into v_fma_mixlo_f16 here)
    float vf = (float)v;
    asm volatile("" : "+v"(vf));
    float s = __builtin_fmaf(vf, f.a, (float)uh);
    asm volatile("" : "+v"(s));
    f.r2[row] = f16_bits(s);
}

#define F16_ALIGNED(p) (((uintptr_t)(p) & 15u) == 0)

// streaming loads / stores once the operands cannot stay in the 256 MiB Infinity Cache (the clm4_mvm rule)
#define F16_STREAMING(bytes) ((bytes) > (256ull << 20))

// the workgroup rule of f16_mvm() (half16.hip), the batched launches' too: four waves (64 rows) per workgroup; one wave (16 rows) while
// that leaves fewer than two workgroups per CU
static inline bool f16_mvm_wide(uint64_t rows) { return rows / 64 >= 2 * (uint64_t)clv_cu_count(); }

// CloverVector16::clear() of n_pad elements on the stream, one launch (half16.hip): the first step of clm_f16_iht and clm_f16_iht_batch
int clv_internal_f16_clear(uint16_t *x, uint64_t n_pad, hipStream_t st);
