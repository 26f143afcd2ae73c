// mvm_batch_device.h -- the stochastic-rounding plumbing shared by the batched mvm kernels: k_m4_mvm_batch (mvm_batch4.hip),
// k_m4_mvm8_batch (mvm_batch8.hip), k_m8_mvm_batch (matrix8_batch.hip), k_m4_mvm_t_batch (mvm_t4_batch.hip), k_m4_mvm8_t_batch (mvm_t8_batch.hip) and k_m8_mvm_t_batch (matrix8_t_batch.hip).  All place a vector's draws where the sequence of single calls has them, by the same jump-ahead.
#pragma once

#include "rng_device.h"

// ST: where the draws of the launch lie in the XORShift stream, counted in draws (one draw = one step of the 4-lane generator) from the
// state the launch reads.  Slot v's window begins at draw_base + v * draw_stride: row group rb uses draws 2 rb, 2 rb + 1 of it for the mvm
// and, with FUSE, 2 G + 2 rb, 2 G + 2 rb + 1 for the scaleAndAdd (G = row groups), as the single-vector kernels do from position 0.
// commit_draws == 0: the launch leaves the state as it is (no slot, no stamp written); otherwise workgroup 0 writes the state advanced by
// commit_draws.
struct MvmBatchRng {
    uint64_t *state;
    uint64_t seq;
    const uint64_t *pow_rows;
    uint64_t draw_base, draw_stride, commit_draws;
};

// T^(e[i])(v0) for NE wave-uniform exponents at once (wave_pow_apply for one).  The rows of a table level are the same for every exponent:
// one memory round trip per 8 bits of the LARGEST exponent serves all of them, and the NE chains of ballots are independent of each other,
// so they overlap instead of queueing behind NE x (round trip + chain).  Powers of one matrix commute: any order of the levels.
template <int NE>
__device__ __forceinline__ void wave_pow_apply_many(const uint64_t *__restrict__ pow_rows, uint64_t v0, uint64_t *e, uint64_t *v)
{
    const uint64_t *row = pow_rows + (threadIdx.x & 63);
    uint64_t any = 0;
    v0 = uniform64(v0);
#pragma unroll
    for (int i = 0; i < NE; i++) {
        e[i] = uniform64(e[i]);
        v[i] = v0;
        any |= e[i];
    }
    while (any) {
        uint64_t R[8];
#pragma unroll
        for (int k = 0; k < 8; k++) R[k] = ((any >> k) & 1ull) ? row[64 * k] : 0ull;
#pragma unroll
        for (int k = 0; k < 8; k++)
#pragma unroll
            for (int i = 0; i < NE; i++)
                if ((e[i] >> k) & 1ull) v[i] = wave_matvec(R[k], v[i]);
#pragma unroll
        for (int i = 0; i < NE; i++) e[i] >>= 8;
        any >>= 8;
        row += 8 * 64;
    }
}

// the noise of an epilogue lane from the window whose four lane starts are base[0..3]: the window's two draws are generated in the
// lane itself (gen_blocks on generator lane j >> 1; every lane of an AVX lane pair repeats them, which costs a wave nothing), then
// dword j of the eight of draw grp >> 2, byte grp & 3 -- what the single-vector kernels read from their raw[]
__device__ __forceinline__ float mvmb_noise(const uint64_t *base, int grp, int j)
{
    uint64_t raw[8];
    gen_blocks(base[j >> 1], 1, raw, 0);                       // raw[0], raw[4]: this generator lane's output of draw 0, draw 1
    const uint64_t o = (grp >> 2) ? raw[4] : raw[0];
    return noise_of((j & 1) ? (uint32_t)(o >> 32) : (uint32_t)o, grp & 3);
}

// The jump-ahead of a batched launch, in the PROLOGUE, before x is staged (256 threads: wave k owns generator lane k): T^e applied to
// the state the launch reads, for every vector and window in one walk over the table levels (NV = 8 fused: two), the starts left in
// sbase[(v * NW + w) * 4 + k]; nothing of it lives in registers across the column loop.  NW = windows per vector (the mvm's draws,
// the scaleAndAdd's).  rb = the workgroup's (first) output block, G = the output blocks of the launch: one block per workgroup in the
// row-major kernels (G = gridDim.x), MVT_W / MVT8B_W / M8TB_W consecutive ones in the transposed kernels (mvm_t4_batch.hip, mvm_t8_batch.hip, matrix8_t_batch.hip), whose starts are those of rb.  Returns, in workgroup 0 of a committing launch, the slot whose state this wave has written -- the caller stamps
// it with st_seq behind its last barrier (mvmb_rng_stamp) -- and NULL elsewhere.
template <int NV, int NW>
__device__ __forceinline__ uint64_t *mvmb_rng_prologue(const MvmBatchRng &rs, int nv, uint64_t rb, uint64_t G, uint64_t *sbase, uint64_t &st_seq)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t *st_next = nullptr;
    st_seq = rng_effective_seq(rs.state, rs.seq);
    const int slot = rng_read_slot(rs.state, st_seq);
    const uint64_t a0 = rs.state[slot * RNG_SLOT_WORDS + 4 + wave];
    // exponent NV * NW: the committed state, workgroup 0 only (what rng_commit writes; the stamp follows the last barrier)
    const bool commits = rs.commit_draws && rb == 0;
    uint64_t e[NV * NW + 1], b[NV * NW + 1];
#pragma unroll
    for (int v = 0; v < NV; v++)
#pragma unroll
        for (int w = 0; w < NW; w++)
            e[v * NW + w] = v < nv ? rs.draw_base + (uint64_t)v * rs.draw_stride + 2 * (rb + (uint64_t)w * G) : 0;
    e[NV * NW] = commits ? rs.commit_draws - 1 : 0;
    // at most 9 exponents per walk: the values and exponents live in SGPR pairs, and 17 of each spill
    constexpr int NE = NV * NW + 1, H = NE <= 9 ? NE : NE / 2;
    wave_pow_apply_many<H>(rs.pow_rows, a0, e, b);
    if constexpr (H < NE) wave_pow_apply_many<NE - H>(rs.pow_rows, a0, e + H, b + H);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < NV * NW; i++) sbase[i * 4 + wave] = b[i];      // read in the epilogue, barriers in between
    }
    if (commits) {
        st_next = rs.state + (slot ^ 1) * RNG_SLOT_WORDS;
        if (lane == 0) {
            st_next[wave] = b[NV * NW];
            st_next[4 + wave] = xs_T(b[NV * NW]);
        }
    }
    return st_next;
}

// behind a barrier that follows the prologue: every wave's part of the new state has been written
__device__ __forceinline__ void mvmb_rng_stamp(uint64_t *st_next, uint64_t st_seq)
{
    if (st_next && threadIdx.x == 0) {
        __threadfence();
        st_next[RNG_STAMP_WORD] = st_seq;
    }
}
