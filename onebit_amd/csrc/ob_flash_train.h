// Causal self-attention for TRAINING on gfx950: forward with softmax statistics, and the backward (dq, dk, dv).  fp16, head_dim 64 /
// 128, GQA, no KV cache and no `past`; flash style in both directions -- no [S, S] tensor in HBM, fp32 statistics and sums, MFMA
// 16x16x32 f16 -- and NO atomics: every output element is summed by one lane in a fixed order, so the gradients are bit-reproducible.
// The eager counterpart is modeling_bitllama.py:389-406 (scores / sqrt(D) + causal mask, softmax in fp32, probabilities . v).
//
// Layout: q, o, dO, dq [B, S, H, D] and k, v, dk, dv [B, S, Hkv, D], token-major -- the contiguous views of the projections' outputs,
// so the model makes no transposed copy in either direction.  lse [B, H, S] fp32 (natural log of the row's sum of exp(score)),
// delta [B, H, S] fp32 (workspace).  ob_flash.h (the inference prefill kernel) reads K / V in the cache layout [B][Hkv][max_len][D]
// and is tuned around that; these kernels are SIBLINGS that share its arithmetic (transposed products, deferred running maximum,
// ds_read_b64_tr_b16 operand reads) and its helpers, not its staging pipeline: ob_flash.h and its instantiations are untouched.
//
// One scheme serves all four matrix-product chains.  A workgroup (4 waves) OWNS 64 rows -- queries (forward, dQ) or keys (dK / dV)
// -- 16 per wave, held as MFMA B operands in registers (lane: row lane & 15, 8 consecutive d), and SWEEPS 64-row tiles of the other
// side through LDS.  With `own` the wave's rows and `swp` a tile's:
//   first product   C[swp][own] = T . X^T      A = rows of the LDS tile T (one 16-byte read per lane), B = the owner fragment X
//                   -> a lane holds 4 consecutive swept rows (4 (lane >> 4) + e) of ONE owner row (lane & 15), per 16-row tile
//   second product  acc[d][own] += T^T . C     B = C: the lane's 4 + 4 swept rows of two adjacent tiles ARE its 8 k-elements,
//                   A = T^T by the transposing LDS read (two ds_read_b64_tr_b16 of the row-major tile, as ob_flash.h reads V)
//                   -> a lane holds 4 consecutive d of one owner row: one 8-byte store per 16-d tile at the end
//   forward  (own = queries, swp = keys):   S^T = K . Q^T, online softmax down the lane column, O^T += V^T . P^T
//   delta    (own = queries, swp = keys):   S^T = K . Q^T, dP^T = V . dO^T, delta = sum over the keys of P dP
//   dQ       (own = queries, swp = keys):   S^T = K . Q^T, dP^T = V . dO^T, dS = P (dP - delta), dQ^T += K^T . dS^T
//   dK / dV  (own = keys, swp = queries):   S = Q . K^T, dP = dO . V^T, dV^T += dO^T . P, dK^T += Q^T . dS; sweeps every query
//            block at or below the diagonal, of every query head of the kv head's group
// P is recomputed as exp2(score * scale * log2e - lse * log2e); `scale` multiplies dQ and dK in fp32 at the store.  Blocks above the
// diagonal are never loaded; only blocks that touch the diagonal (or, for dK / dV, the last query block) are masked per element, by
// SELECTING 0 for P, so an out-of-range row or key contributes exactly zero; rows past S are staged as zeros, never read.
// Rounding points that differ from eager: scores stay fp32 (eager rounds q k^T to fp16 before the softmax), P and dS are rounded to
// fp16 once as MFMA operands, every sum is fp32.
// The tiles are single-buffered with two barriers per block: this is the plain form of the scheme, measured in
// profiles/train_attention.txt; the staging pipeline of ob_flash.h is the known next step.
#pragma once
#include "ob_flash.h"       // ob_fl_col_max / ob_fl_col_sum, OB_FL_DEFER_THR

#define OB_FT_BLK 64
#define OB_FT_THREADS 256
#define OB_FT_PAD 8         // halves: a 16-lane group of the row reads (16 rows x 16 bytes) then covers all 64 banks once

struct ObFlashTrainArgs {
    const _Float16 *q, *k, *v;      // [B, S, H, D], [B, S, Hkv, D] x 2
    _Float16 *o;                    // [B, S, H, D]: written by the forward (the backward does not read it: see the delta kernel)
    float *lse;                     // [B, H, S]: written by the forward, read by the backward
    const _Float16 *d_o;            // [B, S, H, D]
    float *delta;                   // [B, H, S]
    _Float16 *dq, *dk, *dv;
    int B, S, H, Hkv, nblk;         // nblk = ceil(S / 64)
    float scale, scale_log2e;       // 1 / sqrt(D), log2(e) / sqrt(D)
};

typedef short ob_ft_v4s __attribute__((ext_vector_type(4)));
typedef short ob_ft_v8s __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) ob_ft_v4s ob_ft_lds_v4s;

// rows r0 .. r0 + 63 of a token-major [S][ld] matrix (D halves of each) -> LDS, rows past S as zeros
template <int D>
__device__ __forceinline__ void ob_ft_stage(_Float16 (*dst)[D + OB_FT_PAD], const _Float16 *src, int64_t ld, int r0, int S)
{
    constexpr int NPC = D / 8;
#pragma unroll
    for (int i = 0; i < OB_FT_BLK * NPC / OB_FT_THREADS; ++i) {
        const int idx = threadIdx.x + OB_FT_THREADS * i, r = idx / NPC, pc = idx % NPC;
        ob_u32x4 val = {0u, 0u, 0u, 0u};
        if (r0 + r < S) val = *reinterpret_cast<const ob_u32x4 *>(src + (int64_t)(r0 + r) * ld + 8 * pc);
        *reinterpret_cast<ob_u32x4 *>(&dst[r][8 * pc]) = val;
    }
}

// owner fragment: lane (row lr of the wave's 16, d = 32 ds + 8 g .. + 7); zeros past S
template <int D>
__device__ __forceinline__ void ob_ft_owner(ob_half8 (&f)[D / 32], const _Float16 *src, int64_t ld, int row, int S, int g)
{
#pragma unroll
    for (int ds = 0; ds < D / 32; ++ds) {
        ob_u32x4 val = {0u, 0u, 0u, 0u};
        if (row < S) val = *reinterpret_cast<const ob_u32x4 *>(src + (int64_t)row * ld + 32 * ds + 8 * g);
        f[ds] = __builtin_bit_cast(ob_half8, val);
    }
}

// first product of k-step ks (tile rows 32 ks .. + 31): c[t][e] = <tile row 32 ks + 16 t + 4 g + e, owner row lr>
template <int D>
__device__ __forceinline__ void ob_ft_prod1(ob_float4 (&c)[2], const _Float16 (*tile)[D + OB_FT_PAD], const ob_half8 (&x)[D / 32], int ks, int lr, int g)
{
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        c[t] = (ob_float4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ds = 0; ds < D / 32; ++ds) {
            const ob_half8 a = *reinterpret_cast<const ob_half8 *>(&tile[32 * ks + 16 * t + lr][32 * ds + 8 * g]);
            c[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, x[ds], c[t], 0, 0, 0);
        }
    }
}

// second product of k-step ks: acc[dt][e] (d = 16 dt + 4 g + e of owner row lr) += sum over the 32 tile rows of tile[row][d] * p[row];
// p = the lane's values of rows 32 ks + 4 g + e (elements 0-3) and 32 ks + 16 + 4 g + e (elements 4-7).  The transposing read: in a
// 16-lane group lane i gives the address of chunk (row i >> 2, columns 4 (i & 3) .. + 3) of a 4 x 16 block and receives column i.
template <int D>
__device__ __forceinline__ void ob_ft_prod2(ob_float4 (&acc)[D / 16], const _Float16 (*tile)[D + OB_FT_PAD], const ob_half8 p, int ks, int lr, int g)
{
    const _Float16 *base = &tile[32 * ks + 4 * g + (lr >> 2)][4 * (lr & 3)];
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt) {
        const ob_ft_v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((ob_ft_lds_v4s *)(base + 16 * dt));
        const ob_ft_v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((ob_ft_lds_v4s *)(base + 16 * (D + OB_FT_PAD) + 16 * dt));
        const ob_ft_v8s a8 = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(ob_half8, a8), p, acc[dt], 0, 0, 0);
    }
}

__device__ __forceinline__ ob_half8 ob_ft_pack(const ob_float4 (&c)[2])
{
    ob_half8 p;
#pragma unroll
    for (int e = 0; e < 4; ++e) { p[e] = (_Float16)c[0][e]; p[4 + e] = (_Float16)c[1][e]; }
    return p;
}

// acc[dt] (x mul) -> row `dst` (D halves), 4 halves per 16-d tile at d = 16 dt + 4 g
template <int D>
__device__ __forceinline__ void ob_ft_store_row(_Float16 *dst, const ob_float4 (&acc)[D / 16], float mul, int g)
{
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt) {
        ob_half4 ov;
#pragma unroll
        for (int e = 0; e < 4; ++e) ov[e] = (_Float16)(acc[dt][e] * mul);
        *reinterpret_cast<ob_half4 *>(dst + 16 * dt + 4 * g) = ov;
    }
}

// workgroup id -> (block, batch * head): the heaviest blocks (`heavy_last`: the highest block index sweeps most; else the lowest) first
__device__ __forceinline__ void ob_ft_ids(int nbh, int nblk, bool heavy_last, int &blk, int &bh)
{
    const int i = (int)blockIdx.x / nbh;
    bh = (int)blockIdx.x % nbh;
    blk = heavy_last ? nblk - 1 - i : i;
}

// ---- forward: o and lse ------------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(OB_FT_THREADS) void ob_flash_train_fwd_kernel(const ObFlashTrainArgs A)
{
    constexpr int DT = D / 16, DK = D / 32;
    __shared__ __attribute__((aligned(16))) _Float16 Ks[OB_FT_BLK][D + OB_FT_PAD];
    __shared__ __attribute__((aligned(16))) _Float16 Vs[OB_FT_BLK][D + OB_FT_PAD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, g = lane >> 4;
    int ib, bh;
    ob_ft_ids(A.B * A.H, A.nblk, true, ib, bh);
    const int head = bh % A.H, b = bh / A.H, kvh = head / (A.H / A.Hkv), S = A.S;
    const int64_t ldq = (int64_t)A.H * D, ldk = (int64_t)A.Hkv * D;
    const _Float16 *qb = A.q + ((int64_t)b * S * A.H + head) * D;
    const _Float16 *kb = A.k + ((int64_t)b * S * A.Hkv + kvh) * D, *vb = A.v + ((int64_t)b * S * A.Hkv + kvh) * D;
    const int row = ib * OB_FT_BLK + 16 * wave + lr;            // this lane's query
    ob_half8 qf[DK];
    ob_ft_owner<D>(qf, qb, ldq, row, S, g);
    ob_float4 acc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) acc[dt] = (ob_float4){0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;

    for (int jb = 0; jb <= ib; ++jb) {
        __syncthreads();                                        // the previous tile's readers are done
        ob_ft_stage<D>(Ks, kb, ldk, jb * OB_FT_BLK, S);
        ob_ft_stage<D>(Vs, vb, ldk, jb * OB_FT_BLK, S);
        __syncthreads();
        ob_float4 sc[2][2];
        ob_ft_prod1<D>(sc[0], Ks, qf, 0, lr, g);
        ob_ft_prod1<D>(sc[1], Ks, qf, 1, lr, g);
        if (jb == ib) {                                         // the diagonal block (keys past S are above every stored query's diagonal)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (jb * OB_FT_BLK + 32 * ks + 16 * t + 4 * g + e > row) sc[ks][t][e] = -INFINITY;
        }
        float mx = sc[0][0][0];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int e = 0; e < 4; ++e) mx = fmaxf(mx, sc[ks][t][e]);
        mx = ob_fl_col_max(mx);
        // the deferred running maximum of ob_flash.h: it moves only when some query of the tile sees a maximum more than
        // 2^OB_FL_DEFER_THR above it (wave-uniform).  lse below is formed from whatever maximum the row ended with, so it is
        // exact either way: l_run is the sum of exp2(s - m_run) under the SAME m_run.
        if (__builtin_amdgcn_ballot_w64((mx - m_run) * A.scale_log2e > OB_FL_DEFER_THR) != 0) {
            const float m_new = fmaxf(m_run, mx);
            const float alpha = m_new == -INFINITY ? 1.f : __builtin_amdgcn_exp2f((m_run - m_new) * A.scale_log2e);
            l_run *= alpha;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) acc[dt] *= alpha;
            m_run = m_new;
        }
        const float nm = m_run == -INFINITY ? 0.f : -m_run * A.scale_log2e;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(sc[ks][t][e], A.scale_log2e, nm));
                    sc[ks][t][e] = p;
                    l_run += p;
                }
            ob_ft_prod2<D>(acc, Vs, ob_ft_pack(sc[ks]), ks, lr, g);
        }
    }
    const float l = ob_fl_col_sum(l_run);
    if (row < S) {
        ob_ft_store_row<D>(A.o + ((int64_t)(b * (int64_t)S + row) * A.H + head) * D, acc, l > 0.f ? 1.0f / l : 0.f, g);
        if (g == 0) A.lse[((int64_t)b * A.H + head) * S + row] = (m_run * A.scale_log2e + __builtin_amdgcn_logf(l)) * 0.6931471805599453f;
    }
}

// ---- delta[b, h, s] = sum_j P_ij dP_ij (fp32): the first two products of the dQ sweep, summed down the lane column ---------------
// In exact arithmetic this is sum_d dO . O.  It is NOT formed that way: o is rounded to fp16, and where one key holds nearly all of a
// row's probability dS = P (dP - delta) is a small difference of two nearly equal numbers -- delta from the rounded o then carries
// an error of 2^-11 |dO| |o| sqrt(D) into it, as large as dS itself (measured: 4 % of |dq| on the three-spike rows of
// tests/test_gpu_train_attention.py, ten times eager fp16's own error).  Summed from the SAME fp32 P and dP that dS is formed from,
// the difference cancels as it does in eager's fp32 softmax backward.  Cost: two more products per (query, key) pair, 9 instead of 7.
template <int D>
__global__ __launch_bounds__(OB_FT_THREADS) void ob_flash_train_delta_kernel(const ObFlashTrainArgs A)
{
    constexpr int DK = D / 32;
    __shared__ __attribute__((aligned(16))) _Float16 Ks[OB_FT_BLK][D + OB_FT_PAD];
    __shared__ __attribute__((aligned(16))) _Float16 Vs[OB_FT_BLK][D + OB_FT_PAD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, g = lane >> 4;
    int ib, bh;
    ob_ft_ids(A.B * A.H, A.nblk, true, ib, bh);
    const int head = bh % A.H, b = bh / A.H, kvh = head / (A.H / A.Hkv), S = A.S;
    const int64_t ldq = (int64_t)A.H * D, ldk = (int64_t)A.Hkv * D;
    const int64_t qoff = ((int64_t)b * S * A.H + head) * D, koff = ((int64_t)b * S * A.Hkv + kvh) * D;
    const int row = ib * OB_FT_BLK + 16 * wave + lr;
    ob_half8 qf[DK], gf[DK];
    ob_ft_owner<D>(qf, A.q + qoff, ldq, row, S, g);
    ob_ft_owner<D>(gf, A.d_o + qoff, ldq, row, S, g);
    const int64_t st = ((int64_t)b * A.H + head) * S + row;
    const float nl = row < S ? -A.lse[st] * 1.4426950408889634f : 0.f;
    float dsum = 0.f;
    for (int jb = 0; jb <= ib; ++jb) {
        __syncthreads();
        ob_ft_stage<D>(Ks, A.k + koff, ldk, jb * OB_FT_BLK, S);
        ob_ft_stage<D>(Vs, A.v + koff, ldk, jb * OB_FT_BLK, S);
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            ob_float4 sc[2], dp[2];
            ob_ft_prod1<D>(sc, Ks, qf, ks, lr, g);
            ob_ft_prod1<D>(dp, Vs, gf, ks, lr, g);
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float p = __builtin_amdgcn_exp2f(__builtin_fmaf(sc[t][e], A.scale_log2e, nl));
                    if (jb == ib && jb * OB_FT_BLK + 32 * ks + 16 * t + 4 * g + e > row) p = 0.f;
                    dsum = __builtin_fmaf(p, dp[t][e], dsum);
                }
        }
    }
    dsum = ob_fl_col_sum(dsum);
    if (row < S && g == 0) A.delta[st] = dsum;
}

// ---- dQ: own = 64 queries of one (batch, head), sweeps the key blocks up to the diagonal ------------------------------------------
template <int D>
__global__ __launch_bounds__(OB_FT_THREADS) void ob_flash_train_dq_kernel(const ObFlashTrainArgs A)
{
    constexpr int DT = D / 16, DK = D / 32;
    __shared__ __attribute__((aligned(16))) _Float16 Ks[OB_FT_BLK][D + OB_FT_PAD];
    __shared__ __attribute__((aligned(16))) _Float16 Vs[OB_FT_BLK][D + OB_FT_PAD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, g = lane >> 4;
    int ib, bh;
    ob_ft_ids(A.B * A.H, A.nblk, true, ib, bh);
    const int head = bh % A.H, b = bh / A.H, kvh = head / (A.H / A.Hkv), S = A.S;
    const int64_t ldq = (int64_t)A.H * D, ldk = (int64_t)A.Hkv * D;
    const int64_t qoff = ((int64_t)b * S * A.H + head) * D, koff = ((int64_t)b * S * A.Hkv + kvh) * D;
    const int row = ib * OB_FT_BLK + 16 * wave + lr;
    ob_half8 qf[DK], gf[DK];
    ob_ft_owner<D>(qf, A.q + qoff, ldq, row, S, g);
    ob_ft_owner<D>(gf, A.d_o + qoff, ldq, row, S, g);
    const int64_t st = ((int64_t)b * A.H + head) * S + row;
    const float nl = row < S ? -A.lse[st] * 1.4426950408889634f : 0.f, dl = row < S ? A.delta[st] : 0.f;
    ob_float4 acc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) acc[dt] = (ob_float4){0.f, 0.f, 0.f, 0.f};

    for (int jb = 0; jb <= ib; ++jb) {
        __syncthreads();
        ob_ft_stage<D>(Ks, A.k + koff, ldk, jb * OB_FT_BLK, S);
        ob_ft_stage<D>(Vs, A.v + koff, ldk, jb * OB_FT_BLK, S);
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            ob_float4 sc[2], dp[2];
            ob_ft_prod1<D>(sc, Ks, qf, ks, lr, g);
            ob_ft_prod1<D>(dp, Vs, gf, ks, lr, g);
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float p = __builtin_amdgcn_exp2f(__builtin_fmaf(sc[t][e], A.scale_log2e, nl));
                    if (jb == ib && jb * OB_FT_BLK + 32 * ks + 16 * t + 4 * g + e > row) p = 0.f;
                    sc[t][e] = p * (dp[t][e] - dl);
                }
            ob_ft_prod2<D>(acc, Ks, ob_ft_pack(sc), ks, lr, g);
        }
    }
    if (row < S) ob_ft_store_row<D>(A.dq + qoff + (int64_t)row * ldq, acc, A.scale, g);
}

// ---- dK / dV: own = 64 keys of one (batch, kv head), sweeps the query blocks from the diagonal down, of every head of the group ----
template <int D>
__global__ __launch_bounds__(OB_FT_THREADS) void ob_flash_train_dkv_kernel(const ObFlashTrainArgs A)
{
    constexpr int DT = D / 16, DK = D / 32;
    __shared__ __attribute__((aligned(16))) _Float16 Qs[OB_FT_BLK][D + OB_FT_PAD];
    __shared__ __attribute__((aligned(16))) _Float16 Gs[OB_FT_BLK][D + OB_FT_PAD];
    __shared__ __attribute__((aligned(16))) float Ls[OB_FT_BLK], Ds[OB_FT_BLK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, g = lane >> 4;
    int jb, bk;
    ob_ft_ids(A.B * A.Hkv, A.nblk, false, jb, bk);
    const int kvh = bk % A.Hkv, b = bk / A.Hkv, rep = A.H / A.Hkv, S = A.S;
    const int64_t ldq = (int64_t)A.H * D, ldk = (int64_t)A.Hkv * D;
    const int64_t koff = ((int64_t)b * S * A.Hkv + kvh) * D;
    const int key = jb * OB_FT_BLK + 16 * wave + lr;            // this lane's key
    ob_half8 kf[DK], vf[DK];
    ob_ft_owner<D>(kf, A.k + koff, ldk, key, S, g);
    ob_ft_owner<D>(vf, A.v + koff, ldk, key, S, g);
    ob_float4 acc_k[DT], acc_v[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) acc_k[dt] = acc_v[dt] = (ob_float4){0.f, 0.f, 0.f, 0.f};

    for (int hq = kvh * rep; hq < (kvh + 1) * rep; ++hq) {
        const int64_t qoff = ((int64_t)b * S * A.H + hq) * D, st = ((int64_t)b * A.H + hq) * S;
        for (int ib = jb; ib < A.nblk; ++ib) {
            const int q0 = ib * OB_FT_BLK;
            __syncthreads();
            ob_ft_stage<D>(Qs, A.q + qoff, ldq, q0, S);
            ob_ft_stage<D>(Gs, A.d_o + qoff, ldq, q0, S);
            if (threadIdx.x < OB_FT_BLK) Ls[threadIdx.x] = q0 + (int)threadIdx.x < S ? -A.lse[st + q0 + threadIdx.x] * 1.4426950408889634f : 0.f;
            else if (threadIdx.x < 2 * OB_FT_BLK) Ds[threadIdx.x - OB_FT_BLK] = q0 + (int)threadIdx.x - OB_FT_BLK < S ? A.delta[st + q0 + threadIdx.x - OB_FT_BLK] : 0.f;
            __syncthreads();
            const bool edge = ib == jb || ib == A.nblk - 1;     // the diagonal, or queries past S
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                ob_float4 sc[2], dp[2];
                ob_ft_prod1<D>(sc, Qs, kf, ks, lr, g);
                ob_ft_prod1<D>(dp, Gs, vf, ks, lr, g);
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const int r = 32 * ks + 16 * t + 4 * g;
                    const ob_float4 nl = *reinterpret_cast<const ob_float4 *>(&Ls[r]), dl = *reinterpret_cast<const ob_float4 *>(&Ds[r]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float p = __builtin_amdgcn_exp2f(__builtin_fmaf(sc[t][e], A.scale_log2e, nl[e]));
                        if (edge && (key > q0 + r + e || q0 + r + e >= S)) p = 0.f;
                        sc[t][e] = p;
                        dp[t][e] = p * (dp[t][e] - dl[e]);
                    }
                }
                ob_ft_prod2<D>(acc_v, Gs, ob_ft_pack(sc), ks, lr, g);
                ob_ft_prod2<D>(acc_k, Qs, ob_ft_pack(dp), ks, lr, g);
            }
        }
    }
    if (key < S) {
        ob_ft_store_row<D>(A.dk + koff + (int64_t)key * ldk, acc_k, A.scale, g);
        ob_ft_store_row<D>(A.dv + koff + (int64_t)key * ldk, acc_v, 1.f, g);
    }
}
