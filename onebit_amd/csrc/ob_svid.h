// SVID start-checkpoint kernels: the rank-1 NMF of |A| (A = a teacher projection [N, K], fp16 or fp32, row pitch lda) by
// alternating least squares -- what sklearn's coordinate-descent NMF does for n_components = 1 (scripts/build_start_ckpt.py:21-34)
// -- and the pass that emits sign(A) as latent weights and / or packed bits.  One iteration:
//     hh = h.h ; xh = |A| h ; viol_w = sum_i |pg(w_i, w_i hh - xh_i)| ; w = max(xh / hh, 0)   (w kept when hh == 0)
//     ww = w.w ; xw = |A|^T w ; viol_h = sum_j |pg(h_j, h_j ww - xw_j)| ; h = max(xw / ww, 0) (h kept when ww == 0)
//     pg(v, g) = v == 0 ? min(0, g) : g
// All arithmetic fp32, |A| is never materialised, no atomics: every sum has a fixed order (bit-reproducible).
//
// Rows are handled in chunks of 8 elements (16 bytes of fp16, two 16-byte loads of fp32); chunk c of a row belongs to thread
// c % THREADS of the workgroup, so consecutive lanes read consecutive 16 bytes.
//   one-pass  (K <= OB_SVID_ONEPASS_MAX_K = 16384): a workgroup owns a band of rows and keeps h and its column accumulators in
//             registers; it reads up to OB_SVID_R rows per step (K <= 4096: the next step's rows already in flight), dots them with h, reduces the
//             dots across the workgroup with ONE barrier per step, updates w_i and adds w_i |a_ij| to the accumulators out of the
//             same registers.  A is read once per iteration.  The band's column sums go to part[band][K].
//   two-pass  (any K % 8 == 0): ob_svid_rows_kernel (xh, w) then ob_svid_cols_kernel (part[band][column tile]).
//   both end with ob_svid_colfin_kernel (band partials summed in band order, h update) and ob_svid_stats_kernel.
#pragma once
#include "ob_common.h"

#define OB_SVID_ONEPASS_MAX_K 16384      // 1024 threads x 2 chunks x 8 elements
#define OB_SVID_R 4                       // rows per reduction step (at most; bands are multiples of it)
#define OB_SVID_STATS 4                   // {violation, hh, ww, hh of the updated h}
#define OB_SVID_FIN_COLS 64               // columns per workgroup of the column finalize (x 4 band groups = 256 threads)
#define OB_SVID_EMIT_ITERS 4              // chunks per thread of the emit pass

// |a| of one chunk as 8 floats
template <typename T> struct ObSvidChunk;
template <> struct ObSvidChunk<_Float16> {
    ob_u32x4 v;
    __device__ __forceinline__ void load(const _Float16 *p) { v = *reinterpret_cast<const ob_u32x4 *>(p); }
    __device__ __forceinline__ void zero() { v = ob_u32x4{0, 0, 0, 0}; }
    __device__ __forceinline__ float get(int i) const { return (float)__builtin_bit_cast(ob_half8, v)[i]; }
};
template <> struct ObSvidChunk<float> {
    ob_float4 lo, hi;
    __device__ __forceinline__ void load(const float *p)
    {
        lo = reinterpret_cast<const ob_float4 *>(p)[0];
        hi = reinterpret_cast<const ob_float4 *>(p)[1];
    }
    __device__ __forceinline__ void zero() { lo = ob_float4{0.f, 0.f, 0.f, 0.f}; hi = lo; }
    __device__ __forceinline__ float get(int i) const { return i < 4 ? lo[i] : hi[i - 4]; }
};

__device__ __forceinline__ void ob_svid_load8(const float *p, float (&o)[8])
{
    const ob_float4 a = reinterpret_cast<const ob_float4 *>(p)[0], b = reinterpret_cast<const ob_float4 *>(p)[1];
#pragma unroll
    for (int i = 0; i < 4; ++i) { o[i] = a[i]; o[4 + i] = b[i]; }
}
__device__ __forceinline__ void ob_svid_store8(float *p, const float (&o)[8])
{
    reinterpret_cast<ob_float4 *>(p)[0] = ob_float4{o[0], o[1], o[2], o[3]};
    reinterpret_cast<ob_float4 *>(p)[1] = ob_float4{o[4], o[5], o[6], o[7]};
}

// OB_SVID_R workgroup-wide sums with one barrier: red is [2][OB_SVID_R][16], `par` alternates between consecutive calls (a wave
// that runs ahead writes the other half; it cannot reach the call after that before every wave has left this one's reads)
template <int THREADS, int R>
__device__ __forceinline__ void ob_svid_reduce_r(float (&v)[R], float *red, int par)
{
    constexpr int NW = THREADS / 64;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float *base = red + par * (OB_SVID_R * 16);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const float s = ob_wave_sum(v[r]);
        if (lane == 0) base[r * 16 + wave] = s;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NW; ++i) s += base[r * 16 + i];
        v[r] = s;
    }
}

// the w side of the iteration for one row; every thread passes the same values.  Returns the new w_i; ww is kept by every
// thread, viol by thread 0 alone.  No thread reads w[row] while another stores it: with hh != 0 the new value needs no old one
// and thread 0 alone reads (for the violation) and then stores, with hh == 0 every thread reads and none stores (w is kept).
__device__ __forceinline__ float ob_svid_row_update(float *w, int row, float xh, float hh, float &ww, float &viol)
{
    const bool upd = hh != 0.f;
    const float wn = upd ? fmaxf(xh / hh, 0.f) : w[row];
    ww += wn * wn;
    if (threadIdx.x == 0) {
        const float wo = upd ? w[row] : wn;
        const float grad = wo * hh - xh;
        const float pg = wo == 0.f ? fminf(0.f, grad) : grad;
        viol += fabsf(pg);
        if (upd) w[row] = wn;
    }
    return wn;
}

// bandstat: [2 * nbands + 1] = {ww, viol_w} per band, then hh (written by band 0).  R rows per reduction step (band_rows is a
// multiple of OB_SVID_R >= R); PREFETCH keeps the next step's rows in flight in a second set of registers, which the 1024-thread
// forms (128 registers per thread) have no room for.
template <typename T, int THREADS, int NCH, int R, bool PREFETCH>
__global__ __launch_bounds__(THREADS) void ob_svid_onepass_kernel(const T *__restrict__ A, int64_t lda, float *w,
                                                                  const float *__restrict__ h, float *__restrict__ part,
                                                                  float *__restrict__ bandstat, int N, int K, int band_rows)
{
    __shared__ float red[2 * OB_SVID_R * 16];
    __shared__ float red1[16];
    const int tid = threadIdx.x, nchunks = K >> 3;
    float hv[NCH][8], acc[NCH][8];
    bool valid[NCH];
    float hsq = 0.f;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int c = tid + j * THREADS;
        valid[j] = c < nchunks;
        if (valid[j]) ob_svid_load8(h + 8 * c, hv[j]);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (!valid[j]) hv[j][i] = 0.f;
            acc[j][i] = 0.f;
            hsq += hv[j][i] * hv[j][i];
        }
    }
    const float hh = ob_block_sum(hsq, red1);
    const int row0 = blockIdx.x * band_rows, row1 = min(N, row0 + band_rows);
    float ww = 0.f, viol = 0.f;

    ObSvidChunk<T> cur[R][NCH], nxt[R][NCH];
    auto fetch = [&](ObSvidChunk<T> (&dst)[R][NCH], int r) {
#pragma unroll
        for (int rr = 0; rr < R; ++rr)
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                if (r + rr < row1 && valid[j]) dst[rr][j].load(A + (int64_t)(r + rr) * lda + 8 * (tid + j * THREADS));
                else dst[rr][j].zero();
            }
    };
    if (PREFETCH) fetch(nxt, row0);
    int par = 0;
    for (int r = row0; r < row1; r += R, par ^= 1) {
        if (PREFETCH) {
#pragma unroll
            for (int rr = 0; rr < R; ++rr)
#pragma unroll
                for (int j = 0; j < NCH; ++j) cur[rr][j] = nxt[rr][j];
            if (r + R < row1) fetch(nxt, r + R);
        } else {
            fetch(cur, r);
        }
        float dots[R];
#pragma unroll
        for (int rr = 0; rr < R; ++rr) {
            float d = 0.f;
#pragma unroll
            for (int j = 0; j < NCH; ++j)
#pragma unroll
                for (int i = 0; i < 8; ++i) d += fabsf(cur[rr][j].get(i)) * hv[j][i];
            dots[rr] = d;
        }
        ob_svid_reduce_r<THREADS, R>(dots, red, par);
#pragma unroll
        for (int rr = 0; rr < R; ++rr) {
            if (r + rr >= row1) break;
            const float wn = ob_svid_row_update(w, r + rr, dots[rr], hh, ww, viol);
#pragma unroll
            for (int j = 0; j < NCH; ++j)
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[j][i] += wn * fabsf(cur[rr][j].get(i));
        }
    }
#pragma unroll
    for (int j = 0; j < NCH; ++j)
        if (valid[j]) ob_svid_store8(part + (int64_t)blockIdx.x * K + 8 * (tid + j * THREADS), acc[j]);
    if (tid == 0) {
        bandstat[2 * blockIdx.x] = ww;
        bandstat[2 * blockIdx.x + 1] = viol;
        if (blockIdx.x == 0) bandstat[2 * gridDim.x] = hh;
    }
}

// two-pass, first half: xh of a band's rows for any K, then the same w update
template <typename T>
__global__ __launch_bounds__(256) void ob_svid_rows_kernel(const T *__restrict__ A, int64_t lda, float *w,
                                                           const float *__restrict__ h, float *__restrict__ bandstat, int N, int K,
                                                           int band_rows)
{
    __shared__ float red[2 * OB_SVID_R * 16];
    __shared__ float red1[16];
    const int tid = threadIdx.x, nchunks = K >> 3;
    float hsq = 0.f;
    for (int c = tid; c < nchunks; c += 256) {
        float hv[8];
        ob_svid_load8(h + 8 * c, hv);
#pragma unroll
        for (int i = 0; i < 8; ++i) hsq += hv[i] * hv[i];
    }
    const float hh = ob_block_sum(hsq, red1);
    const int row0 = blockIdx.x * band_rows, row1 = min(N, row0 + band_rows);
    float ww = 0.f, viol = 0.f;
    int par = 0;
    for (int r = row0; r < row1; r += OB_SVID_R, par ^= 1) {
        float dots[OB_SVID_R];
#pragma unroll
        for (int rr = 0; rr < OB_SVID_R; ++rr) dots[rr] = 0.f;
        for (int c = tid; c < nchunks; c += 256) {
            float hv[8];
            ob_svid_load8(h + 8 * c, hv);
            ObSvidChunk<T> a[OB_SVID_R];
#pragma unroll
            for (int rr = 0; rr < OB_SVID_R; ++rr) {
                if (r + rr < row1) a[rr].load(A + (int64_t)(r + rr) * lda + 8 * c);
                else a[rr].zero();
            }
#pragma unroll
            for (int rr = 0; rr < OB_SVID_R; ++rr)
#pragma unroll
                for (int i = 0; i < 8; ++i) dots[rr] += fabsf(a[rr].get(i)) * hv[i];
        }
        ob_svid_reduce_r<256, OB_SVID_R>(dots, red, par);
#pragma unroll
        for (int rr = 0; rr < OB_SVID_R; ++rr) {
            if (r + rr >= row1) break;
            ob_svid_row_update(w, r + rr, dots[rr], hh, ww, viol);
        }
    }
    if (tid == 0) {
        bandstat[2 * blockIdx.x] = ww;
        bandstat[2 * blockIdx.x + 1] = viol;
        if (blockIdx.x == 0) bandstat[2 * gridDim.x] = hh;
    }
}

// two-pass, second half: part[band][c] = sum over the band's rows of w_i |a_ic|; grid (bands, column tiles of 256 chunks)
template <typename T>
__global__ __launch_bounds__(256) void ob_svid_cols_kernel(const T *__restrict__ A, int64_t lda, const float *__restrict__ w,
                                                           float *__restrict__ part, int N, int K, int band_rows)
{
    const int c = blockIdx.y * 256 + threadIdx.x;
    if (c >= (K >> 3)) return;
    const int row0 = blockIdx.x * band_rows, row1 = min(N, row0 + band_rows);
    float acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = 0.f;
    for (int r = row0; r < row1; r += OB_SVID_R) {
        ObSvidChunk<T> a[OB_SVID_R];
        float wr[OB_SVID_R];
#pragma unroll
        for (int rr = 0; rr < OB_SVID_R; ++rr) {
            const bool ok = r + rr < row1;
            wr[rr] = ok ? w[r + rr] : 0.f;
            if (ok) a[rr].load(A + (int64_t)(r + rr) * lda + 8 * c);
            else a[rr].zero();
        }
#pragma unroll
        for (int rr = 0; rr < OB_SVID_R; ++rr)
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i] += wr[rr] * fabsf(a[rr].get(i));
    }
    ob_svid_store8(part + (int64_t)blockIdx.x * K + 8 * c, acc);
}

// sum of p[0], p[stride], ... (n terms) over the workgroup in a fixed order; every thread gets it
__device__ __forceinline__ float ob_svid_strided_sum(const float *p, int n, int stride, float *red)
{
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += blockDim.x) s += p[(int64_t)i * stride];
    return ob_block_sum(s, red);
}

// xw_j = sum of the bands' partials in band order (four contiguous band groups, combined as (g0 + g1) + (g2 + g3)), then the h
// side of the iteration.  finstat: {viol_h, sum of the new h_j^2} per workgroup.
__global__ __launch_bounds__(256) void ob_svid_colfin_kernel(const float *__restrict__ part, const float *__restrict__ bandstat,
                                                             float *h, float *__restrict__ finstat, int nbands, int K)
{
    __shared__ float red[16];
    __shared__ float grp[4][OB_SVID_FIN_COLS];
    const int tid = threadIdx.x, g = tid >> 6, lane = tid & 63;
    const int c = blockIdx.x * OB_SVID_FIN_COLS + lane;
    const float ww = ob_svid_strided_sum(bandstat, nbands, 2, red);
    const int per = (nbands + 3) >> 2, b0 = g * per, b1 = min(nbands, b0 + per);
    float s = 0.f;
    if (c < K) {
        int b = b0;
        for (; b + 4 <= b1; b += 4) {
            const float p0 = part[(int64_t)b * K + c], p1 = part[(int64_t)(b + 1) * K + c];
            const float p2 = part[(int64_t)(b + 2) * K + c], p3 = part[(int64_t)(b + 3) * K + c];
            s = (((s + p0) + p1) + p2) + p3;
        }
        for (; b < b1; ++b) s += part[(int64_t)b * K + c];
    }
    grp[g][lane] = s;
    __syncthreads();
    if (g != 0) return;
    float av = 0.f, hs = 0.f;
    if (c < K) {
        const float xw = (grp[0][lane] + grp[1][lane]) + (grp[2][lane] + grp[3][lane]);
        const float ho = h[c];
        const float grad = ho * ww - xw;
        const float pg = ho == 0.f ? fminf(0.f, grad) : grad;
        const float hn = ww != 0.f ? fmaxf(xw / ww, 0.f) : ho;
        h[c] = hn;
        av = fabsf(pg);
        hs = hn * hn;
    }
    av = ob_wave_sum(av);
    hs = ob_wave_sum(hs);
    if (lane == 0) {
        finstat[2 * blockIdx.x] = av;
        finstat[2 * blockIdx.x + 1] = hs;
    }
}

__global__ __launch_bounds__(256) void ob_svid_stats_kernel(const float *__restrict__ bandstat, const float *__restrict__ finstat,
                                                            float *__restrict__ stats, int nbands, int nfin)
{
    __shared__ float red[16];
    const float ww = ob_svid_strided_sum(bandstat, nbands, 2, red);
    const float vw = ob_svid_strided_sum(bandstat + 1, nbands, 2, red);
    const float vh = ob_svid_strided_sum(finstat, nfin, 2, red);
    const float hn = ob_svid_strided_sum(finstat + 1, nfin, 2, red);
    if (threadIdx.x == 0) {
        stats[0] = vw + vh;
        stats[1] = bandstat[2 * nbands];
        stats[2] = ww;
        stats[3] = hn;
    }
}

// Emit pass: one read of A.  latent (TL, [N, K] contiguous) = sign(a) * scale with +-0 and NaN -> 0 (torch.sign), packed
// ([N, K / 8], LSB first, bit = a < 0: ob_pack_kernel's rule), blockpart {sum (|a| - w_i h_j)^2, sum a^2} per workgroup -- each
// skipped when its pointer is null.
template <typename T, typename TL>
__global__ __launch_bounds__(256) void ob_svid_emit_kernel(const T *__restrict__ A, int64_t lda, const float *__restrict__ w,
                                                           const float *__restrict__ h, TL *__restrict__ latent, float scale,
                                                           uint8_t *__restrict__ packed, float *__restrict__ blockpart,
                                                           int64_t total, int kchunks)
{
    __shared__ float red[16];
    float s0 = 0.f, s1 = 0.f;
    const TL pos = (TL)scale, neg = (TL)-scale, zero = (TL)0.f;
    const bool small = total <= 0xffffffffLL;          // every projection of a real model: a 32-bit division per chunk, not a 64-bit one
#pragma unroll
    for (int it = 0; it < OB_SVID_EMIT_ITERS; ++it) {
        const int64_t idx = ((int64_t)blockIdx.x * OB_SVID_EMIT_ITERS + it) * 256 + threadIdx.x;
        if (idx >= total) break;
        const int64_t row = small ? (int64_t)((uint32_t)idx / (uint32_t)kchunks) : idx / kchunks;
        const int c = (int)(idx - row * kchunks);
        ObSvidChunk<T> a;
        a.load(A + row * lda + 8 * c);
        if (latent) {
            alignas(16) TL o[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float v = a.get(i);
                o[i] = v > 0.f ? pos : (v < 0.f ? neg : zero);
            }
            TL *dst = latent + idx * 8;
            if (sizeof(TL) == 2) {
                *reinterpret_cast<ob_u32x4 *>(dst) = *reinterpret_cast<ob_u32x4 *>(o);
            } else {
                reinterpret_cast<ob_u32x4 *>(dst)[0] = reinterpret_cast<ob_u32x4 *>(o)[0];
                reinterpret_cast<ob_u32x4 *>(dst)[1] = reinterpret_cast<ob_u32x4 *>(o)[1];
            }
        }
        if (packed) {
            unsigned byte = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) byte |= (unsigned)(a.get(i) < 0.0f) << i;
            packed[idx] = (uint8_t)byte;
        }
        if (blockpart) {
            const float wi = w[row];
            float hv[8];
            ob_svid_load8(h + 8 * c, hv);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float v = a.get(i), d = fabsf(v) - wi * hv[i];
                s0 += d * d;
                s1 += v * v;
            }
        }
    }
    if (blockpart) {
        s0 = ob_block_sum(s0, red);
        s1 = ob_block_sum(s1, red);
        if (threadIdx.x == 0) {
            blockpart[2 * blockIdx.x] = s0;
            blockpart[2 * blockIdx.x + 1] = s1;
        }
    }
}

__global__ __launch_bounds__(1024) void ob_svid_emit_sum_kernel(const float *__restrict__ blockpart, int nblocks, float *__restrict__ sums)
{
    __shared__ float red[16];
    const float s0 = ob_svid_strided_sum(blockpart, nblocks, 2, red);
    const float s1 = ob_svid_strided_sum(blockpart + 1, nblocks, 2, red);
    if (threadIdx.x == 0) {
        sums[0] = s0;
        sums[1] = s1;
    }
}
