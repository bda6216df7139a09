// Knowledge-distillation loss kernels (KDTrainer.compute_loss of the reference, llamafactory/kd.py:34-113): the token loss
// (KL(teacher || student) over the vocabulary + the causal-LM cross-entropy) and the hidden-state loss
// (squared distance of the L2-normalised rows), forward and backward.  gfx950, wave64, fp32 arithmetic on fp32 / fp16 rows.
//
// Every kernel is row-local and bandwidth-bound.  The forward kernels give ONE workgroup to a row and keep both operands' rows
// in registers between the max / sum pass and the pointwise pass, so each tensor is read from HBM once: OB_KD_NV groups of
// four elements per thread and tensor = 64 data VGPRs, which at 1024 threads (four waves per SIMD, 128 VGPRs each) is two
// rows of 32768 elements -- LLaMA's 32000-entry vocabulary in fp32 is 2 x 128 KB, more than the 160 KB of LDS but half of the
// CU's 512 KB register file.  Rows up to 8192 elements take 256 threads (several workgroups per CU).  A longer row is
// walked in chunks of that capacity, once per pass (the second and third walk come out of L2 / the Infinity Cache).
//
// A row whose pitch and base keep every group of four elements aligned (16 B fp32, 8 B fp16) is loaded one group per lane
// (VEC); any other row (V = 32001, 32003, an odd H) takes the element-wise form, lane-contiguous so it still coalesces.
//
// No atomics: a row's sums are a fixed shuffle tree + a fixed-order sum over the waves, the rows are summed by one workgroup
// in a fixed order (ob_kd_rows_sum_kernel), so loss and gradient are bit-reproducible.  exp is v_exp_f32 (__expf): relative
// error ~|x| * 1e-7 on the terms that matter, far inside the fp32 bars; each row's log-sum takes the accurate logf.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define OB_KD_NV 8                 // groups of 4 elements per thread, tensor and chunk
#define OB_KD_SMALL 256            // workgroup of a row of <= OB_KD_SMALL * OB_KD_NV * 4 elements
#define OB_KD_LARGE 1024           // ... of a longer one
#define OB_KD_HNV 4                // hidden-state rows: 16 elements per thread and tensor, 256 threads up to H = 4096, 512 beyond
#define OB_KD_BWD_THREADS 256      // backward: one workgroup per OB_KD_BWD_THREADS * 16 elements of a row
#define OB_KD_BWD_GROUPS 4
#define OB_KD_TSTATS 6             // floats per row of the token loss's stats (ONEBIT_KD_TOKEN_STATS)
#define OB_KD_HSTATS 4             // ... of the hidden-state loss's (ONEBIT_KD_HIDDEN_STATS)
#define OB_KD_NORM_EPS 1e-12f      // F.normalize's eps

typedef _Float16 ob_kd_h4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void ob_kd_load4(const float *p, float *v)
{
    const float4 x = *reinterpret_cast<const float4 *>(p);
    v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
}
__device__ __forceinline__ void ob_kd_load4(const _Float16 *p, float *v)
{
    const ob_kd_h4 x = *reinterpret_cast<const ob_kd_h4 *>(p);
    v[0] = (float)x[0]; v[1] = (float)x[1]; v[2] = (float)x[2]; v[3] = (float)x[3];
}
__device__ __forceinline__ void ob_kd_store4(float *p, const float *v)
{
    *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void ob_kd_store4(_Float16 *p, const float *v)
{
    ob_kd_h4 x;
    x[0] = (_Float16)v[0]; x[1] = (_Float16)v[1]; x[2] = (_Float16)v[2]; x[3] = (_Float16)v[3];
    *reinterpret_cast<ob_kd_h4 *>(p) = x;
}

// element of a row that register slot (group i, member j) of this thread holds, relative to the chunk's first element
template <int THREADS, bool VEC>
__device__ __forceinline__ int ob_kd_slot(int i, int j)
{
    return VEC ? (i * THREADS + (int)threadIdx.x) * 4 + j : (i * 4 + j) * THREADS + (int)threadIdx.x;
}

// one chunk (THREADS * NV * 4 elements from `base`) of a row of n elements into registers; `fill` beyond the row
template <typename T, int THREADS, int NV, bool VEC>
__device__ __forceinline__ void ob_kd_load_chunk(const T *row, int base, int n, float (&r)[NV * 4], float fill)
{
#pragma unroll
    for (int i = 0; i < NV; i++) {
        if (VEC) {                                       // n % 4 == 0: a group is inside the row or beyond it as a whole
            const int e = base + ob_kd_slot<THREADS, true>(i, 0);
            if (e < n) ob_kd_load4(row + e, &r[i * 4]);
            else r[i * 4] = r[i * 4 + 1] = r[i * 4 + 2] = r[i * 4 + 3] = fill;
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int e = base + ob_kd_slot<THREADS, false>(i, j);
                r[i * 4 + j] = e < n ? (float)row[e] : fill;
            }
        }
    }
}

// (a, b) reduced over the workgroup, the result in every thread: xor butterfly inside a wave (both partners add the same two
// numbers, so all lanes agree), then the waves' values in wave order.  `red`: 2 * THREADS / 64 floats of LDS.
template <int THREADS, bool MAX>
__device__ __forceinline__ void ob_kd_block2(float &a, float &b, float *red)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float a2 = __shfl_xor(a, o, 64), b2 = __shfl_xor(b, o, 64);
        a = MAX ? fmaxf(a, a2) : a + a2;
        b = MAX ? fmaxf(b, b2) : b + b2;
    }
    constexpr int NW = THREADS / 64;
    const int w = threadIdx.x >> 6;
    __syncthreads();                                     // the previous reduction's readers are done with `red`
    if ((threadIdx.x & 63) == 0) { red[2 * w] = a; red[2 * w + 1] = b; }
    __syncthreads();
    a = red[0]; b = red[1];
#pragma unroll
    for (int i = 1; i < NW; i++) {
        a = MAX ? fmaxf(a, red[2 * i]) : a + red[2 * i];
        b = MAX ? fmaxf(b, red[2 * i + 1]) : b + red[2 * i + 1];
    }
}

// ---- token loss, forward: stats[r] = {max_s, log z_s, max_t, log z_t, kl_row, ce_row},  lse = max + log z ------------------
//   kl_row = sum_v p_t[v] * ((t[v] - lse_t) - (s[v] - lse_s)), an entry with p_t == 0 (a teacher logit of -inf) adds exactly 0
//   (F.kl_div's xlogy);  ce_row = lse_s - s[label] on a labelled row (NaN for a label outside the vocabulary), else 0
// x - lse is always formed as (x - max) - log z, as log_softmax does: the sum max + log z would round log z to ulp(max) (0.004
// at logits of 6e4), and exp of that error is a relative error of every probability of the row.  That is why the two parts of
// each lse are saved separately for the backward pass.
template <typename T, int THREADS, bool VEC>
__global__ __launch_bounds__(THREADS) void ob_kd_token_fwd_kernel(const T *__restrict__ S, const T *__restrict__ Tt,
                                                                   const int64_t *__restrict__ labels, float *__restrict__ stats,
                                                                   int V, int64_t ignore_index)
{
    __shared__ float red[2 * THREADS / 64];
    constexpr int NV = OB_KD_NV, CH = THREADS * NV * 4;
    const int64_t r = blockIdx.x;
    const T *s_row = S + r * V, *t_row = Tt + r * V;
    const int nch = (V + CH - 1) / CH;
    float s[NV * 4], t[NV * 4];
    ob_kd_load_chunk<T, THREADS, NV, VEC>(s_row, 0, V, s, -INFINITY);
    const bool use_t = Tt != nullptr;                    // no teacher: the KL term is switched off, only lse_s and ce_row matter
    if (use_t) ob_kd_load_chunk<T, THREADS, NV, VEC>(t_row, 0, V, t, -INFINITY);
    else {
#pragma unroll
        for (int k = 0; k < NV * 4; k++) t[k] = 0.f;
    }

    float ms = -INFINITY, mt = -INFINITY;
    for (int c = 0; c < nch; c++) {
        if (c > 0) {
            ob_kd_load_chunk<T, THREADS, NV, VEC>(s_row, c * CH, V, s, -INFINITY);
            if (use_t) ob_kd_load_chunk<T, THREADS, NV, VEC>(t_row, c * CH, V, t, -INFINITY);
        }
#pragma unroll
        for (int k = 0; k < NV * 4; k++) { ms = fmaxf(ms, s[k]); mt = fmaxf(mt, t[k]); }
    }
    ob_kd_block2<THREADS, true>(ms, mt, red);

    float zs = 0.f, zt = 0.f;
    for (int c = 0; c < nch; c++) {
        if (nch > 1) {
            ob_kd_load_chunk<T, THREADS, NV, VEC>(s_row, c * CH, V, s, -INFINITY);
            if (use_t) ob_kd_load_chunk<T, THREADS, NV, VEC>(t_row, c * CH, V, t, -INFINITY);
        }
#pragma unroll
        for (int k = 0; k < NV * 4; k++) { zs += __expf(s[k] - ms); zt += __expf(t[k] - mt); }
    }
    ob_kd_block2<THREADS, false>(zs, zt, red);
    const float ls = logf(zs), lt_ = logf(zt);

    float kl = 0.f, unused = 0.f;
    for (int c = 0; use_t && c < nch; c++) {
        if (nch > 1) {
            ob_kd_load_chunk<T, THREADS, NV, VEC>(s_row, c * CH, V, s, -INFINITY);
            ob_kd_load_chunk<T, THREADS, NV, VEC>(t_row, c * CH, V, t, -INFINITY);
        }
#pragma unroll
        for (int k = 0; k < NV * 4; k++) {
            const float lt = (t[k] - mt) - lt_;
            const float pt = __expf(lt);
            const float term = pt * (lt - ((s[k] - ms) - ls));
            kl += pt > 0.f ? term : 0.f;                 // also the padding beyond the row (t = -inf)
        }
    }
    ob_kd_block2<THREADS, false>(kl, unused, red);

    if (threadIdx.x == 0) {
        float ce = 0.f;
        if (labels) {
            const int64_t lab = labels[r];
            if (lab != ignore_index) ce = (lab >= 0 && lab < V) ? ls - ((float)s_row[lab] - ms) : NAN;
        }
        float *st = stats + OB_KD_TSTATS * r;
        st[0] = ms; st[1] = ls; st[2] = use_t ? mt : 0.f; st[3] = use_t ? lt_ : 0.f; st[4] = kl; st[5] = ce;
    }
}

// ---- token loss, backward: grad[v] = c_kl * (p_s - p_t) + c_ce * (p_s - [v == label]), c_ce on labelled rows only -----------
// coef = {c_kl, c_ce} is read from device memory; the products are formed in fp32 and rounded once to the output type.
// c_kl == 0 (the KL term switched off) drops the teacher's part altogether, so nothing of the teacher reaches the gradient.
template <typename T, bool VEC>
__global__ __launch_bounds__(OB_KD_BWD_THREADS) void ob_kd_token_bwd_kernel(const T *__restrict__ S, const T *__restrict__ Tt,
                                                                             const int64_t *__restrict__ labels,
                                                                             const float *__restrict__ stats,
                                                                             const float *__restrict__ coef, T *__restrict__ G,
                                                                             int V, int nchunk, int64_t ignore_index)
{
    constexpr int THREADS = OB_KD_BWD_THREADS, NG = OB_KD_BWD_GROUPS, CH = THREADS * NG * 4;
    const int64_t r = blockIdx.x / nchunk;
    const int base = (int)(blockIdx.x % nchunk) * CH;
    const T *s_row = S + r * V, *t_row = Tt + r * V;
    T *g_row = G + r * V;
    const float *st = stats + OB_KD_TSTATS * r;
    const float ms = st[0], ls = st[1], mt = st[2], lt = st[3];
    const float c_kl = coef[0];
    int64_t lab = -1;
    if (labels) {
        const int64_t l = labels[r];
        if (l != ignore_index) lab = l;
    }
    const bool labelled = lab >= 0;                      // (a label outside the vocabulary has made the loss NaN already)
    const float c_ce = labelled ? coef[1] : 0.f;
    const bool use_t = Tt != nullptr && c_kl != 0.f;
#pragma unroll
    for (int i = 0; i < NG; i++) {
        float s[4], t[4], g[4];
        int e[4];
#pragma unroll
        for (int j = 0; j < 4; j++) e[j] = base + ob_kd_slot<THREADS, VEC>(i, j);
        if (VEC) {
            if (e[0] >= V) continue;
            ob_kd_load4(s_row + e[0], s);
            if (use_t) ob_kd_load4(t_row + e[0], t);
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                s[j] = e[j] < V ? (float)s_row[e[j]] : 0.f;
                if (use_t) t[j] = e[j] < V ? (float)t_row[e[j]] : 0.f;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const float ps = __expf((s[j] - ms) - ls);
            float v = use_t ? c_kl * (ps - __expf((t[j] - mt) - lt)) : 0.f;
            if (labelled) v += c_ce * (ps - (e[j] == lab ? 1.f : 0.f));
            g[j] = v;
        }
        if (VEC) ob_kd_store4(g_row + e[0], g);
        else {
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (e[j] < V) g_row[e[j]] = (T)g[j];
        }
    }
}

// ---- hidden-state loss, forward: stats[r] = {|s|, |t|, d_r, s^ . delta} ------------------------------------------------------
//   s^ = s / max(|s|, eps), t^ likewise, delta = t^ - s^, d_r = sum delta^2 (a sum of squared differences, not 2 - 2 cos)
// Hidden widths are a few thousand: 32 data VGPRs keep eight waves per SIMD, i.e. several rows per CU in flight.
template <typename T, int THREADS, bool VEC>
__global__ __launch_bounds__(THREADS) void ob_kd_hidden_fwd_kernel(const T *__restrict__ S, const T *__restrict__ Tt,
                                                                    float *__restrict__ stats, int H)
{
    __shared__ float red[2 * THREADS / 64];
    constexpr int NV = OB_KD_HNV, CH = THREADS * NV * 4;
    const int64_t r = blockIdx.x;
    const T *s_row = S + r * H, *t_row = Tt + r * H;
    const int nch = (H + CH - 1) / CH;
    float s[NV * 4], t[NV * 4];
    ob_kd_load_chunk<T, THREADS, NV, VEC>(s_row, 0, H, s, 0.f);
    ob_kd_load_chunk<T, THREADS, NV, VEC>(t_row, 0, H, t, 0.f);

    float ss = 0.f, tt = 0.f;
    for (int c = 0; c < nch; c++) {
        if (c > 0) {
            ob_kd_load_chunk<T, THREADS, NV, VEC>(s_row, c * CH, H, s, 0.f);
            ob_kd_load_chunk<T, THREADS, NV, VEC>(t_row, c * CH, H, t, 0.f);
        }
#pragma unroll
        for (int k = 0; k < NV * 4; k++) { ss += s[k] * s[k]; tt += t[k] * t[k]; }
    }
    ob_kd_block2<THREADS, false>(ss, tt, red);
    const float ns = sqrtf(ss), nt = sqrtf(tt);
    const float is = 1.f / fmaxf(ns, OB_KD_NORM_EPS), it = 1.f / fmaxf(nt, OB_KD_NORM_EPS);

    float d = 0.f, sd = 0.f;
    for (int c = 0; c < nch; c++) {
        if (nch > 1) {
            ob_kd_load_chunk<T, THREADS, NV, VEC>(s_row, c * CH, H, s, 0.f);
            ob_kd_load_chunk<T, THREADS, NV, VEC>(t_row, c * CH, H, t, 0.f);
        }
#pragma unroll
        for (int k = 0; k < NV * 4; k++) {
            const float sh = s[k] * is;
            const float dl = t[k] * it - sh;
            d += dl * dl;
            sd += sh * dl;
        }
    }
    ob_kd_block2<THREADS, false>(d, sd, red);
    if (threadIdx.x == 0) *reinterpret_cast<float4 *>(stats + 4 * r) = make_float4(ns, nt, d, sd);
}

// ---- hidden-state loss, backward: grad = coef * dd_r/ds,  dd_r/ds = -(2 / |s|) * (delta - s^ (s^ . delta)) -------------------
// (below eps the normalisation is the constant 1 / eps and the projection term drops out)
template <typename T, bool VEC>
__global__ __launch_bounds__(OB_KD_BWD_THREADS) void ob_kd_hidden_bwd_kernel(const T *__restrict__ S, const T *__restrict__ Tt,
                                                                              const float *__restrict__ stats,
                                                                              const float *__restrict__ coef, T *__restrict__ G,
                                                                              int H, int nchunk)
{
    constexpr int THREADS = OB_KD_BWD_THREADS, NG = OB_KD_BWD_GROUPS, CH = THREADS * NG * 4;
    const int64_t r = blockIdx.x / nchunk;
    const int base = (int)(blockIdx.x % nchunk) * CH;
    const T *s_row = S + r * H, *t_row = Tt + r * H;
    T *g_row = G + r * H;
    const float4 st = *reinterpret_cast<const float4 *>(stats + 4 * r);
    const float is = 1.f / fmaxf(st.x, OB_KD_NORM_EPS), it = 1.f / fmaxf(st.y, OB_KD_NORM_EPS);
    const float sd = st.x >= OB_KD_NORM_EPS ? st.w : 0.f;
    const float c = -2.f * is * coef[0];
#pragma unroll
    for (int i = 0; i < NG; i++) {
        float s[4], t[4], g[4];
        int e[4];
#pragma unroll
        for (int j = 0; j < 4; j++) e[j] = base + ob_kd_slot<THREADS, VEC>(i, j);
        if (VEC) {
            if (e[0] >= H) continue;
            ob_kd_load4(s_row + e[0], s);
            ob_kd_load4(t_row + e[0], t);
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                s[j] = e[j] < H ? (float)s_row[e[j]] : 0.f;
                t[j] = e[j] < H ? (float)t_row[e[j]] : 0.f;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const float sh = s[j] * is;
            g[j] = c * ((t[j] * it - sh) - sh * sd);
        }
        if (VEC) ob_kd_store4(g_row + e[0], g);
        else {
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (e[j] < H) g_row[e[j]] = (T)g[j];
        }
    }
}

// ---- the rows' sums in a fixed order: out = {sum stats[r][col], sum over labelled rows of stats[r][col + 1], labelled rows} ---
// (stats rows of `stride` floats)
// One workgroup: thread i adds rows i, i + 1024, ... in that order, then the fixed tree of ob_kd_block2.
__global__ __launch_bounds__(1024) void ob_kd_rows_sum_kernel(const float *__restrict__ stats, const int64_t *__restrict__ labels,
                                                              int64_t ignore_index, int64_t T, int stride, int col,
                                                              float *__restrict__ out)
{
    __shared__ float red[2 * 1024 / 64];
    __shared__ long long cnt[1024 / 64];
    float a = 0.f, b = 0.f;
    long long n = 0;                                     // counted in integers: a float count is inexact beyond 2^24 rows
    for (int64_t r = threadIdx.x; r < T; r += 1024) {
        a += stats[stride * r + col];
        if (labels && labels[r] != ignore_index) { b += stats[stride * r + col + 1]; n++; }
    }
    ob_kd_block2<1024, false>(a, b, red);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if ((threadIdx.x & 63) == 0) cnt[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long total = 0;
        for (int i = 0; i < 1024 / 64; i++) total += cnt[i];
        out[0] = a; out[1] = b; out[2] = (float)total;   // converted once
    }
}
