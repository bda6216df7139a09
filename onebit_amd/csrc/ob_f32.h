// fp32 route of the 1-bit linear layer (checkpoints loaded as fp32, bitnet.py:99): everything in fp32 with the reference's
// rounding points -- a = x * h (one rounding, bitnet.py:113, a separate multiply), z = sum +-a in fp32, u = z * g (one
// rounding, :116), LayerNorm with fp32 statistics, then the bias.  The weights are +-1, so every product is exact and
// v_mfma_f32_16x16x4_f32 (bit-for-bit a k-ordered fp32 fmaf chain, no xf32 truncation) computes exactly the sum of the
// generic kernel in another order.
//
//   ob_f32_gemm_kernel   T >= 2 (and T == 1 where the GEMV cannot run): tiled MFMA GEMM
//   ob_f32_gemv_kernel   T == 1: packed rows streamed once with 16-byte loads, sign by xor, fp32 adds
//   ob_f32_ln_rows_kernel  one workgroup per token, the u row read once and kept in registers
#pragma once
#include "ob_common.h"

#define OB_F32_BK 128                          // k per LDS stage: four packed words per row
#define OB_F32_PITCH (OB_F32_BK + 4)           // floats per staged activation row (rows stay 16-byte aligned)
#define OB_F32_CUS 256                         // dispatch thresholds are a pure function of the shape (onebit_linear_f32_route)

// ---------------------------------------------------------------------------------------------------------------------
// Tiled GEMM.  Workgroup = 4 waves as WN (along n) x WK (along k inside a stage); a wave owns RN x RT tiles of 16 rows x
// 16 tokens, i.e. RN * RT independent accumulators (the 16x16x4 form has a 40-cycle dependent latency on a 32-cycle
// issue interval: >= 2 are needed).  Tile = (WN * RN * 16) rows x (RT * 16) tokens:
//   WN = 4, WK = 1, RN = 2, RT = 4   128 x 64   large T (4 waves share one staged activation tile)
//   WN = 1, WK = 4, RN = 2, RT = 1/2/4   32 x 16/32/64: few tokens or few rows -- the four waves split every stage's k and
//                                     their sums are added in a fixed order through LDS, so the chip is not left idle
// The activation tile is scaled by h on its way into LDS (one pass over x, no workspace): the next stage's x is fetched
// into registers before this stage's MFMAs and written after them.  The packed words are the MFMA's row operand, read
// straight from global memory one stage ahead and expanded in registers: bit -> sign bit of 0x3f800000.
//
// MFMA operands (A[l & 15][k = l >> 4], B[k = l >> 4][l & 15]): a lane reads the 4 consecutive activations
// a[t][16 hf + 4 lg .. + 3] of a packed word's half hf with ONE ds_read_b128 and uses element j in sub-step j, so sub-step
// j sums k = 16 hf + 4 lg + j over the lane groups lg -- the weight operand takes the same bit of the row's word.  The
// order of k inside a word is permuted with respect to memory; the sum is the same set of exact products.
// D: lane holds rows n0 + 4 lg + i (i = 0..3) of token t0 + (l & 15).
template <bool PARTIAL, int WN, int WK, int RN, int RT>
__global__ __launch_bounds__(256) void ob_f32_gemm_kernel(
    const uint32_t *__restrict__ W, int64_t ldw_words, const float *__restrict__ x, int64_t ldx, const float *__restrict__ h,
    const float *__restrict__ g, float *__restrict__ out, int T, int K, int N, int nbn, int vec_out)
{
    static_assert(WN * WK == 4, "four waves");
    constexpr int BT = RT * 16, BN = WN * RN * 16;
    constexpr int NW = 4 / WK;                                       // packed words of a stage per wave
    constexpr int NLD = BT * (OB_F32_BK / 4) / 256;                  // float4 per thread and stage
    constexpr int RED = WK > 1 ? (WK - 1) * RN * RT * 256 : 0;       // floats of the cross-wave reduction
    constexpr int STAGE = BT * OB_F32_PITCH;
    __shared__ __attribute__((aligned(16))) float smem[STAGE > RED ? STAGE : RED];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, lg = lane >> 4;
    const int wn = wave % WN, wk = wave / WN;
    const int bn = (int)blockIdx.x % nbn, bt = (int)blockIdx.x / nbn;
    const int n0 = bn * BN + wn * RN * 16, t0 = bt * BT;

    // staging: thread -> (row = tid / 32 + 8 i, float4 column tid % 32)
    const int c4 = tid & 31, srow = tid >> 5;
    ob_float4 xs[NLD];
    auto fetch = [&](int k0) {
        const int k = k0 + 4 * c4;
        const bool kok = k < K;                                      // K % 4 == 0: whole float4 inside or outside
        ob_float4 hv = {0.f, 0.f, 0.f, 0.f};
        if (kok) hv = *reinterpret_cast<const ob_float4 *>(h + k);
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int t = t0 + srow + 8 * i;
            ob_float4 xv = {0.f, 0.f, 0.f, 0.f};
            if (kok && t < T) xv = *reinterpret_cast<const ob_float4 *>(x + (int64_t)t * ldx + k);
            xs[i] = xv * hv;                                         // a = x * h: the one fp32 rounding of bitnet.py:113
        }
    };
    // this lane's rows of the packed matrix (clamped: rows beyond N are computed and dropped)
    const uint32_t *Wrow[RN];
#pragma unroll
    for (int a = 0; a < RN; ++a) Wrow[a] = W + (int64_t)min(n0 + a * 16 + r, N - 1) * ldw_words;
    const int kwords = K >> 5;
    uint32_t wcur[RN][NW], wnext[RN][NW];
    auto fetch_w = [&](int k0, uint32_t (&w)[RN][NW]) {
#pragma unroll
        for (int q = 0; q < NW; ++q) {
            const int kw = (k0 >> 5) + wk * NW + q;
#pragma unroll
            for (int a = 0; a < RN; ++a) w[a][q] = kw < kwords ? Wrow[a][kw] : 0u;    // (beyond K the activations are 0)
        }
    };

    ob_float4 acc[RN][RT];
#pragma unroll
    for (int a = 0; a < RN; ++a)
#pragma unroll
        for (int b = 0; b < RT; ++b) acc[a][b] = (ob_float4){0.f, 0.f, 0.f, 0.f};

    uint32_t smask = 0x80000000u;
    asm("" : "+s"(smask));                                            // opaque: (s & mask) | (one & ~mask) becomes one v_bfi_b32

    fetch(0);
    fetch_w(0, wnext);
    for (int k0 = 0; k0 < K; k0 += OB_F32_BK) {
        __syncthreads();                                              // the previous stage's reads are done
#pragma unroll
        for (int i = 0; i < NLD; ++i)
            *reinterpret_cast<ob_float4 *>(&smem[(srow + 8 * i) * OB_F32_PITCH + 4 * c4]) = xs[i];
#pragma unroll
        for (int a = 0; a < RN; ++a)
#pragma unroll
            for (int q = 0; q < NW; ++q) wcur[a][q] = wnext[a][q];
        __syncthreads();
        if (k0 + OB_F32_BK < K) {
            fetch(k0 + OB_F32_BK);
            fetch_w(k0 + OB_F32_BK, wnext);
        }
#pragma unroll
        for (int q = 0; q < NW; ++q) {
            const int kq = (wk * NW + q) * 32;
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                ob_float4 bv[RT];
#pragma unroll
                for (int b = 0; b < RT; ++b)
                    bv[b] = *reinterpret_cast<const ob_float4 *>(&smem[(b * 16 + r) * OB_F32_PITCH + kq + 16 * hf + 4 * lg]);
                uint32_t wl[RN];
#pragma unroll
                for (int a = 0; a < RN; ++a) wl[a] = wcur[a][q] >> (16 * hf + 4 * lg);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
#pragma unroll
                    for (int a = 0; a < RN; ++a) {
                        const uint32_t sb = ((wl[a] << (31 - j)) & smask) | (0x3f800000u & ~smask);
                        const float av = __builtin_bit_cast(float, sb);
#pragma unroll
                        for (int b = 0; b < RT; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[b][j], acc[a][b], 0, 0, 0);
                    }
                }
            }
        }
    }

    if (WK > 1) {
        // waves 1.. hand their sums to wave 0, which adds them in wave order
        __syncthreads();
        if (wk > 0) {
#pragma unroll
            for (int a = 0; a < RN; ++a)
#pragma unroll
                for (int b = 0; b < RT; ++b)
                    *reinterpret_cast<ob_float4 *>(&smem[(((wk - 1) * RN + a) * RT + b) * 256 + lane * 4]) = acc[a][b];
        }
        __syncthreads();
        if (wk > 0) return;
#pragma unroll
        for (int w2 = 1; w2 < WK; ++w2)
#pragma unroll
            for (int a = 0; a < RN; ++a)
#pragma unroll
                for (int b = 0; b < RT; ++b)
                    acc[a][b] += *reinterpret_cast<const ob_float4 *>(&smem[(((w2 - 1) * RN + a) * RT + b) * 256 + lane * 4]);
    }

#pragma unroll
    for (int a = 0; a < RN; ++a) {
        const int n = n0 + a * 16 + 4 * lg;
        if (n >= N) continue;
        ob_float4 gv = {1.f, 1.f, 1.f, 1.f};
        if (!PARTIAL) {
#pragma unroll
            for (int i = 0; i < 4; ++i) gv[i] = g[min(n + i, N - 1)];
        }
#pragma unroll
        for (int b = 0; b < RT; ++b) {
            const int t = t0 + b * 16 + r;
            if (t >= T) continue;
            ob_float4 v = acc[a][b];
            if (!PARTIAL) v = v * gv;                                 // u = z * g: the one rounding of bitnet.py:116
            float *o = out + (int64_t)t * N + n;
            if (vec_out) *reinterpret_cast<ob_float4 *>(o) = v;       // (N % 4 == 0: the four rows are inside)
            else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (n + i < N) o[i] = v[i];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// GEMV (one token).  a = x * h is staged once per workgroup in LDS, one spare 16-byte slot after every 128 floats so that
// the lanes' 16-byte reads (512 bytes apart) fall on different banks.  A wave takes 4 rows at a time; a lane owns chunks of
// 128 k: it loads the 16 packed bytes of the 4 rows (four 16-byte loads in flight), reads the chunk's activations from LDS
// and adds them with the sign bit flipped where the weight bit is set.  Rows of at most 32 chunks (K <= 4096) are taken by
// half a wave, so a wave covers 8 rows.  Bound by the packed bytes like the fp16 decode GEMV.
// Needs K % 128 == 0, K <= 16384, 16-byte aligned packed rows.
#define OB_F32_GEMV_MAXK 16384
#define OB_F32_GEMV_LDS(K) ((size_t)((K) + (K) / 32) * 4)
template <bool PARTIAL>
__global__ __launch_bounds__(256) void ob_f32_gemv_kernel(
    const uint8_t *__restrict__ W, int64_t ldw_bytes, const float *__restrict__ x, const float *__restrict__ h,
    const float *__restrict__ g, float *__restrict__ out, int K, int N)
{
    extern __shared__ __attribute__((aligned(16))) float a_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int k = 4 * tid; k < K; k += 1024) {
        const ob_float4 xv = *reinterpret_cast<const ob_float4 *>(x + k);
        const ob_float4 hv = *reinterpret_cast<const ob_float4 *>(h + k);
        *reinterpret_cast<ob_float4 *>(&a_lds[k + 4 * (k >> 7)]) = xv * hv;       // a = x * h, one rounding
    }
    __syncthreads();
    const int C = K >> 7;                                             // chunks per row
    const bool split = C <= 32;
    const int sub = split ? lane >> 5 : 0, c0 = split ? lane & 31 : lane, cstep = split ? 32 : 64;
    const int rows_wave = split ? 8 : 4, rows_wg = 4 * rows_wave;
    for (int nb = (int)blockIdx.x * rows_wg + wave * rows_wave; nb < N; nb += (int)gridDim.x * rows_wg) {   // (wave-uniform)
        const int nr = nb + 4 * sub;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int c = c0; c < C; c += cstep) {
            ob_u32x4 w[4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
                w[i] = *reinterpret_cast<const ob_u32x4 *>(W + (int64_t)min(nr + i, N - 1) * ldw_bytes + 16 * c);
            const float *ac = a_lds + 132 * c;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const ob_float4 av = *reinterpret_cast<const ob_float4 *>(ac + 32 * q + 4 * e);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float aj = av[j];                       // (a scalar copy: bit_cast of a vector ELEMENT reads element 0)
                        const uint32_t ab = __builtin_bit_cast(uint32_t, aj);
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            acc[i] += __builtin_bit_cast(float, ab ^ ((w[i][q] << (31 - (4 * e + j))) & 0x80000000u));
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (split) {
                const float lo = ob_wave_sum(sub == 0 ? acc[i] : 0.f), hi = ob_wave_sum(sub == 1 ? acc[i] : 0.f);
                if (lane == 0 && nb + i < N) out[nb + i] = PARTIAL ? lo : lo * g[nb + i];
                if (lane == 0 && nb + 4 + i < N) out[nb + 4 + i] = PARTIAL ? hi : hi * g[nb + 4 + i];
            } else {
                const float s = ob_wave_sum(acc[i]);
                if (lane == 0 && nb + i < N) out[nb + i] = PARTIAL ? s : s * g[nb + i];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Row LayerNorm: the fp32 analogue of ob_layernorm_rows_kernel.  One 256-thread workgroup per token reads the u row once
// (up to 16 float4 per thread: N <= 16384, N % 4 == 0), exact two-pass statistics (mean, then centred sum of squares,
// biased variance, eps), writes y and, when asked, u.  y may alias uin: every thread reads its elements before it writes.
#define OB_F32_LN_MAXN 16384
__global__ __launch_bounds__(256) void ob_f32_ln_rows_kernel(const float *uin, const float *__restrict__ bias, float *y, float *uout,
                                                             int N, float eps, int skip_ln)
{
    __shared__ float red[16];
    const int64_t t = blockIdx.x;
    const int tid = threadIdx.x;
    ob_float4 u[16];
    bool ok[16];
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int base = (v * 256 + tid) * 4;
        ok[v] = base < N;
        if (ok[v]) u[v] = *reinterpret_cast<const ob_float4 *>(uin + t * N + base);
    }
    float mean = 0.f, rstd = 1.f;
    if (!skip_ln) {
        float s = 0.f;
#pragma unroll
        for (int v = 0; v < 16; ++v)
            if (ok[v]) s += (u[v][0] + u[v][1]) + (u[v][2] + u[v][3]);
        mean = ob_block_sum(s, red) / (float)N;
        float q = 0.f;
#pragma unroll
        for (int v = 0; v < 16; ++v)
            if (ok[v]) {
#pragma unroll
                for (int i = 0; i < 4; ++i) { const float d = u[v][i] - mean; q = fmaf(d, d, q); }
            }
        const float var = ob_block_sum(q, red + 8) / (float)N;
        rstd = 1.0f / sqrtf(var + eps);
    }
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int base = (v * 256 + tid) * 4;
        if (ok[v]) {
            ob_float4 o = u[v];
            if (!skip_ln) {
#pragma unroll
                for (int i = 0; i < 4; ++i) o[i] = (u[v][i] - mean) * rstd;
                if (bias) o = o + *reinterpret_cast<const ob_float4 *>(bias + base);
            }
            if (uout) *reinterpret_cast<ob_float4 *>(uout + t * N + base) = u[v];
            *reinterpret_cast<ob_float4 *>(y + t * N + base) = o;
        }
    }
}
