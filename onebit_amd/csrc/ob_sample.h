// Sampled decoding: temperature / top-k / top-p and a Gumbel-max draw over one fp16 logits row per workgroup (ABI 10).
// The contract (what the kernel computes, bit for bit where it is exact) is stated at onebit_sample_params_t in onebit.h.
//
// One workgroup of 1024 threads per row; the row is copied to LDS once (V <= 65536 fp16: at most 128 KiB) and every
// pass reads it from there:
//   1. max pass         order-preserving 16-bit keys of the fp16 logits; max key + first index (the greedy token)
//   2. top-k            radix select of the k-th largest key: two 8-bit digit passes, integer LDS histograms
//   3. top-p            the same radix walk over 40-bit fixed-point softmax masses (uint64 LDS histograms) of the rows
//                       top-k kept: the first key, from the top, at which the cumulative mass reaches ceil(top_p * Z)
//   4. draw             argmax of s_i + g_i over the kept set; g_i from Philox4x32-10, four tokens per counter
// Division by a positive finite temperature is monotone, so the order of the scores s_i = logit_i / T is the order of the
// fp16 keys: both selections run on the 16-bit keys and compare the scores only at the end (s_i >= s(threshold key)).
// Every reduction that decides a threshold or the token is an integer histogram or a max over packed integer keys:
// the result does not depend on the grid, the row index or the order in which waves arrive.
#pragma once
#include "ob_common.h"
#include "../../include/onebit.h"

#define OB_SAMPLE_THREADS 1024
#define OB_SAMPLE_WAVES (OB_SAMPLE_THREADS / 64)
#define OB_SAMPLE_MAXV 65536
#define OB_SAMPLE_KEY_NINF 0x03ffu      // key of -inf (every NaN maps here too)

// where the kernel reads the sequence index n of a row and writes its token
struct ObSampleArgs {
    const _Float16 *logits;          // row r at logits + r * ld
    long long ld;
    int V;
    const onebit_sample_params_t *params;   // [rows]
    const int *pos;                  // n of row r = pos[pos_rows ? pos_rows[r] : r] + pos_add
    const int *pos_rows;
    int pos_add;
    int *out;                        // out[r] = token (NULL in the single-stream form)
    // single-stream form (one row): *token = t; out_tokens[p] = t when p < max_out; *pos_w = p + 1 with p = *pos_w on entry
    int *token, *pos_w, *out_tokens;
    int max_out;
};

__device__ __forceinline__ uint32_t ob_s_key(uint32_t b)
{
    b &= 0xffffu;
    if ((b & 0x7fffu) > 0x7c00u) b = 0xfc00u;                    // NaN -> -inf
    if (b == 0x8000u) b = 0u;                                    // -0 == +0, as the argmax kernels' float compares have it
    return (b & 0x8000u) ? (~b & 0xffffu) : (b | 0x8000u);
}

__device__ __forceinline__ float ob_s_key_half(uint32_t k)
{
    const uint32_t b = (k & 0x8000u) ? (k & 0x7fffu) : (~k & 0xffffu);
    return (float)__builtin_bit_cast(_Float16, (unsigned short)b);
}

// s = logit / T in fp32 (correctly rounded division), NaN -> -inf
__device__ __forceinline__ float ob_s_score(uint32_t bits16, float T)
{
    const float s = ob_s_key_half(ob_s_key(bits16)) / T;
    return s != s ? -INFINITY : s;
}

__device__ __forceinline__ void ob_philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, n3 = (uint32_t)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

// g = -log(-log(u)), u = ((r >> 8) + 0.5) * 2^-24 in (0, 1): -log(u) is formed from an exact fp32 operand on either side of 1/2
// (u itself needs 25 bits), so it is never 0 and g is always finite
__device__ __forceinline__ float ob_s_gumbel(uint32_t r)
{
    const uint32_t m = r >> 8;
    const float t = m >= (1u << 23) ? -log1pf(-(float)((1u << 25) - 2u * m - 1u) * 0x1p-25f)
                                    : -logf((float)(2u * m + 1u) * 0x1p-25f);
    return -logf(t);
}

__device__ __forceinline__ uint32_t ob_s_ordf(float f)
{
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Wave 0: walk hist[255] down to hist[0] and find the first bin b at which above_in + (sum of bins > b) + hist[b] >= target.
// Writes the bin (or -1: the total stays below the target) and the mass above it to res_bin / res_above.
__device__ __forceinline__ void ob_s_find(const unsigned long long *hist, unsigned long long above_in, unsigned long long target,
                                          int *res_bin, unsigned long long *res_above)
{
    const int lane = threadIdx.x & 63;
    unsigned long long c[4], t = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) { c[j] = hist[255 - 4 * lane - j]; t += c[j]; }
    unsigned long long inc = t;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long o = __shfl_up(inc, off, 64);
        if (lane >= off) inc += o;
    }
    unsigned long long above = above_in + inc - t;
    int hit = -1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (hit < 0) {
            if (above + c[j] >= target) hit = j;
            else above += c[j];
        }
    }
    const unsigned long long mask = __ballot(hit >= 0);
    const unsigned long long total = __shfl(inc, 63, 64);          // (all lanes: lane 63's inclusive sum is the total)
    if (mask == 0) {
        if (lane == 0) { *res_bin = -1; *res_above = above_in + total; }
    } else if (lane == __ffsll((long long)mask) - 1) {
        *res_bin = 255 - 4 * lane - hit;
        *res_above = above;
    }
}

__global__ __launch_bounds__(OB_SAMPLE_THREADS) void ob_sample_kernel(ObSampleArgs A)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned short *row = reinterpret_cast<unsigned short *>(smem);
    __shared__ unsigned long long hist[256];
    __shared__ uint32_t red32[OB_SAMPLE_WAVES];
    __shared__ unsigned long long best64;
    __shared__ int res_bin;
    __shared__ unsigned long long res_above;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = blockIdx.x, V = A.V;
    const onebit_sample_params_t P = A.params[r];
    const int p_in = A.pos[A.pos_rows ? A.pos_rows[r] : r];
    const uint32_t n = (uint32_t)(p_in + A.pos_add);
    // 1. the row into LDS; max over (key << 16 | 65535 - index): the largest key, first index on ties
    const unsigned short *src = reinterpret_cast<const unsigned short *>(A.logits + (size_t)r * (size_t)A.ld);
    uint32_t mk = 0;
    if (((uintptr_t)src & 15) == 0 && (V & 7) == 0) {
        for (int v = tid; v < V / 8; v += OB_SAMPLE_THREADS) {
            const ob_u32x4 q = *reinterpret_cast<const ob_u32x4 *>(src + 8 * v);
            *reinterpret_cast<ob_u32x4 *>(row + 8 * v) = q;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const uint32_t b = (q[e >> 1] >> (16 * (e & 1))) & 0xffffu;
                mk = max(mk, (ob_s_key(b) << 16) | (uint32_t)(65535 - (8 * v + e)));
            }
        }
    } else {
        for (int i = tid; i < V; i += OB_SAMPLE_THREADS) {
            const uint32_t b = src[i];
            row[i] = (unsigned short)b;
            mk = max(mk, (ob_s_key(b) << 16) | (uint32_t)(65535 - i));
        }
    }
    mk = ob_wave_max_u32(mk);
    if (lane == 0) red32[wave] = mk;
    __syncthreads();
    mk = red32[0];
#pragma unroll
    for (int w = 1; w < OB_SAMPLE_WAVES; ++w) mk = max(mk, red32[w]);
    const uint32_t kmax = mk >> 16;
    int tok = kmax > OB_SAMPLE_KEY_NINF ? 65535 - (int)(mk & 0xffffu) : 0;     // greedy: only a value above -inf wins
    const float T = P.temperature;
    const bool sampled = P.do_sample != 0 && T > 0.f && T < INFINITY;
    if (sampled && kmax > OB_SAMPLE_KEY_NINF) {
        const float smax = ob_s_key_half(kmax) / T;
        if (smax == INFINITY) {
            // the first index whose score is +inf (the scores' order is the keys', so it is a key range)
            uint32_t first = 0;
            for (int i = tid; i < V; i += OB_SAMPLE_THREADS)
                if (ob_s_key_half(ob_s_key(row[i])) / T == INFINITY) first = max(first, (uint32_t)(65535 - i));
            first = ob_wave_max_u32(first);
            __syncthreads();
            if (lane == 0) red32[wave] = first;
            __syncthreads();
            first = red32[0];
#pragma unroll
            for (int w = 1; w < OB_SAMPLE_WAVES; ++w) first = max(first, red32[w]);
            tok = 65535 - (int)first;
        } else {
            // 2. top-k: the k-th largest key; kept: s >= s(key)
            float tau = -INFINITY;
            const int K = P.top_k;
            if (K > 0 && K < V) {
                uint32_t prefix = 0;
                unsigned long long above = 0;
                for (int d = 0; d < 2; ++d) {
                    if (tid < 256) hist[tid] = 0;
                    __syncthreads();
                    for (int i = tid; i < V; i += OB_SAMPLE_THREADS) {
                        const uint32_t k = ob_s_key(row[i]);
                        if (d == 0) atomicAdd(&hist[k >> 8], 1ull);
                        else if ((k >> 8) == prefix) atomicAdd(&hist[k & 0xffu], 1ull);
                    }
                    __syncthreads();
                    if (wave == 0) ob_s_find(hist, above, (unsigned long long)K, &res_bin, &res_above);
                    __syncthreads();
                    prefix = (prefix << 8) | (uint32_t)res_bin;        // (K <= V: the count always reaches K)
                    above = res_above;
                    __syncthreads();
                }
                tau = ob_s_key_half(prefix) / T;
            }
            // 3. top-p over the rows top-k kept: q_i = floor(exp(s_i - smax) * 2^40), Z = sum q <= 2^56
            const float TP = P.top_p;
            if (TP < 1.f) {
                uint32_t prefix = 0;
                unsigned long long above = 0, target = 1;
                for (int d = 0; d < 2; ++d) {
                    if (tid < 256) hist[tid] = 0;
                    __syncthreads();
                    for (int i = tid; i < V; i += OB_SAMPLE_THREADS) {
                        const uint32_t b = row[i], k = ob_s_key(b);
                        if (d == 1 && (k >> 8) != prefix) continue;
                        const float s = ob_s_score(b, T);
                        if (!(s >= tau)) continue;
                        const unsigned long long q = (unsigned long long)(expf(s - smax) * 0x1p40f);
                        if (q) atomicAdd(&hist[d == 0 ? k >> 8 : k & 0xffu], q);
                    }
                    __syncthreads();
                    if (d == 0) {
                        // Z: the total of the first pass's bins, summed in a fixed order by wave 0
                        if (wave == 0) ob_s_find(hist, 0, ~0ull, &res_bin, &res_above);
                        __syncthreads();
                        const double z = (double)res_above;
                        const double pz = TP > 0.f ? ceil((double)TP * z) : 1.0;
                        target = pz < 1.0 ? 1ull : (unsigned long long)pz;
                        __syncthreads();
                    }
                    if (wave == 0) ob_s_find(hist, above, target, &res_bin, &res_above);
                    __syncthreads();
                    const int bin = res_bin;
                    above = res_above;
                    __syncthreads();
                    if (bin < 0) { prefix = 0xffffffffu; break; }          // never reached (rounding): keep all
                    prefix = (prefix << 8) | (uint32_t)bin;
                }
                if (prefix != 0xffffffffu) tau = fmaxf(tau, ob_s_key_half(prefix) / T);
            }
            // 4. Gumbel-max over the kept set: four tokens per Philox counter (n, stream, i / 4, 0)
            unsigned long long best = 0;
            for (int j = tid; 4 * j < V; j += OB_SAMPLE_THREADS) {
                float s[4];
                bool any = false;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int i = 4 * j + e;
                    s[e] = i < V ? ob_s_score(row[i], T) : -INFINITY;
                    any |= i < V && s[e] >= tau;
                }
                if (!any) continue;
                uint32_t c[4] = {n, P.stream, (uint32_t)j, 0u};
                ob_philox4x32_10(c, P.seed_lo, P.seed_hi);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int i = 4 * j + e;
                    if (i < V && s[e] >= tau) {
                        const float sc = s[e] + ob_s_gumbel(c[e]);
                        const unsigned long long key = ((unsigned long long)ob_s_ordf(sc) << 32) | (uint32_t)(0xffffffffu - (uint32_t)i);
                        best = key > best ? key : best;
                    }
                }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const unsigned long long o = __shfl_xor(best, off, 64);
                best = o > best ? o : best;
            }
            if (tid == 0) best64 = 0;
            __syncthreads();
            if (lane == 0) atomicMax(&best64, best);
            __syncthreads();
            tok = (int)(0xffffffffu - (uint32_t)(best64 & 0xffffffffu));
        }
    }
    if (tid == 0) {
        const int t = (tok >= 0 && tok < V) ? tok : 0;
        if (A.token) {
            const int p = p_in;
            *A.token = t;
            if (A.out_tokens && p >= 0 && p < A.max_out) A.out_tokens[p] = t;
            *A.pos_w = p + 1;
        } else {
            A.out[r] = t;
        }
    }
}
