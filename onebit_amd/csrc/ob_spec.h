// Speculative decoding on the single-stream engine, gfx950: the two kernels a speculative step adds to the mixed step's layer body.
//   ob_fdec_mq_kernel      key-block decode attention for Q <= 16 CONSECUTIVE query rows of one sequence (positions pos .. pos + Q - 1):
//                          grid (head, sequence, split); one workgroup streams its split's keys / values ONCE and serves all Q rows,
//                          where ob_fdec_kernel (one query row per workgroup) would stream them Q times
//   ob_spec_commit_kernel  one workgroup at the end of the step: accept the longest verified draft prefix, append the emitted tokens to
//                          the sequence's history, draft the next step's tokens by prompt lookup, write the next step's inputs
// Neither has a counterpart in the reference (greedy_search / sample emit one token per forward, generation/utils.py:2491-2540); per
// row the attention arithmetic is modeling_bitllama.py:546-563 exactly as ob_fdec_kernel restates it.
#pragma once
#include "ob_common.h"
#include "ob_fdec.h"

// ---------------------------------------------------------------------------------------- multi-query key-block attention --
// Row i of a sequence attends to keys 0 .. pos + i (its own key / value and those of the rows before it were appended by
// onebit_rows_qkv_rope_ragged).  Per row the arithmetic, the key -> lane assignment (key p of a split: position group (p - p_lo) & 15,
// register (p - p_lo) / 16 % NI) and the sweep order are ob_fdec_kernel's, so a row's output has the bits that kernel gives for the row
// alone: scores rounded to fp16 as the eager path rounds them, probabilities not rounded, fp32 online softmax per 16-lane row, the
// workgroup's 16 position groups merged through LDS in the same order, partials published write-through (relaxed agent-scope stores,
// every wave drains vmcnt), ONE ticket per (sequence, head) -- the ticket word of the sequence's first row --, the last arriver combining
// every row's partials in split order, the ticket back at zero.  The causal tail is a per-row mask: row i takes keys p < min(pos + i + 1,
// p_lo + chunk) of a split and sits out the sweeps and splits that start beyond its last key (its `nlive` partials are fewer; the
// combine reads only those).  A key past a row's last one that the workgroup holds anyway (a later row needs it) enters that row with
// weight 0, as the clamped tail keys of ob_fdec_kernel do.
// Coverage: L = min(pos + i + 1, nsplit * chunk) and nlive = min(ceil(L / chunk), nsplit): a grid that does not cover the context
// attends to what it covers, writes every row and returns the ticket (onebit.h has always said so; ob_fdec_kernel does not clamp).
// Registers: the per-row state is (max, sum, out[8]) = 10 VGPRs, 160 at QT = 16, next to 64 for the sweep's keys / values (NI = 8); the
// queries wait in LDS (one ds_read_b128 per row and sweep).  Two workgroups per CU (2 waves per SIMD: 256 VGPRs) are kept by NOT
// double-buffering the sweeps at QT = 16 -- there the second workgroup's arithmetic (16 rows per key) covers the first one's loads --;
// QT <= 8 requests the next sweep before the current one's arithmetic as ob_fdec_kernel does.  LDS: 4 * QT * 512 B of merge room +
// QT * 256 B of queries (36 KiB at QT = 16: two workgroups fit in 160 KiB).
struct ObFdecMqArgs {
    ObFdecArgs a;                 // q [n_seq * Q, H, D], o [n_seq * Q, H * D]; row_slot / row_pos are read at a sequence's FIRST row
    int Q;                        // rows per sequence, 1 .. 16
};

template <int NI, int QT>
__global__ __launch_bounds__(OB_FD_THREADS) __attribute__((amdgpu_waves_per_eu(2))) void ob_fdec_mq_kernel(const ObFdecMqArgs B)
{
    constexpr bool PF = QT <= 8;
    __shared__ __attribute__((aligned(16))) float po[4 * QT * 128];       // [wave][row][128]
    __shared__ float red[QT * 8 + 4];                                      // [row][max x 4 | sum x 4] | last-arriver flag
    __shared__ __attribute__((aligned(16))) _Float16 q_s[QT * 128];
    const ObFdecArgs &A = B.a;
    const int head = blockIdx.x, seq = blockIdx.y, split = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ds = tid & 15, pg = tid >> 4;
    const int row0 = seq * B.Q;
    const int slot = A.row_slot ? A.row_slot[row0] : seq;
    const int pos = A.row_pos[row0];
    if (slot < 0 || slot >= A.n_slots || pos < 0 || pos >= A.max_len) return;        // idle sequence (uniform)
    const int nq = min(min(B.Q, QT), A.max_len - pos);                               // rows inside the cache
    const int cover = A.nsplit * A.chunk;
    const int Lmax = min(pos + nq, cover);                                           // keys the LAST row attends to
    const int p_lo = split * A.chunk;
    if (p_lo >= Lmax) return;                                                        // empty split (uniform)
    const int p_end = p_lo + A.chunk;
    const int p_hi_max = min(Lmax, p_end);
    const int nlive_max = (Lmax + A.chunk - 1) / A.chunk;                            // workgroups that take a ticket (<= nsplit)
    const int D = A.D, H = A.H;
    const int kvh = head / (H / A.Hkv);
    const bool dok = 8 * ds < D;
    const int dcl = dok ? 8 * ds : 0;
    const _Float16 *kb = A.k + (((int64_t)slot * A.Hkv + kvh) * A.max_len) * D + dcl;
    const _Float16 *vb = A.v + (((int64_t)slot * A.Hkv + kvh) * A.max_len) * D + dcl;
    ob_half8 k8[NI], v8[NI], kn[PF ? NI : 1], vn[PF ? NI : 1];
    auto fetch = [&](ob_half8 *kd, ob_half8 *vd, int base) {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int64_t off = (int64_t)min(base + pg + OB_FD_PG * i, Lmax - 1) * D;
            kd[i] = __builtin_nontemporal_load(reinterpret_cast<const ob_half8 *>(kb + off));
            vd[i] = __builtin_nontemporal_load(reinterpret_cast<const ob_half8 *>(vb + off));
        }
    };
    fetch(k8, v8, p_lo);
    for (int t = tid; t < QT * 16; t += OB_FD_THREADS) {                             // queries -> LDS, zero beyond D and beyond nq
        const int r = t >> 4, d8 = t & 15;
        ob_half8 qv = (ob_half8)(_Float16)0;
        if (r < nq && 8 * d8 < D) qv = *reinterpret_cast<const ob_half8 *>(A.q + ((int64_t)(row0 + r) * H + head) * D + 8 * d8);
        *reinterpret_cast<ob_half8 *>(q_s + r * 128 + 8 * d8) = qv;
    }
    __syncthreads();
    auto dot8 = [](const ob_half8 a, const ob_half8 b) {
        float acc = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const ob_half2 x = {a[2 * e], a[2 * e + 1]}, y = {b[2 * e], b[2 * e + 1]};
            acc = __builtin_amdgcn_fdot2(x, y, acc, false);
        }
        return acc;
    };
    float m[QT], l[QT], o[QT][8];
#pragma unroll
    for (int r = 0; r < QT; ++r) {
        m[r] = -INFINITY; l[r] = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[r][e] = 0.f;
    }
    for (int base = p_lo; base < p_hi_max; base += OB_FD_PG * NI) {
        const bool more = base + OB_FD_PG * NI < p_hi_max;                           // (uniform)
        if (PF && more) fetch(kn, vn, base + OB_FD_PG * NI);
#pragma unroll
        for (int r = 0; r < QT; ++r) {
            const int p_hi = min(min(pos + r + 1, cover), p_end);                    // this row's last key of the split, exclusive
            if (r < nq && base < p_hi) {                                             // (uniform) the row alone would sweep here too
                const ob_half8 q8 = *reinterpret_cast<const ob_half8 *>(q_s + r * 128 + 8 * ds);
                float sc[NI];
                float mx = -INFINITY;
#pragma unroll
                for (int i = 0; i < NI; ++i) {
                    const int p = base + pg + OB_FD_PG * i;
                    const float dot = ob_fd_row_sum(dot8(q8, k8[i]));
                    const float sv = ob_round_h(ob_round_h(dot) * A.inv_sqrt_d);
                    sc[i] = p < p_hi ? sv : -INFINITY;
                    mx = fmaxf(mx, sc[i]);
                }
                if (mx > m[r]) {
                    const float f = __expf(m[r] - mx);
                    l[r] *= f;
#pragma unroll
                    for (int e = 0; e < 8; ++e) o[r][e] *= f;
                    m[r] = mx;
                }
#pragma unroll
                for (int i = 0; i < NI; ++i) {
                    const float pe = sc[i] == -INFINITY ? 0.f : __expf(sc[i] - m[r]);
                    l[r] += pe;
#pragma unroll
                    for (int e = 0; e < 8; ++e) o[r][e] = __builtin_fmaf(pe, (float)v8[i][e], o[r][e]);
                }
            }
        }
        if (more) {
            if (PF) {
#pragma unroll
                for (int i = 0; i < NI; ++i) { k8[i] = kn[i]; v8[i] = vn[i]; }
            } else fetch(k8, v8, base + OB_FD_PG * NI);
        }
    }
    // ---- merge the workgroup's 16 position groups, row by row as ob_fdec_kernel does for its one row
#pragma unroll
    for (int r = 0; r < QT; ++r) {
        const float mw = ob_fd_rows_max(m[r]);
        if (lane == 0) red[r * 8 + wave] = mw;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < QT; ++r) {
        if (r < nq && p_lo < min(pos + r + 1, cover)) {                              // (uniform) the row has keys in this split
            const float M = fmaxf(fmaxf(red[r * 8], red[r * 8 + 1]), fmaxf(red[r * 8 + 2], red[r * 8 + 3]));
            const float f = m[r] == -INFINITY ? 0.f : __expf(m[r] - M);
            const float ls = ob_fd_rows_sum(l[r] * f);
            float os[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) os[e] = ob_fd_rows_sum(o[r][e] * f);
            if (lane < 16) {
                float *dst = po + (wave * QT + r) * 128 + 8 * ds;
                *reinterpret_cast<ob_float4 *>(dst) = (ob_float4){os[0], os[1], os[2], os[3]};
                *reinterpret_cast<ob_float4 *>(dst + 4) = (ob_float4){os[4], os[5], os[6], os[7]};
            }
            if (lane == 0) red[r * 8 + 4 + wave] = ls;
        }
    }
    __syncthreads();
    // ---- per row: the whole context in this split -> the output; else publish the partial (threads 0 .. 127 even rows, 128 .. 255 odd)
    const int th = tid >> 7, td = tid & 127;
    for (int r = th; r < nq; r += 2) {
        const int L = min(pos + r + 1, cover);
        if (p_lo >= L) continue;
        const int nlive = (L + A.chunk - 1) / A.chunk;
        const float acc = (po[(0 * QT + r) * 128 + td] + po[(1 * QT + r) * 128 + td]) + (po[(2 * QT + r) * 128 + td] + po[(3 * QT + r) * 128 + td]);
        const float lt = (red[r * 8 + 4] + red[r * 8 + 5]) + (red[r * 8 + 6] + red[r * 8 + 7]);
        const int64_t rh = (int64_t)(row0 + r) * H + head;
        if (nlive == 1) {
            if (td < D) {
                _Float16 oh = (_Float16)(acc / lt);
                if (A.h_next) oh = oh * A.h_next[head * D + td];
                A.o[rh * D + td] = oh;
            }
            continue;
        }
        const float M = fmaxf(fmaxf(red[r * 8], red[r * 8 + 1]), fmaxf(red[r * 8 + 2], red[r * 8 + 3]));
        float *pso = A.part_o + (rh * A.nsplit) * 128;
        float *pml = A.part_ml + (rh * A.nsplit) * 2;
        __hip_atomic_store(pso + split * 128 + td, acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (td == 0) __hip_atomic_store(pml + split * 2, M, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (td == 1) __hip_atomic_store(pml + split * 2 + 1, lt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (nlive_max == 1) return;                                                      // (uniform) no row has a second split
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                 // every wave: its stores have left
    __syncthreads();
    const int64_t tk = (int64_t)row0 * H + head;                                     // the sequence's ticket: its first row's word
    if (tid == 0) {
        const int prev = __hip_atomic_fetch_add(A.counter + tk, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = prev == nlive_max - 1;
        if (last) __hip_atomic_store(A.counter + tk, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        red[QT * 8] = last ? 1.f : 0.f;
    }
    __syncthreads();
    if (red[QT * 8] == 0.f) return;
    for (int r = th; r < nq; r += 2) {
        const int L = min(pos + r + 1, cover);
        const int nlive = (L + A.chunk - 1) / A.chunk;
        if (nlive == 1 || td >= D) continue;
        const int64_t rh = (int64_t)(row0 + r) * H + head;
        const float *pso = A.part_o + (rh * A.nsplit) * 128;
        const float *pml = A.part_ml + (rh * A.nsplit) * 2;
        float Mg = -INFINITY, ls = 0.f, os = 0.f;
        for (int s0 = 0; s0 < nlive; s0 += 16) {
            float pm[16], pl[16], pv[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int s = min(s0 + j, nlive - 1);
                pm[j] = __hip_atomic_load(pml + 2 * s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                pl[j] = __hip_atomic_load(pml + 2 * s + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                pv[j] = __hip_atomic_load(pso + s * 128 + td, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            float mb = Mg;
#pragma unroll
            for (int j = 0; j < 16; ++j) mb = fmaxf(mb, pm[j]);
            const float fo = Mg == -INFINITY ? 0.f : __expf(Mg - mb);
            ls *= fo; os *= fo; Mg = mb;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                if (s0 + j < nlive) {
                    const float w = __expf(pm[j] - Mg);
                    ls = __builtin_fmaf(pl[j], w, ls);
                    os = __builtin_fmaf(pv[j], w, os);
                }
            }
        }
        _Float16 oh = (_Float16)(os / ls);
        if (A.h_next) oh = oh * A.h_next[head * D + td];
        A.o[rh * D + td] = oh;
    }
}

// ------------------------------------------------------------------------------------------------------- the commit kernel --
// One workgroup, integers only, a pure function of its inputs.  With p = *pos (the position of tokens[0], the sequence's last token):
//   n_emit = max(0, min(1 + |longest prefix with drafts[i] == chosen[i]|, max_len - 1 - p, *remaining));  n_acc = n_emit - 1
//   history[p + 1 .. p + n_emit] = chosen[0 .. n_emit - 1];  P = p + n_emit;  *pos = P;  *remaining -= n_emit
//   next drafts: for n = ngram_max .. ngram_min (n <= P): the LATEST e in [n - 1, P - 1] with history[e - n + 1 .. e] ==
//   history[P - n + 1 .. P]; the first n that has one gives the followers history[e + 1 .. min(e + k, P)] (n_drafted of them, >= 1);
//   the remaining draft slots repeat history[P]
//   tokens = [history[P], drafts], row_pos = [P, P + 1, .. P + k], record = (n_acc, P, n_drafted)
// The history lives in LDS for the search (dynamic, 4 * max_len bytes).
struct ObSpecCommitArgs {
    const int32_t *chosen;        // [k + 1] the step's tokens (argmax or the sampler's draw per row)
    int32_t *drafts;              // [k] in: the drafts the step verified; out: the next step's
    int32_t *tokens, *row_pos;    // [k + 1] out
    int32_t *pos, *remaining;     // [1] in / out
    int32_t *history;             // [max_len]
    int32_t *record;              // [3] out
    int k, max_len, ngram_max, ngram_min;
};
#define OB_SPEC_THREADS 256
#define OB_SPEC_MAX_LEN 15360     // 60 KiB of LDS

__global__ __launch_bounds__(OB_SPEC_THREADS) void ob_spec_commit_kernel(const ObSpecCommitArgs A)
{
    extern __shared__ int32_t hist[];
    __shared__ int best[OB_SPEC_THREADS / 64];
    const int tid = threadIdx.x, k = A.k;
    const int p = min(max(A.pos[0], 0), A.max_len - 1);
    const int rem = A.remaining[0];
    int n_match = 0;
    while (n_match < k && A.drafts[n_match] == A.chosen[n_match]) ++n_match;         // (uniform; <= 15 scalar compares)
    const int n_emit = max(0, min(min(n_match + 1, A.max_len - 1 - p), rem));
    const int P = p + n_emit;
    for (int i = tid; i <= P; i += OB_SPEC_THREADS) {
        const int t = i <= p ? A.history[i] : A.chosen[i - p - 1];
        hist[i] = t;
        if (i > p) A.history[i] = t;
    }
    __syncthreads();                                                                 // (also: every thread has read the old drafts)
    int e_best = -1;
    for (int n = min(A.ngram_max, P); n >= max(A.ngram_min, 1); --n) {               // (uniform)
        int e_max = -1;
        for (int e = n - 1 + tid; e <= P - 1; e += OB_SPEC_THREADS) {
            bool eq = true;
            for (int j = 0; j < n; ++j) eq = eq && hist[e - j] == hist[P - j];
            if (eq) e_max = e;                                                       // (ascending: the thread's latest)
        }
        for (int o = 32; o > 0; o >>= 1) e_max = max(e_max, __shfl_xor(e_max, o));
        if ((tid & 63) == 0) best[tid >> 6] = e_max;
        __syncthreads();
        e_max = max(max(best[0], best[1]), max(best[2], best[3]));
        __syncthreads();
        if (e_max >= 0) { e_best = e_max; break; }
    }
    const int n_drafted = e_best >= 0 ? min(k, P - e_best) : 0;
    if (tid <= k) {
        const int t = tid == 0 || tid > n_drafted ? hist[P] : hist[e_best + tid];
        A.tokens[tid] = t;
        A.row_pos[tid] = P + tid;
        if (tid > 0) A.drafts[tid - 1] = t;
    }
    if (tid == 0) {
        A.pos[0] = P;
        A.remaining[0] = rem - n_emit;
        A.record[0] = n_emit - 1; A.record[1] = P; A.record[2] = n_drafted;
    }
}
