// SVID start checkpoints (additive to ABI 10): the rank-1 NMF of |A| that gives a teacher projection its weight_scale and
// input_factor, one alternating iteration per call, and the pass that emits sign(A) as latent weights / packed bits with the
// residual sums.  Kernels: ob_svid.h.  Stream-ordered, no allocation, caller-owned memory.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/onebit.h"
#include "ob_host.h"
#include "ob_svid.h"

static_assert(OB_SVID_STATS == ONEBIT_SVID_STATS && OB_SVID_ONEPASS_MAX_K == ONEBIT_SVID_ONEPASS_MAX_K, "constants of the header");

// how one iteration is cut into workgroups, and where its partials live in the workspace (offsets in floats)
struct ObSvidPlan {
    int route, threads, nch;
    int band_rows, nbands, nfin;
    size_t off_bandstat, off_finstat, floats;
};

static ObSvidPlan ob_svid_plan(int64_t N, int64_t K, int route)
{
    ObSvidPlan p = {};
    p.route = route;
    int max_bands = 256;
    if (route == 1) {
        p.threads = K <= 4096 ? 256 : 1024;
        p.nch = K <= (int64_t)p.threads * 8 ? 1 : 2;
        max_bands = p.threads == 256 ? 512 : 256;       // the chip's 256 CUs hold one 1024-thread workgroup each
    } else {
        p.threads = 256;
    }
    int64_t rows = (N + max_bands - 1) / max_bands;
    rows = (rows + OB_SVID_R - 1) / OB_SVID_R * OB_SVID_R;
    p.band_rows = (int)rows;
    p.nbands = (int)((N + rows - 1) / rows);
    p.nfin = (int)((K + OB_SVID_FIN_COLS - 1) / OB_SVID_FIN_COLS);
    p.off_bandstat = (size_t)p.nbands * (size_t)K;
    p.off_finstat = p.off_bandstat + (((size_t)2 * p.nbands + 1 + 3) & ~(size_t)3);
    p.floats = p.off_finstat + (size_t)2 * p.nfin;
    return p;
}

static int64_t ob_svid_emit_blocks(int64_t N, int64_t K)
{
    const int64_t per = 256 * OB_SVID_EMIT_ITERS;
    return (N * (K >> 3) + per - 1) / per;
}

static int ob_svid_check_shape(const char *what, int64_t N, int64_t K, int dtype)
{
    if (dtype != ONEBIT_F16 && dtype != ONEBIT_F32) return ob_fail(ONEBIT_E_DTYPE, "%s: unknown dtype %d", what, dtype);
    if (N < 1 || K < 1) return ob_fail(ONEBIT_E_ARG, "%s: N = %lld, K = %lld", what, (long long)N, (long long)K);
    if (K % 8 != 0) return ob_fail(ONEBIT_E_SHAPE, "%s: K = %lld is not a multiple of 8", what, (long long)K);
    if (N > 0x7fffffffLL || K > 0x7fffffffLL || ob_svid_emit_blocks(N, K) > 0x7fffffffLL)
        return ob_fail(ONEBIT_E_SHAPE, "%s: %lld x %lld exceeds one grid", what, (long long)N, (long long)K);
    return 0;
}

static int ob_svid_check_a(const char *what, const void *A, int dtype, int64_t lda, int64_t K)
{
    if (!A) return ob_fail(ONEBIT_E_ARG, "%s: null pointer", what);
    if (lda < K) return ob_fail(ONEBIT_E_ARG, "%s: row pitch %lld below K = %lld", what, (long long)lda, (long long)K);
    if (lda % 8 != 0 || !ob_aligned(A, 16)) return ob_fail(ONEBIT_E_ALIGN, "%s: A needs a 16-byte aligned base and a pitch that is a multiple of 8", what);
    return 0;
}

extern "C" int onebit_svid_route(int64_t N, int64_t K, int dtype)
{
    const int rc = ob_svid_check_shape("svid_route", N, K, dtype);
    if (rc) return rc;
    return K <= OB_SVID_ONEPASS_MAX_K ? 1 : 2;
}

extern "C" size_t onebit_svid_workspace_bytes(int64_t N, int64_t K, int dtype)
{
    if (ob_svid_check_shape("svid_workspace_bytes", N, K, dtype)) return 0;
    size_t floats = ob_svid_plan(N, K, 2).floats;
    if (K <= OB_SVID_ONEPASS_MAX_K) {
        const size_t f1 = ob_svid_plan(N, K, 1).floats;
        if (f1 > floats) floats = f1;
    }
    const size_t fe = (size_t)2 * (size_t)ob_svid_emit_blocks(N, K);
    if (fe > floats) floats = fe;
    return floats * sizeof(float);
}

template <typename T>
static int ob_svid_iterate_t(const void *A, int64_t lda, float *w, float *h, float *stats, float *ws, const ObSvidPlan &p, int N, int K,
                             hipStream_t st)
{
    const T *a = (const T *)A;
    float *part = ws, *bandstat = ws + p.off_bandstat, *finstat = ws + p.off_finstat;
    if (p.route == 1) {
        // 1024 threads have 128 registers each: two rows per step and no second register set (four rows spill)
        constexpr int RBIG = 2;
#define OB_SVID_ONE(THREADS, NCH) \
    hipLaunchKernelGGL((ob_svid_onepass_kernel<T, THREADS, NCH, (THREADS == 256 ? OB_SVID_R : RBIG), (THREADS == 256)>), dim3(p.nbands), dim3(THREADS), 0, st, a, lda, w, h, part, bandstat, N, K, p.band_rows)
        if (p.threads == 256) { if (p.nch == 1) OB_SVID_ONE(256, 1); else OB_SVID_ONE(256, 2); }
        else                  { if (p.nch == 1) OB_SVID_ONE(1024, 1); else OB_SVID_ONE(1024, 2); }
#undef OB_SVID_ONE
        if (int rc = ob_launch_status("svid one-pass")) return rc;
    } else {
        hipLaunchKernelGGL((ob_svid_rows_kernel<T>), dim3(p.nbands), dim3(256), 0, st, a, lda, w, h, bandstat, N, K, p.band_rows);
        if (int rc = ob_launch_status("svid rows")) return rc;
        const unsigned tiles = (unsigned)(((K >> 3) + 255) / 256);
        hipLaunchKernelGGL((ob_svid_cols_kernel<T>), dim3(p.nbands, tiles), dim3(256), 0, st, a, lda, w, part, N, K, p.band_rows);
        if (int rc = ob_launch_status("svid columns")) return rc;
    }
    hipLaunchKernelGGL(ob_svid_colfin_kernel, dim3(p.nfin), dim3(256), 0, st, part, bandstat, h, finstat, p.nbands, K);
    if (int rc = ob_launch_status("svid column finalize")) return rc;
    hipLaunchKernelGGL(ob_svid_stats_kernel, dim3(1), dim3(256), 0, st, bandstat, finstat, stats, p.nbands, p.nfin);
    return ob_launch_status("svid stats");
}

extern "C" int onebit_svid_iterate(const void *A, int dtype, int64_t lda, float *w, float *h, float *stats, void *workspace,
                                   size_t workspace_bytes, int64_t N, int64_t K, int route, void *stream)
{
    int rc = ob_svid_check_shape("svid_iterate", N, K, dtype);
    if (rc) return rc;
    if (!w || !h || !stats || !workspace) return ob_fail(ONEBIT_E_ARG, "svid_iterate: null pointer");
    if ((rc = ob_svid_check_a("svid_iterate", A, dtype, lda, K))) return rc;
    if (route < 0 || route > 2) return ob_fail(ONEBIT_E_ARG, "svid_iterate: route %d (0 automatic, 1 one-pass, 2 two-pass)", route);
    if (route == 1 && K > OB_SVID_ONEPASS_MAX_K)
        return ob_fail(ONEBIT_E_ARG, "svid_iterate: the one-pass route covers K <= %d, got %lld", OB_SVID_ONEPASS_MAX_K, (long long)K);
    if (!ob_aligned(h, 16) || !ob_aligned(workspace, 16)) return ob_fail(ONEBIT_E_ALIGN, "svid_iterate: h and the workspace must be 16-byte aligned");
    if (route == 0) route = K <= OB_SVID_ONEPASS_MAX_K ? 1 : 2;
    const ObSvidPlan p = ob_svid_plan(N, K, route);
    if (workspace_bytes < p.floats * sizeof(float))
        return ob_fail(ONEBIT_E_WSPACE, "svid_iterate: workspace %zu bytes, need %zu", workspace_bytes, p.floats * sizeof(float));
    hipStream_t st = (hipStream_t)stream;
    return dtype == ONEBIT_F16 ? ob_svid_iterate_t<_Float16>(A, lda, w, h, stats, (float *)workspace, p, (int)N, (int)K, st)
                               : ob_svid_iterate_t<float>(A, lda, w, h, stats, (float *)workspace, p, (int)N, (int)K, st);
}

template <typename T, typename TL>
static void ob_svid_emit_launch(const void *A, int64_t lda, const float *w, const float *h, void *latent, float scale, void *packed,
                                float *blockpart, int64_t N, int64_t K, hipStream_t st)
{
    hipLaunchKernelGGL((ob_svid_emit_kernel<T, TL>), dim3((unsigned)ob_svid_emit_blocks(N, K)), dim3(256), 0, st, (const T *)A, lda, w, h,
                       (TL *)latent, scale, (uint8_t *)packed, blockpart, N * (K >> 3), (int)(K >> 3));
}

extern "C" int onebit_svid_emit(const void *A, int dtype, int64_t lda, const float *w, const float *h, void *latent_or_null,
                                int latent_dtype, float scale, void *packed_or_null, float *sums_or_null, void *workspace,
                                size_t workspace_bytes, int64_t N, int64_t K, void *stream)
{
    int rc = ob_svid_check_shape("svid_emit", N, K, dtype);
    if (rc) return rc;
    if ((rc = ob_svid_check_a("svid_emit", A, dtype, lda, K))) return rc;
    if (latent_or_null && latent_dtype != ONEBIT_F16 && latent_dtype != ONEBIT_F32)
        return ob_fail(ONEBIT_E_DTYPE, "svid_emit: unknown latent dtype %d", latent_dtype);
    if (latent_or_null && !ob_aligned(latent_or_null, 16)) return ob_fail(ONEBIT_E_ALIGN, "svid_emit: latent output not 16-byte aligned");
    if (!latent_or_null && !packed_or_null && !sums_or_null) return 0;
    float *blockpart = nullptr;
    const int64_t nblocks = ob_svid_emit_blocks(N, K);
    if (sums_or_null) {
        if (!w || !h || !workspace) return ob_fail(ONEBIT_E_ARG, "svid_emit: the residual sums need w, h and the workspace");
        if (!ob_aligned(h, 16) || !ob_aligned(workspace, 16)) return ob_fail(ONEBIT_E_ALIGN, "svid_emit: h and the workspace must be 16-byte aligned");
        if (workspace_bytes < (size_t)2 * nblocks * sizeof(float))
            return ob_fail(ONEBIT_E_WSPACE, "svid_emit: workspace %zu bytes, need %zu", workspace_bytes, (size_t)2 * nblocks * sizeof(float));
        blockpart = (float *)workspace;
    }
    hipStream_t st = (hipStream_t)stream;
    const bool l16 = latent_or_null && latent_dtype == ONEBIT_F16;
    if (dtype == ONEBIT_F16) {
        if (l16) ob_svid_emit_launch<_Float16, _Float16>(A, lda, w, h, latent_or_null, scale, packed_or_null, blockpart, N, K, st);
        else     ob_svid_emit_launch<_Float16, float>(A, lda, w, h, latent_or_null, scale, packed_or_null, blockpart, N, K, st);
    } else {
        if (l16) ob_svid_emit_launch<float, _Float16>(A, lda, w, h, latent_or_null, scale, packed_or_null, blockpart, N, K, st);
        else     ob_svid_emit_launch<float, float>(A, lda, w, h, latent_or_null, scale, packed_or_null, blockpart, N, K, st);
    }
    if ((rc = ob_launch_status("svid emit"))) return rc;
    if (!sums_or_null) return 0;
    hipLaunchKernelGGL(ob_svid_emit_sum_kernel, dim3(1), dim3(1024), 0, st, blockpart, (int)nblocks, sums_or_null);
    return ob_launch_status("svid emit sums");
}
