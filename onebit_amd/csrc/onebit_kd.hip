// Knowledge-distillation loss (additive to ABI 10): the token loss (KL + shifted cross-entropy) and the hidden-state loss of the
// reference's KDTrainer.compute_loss, forward and backward.  Kernels: ob_kd.h.  Stream-ordered, no allocation, caller-owned memory.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/onebit.h"
#include "ob_host.h"
#include "ob_kd.h"

#define OB_KD_MAX_WIDTH (1 << 30)
static_assert(OB_KD_TSTATS == ONEBIT_KD_TOKEN_STATS && OB_KD_HSTATS == ONEBIT_KD_HIDDEN_STATS, "stats row widths of the header");

// argument checks shared by the four entry points; > 0: nothing to do (T == 0)
static int ob_kd_check(const char *what, int64_t T, int64_t W, int dtype, bool ptrs_ok, int64_t chunk)
{
    if (T < 0) return ob_fail(ONEBIT_E_ARG, "%s: negative row count", what);
    if (W <= 0 || W > OB_KD_MAX_WIDTH) return ob_fail(ONEBIT_E_SHAPE, "%s: row width %lld outside 1..%d", what, (long long)W, OB_KD_MAX_WIDTH);
    if (dtype != ONEBIT_F16 && dtype != ONEBIT_F32) return ob_fail(ONEBIT_E_DTYPE, "%s: unknown dtype %d", what, dtype);
    if (T == 0) return 1;
    if (!ptrs_ok) return ob_fail(ONEBIT_E_ARG, "%s: null pointer", what);
    if (T * ((W + chunk - 1) / chunk) > 0x7fffffffLL) return ob_fail(ONEBIT_E_SHAPE, "%s: %lld rows of %lld exceed one grid", what, (long long)T, (long long)W);
    return 0;
}

// every group of four elements of every row aligned for one load: the base for the group's width, the pitch a whole number of groups
template <typename T>
static bool ob_kd_vec_ok(int64_t W, const void *a, const void *b, const void *c = nullptr)
{
    const size_t w = 4 * sizeof(T);
    return W % 4 == 0 && ob_aligned(a, w) && ob_aligned(b, w) && (!c || ob_aligned(c, w));
}

static int ob_kd_rows_sum(const float *stats, const int64_t *labels, int64_t ignore_index, int64_t T, int stride, int col, float *sums,
                          hipStream_t st)
{
    hipLaunchKernelGGL(ob_kd_rows_sum_kernel, dim3(1), dim3(1024), 0, st, stats, labels, ignore_index, T, stride, col, sums);
    return ob_launch_status("kd rows sum");
}

template <typename T>
static int ob_kd_token_forward_t(const void *s, const void *t, const int64_t *labels, float *stats, int64_t rows, int V,
                                 int64_t ignore_index, hipStream_t st)
{
    const T *sp = (const T *)s, *tp = (const T *)t;
    const bool vec = ob_kd_vec_ok<T>(V, s, t), small = V <= OB_KD_SMALL * OB_KD_NV * 4;
#define OB_KD_TF(THREADS, VEC) \
    hipLaunchKernelGGL((ob_kd_token_fwd_kernel<T, THREADS, VEC>), dim3((unsigned)rows), dim3(THREADS), 0, st, sp, tp, labels, stats, V, ignore_index)
    if (small) { if (vec) OB_KD_TF(OB_KD_SMALL, true); else OB_KD_TF(OB_KD_SMALL, false); }
    else       { if (vec) OB_KD_TF(OB_KD_LARGE, true); else OB_KD_TF(OB_KD_LARGE, false); }
#undef OB_KD_TF
    return ob_launch_status("kd_token_forward");
}

template <typename T>
static int ob_kd_hidden_forward_t(const void *s, const void *t, float *stats, int64_t rows, int H, hipStream_t st)
{
    const T *sp = (const T *)s, *tp = (const T *)t;
    const bool vec = ob_kd_vec_ok<T>(H, s, t), small = H <= OB_KD_SMALL * OB_KD_HNV * 4;
#define OB_KD_HF(THREADS, VEC) \
    hipLaunchKernelGGL((ob_kd_hidden_fwd_kernel<T, THREADS, VEC>), dim3((unsigned)rows), dim3(THREADS), 0, st, sp, tp, stats, H)
    if (small) { if (vec) OB_KD_HF(OB_KD_SMALL, true); else OB_KD_HF(OB_KD_SMALL, false); }
    else       { if (vec) OB_KD_HF(2 * OB_KD_SMALL, true); else OB_KD_HF(2 * OB_KD_SMALL, false); }
#undef OB_KD_HF
    return ob_launch_status("kd_hidden_forward");
}

static const int64_t OB_KD_BWD_CHUNK = OB_KD_BWD_THREADS * OB_KD_BWD_GROUPS * 4;

template <typename T>
static int ob_kd_token_backward_t(const void *s, const void *t, const int64_t *labels, const float *stats, const float *coef,
                                  void *grad, int64_t rows, int V, int64_t ignore_index, hipStream_t st)
{
    const int nchunk = (int)((V + OB_KD_BWD_CHUNK - 1) / OB_KD_BWD_CHUNK);
    const dim3 grid((unsigned)(rows * nchunk));
    if (ob_kd_vec_ok<T>(V, s, t, grad))
        hipLaunchKernelGGL((ob_kd_token_bwd_kernel<T, true>), grid, dim3(OB_KD_BWD_THREADS), 0, st, (const T *)s, (const T *)t, labels, stats,
                           coef, (T *)grad, V, nchunk, ignore_index);
    else
        hipLaunchKernelGGL((ob_kd_token_bwd_kernel<T, false>), grid, dim3(OB_KD_BWD_THREADS), 0, st, (const T *)s, (const T *)t, labels, stats,
                           coef, (T *)grad, V, nchunk, ignore_index);
    return ob_launch_status("kd_token_backward");
}

template <typename T>
static int ob_kd_hidden_backward_t(const void *s, const void *t, const float *stats, const float *coef, void *grad, int64_t rows,
                                   int H, hipStream_t st)
{
    const int nchunk = (int)((H + OB_KD_BWD_CHUNK - 1) / OB_KD_BWD_CHUNK);
    const dim3 grid((unsigned)(rows * nchunk));
    if (ob_kd_vec_ok<T>(H, s, t, grad))
        hipLaunchKernelGGL((ob_kd_hidden_bwd_kernel<T, true>), grid, dim3(OB_KD_BWD_THREADS), 0, st, (const T *)s, (const T *)t, stats, coef,
                           (T *)grad, H, nchunk);
    else
        hipLaunchKernelGGL((ob_kd_hidden_bwd_kernel<T, false>), grid, dim3(OB_KD_BWD_THREADS), 0, st, (const T *)s, (const T *)t, stats, coef,
                           (T *)grad, H, nchunk);
    return ob_launch_status("kd_hidden_backward");
}

extern "C" int onebit_kd_token_forward(const void *student, const void *teacher_or_null, const int64_t *labels_or_null, float *stats,
                                       float *sums, int64_t T, int64_t V, int dtype, int64_t ignore_index, void *stream)
{
    int rc = ob_kd_check("kd_token_forward", T, V, dtype, student && stats && sums, OB_KD_MAX_WIDTH);
    if (rc) return rc < 0 ? rc : 0;
    hipStream_t st = (hipStream_t)stream;
    rc = dtype == ONEBIT_F16 ? ob_kd_token_forward_t<_Float16>(student, teacher_or_null, labels_or_null, stats, T, (int)V, ignore_index, st)
                             : ob_kd_token_forward_t<float>(student, teacher_or_null, labels_or_null, stats, T, (int)V, ignore_index, st);
    return rc ? rc : ob_kd_rows_sum(stats, labels_or_null, ignore_index, T, OB_KD_TSTATS, 4, sums, st);
}

extern "C" int onebit_kd_token_backward(const void *student, const void *teacher_or_null, const int64_t *labels_or_null, const float *stats,
                                        const float *coef, void *grad, int64_t T, int64_t V, int dtype, int64_t ignore_index,
                                        void *stream)
{
    int rc = ob_kd_check("kd_token_backward", T, V, dtype, student && stats && coef && grad, OB_KD_BWD_CHUNK);
    if (rc) return rc < 0 ? rc : 0;
    hipStream_t st = (hipStream_t)stream;
    return dtype == ONEBIT_F16
        ? ob_kd_token_backward_t<_Float16>(student, teacher_or_null, labels_or_null, stats, coef, grad, T, (int)V, ignore_index, st)
        : ob_kd_token_backward_t<float>(student, teacher_or_null, labels_or_null, stats, coef, grad, T, (int)V, ignore_index, st);
}

extern "C" int onebit_kd_hidden_forward(const void *student, const void *teacher, float *stats, float *sums, int64_t T, int64_t H,
                                        int dtype, void *stream)
{
    int rc = ob_kd_check("kd_hidden_forward", T, H, dtype, student && teacher && stats && sums, OB_KD_MAX_WIDTH);
    if (rc) return rc < 0 ? rc : 0;
    if (!ob_aligned(stats, 16)) return ob_fail(ONEBIT_E_ALIGN, "kd_hidden_forward: stats not 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    rc = dtype == ONEBIT_F16 ? ob_kd_hidden_forward_t<_Float16>(student, teacher, stats, T, (int)H, st)
                             : ob_kd_hidden_forward_t<float>(student, teacher, stats, T, (int)H, st);
    return rc ? rc : ob_kd_rows_sum(stats, nullptr, 0, T, OB_KD_HSTATS, 2, sums, st);
}

extern "C" int onebit_kd_hidden_backward(const void *student, const void *teacher, const float *stats, const float *coef, void *grad,
                                         int64_t T, int64_t H, int dtype, void *stream)
{
    int rc = ob_kd_check("kd_hidden_backward", T, H, dtype, student && teacher && stats && coef && grad, OB_KD_BWD_CHUNK);
    if (rc) return rc < 0 ? rc : 0;
    if (!ob_aligned(stats, 16)) return ob_fail(ONEBIT_E_ALIGN, "kd_hidden_backward: stats not 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    return dtype == ONEBIT_F16 ? ob_kd_hidden_backward_t<_Float16>(student, teacher, stats, coef, grad, T, (int)H, st)
                               : ob_kd_hidden_backward_t<float>(student, teacher, stats, coef, grad, T, (int)H, st);
}
