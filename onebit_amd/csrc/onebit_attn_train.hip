// Train-mode causal self-attention (additive to ABI 10): forward with log-sum-exp, and the backward (dq, dk, dv) in three launches
// (delta, dK / dV, dQ).  Kernels: ob_flash_train.h.  Stream-ordered, no allocation, no atomics, caller-owned memory.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/onebit.h"
#include "ob_host.h"
#include "ob_flash_train.h"

// size checks shared by the three entry points; > 0: nothing to do (B == 0 or S == 0)
static int ob_ft_check(const char *what, int64_t B, int64_t S, int32_t H, int32_t Hkv, int32_t D)
{
    if (B < 0 || S < 0 || H <= 0 || Hkv <= 0) return ob_fail(ONEBIT_E_ARG, "%s: bad size", what);
    if ((D != 64 && D != 128) || H % Hkv != 0) return ob_fail(ONEBIT_E_SHAPE, "%s: head_dim %d (64 or 128), heads %d / %d", what, D, H, Hkv);
    if (B == 0 || S == 0) return 1;
    const int64_t nblk = (S + OB_FT_BLK - 1) / OB_FT_BLK;
    if (S > 0x7fffffffLL - OB_FT_BLK || nblk * H * B > 0x7fffffffLL || B * S * H > 0x7fffffffLL * OB_FT_THREADS)
        return ob_fail(ONEBIT_E_ARG, "%s: dimension too large", what);
    return 0;
}

static ObFlashTrainArgs ob_ft_args(int64_t B, int64_t S, int32_t H, int32_t Hkv, int32_t D)
{
    ObFlashTrainArgs a = {};
    a.B = (int)B; a.S = (int)S; a.H = H; a.Hkv = Hkv; a.nblk = (int)((S + OB_FT_BLK - 1) / OB_FT_BLK);
    a.scale = 1.0f / sqrtf((float)D);
    a.scale_log2e = 1.4426950408889634f / sqrtf((float)D);
    return a;
}

extern "C" int onebit_attention_train_forward(const void *q, const void *k, const void *v, void *o, float *lse, int64_t B, int64_t S,
                                              int32_t n_heads, int32_t n_kv_heads, int32_t head_dim, void *stream)
{
    const int rc = ob_ft_check("attention_train_forward", B, S, n_heads, n_kv_heads, head_dim);
    if (rc) return rc < 0 ? rc : 0;
    if (!q || !k || !v || !o || !lse) return ob_fail(ONEBIT_E_ARG, "attention_train_forward: null pointer");
    if (!ob_aligned(q, 16) || !ob_aligned(k, 16) || !ob_aligned(v, 16) || !ob_aligned(o, 16) || !ob_aligned(lse, 4))
        return ob_fail(ONEBIT_E_ALIGN, "attention_train_forward: q / k / v / o must be 16-byte aligned");
    ObFlashTrainArgs a = ob_ft_args(B, S, n_heads, n_kv_heads, head_dim);
    a.q = (const _Float16 *)q; a.k = (const _Float16 *)k; a.v = (const _Float16 *)v; a.o = (_Float16 *)o; a.lse = lse;
    const dim3 grid((unsigned)((int64_t)a.nblk * n_heads * B));
    if (head_dim == 128) hipLaunchKernelGGL((ob_flash_train_fwd_kernel<128>), grid, dim3(OB_FT_THREADS), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((ob_flash_train_fwd_kernel<64>), grid, dim3(OB_FT_THREADS), 0, (hipStream_t)stream, a);
    return ob_launch_status("attention_train_forward");
}

extern "C" size_t onebit_attention_train_workspace_bytes(int64_t B, int64_t S, int32_t n_heads, int32_t n_kv_heads, int32_t head_dim)
{
    (void)n_kv_heads; (void)head_dim;
    if (B <= 0 || S <= 0 || n_heads <= 0) return 256;
    return (size_t)(((uint64_t)B * (uint64_t)S * (uint64_t)n_heads * sizeof(float) + 255) / 256 * 256);     // delta [B, H, S]
}

extern "C" int onebit_attention_train_backward(const void *q, const void *k, const void *v, const void *o, const float *lse, const void *d_o,
                                               void *dq, void *dk, void *dv, void *workspace, size_t workspace_bytes, int64_t B, int64_t S,
                                               int32_t n_heads, int32_t n_kv_heads, int32_t head_dim, void *stream)
{
    const int rc = ob_ft_check("attention_train_backward", B, S, n_heads, n_kv_heads, head_dim);
    if (rc) return rc < 0 ? rc : 0;
    if (!q || !k || !v || !o || !lse || !d_o || !dq || !dk || !dv || !workspace) return ob_fail(ONEBIT_E_ARG, "attention_train_backward: null pointer");
    if (workspace_bytes < onebit_attention_train_workspace_bytes(B, S, n_heads, n_kv_heads, head_dim))
        return ob_fail(ONEBIT_E_WSPACE, "attention_train_backward: workspace of %zu bytes, %zu needed", workspace_bytes,
                       onebit_attention_train_workspace_bytes(B, S, n_heads, n_kv_heads, head_dim));
    const void *al16[] = {q, k, v, o, d_o, dq, dk, dv};
    for (const void *p : al16)
        if (!ob_aligned(p, 16)) return ob_fail(ONEBIT_E_ALIGN, "attention_train_backward: the fp16 tensors must be 16-byte aligned");
    if (!ob_aligned(lse, 4) || !ob_aligned(workspace, 16)) return ob_fail(ONEBIT_E_ALIGN, "attention_train_backward: lse / workspace alignment");
    ObFlashTrainArgs a = ob_ft_args(B, S, n_heads, n_kv_heads, head_dim);
    a.q = (const _Float16 *)q; a.k = (const _Float16 *)k; a.v = (const _Float16 *)v; a.o = (_Float16 *)o; a.lse = (float *)lse;
    a.d_o = (const _Float16 *)d_o; a.delta = (float *)workspace;
    a.dq = (_Float16 *)dq; a.dk = (_Float16 *)dk; a.dv = (_Float16 *)dv;
    hipStream_t st = (hipStream_t)stream;
    const dim3 thr(OB_FT_THREADS);
    const dim3 grid_kv((unsigned)((int64_t)a.nblk * n_kv_heads * B)), grid_q((unsigned)((int64_t)a.nblk * n_heads * B));
    if (head_dim == 128) {
        hipLaunchKernelGGL((ob_flash_train_delta_kernel<128>), grid_q, thr, 0, st, a);
        hipLaunchKernelGGL((ob_flash_train_dkv_kernel<128>), grid_kv, thr, 0, st, a);
        hipLaunchKernelGGL((ob_flash_train_dq_kernel<128>), grid_q, thr, 0, st, a);
    } else {
        hipLaunchKernelGGL((ob_flash_train_delta_kernel<64>), grid_q, thr, 0, st, a);
        hipLaunchKernelGGL((ob_flash_train_dkv_kernel<64>), grid_kv, thr, 0, st, a);
        hipLaunchKernelGGL((ob_flash_train_dq_kernel<64>), grid_q, thr, 0, st, a);
    }
    return ob_launch_status("attention_train_backward");
}
