// Sampled decoding (ABI 10): the standalone sampler over fp16 logits rows and the launcher the *_sampled decode steps
// use in place of their final argmax launch.  Kernel: ob_sample.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/onebit.h"
#include "ob_host.h"
#include "ob_sample.h"

int ob_sample_launch(const ObSampleCall &c, hipStream_t s)
{
    if (c.V < 1 || c.V > OB_SAMPLE_MAXV) return ob_fail(ONEBIT_E_SHAPE, "sample: vocab %d outside 1..%d", c.V, OB_SAMPLE_MAXV);
    if (c.rows < 1 || c.rows > (1 << 24)) return ob_fail(ONEBIT_E_SHAPE, "sample: %d rows outside 1..%d", c.rows, 1 << 24);
    if (!c.logits || !c.params || !c.pos || (!c.out && !(c.token && c.pos_w)) || (c.token && c.rows != 1))
        return ob_fail(ONEBIT_E_ARG, "sample: null pointer");
    if (c.ld != 0 && c.ld < c.V) return ob_fail(ONEBIT_E_SHAPE, "sample: row stride %lld < vocab %d", (long long)c.ld, c.V);
    ObSampleArgs a = {};
    a.logits = (const _Float16 *)c.logits; a.ld = c.ld; a.V = c.V; a.params = c.params;
    a.pos = c.pos; a.pos_rows = c.pos_rows; a.pos_add = c.pos_add; a.out = c.out;
    a.token = c.token; a.pos_w = c.pos_w; a.out_tokens = c.out_tokens; a.max_out = c.max_out;
    const size_t lds = ((size_t)c.V * 2 + 15) & ~(size_t)15;
    static bool attr_set[OB_MAX_DEVICES] = {};
    ob_set_max_lds_once(ob_sample_kernel, attr_set, OB_SAMPLE_MAXV * 2);
    hipLaunchKernelGGL(ob_sample_kernel, dim3(c.rows), dim3(OB_SAMPLE_THREADS), lds, s, a);
    return ob_launch_status("sample");
}

extern "C" int onebit_sample_rows(const void *logits, int64_t ld, int32_t vocab, int32_t rows, const onebit_sample_params_t *params,
                                  const int32_t *positions, int32_t *out_tokens, void *stream)
{
    if (!logits || !params || !positions || !out_tokens) return ob_fail(ONEBIT_E_ARG, "sample_rows: null pointer");
    ObSampleCall c = {};
    c.logits = logits; c.ld = ld; c.V = vocab; c.rows = rows; c.params = params;
    c.pos = positions; c.out = out_tokens;
    return ob_sample_launch(c, (hipStream_t)stream);
}
