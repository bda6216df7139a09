"""The A/B route switches of the native library and what each one is held to.

Every ``OB_*`` environment variable the library reads selects another kernel, kernel instance, grid or launch plan.  One row per
(variable, value) to test; ``tests/test_gpu_route_switches.py`` runs each row's workloads in a fresh interpreter
(``tests/route_switch_child.py``: the switches are read once per process) and ``tests/test_route_switches_cpu.py`` keeps this table,
the sources and DESIGN.md section 6a in step.

Row fields:
  env       the switch (several variables: a switch that only acts within another one's route)
  base      the environment the row is compared with ({} = the product's routes)
  workloads what the child runs (route_switch_child.WORKLOADS); the child asserts each workload's own bars (oracle / reference)
  acts_on   workloads whose launched kernels (names, grids, counts) must differ from the base run's: the row's route was taken.
            Empty: the switch must change nothing at all here (the kernel lists must be equal)
  relation  "bits": every output bit-identical to the base run; "oracle": within the workload's bars, like every other route
  why       the reading of the code the relation rests on
"""

BITS, ORACLE = "bits", "oracle"


def _row(env, workloads, relation, why, acts_on=None, base=None):
    return {"env": dict(env), "base": dict(base or {}), "workloads": list(workloads),
            "acts_on": list(workloads if acts_on is None else acts_on), "relation": relation, "why": why}


ROWS = [
    # ---- prefill GEMMs of onebit_linear_forward / the mixed step
    _row({"OB_GEMM3": "0"}, ["linear", "mixed"], ORACLE, "register-staged kernels instead of the LDS-DMA GEMM, grouped and K-sliced launches: other fp32 summation orders"),
    _row({"OB_GEMM3": "2"}, ["linear"], ORACLE, "the LDS-DMA GEMM forced onto small ragged shapes the default sends to the 128 x 128 / K-sliced kernels"),
    _row({"OB_GEMM2": "2"}, ["linear"], ORACLE, "register-staged 256 x 256 kernel on the no-workspace-route shapes with T >= 192 (300 x 512 -> 260)"),
    _row({"OB_GEMM3": "0", "OB_GEMM2": "2"}, ["linear"], ORACLE, "the register-staged 256 x 256 kernel on every eligible shape"),
    _row({"OB_GEMM3": "2", "OB_GEMM4": "1"}, ["linear"], ORACLE, "32x32x16-MFMA form: another MFMA shape, another summation order"),
    _row({"OB_GEMM4": "1"}, ["mixed"], ORACLE, "grouped q|k|v / gate|up launches of the mixed step on the 32x32x16-MFMA kernel"),
    _row({"OB_GEMM3": "2", "OB_GEMM3_WT": "2"}, ["linear"], BITS,
         "8-wave 256 x 256 tiles run the same per-output K loop as the 4-wave 256 x 128 tiles (onebit_hip.hip: 'bit-identical')",
         base={"OB_GEMM3": "2"}),
    _row({"OB_GEMM3_GROUPED": "0"}, ["mixed"], ORACLE, "one launch per projection: un-scaled rows, K-sliced / register-staged kernels instead of the grouped GEMM"),
    _row({"OB_GEMM3_GROUP_DEN": "1"}, ["mixed"], ORACLE, "13B q|k|v at 321 rows (180 tiles < 256 CUs) loses its grouped launch"),
    _row({"OB_GEMM3_GROUP_DEN": "8"}, ["mixed"], ORACLE, "13B q|k|v at 200 rows (120 tiles) is grouped instead of run as skinny passes"),
    _row({"OB_GEMM3_KSPLIT": "0"}, ["linear", "mixed"], ORACLE, "no K-sliced GEMM: one fp32 sum per output instead of slice sums added by the row pass"),
    _row({"OB_GEMM3_KSPLIT": "2"}, ["linear"], ORACLE, "K = 4096 in 2 slices instead of 4: another grouping of the fp32 sum"),
    _row({"OB_GEMM3_KSPLIT": "3"}, ["linear"], ORACLE, "K = 4096 in 3 slices instead of 4"),
    _row({"OB_GEMM3_KSPLIT_TILES": "1"}, ["linear"], ORACLE, "low: no projection is sliced (every shape has >= 1 tile)"),
    _row({"OB_GEMM3_KSPLIT_TILES": "4"}, ["linear"], ORACLE, "high: the 6-tile shape (130 x 2048 -> 520) leaves the sliced route, the 1-tile shapes keep it"),
    _row({"OB_GEMM3_KSPLIT_TMIN": "32"}, ["linear"], ORACLE, "low: 48 rows (a skinny-GEMM call by default) take the K-sliced GEMM"),
    _row({"OB_GEMM3_KSPLIT_TMIN": "128"}, ["linear"], ORACLE, "high: 66 rows leave the K-sliced GEMM for the 128 x 128 kernel"),
    _row({"OB_MIXED_SK_ROWS": "64"}, ["mixed"], ORACLE, "low: 65 / 200 rows run one GEMM per projection instead of <= 64-row skinny passes"),
    _row({"OB_MIXED_SK_ROWS": "1024", "OB_GEMM3_GROUPED": "0"}, ["mixed"], ORACLE,
         "high: without grouped launches 543 / 700 rows run as skinny passes (the grouped GEMM comes first otherwise)",
         base={"OB_GEMM3_GROUPED": "0"}),
    _row({"OB_MIXED_TAIL": "0"}, ["mixed"], ORACLE, "543 rows at 13B: the 31-row tail stays in the grouped launch (one more round) instead of skinny passes"),
    _row({"OB_MIXED_TAIL": "16"}, ["mixed"], ORACLE, "low: the 31-row tail is above the limit -- the same route as 0"),
    _row({"OB_LN_ROWS": "0"}, ["linear"], ORACLE, "ob_layernorm_rows_kernel: another reduction order of the LayerNorm statistics"),
    # ---- skinny GEMMs: module path and batched step
    _row({"OB_SKINNY": "0"}, ["linear"], ORACLE, "2..64 rows on the 64-row MFMA GEMM tiles instead of the skinny kernel"),
    _row({"OB_SKINNY3": "0"}, ["batched"], ORACLE, "first-form skinny kernels (x scaled in the kernel, split-K o / down) instead of the LDS-DMA form"),
    _row({"OB_SKINNY3": "0", "OB_BATCH_SPLITK": "0"}, ["batched"], ORACLE, "first form without split-K: o / down as one K range",
         base={"OB_SKINNY3": "0"}),
    _row({"OB_SKINNY3": "0", "OB_SKINNY": "0"}, ["batched"], ORACLE, "first form on the 64-row MFMA GEMM tiles (no skinny kernel at all)",
         base={"OB_SKINNY3": "0"}),
] + [
    _row({"OB_SK3_RNT": str(r)}, ["batched"], ORACLE,
         f"{r} row tiles per workgroup: a row tile lands in another workgroup, whose first K piece (OB_SK3_ROT, ob_skinny3.h) and so "
         "the order of a wave's fp32 additions follow the workgroup index")
    for r in (1, 2, 3, 4, 6, 8)
] + [
    _row({"OB_SK3_OSPLIT": "0"}, ["batched"], ORACLE, "o_proj as one K range instead of two fp32 halves added by the norm kernel"),
    _row({"OB_SK3_PREFETCH": "0"}, ["batched"], BITS, "drops the prefetch-only workgroups of the norm kernels: L2 warming, no arithmetic"),
    _row({"OB_BATCH_CHAINS": "2"}, ["batched"], BITS, "two chains of consecutive slots; a row's sums never mix with other rows' and take the same K order"),
    _row({"OB_BATCH_ATTN_THREADS": "512"}, ["batched"], ORACLE, "8-wave attention workgroups: another split of the positions over the waves"),
    # ---- decode attention
    _row({"OB_FDEC_FUSED": "0"}, ["decode", "batched"], ORACLE, "rope / append launch + key-block attention instead of the fused form"),
    _row({"OB_ATTN_BLIND": "64"}, ["decode"], BITS, "blind window of 64 at position 92: the same arithmetic, fewer rows requested early", acts_on=["decode"]),
    _row({"OB_ATTN_BLIND": "128"}, ["decode"], BITS, "blind window of 128 at positions < 64: the same arithmetic, more rows requested early"),
    _row({"OB_ATTN_THREADS": "512"}, ["decode"], ORACLE, "8-wave single-stream attention: another split of the positions over the waves"),
    _row({"OB_DEC_PREFETCH_O": "0"}, ["decode"], BITS, "drops the attention launch's prefetch-only workgroups: L2 warming, no arithmetic"),
    # ---- decode GEMV
    _row({"OB_DECODE_MATH": "f16"}, ["linear", "gemv", "decode"], ORACLE, "fp16 sign-expansion MFMA instead of the exact integer dot products"),
    _row({"OB_DEC_WGP": "0"}, ["gemv", "decode"], ORACLE, "multi-projection launches in the per-slot form: another combination of the wave partials"),
    _row({"OB_DEC_I8_SINGLE": "0"}, ["gemv", "decode"], ORACLE, "single-chunk launches (o_proj) on the fp16 path instead of the integer path"),
    _row({"OB_DEC_WGS_PER_CU": "2"}, ["linear", "gemv"], BITS, "a grid of two workgroups per CU: a tile's dot products do not depend on the workgroup or slot that runs it",
         acts_on=["linear"]),
    _row({"OB_DEC_SWIGLU_WGS": "128"}, ["gemv", "decode"], BITS, "down_proj on 128 workgroups of two tiles: a tile's dot products do not depend on the workgroup or slot"),
    # ---- train mode
    _row({"OB_TRAIN_GEMM64": "1"}, ["train"], ORACLE, "fp16 train GEMMs on the 64 x 64 tiles: another MFMA tiling"),
    # ---- profiling builds only
    _row({"OB_ABLATE": "1"}, ["gemv"], BITS, "read by the decode GEMV but acted on only in -DOB_PROFILE_ABLATE builds", acts_on=[]),
    _row({"OB_TIMING": "1"}, ["gemv"], BITS, "read only in -DOB_PROFILE_STAMPS builds (there it allocates and passes the debug buffer)", acts_on=[]),
]

# variable -> id of the test that covers a switch no row sets (empty: every switch has rows.  The forced-route values of
# tests/test_gpu_parity.py::test_large_tile_kernels_forced_on_ragged_shapes are repeated above at this table's shapes)
COVERED_ELSEWHERE = {}


def row_id(row):
    base = "" if not row["base"] else "|base:" + ",".join(f"{k}={v}" for k, v in sorted(row["base"].items()))
    return ",".join(f"{k}={v}" for k, v in sorted(row["env"].items())) + base


def variables():
    """every variable the table sets"""
    return sorted({k for r in ROWS for k in r["env"]} | set(COVERED_ELSEWHERE))
