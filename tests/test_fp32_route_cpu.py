"""The fp32 route query ``onebit_linear_f32_route``: declared in the header, listed in the binding, exported by the
library, and answering without a GPU (it is a pure function of the shape and the packed row pitch)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "onebit_linear_f32_route"


def test_symbol_declared_listed_and_exported():
    from onebit_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "onebit.h")).read()
    assert re.search(r"\bint\s+" + NAME + r"\s*\(\s*int64_t\s+T\s*,\s*int64_t\s+K\s*,\s*int64_t\s+N\s*,\s*int64_t\s+ldw_bytes\s*\)\s*;", hdr)
    assert NAME in _lib.SYMBOLS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME)             # (a fresh handle: not what load() cached)


def test_abi_version_unchanged():
    from onebit_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "onebit.h")).read()
    assert re.search(r"#define\s+ONEBIT_ABI_VERSION\s+10\b", hdr)
    assert _lib.ABI_VERSION == 10
    assert _lib.load().onebit_abi_version() == 10


def test_route_of_shapes():
    from onebit_amd import _lib
    route = _lib.load().onebit_linear_f32_route
    assert route(1, 4096, 11008, 512) == 1                       # one token, 16-byte aligned pitch: GEMV
    assert route(2048, 4096, 11008, 512) == 2                    # tiled MFMA GEMM
    assert route(12, 11008, 4096, 1376) == 2
    assert route(2, 688, 48, 86) == 0                            # K % 32 != 0
    assert route(1, 688, 48, 86) == 0
    for T, K, N in ((1, 4096, 11008), (12, 4096, 11008), (2048, 11008, 4096)):
        assert route(T, K, N, K // 8 + 1) == 0                   # pitch not a multiple of 4: the generic kernel (the A/B handle)
    # one token on rows the 16-byte loads cannot take, or too long for the LDS image: the GEMM takes it
    assert route(1, 4096, 11008, 516) == 2
    assert route(1, 352, 48, 44) == 2
    assert route(1, 32768, 64, 4096) == 2
    # empty calls and a pitch shorter than the row
    assert route(0, 4096, 11008, 512) == 0 and route(4, 0, 16, 0) == 0 and route(4, 64, 0, 8) == 0
    assert route(4, 4096, 16, 256) == 0
