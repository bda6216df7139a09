"""CPU-only checks of the drop-in boundary: the C-ABI library loads, exports every symbol the
header declares, rejects bad arguments without touching a GPU, and the nn.Module mirrors the
reference's constructor / parameter contract."""
import ctypes
import os
import re

import pytest
import torch

from onebit_amd import _lib
from onebit_amd.bitnet import BitLinearInf, OneBitLinear

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_symbols():
    src = open(os.path.join(ROOT, "include", "onebit.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(onebit_[a-z0-9_]+)\s*\(", src))


def test_library_exports_every_declared_symbol():
    lib = _lib.load()
    syms = _header_symbols()
    assert syms, "no declarations found in include/onebit.h"
    assert syms == set(_lib.SYMBOLS), "ctypes binding and header disagree"
    for s in syms:
        assert hasattr(lib, s), s
    assert lib.onebit_abi_version() == _lib.ABI_VERSION


def test_argument_errors_without_gpu():
    lib = _lib.load()
    E_ARG, E_SHAPE, E_ALIGN, E_DTYPE, E_FLAG = -1, -2, -3, -4, -6
    assert lib.onebit_pack_signs(None, 0, None, 2, 12, None) == E_SHAPE
    assert b"multiple of 8" in lib.onebit_last_error()
    assert lib.onebit_pack_signs(None, 7, None, 2, 16, None) == E_DTYPE
    assert lib.onebit_pack_signs(None, 0, None, 2, 16, None) == E_ARG
    assert lib.onebit_pack_signs(None, 0, None, 0, 16, None) == 0          # empty is fine
    assert lib.onebit_unpack_signs(None, None, 0, -1, 16, None) == E_ARG
    buf = ctypes.create_string_buffer(4096)
    a = (ctypes.addressof(buf) + 63) & ~63
    fwd = lambda **kw: lib.onebit_linear_forward(
        kw.get("p", a), kw.get("ldw", 8), kw.get("x", a), a, a, None, kw.get("y", a), None, None, 0,
        kw.get("T", 1), kw.get("K", 64), kw.get("N", 4), kw.get("dt", 0), 1e-5, kw.get("fl", 0), None)
    assert fwd(K=44) == E_SHAPE
    assert fwd(dt=3) == E_DTYPE
    assert fwd(p=None) == E_ARG
    assert fwd(x=a + 2) == E_ALIGN
    assert fwd(ldw=6) == E_ALIGN          # pitch smaller than K/8
    assert fwd(K=40, ldw=5) == -5         # generic shape without workspace
    assert fwd(fl=64) == E_FLAG
    assert fwd(T=0) == 0
    # N-sharded LayerNorm halves and the batched step reject bad arguments before any launch
    assert lib.onebit_row_stats(a, a, 2, 0, 0, None) == E_SHAPE
    assert lib.onebit_row_stats(None, a, 2, 8, 0, None) == E_ARG
    assert lib.onebit_row_stats(a, a, 0, 8, 0, None) == 0
    assert lib.onebit_row_stats(a, a, 2, 8, 5, None) == E_DTYPE
    assert lib.onebit_normalize_rows(a, None, a, None, a, 2, 8, 0, None) == E_ARG
    assert lib.onebit_normalize_rows(a, a, a, None, a, -1, 8, 0, None) == E_ARG
    assert lib.onebit_decode_step_batched(None, None, None) == E_ARG
    from onebit_amd.engine import _BatchState, _Layer, _Model
    layers = (_Layer * 1)()
    m = _Model(1, 64, 128, 2, 2, 32, 16, 8, 1e-6, 1e-5, layers, a, a, a, a, a)
    st = _BatchState(ctypes.sizeof(_BatchState), 1, a, a, a, a, a, a, a, a, a, a, a, a, a, a)
    assert lib.onebit_decode_step_batched(ctypes.byref(m), ctypes.byref(st), None) == E_SHAPE      # batch 1
    assert b"batch" in lib.onebit_last_error()
    # ABI 8: a state built against another header (another size) is refused before any field is read
    st.struct_size = ctypes.sizeof(_BatchState) - 8
    assert lib.onebit_decode_step_batched(ctypes.byref(m), ctypes.byref(st), None) == E_ARG
    assert b"struct_size" in lib.onebit_last_error()
    from onebit_amd.engine import _State
    ds = _State()
    assert lib.onebit_decode_step(ctypes.byref(m), ctypes.byref(ds), None) == E_ARG                # struct_size 0
    assert b"struct_size" in lib.onebit_last_error()
    # the K-sharded decode step validates before any launch as well: null / foreign-size state, unknown segment, layer range
    from onebit_amd.engine import _KState
    assert lib.onebit_decode_step_ksharded(None, None, 0, 0, None) == E_ARG
    ks = _KState()
    assert lib.onebit_decode_step_ksharded(ctypes.byref(m), ctypes.byref(ks), 0, 0, None) == E_ARG and b"struct_size" in lib.onebit_last_error()
    ks.struct_size = ctypes.sizeof(_KState)
    m16 = _Model(1, 64, 128, 2, 2, 32, 16, 8, 1e-6, 1e-5, layers, a, a, a, a, a)
    assert lib.onebit_decode_step_ksharded(ctypes.byref(m16), ctypes.byref(ks), 0, 9, None) == E_FLAG      # unknown segment
    assert lib.onebit_decode_step_ksharded(ctypes.byref(m16), ctypes.byref(ks), 5, 0, None) == E_ARG       # layer outside the model
    assert lib.onebit_decode_step_ksharded(ctypes.byref(m16), ctypes.byref(ks), 0, 0, None) == E_ARG       # null buffers
    with pytest.raises(ValueError):
        _lib.check(E_SHAPE, "x")
    with pytest.raises(RuntimeError):
        _lib.check(1, "x")


def test_round6_entry_points_reject_bad_arguments_without_gpu():
    """ABI 9 (ragged rows, key-block decode attention, grouped projections, the mixed step): argument errors come back before any launch."""
    lib = _lib.load()
    E_ARG, E_SHAPE, E_ALIGN, E_WSPACE = -1, -2, -3, -5
    buf = ctypes.create_string_buffer(8192)
    a = (ctypes.addressof(buf) + 255) & ~255
    from onebit_amd.engine import _Layer, _MixedState, _Model, _Proj, _Seg
    # ragged rope: head_dim must be a power of two >= 16; cache rows beyond the rope tables; biases all or none; empty is fine
    rope = lambda **kw: lib.onebit_rows_qkv_rope_ragged(a, a, a, a, a, None, kw.get("pos", a), a, a, a, kw.get("bq", None), None, None, kw.get("T", 2), 2, 2,
                                                        kw.get("D", 64), 4, kw.get("max_len", 16), kw.get("max_pos", 16), 1e-5, None)
    assert rope(D=48) == E_SHAPE and rope(max_len=32) == E_SHAPE and rope(bq=a) == E_ARG and rope(pos=None) == E_ARG and rope(T=0) == 0
    # ragged attention: head_dim 64 / 128, segments inside the cache, no segments = nothing to do
    seg = (_Seg * 2)(_Seg(0, 5, 1, 3), _Seg(5, 4, 9, 0))
    att = lambda **kw: lib.onebit_attention_ragged(a, a, a, a, None, ctypes.cast(seg, ctypes.c_void_p), kw.get("n", 2), 4, kw.get("hkv", 4), kw.get("D", 64),
                                                   kw.get("slots", 4), 16, None)
    assert att(D=32) == E_SHAPE and att(hkv=3) == E_SHAPE and att(n=0) == 0
    assert att() == E_SHAPE and b"segment 1" in lib.onebit_last_error()             # slot 9 of 4
    # key-block decode attention: chunk a multiple of 64, scratch for more than one split
    assert lib.onebit_attention_decode_scratch_bytes(3, 8, 1) == 0
    assert lib.onebit_attention_decode_scratch_bytes(3, 8, 4) >= 3 * 8 * 4 * (128 + 2) * 4 + 3 * 8 * 4
    dec = lambda **kw: lib.onebit_attention_decode_rows(a, a, a, a, None, None, a, 2, 4, 4, kw.get("D", 64), 4, 16, kw.get("chunk", 64), kw.get("ns", 1),
                                                        None, 0, None) if True else None
    assert dec(chunk=96) == E_SHAPE and dec(D=12) == E_SHAPE and dec(ns=3) == E_WSPACE
    fus = lib.onebit_attention_decode_rows_fused(a, a, a, a, a, a, None, None, None, a, a, a, a, a, None, None, a, 2, 4, 4, 48, 4, 16, 16, 64, 1, 1e-5, None, 0, None)
    assert fus == E_SHAPE                                                          # head_dim 48: the rotate_half pairing needs a power of two
    # grouped projections: 1..3 projections, one projection beyond 64 rows goes through onebit_linear_forward
    pr = (_Proj * 3)()
    up = (ctypes.c_void_p * 3)(a, a, a)
    assert lib.onebit_linear_group_prescaled(ctypes.cast(pr, ctypes.c_void_p), up, up, 0, 8, None) == E_ARG
    assert lib.onebit_linear_group_prescaled(ctypes.cast(pr, ctypes.c_void_p), up, up, 1, 500, None) == E_SHAPE
    assert lib.onebit_linear_group_prescaled(ctypes.cast(pr, ctypes.c_void_p), up, up, 2, 0, None) == 0
    # the mixed step: struct size, head_dim, row accounting, workspace
    layers = (_Layer * 1)()
    m = _Model(1, 128, 352, 2, 2, 64, 96, 32, 1e-6, 1e-5, layers, a, a, a, a, a)
    assert lib.onebit_mixed_workspace_bytes(ctypes.byref(m), 0, 4, 0) == 0
    nb = lib.onebit_mixed_workspace_bytes(ctypes.byref(m), 100, 4, 0)
    assert nb > 100 * 128 * 2 * 10 and lib.onebit_mixed_workspace_bytes(ctypes.byref(m), 200, 4, 0) > nb
    st = _MixedState()
    assert lib.onebit_mixed_step(ctypes.byref(m), ctypes.byref(st), None) == E_ARG and b"struct_size" in lib.onebit_last_error()
    sg = (_Seg * 1)(_Seg(1, 5, 0, 0))
    st = _MixedState(ctypes.sizeof(_MixedState), 6, 1, 1, 1, 4, 0, 0, a, a, a, sg, a, a, None, a, a, a, 1 << 30)
    m48 = _Model(1, 96, 352, 2, 2, 48, 96, 32, 1e-6, 1e-5, layers, a, a, a, a, a)
    assert lib.onebit_mixed_step(ctypes.byref(m48), ctypes.byref(st), None) == E_SHAPE        # head_dim 48
    st.n_rows = 9
    assert lib.onebit_mixed_step(ctypes.byref(m), ctypes.byref(st), None) == E_SHAPE and b"n_rows" in lib.onebit_last_error()
    st.n_rows, st.workspace_bytes = 6, 1024
    assert lib.onebit_mixed_step(ctypes.byref(m), ctypes.byref(st), None) == E_WSPACE
    st.n_rows, st.n_dec, st.n_seg = 0, 0, 0
    assert lib.onebit_mixed_step(ctypes.byref(m), ctypes.byref(st), None) == 0                # an empty step


def test_module_contract_matches_reference():
    m = BitLinearInf(64, 48, bias=True, dtype=torch.float16)
    assert OneBitLinear is BitLinearInf
    assert (m.in_features, m.out_features, m.groups) == (64, 48, 1)
    sd = m.state_dict()
    assert list(sd) == ["weight", "weight_scale", "input_factor", "bias"]   # layernorm adds no keys
    assert sd["weight"].dtype == torch.int8 and sd["weight"].shape == (48, 8)
    assert sd["weight_scale"].shape == (48,) and sd["input_factor"].shape == (64,)
    assert all(not p.requires_grad for p in m.parameters())
    assert (m.weight == 0).all() and (m.weight_scale == 1).all() and (m.input_factor == 1).all()
    assert m.bias.abs().max() <= 1 / (8 ** 0.5)                 # fan_in is K // 8, as in the reference
    assert isinstance(m.layernorm, torch.nn.LayerNorm) and m.layernorm.eps == 1e-5
    assert not m.layernorm.elementwise_affine
    m2 = BitLinearInf(64, 48)
    assert m2.bias is None and m2.weight_scale.dtype == torch.float32
    assert list(m2.state_dict()) == ["weight", "weight_scale", "input_factor"]
    # .half() casts floating params only (int8 weight untouched), like from_pretrained(torch_dtype=fp16)
    m2.half()
    assert m2.weight.dtype == torch.int8 and m2.weight_scale.dtype == torch.float16
    # converter-style in-place data assignment keeps working
    m2.weight.data = torch.randint(-128, 127, (48, 8), dtype=torch.int8)
    m2.load_state_dict(m2.state_dict())


def test_cpu_tensors_fail_loudly():
    m = BitLinearInf(64, 48, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 64, dtype=torch.float16))
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 32, dtype=torch.float16))


# ------------------------------------------------------------------------------------------- the struct mirrors and their filling --
_MIRRORS = {"_Proj": "onebit_proj_t", "_Layer": "onebit_layer_t", "_Model": "onebit_model_t", "_State": "onebit_decode_state_t",
            "_BatchState": "onebit_batch_state_t", "_KState": "onebit_kshard_state_t", "_Seg": "onebit_seg_t",
            "_MixedState": "onebit_mixed_state_t", "_SpecState": "onebit_spec_state_t", "_FusedIn": "onebit_fused_in_t"}


def _header_structs():
    """typedef name -> [(base type, is pointer, array length or None, field name)] in declaration order."""
    src = open(os.path.join(ROOT, "include", "onebit.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    out = {}
    for body, name in re.findall(r"typedef\s+struct\s+\w+\s*\{(.*?)\}\s*(onebit_\w+_t)\s*;", src, flags=re.S):
        fields = []
        for decl in body.split(";"):
            decl = " ".join(decl.split())
            if not decl:
                continue
            base, rest = re.fullmatch(r"((?:const )*\w+)\s*(.*)", decl).groups()
            for d in rest.split(","):
                fname, arr = re.search(r"(\w+)\s*(?:\[(\d+)\])?$", d.strip()).groups()
                fields.append((base.replace("const ", ""), "*" in d, int(arr) if arr else None, fname))
        out[name] = fields
    return out


def test_struct_mirrors_match_the_header_field_by_field():
    """The library's struct_size check sees a mirror's total size only: two swapped pointers pass it.  Every mirror's _fields_ against
    the header's declarations, in order: the name, and the type class (any pointer, the integer width and sign, float, a nested
    onebit_proj_t, an array's length)."""
    from onebit_amd import _abi
    scalar = {"int32_t": ctypes.c_int32, "int": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
              "size_t": ctypes.c_size_t, "float": ctypes.c_float, "onebit_proj_t": _abi._Proj}
    is_ptr = lambda t: t is ctypes.c_void_p or issubclass(t, ctypes._Pointer)
    structs = _header_structs()
    assert len(_MIRRORS) == 10
    for mirror, typedef in _MIRRORS.items():
        got, want = getattr(_abi, mirror)._fields_, structs[typedef]
        assert [f[0] for f in got] == [w[3] for w in want], (mirror, typedef)
        for (fname, ftype), (base, ptr, arr, _) in zip(got, want):
            if arr is not None:
                assert issubclass(ftype, ctypes.Array) and ftype._length_ == arr, (mirror, fname)
                ftype = ftype._type_
            assert is_ptr(ftype) if ptr else ftype is scalar[base], (mirror, fname, base)
    # the parser itself: comma lists, pointers that bind to the declarator, an array of pointers
    assert structs["onebit_seg_t"] == [("int32_t", False, None, n) for n in ("row0", "n", "slot", "past")]
    assert structs["onebit_layer_t"][:2] == [("onebit_proj_t", False, None, "q"), ("onebit_proj_t", False, None, "k")]
    assert structs["onebit_layer_t"][9:11] == [("void", True, None, "k_cache"), ("void", True, None, "v_cache")]
    assert structs["onebit_fused_in_t"][-1] == ("float", True, 3, "st_out")


def test_make_state_fills_by_name_and_rejects_unknown_fields():
    from onebit_amd._abi import _Seg, _State, make_state
    t = torch.zeros(4)
    st = make_state(_State, dict(u_q=t, u_k=None), max_out=7)
    assert st.struct_size == ctypes.sizeof(_State) and st.u_q == t.data_ptr() and st.u_k is None and st.max_out == 7 and st.u_v is None
    with pytest.raises(AttributeError):
        make_state(_State, dict(u_qq=t))
    with pytest.raises(AttributeError):
        make_state(_State, attn_blnd=64)
    cp = make_state(st, dict(u_k=t), attn_blind=64)                 # a copy of an instance: the original is left alone
    assert cp.u_q == st.u_q and cp.u_k == t.data_ptr() and cp.attn_blind == 64 and cp.max_out == 7
    assert st.u_k is None and st.attn_blind == 0
    with pytest.raises(AttributeError):
        make_state(st, u_qq=1)
    sg = make_state(_Seg, row0=1, n=2, slot=3, past=4)              # no struct_size field: nothing invented
    assert (sg.row0, sg.n, sg.slot, sg.past) == (1, 2, 3, 4) and not hasattr(sg, "struct_size")


def test_step_variant_table():
    """Which form of onebit_decode_step serves a step, by the number of cached tokens (today's rule worked by hand)."""
    from onebit_amd.engine import step_variant
    kw = dict(long_from=160, short_ok=True, keyblock=True, kb_chunk=128, kb_top=4)
    want = {0: "64", 63: "64", 64: "short", 159: "short", 160: ("kb", 2), 255: ("kb", 2), 256: ("kb", 4), 511: ("kb", 4)}
    for steps, key in want.items():
        assert step_variant(steps, **kw) == key, steps
    assert step_variant(160, **dict(kw, keyblock=False)) == "long"
    assert step_variant(0, **dict(kw, long_from=1, short_ok=False)) == ("kb", 1)
    assert step_variant(400, **dict(kw, long_from=0)) == "short"


def test_library_functions_are_typed_once():
    """_lib.SYMBOLS is the only typing of the library's functions (an argtypes assignment elsewhere would change a process-global
    function object under every other caller).  Last in this file: the tests above have made their calls."""
    assign = re.compile(r"\.(argtypes|restype)\s*=")
    files = [os.path.join(d, f) for d in (os.path.join(ROOT, "onebit_amd"), os.path.join(ROOT, "tests"))
             for f in sorted(os.listdir(d)) if f.endswith(".py") and not (d.endswith("onebit_amd") and f == "_lib.py")]
    assert len(files) > 20
    for path in files:
        hits = [i + 1 for i, line in enumerate(open(path)) if assign.search(line)]
        assert not hits, (path, hits)
    lib = _lib.load()
    for name, (res, args) in _lib.SYMBOLS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
