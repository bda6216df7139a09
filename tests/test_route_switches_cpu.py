"""The switch table (tests/route_switches.py) against the sources and DESIGN.md section 6a: every OB_* environment variable the
native library reads has a tested row (or an entry naming the test that covers it) and a line in section 6a, and neither names a
variable the library does not read.  A switch added without a test fails here."""
import os
import re

from route_switches import COVERED_ELSEWHERE, ROWS, row_id, variables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "onebit_amd", "csrc")
WORKLOADS = {"linear", "gemv", "decode", "batched", "mixed", "train"}


def _source_switches():
    names = set()
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".h")):
            with open(os.path.join(CSRC, f)) as fh:
                names |= set(re.findall(r'getenv\(\s*"(OB_[A-Z0-9_]+)"', fh.read()))
    return names


def _design_switches():
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        text = f.read()
    m = re.search(r"^## 6a\..*?(?=^## )", text, re.S | re.M)
    assert m, "DESIGN.md has no section 6a"
    return set(re.findall(r"`(OB_[A-Z0-9_]+)", m.group(0))), m.group(0)


def test_sources_read_switches():
    assert len(_source_switches()) >= 30


def test_every_source_switch_has_a_row():
    missing = _source_switches() - set(variables())
    assert not missing, f"switches read by the library without a row in tests/route_switches.py: {sorted(missing)}"


def test_every_row_names_a_switch_the_library_reads():
    stale = set(variables()) - _source_switches()
    assert not stale, f"rows for switches the library no longer reads: {sorted(stale)}"


def test_design_6a_lists_exactly_the_source_switches():
    design, _ = _design_switches()
    src = _source_switches()
    assert src - design == set(), f"missing from DESIGN.md 6a: {sorted(src - design)}"
    assert design - src == set(), f"DESIGN.md 6a names switches the library does not read: {sorted(design - src)}"


def test_design_6a_names_the_test():
    _, sec = _design_switches()
    assert "test_gpu_route_switches.py" in sec and "route_switches.py" in sec


def test_rows_are_well_formed():
    ids = [row_id(r) for r in ROWS]
    assert len(ids) == len(set(ids)), "duplicate rows"
    for r in ROWS:
        assert r["env"] and r["workloads"] and r["why"], row_id(r)
        assert r["relation"] in ("bits", "oracle"), row_id(r)
        assert set(r["workloads"]) <= WORKLOADS and set(r["acts_on"]) <= set(r["workloads"]), row_id(r)
        assert any(r["base"].get(k) != v for k, v in r["env"].items()), row_id(r)          # a row differs from its base
        if not r["acts_on"]:                      # a switch expected to change nothing can only be held bit for bit
            assert r["relation"] == "bits", row_id(r)
    for v in COVERED_ELSEWHERE:
        assert "::" in COVERED_ELSEWHERE[v], v


def test_table_has_the_required_values():
    have = {(k, v) for r in ROWS for k, v in r["env"].items()}
    for rnt in ("1", "2", "3", "4", "6", "8"):
        assert ("OB_SK3_RNT", rnt) in have
    for kv in [("OB_BATCH_CHAINS", "2"), ("OB_ATTN_BLIND", "64"), ("OB_ATTN_BLIND", "128"), ("OB_GEMM3_KSPLIT", "0"),
               ("OB_GEMM3_KSPLIT", "2"), ("OB_GEMM3_KSPLIT", "3"), ("OB_SKINNY3", "0"), ("OB_BATCH_SPLITK", "0"),
               ("OB_SK3_OSPLIT", "0"), ("OB_SK3_PREFETCH", "0"), ("OB_FDEC_FUSED", "0"), ("OB_ATTN_THREADS", "512"),
               ("OB_BATCH_ATTN_THREADS", "512"), ("OB_DECODE_MATH", "f16"), ("OB_DEC_WGP", "0"), ("OB_DEC_I8_SINGLE", "0"),
               ("OB_GEMM3_WT", "2"), ("OB_GEMM3_GROUPED", "0"), ("OB_LN_ROWS", "0"), ("OB_SKINNY", "0"), ("OB_DEC_PREFETCH_O", "0")]:
        assert kv in have, kv
    # thresholds: at least two values each
    for v in ("OB_GEMM3_GROUP_DEN", "OB_GEMM3_KSPLIT_TILES", "OB_GEMM3_KSPLIT_TMIN", "OB_MIXED_SK_ROWS", "OB_MIXED_TAIL"):
        assert len({val for k, val in have if k == v}) >= 2, v
    # the switch that only acts within another route is tested inside it
    assert any(r["env"].get("OB_BATCH_SPLITK") == "0" and r["env"].get("OB_SKINNY3", r["base"].get("OB_SKINNY3")) == "0" for r in ROWS)
    for v in ("OB_ABLATE", "OB_TIMING"):
        assert all(r["relation"] == "bits" and not r["acts_on"] for r in ROWS if v in r["env"]), v
