"""The element-wise checker of the train-mode layer (tests/_train_ref.py) checked on its own, without a GPU: the restatement
passes its own bars when it sums in another order, and planted faults of the kind a tile kernel makes trip ``peak``.

What the planted faults show about the whole-tensor L2 bar of tests/test_gpu_train.py (2e-4 in fp32), measured on the float64 truth
of the (129, 130, 131) case:

    fault                                           relative L2      old bar sees it
    gW with the STE constant 1.000977 (fp16's 1.001)  2.5e-5           no    (asserted)
    one element of gW taken from its neighbour        2.5e-3           only when the element is wrong by more than 0.026 rms
    last column of gx zeroed                          1.4e-1           only when the column is wrong by more than 0.14 %
    one row of y shifted by one position              1.3e-1           only when the row is wrong by more than 0.16 %

A whole wrong element, column or row is too large for any relative L2 bar to miss (1 / sqrt(numel), 1 / sqrt(K), sqrt(2 / T)); what
the old bar cannot see is the same fault at a smaller amplitude -- an element, column or row that is off by a fraction of a percent,
which is what a dropped term of a 130-long sum or an fp16 rounding looks like.  So each localised fault is checked twice: as stated
(``peak`` trips), and scaled down until its L2 is half the old bar (the old bar passes it, ``peak`` still trips)."""
import pytest
import torch

import _train_ref as R

OLD_L2_BAR_FP32 = 2e-4          # tests/test_gpu_train.py::test_fp32_ragged_shapes_vs_restatement, gradients
FAULT_CASE = "129x130x131-bias"


@pytest.mark.parametrize("dtype_name", list(R.DTYPES))
@pytest.mark.parametrize("case_id", R.CASE_IDS)
def test_restatement_is_finite_and_a_reordered_sum_stays_inside_the_bars(case_id, dtype_name):
    dtype = R.DTYPES[dtype_name]
    case = R.get_case(case_id, dtype_name)
    own = R.reference(case, dtype)
    for n, v in own.items():
        assert v is None or bool(torch.isfinite(v).all()), n
    truth = R.reference(case, torch.float64)
    bar = R.bars(case, dtype)
    got = R.metrics(R.reference(case, dtype, split_k=True), truth, case)
    assert got.keys() == bar.keys()
    for k in bar:
        print(case_id, dtype_name, k, "reordered %.3e  bar %.3e" % (got[k], bar[k]))
        assert got[k] <= bar[k], (k, got[k], bar[k])


def test_case_table_reaches_what_it_says():
    T, K, N = zip(*R.SHAPES)
    assert 1 in T and any(t < 32 for t in T if t > 1) and 33 in T               # both sides of OB_TC_SLICES = 32
    assert any(k % 2 for k in K) and any(k % 8 == 0 and n % 8 == 0 for _, k, n in R.SHAPES)
    assert {33, 65, 257} <= set(K) | set(N) | set(T)                             # one past a 32-deep step in each role
    for cid in R.CASE_IDS:
        for dn in R.DTYPES:
            c = R.get_case(cid, dn)
            assert (c["weight"][0, :3] == 0).all() and (c["weight_scale"] < 0).any()
            for n in ("weight", "weight_scale", "input_factor", "x", "coef"):
                assert torch.equal(c[n].to(R.DTYPES[dn]).double(), c[n]), n       # representable: the kernels see the same numbers
            if cid.endswith("saturate"):
                assert int(R.saturated_mask(c).sum()) > 50
            if cid.endswith("zero_row"):
                assert float(c["x"][c["dims"][0] // 2].abs().max()) == 0


def _truth():
    case = R.get_case(FAULT_CASE, "float32")
    return case, R.reference(case, torch.float64)


def _fault_one_element(case, truth):
    g = truth["weight"].clone()
    g[64, 65] = truth["weight"][64, 66]
    return "weight", g


def _fault_last_column(case, truth):
    g = truth["gx"].clone()
    g[:, -1] = 0.0
    return "gx", g


def _fault_row_shift(case, truth):
    y = truth["y"].clone()
    y[77] = torch.roll(truth["y"][77], 1)
    return "y", y


def _fault_ste_constant(case, truth):
    # gW = gS * (1.001 - tanh(w)^2): the same gS with the constant an fp16 path would use
    w = case["weight"]
    t2 = torch.tanh(w) ** 2
    return "weight", truth["weight"] / (1.001 - t2) * (float(torch.tensor(1.001).half()) - t2)


LOCAL_FAULTS = {"one_element": _fault_one_element, "last_column": _fault_last_column, "row_shift": _fault_row_shift}


@pytest.mark.parametrize("fault", list(LOCAL_FAULTS))
def test_localised_fault_trips_peak_fp32(fault):
    case, truth = _truth()
    bar = R.bars(case, torch.float32)
    name, bad = LOCAL_FAULTS[fault](case, truth)
    p, e = R.peak(bad, truth[name]), R.l2(bad, truth[name])
    print(fault, name, "as stated: peak %.3e (bar %.3e)  l2 %.3e (bar %.3e, old bar %.1e)" % (p, bar[(name, "peak")], e, bar[(name, "l2")], OLD_L2_BAR_FP32))
    assert p > bar[(name, "peak")]
    # the same fault at the amplitude where the old whole-tensor bar stops seeing it
    small = truth[name] + (0.5 * OLD_L2_BAR_FP32 / e) * (bad - truth[name])
    p2, e2 = R.peak(small, truth[name]), R.l2(small, truth[name])
    print(fault, name, "scaled:    peak %.3e  l2 %.3e" % (p2, e2))
    assert e2 <= OLD_L2_BAR_FP32                # the old bar passes it
    assert p2 > bar[(name, "peak")]             # peak does not
    assert e2 > bar[(name, "l2")]               # (nor does L2 once its bar comes from the restatement's own error)


def test_fp16_ste_constant_on_the_fp32_path_trips_peak_and_passed_the_old_bar():
    case, truth = _truth()
    bar = R.bars(case, torch.float32)
    name, bad = _fault_ste_constant(case, truth)
    p, e = R.peak(bad, truth[name]), R.l2(bad, truth[name])
    print("ste constant: peak %.3e (bar %.3e)  l2 %.3e (bar %.3e, old bar %.1e)" % (p, bar[(name, "peak")], e, bar[(name, "l2")], OLD_L2_BAR_FP32))
    assert 2.0e-5 < e <= OLD_L2_BAR_FP32        # 2.3e-5 relative on every element: a tenth of the old bar
    assert p > bar[(name, "peak")]
    assert e > bar[(name, "l2")]


@pytest.mark.parametrize("fault", ["one_element", "last_column"])
def test_localised_fault_trips_peak_fp16(fault):
    case = R.get_case(FAULT_CASE, "float16")
    truth = R.reference(case, torch.float64)
    bar = R.bars(case, torch.float16)
    name, bad = LOCAL_FAULTS[fault](case, truth)
    p = R.peak(bad, truth[name])
    print(fault, name, "fp16: peak %.3e (bar %.3e)" % (p, bar[(name, "peak")]))
    assert p > bar[(name, "peak")]


def test_peak_on_sees_the_saturated_positions():
    """at |w| >= 4 the STE factor is <= 2.4e-3: an error of 10 % there is 1e-4 of the tensor's rms and invisible to the
    whole-tensor metrics' fp16 bars, peak_on restricts the rms to those positions"""
    case = R.get_case("129x130x131-saturate", "float32")
    truth = R.reference(case, torch.float64)
    bar = R.bars(case, torch.float32)
    mask = R.saturated_mask(case)
    bad = truth["weight"].clone()
    bad[mask] *= 1.1
    assert R.peak_on(bad, truth["weight"], mask) > bar[("weight", "peak_sat")]
    assert R.peak_on(truth["weight"], truth["weight"], mask) == 0.0
    assert R.rms(truth["weight"][mask]) < 0.02 * R.rms(truth["weight"])
