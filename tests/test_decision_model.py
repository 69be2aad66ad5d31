"""tests/decision_model.py against the oracle's restatement of Rtabmap::adjustLikelihood (oracle/lcd_oracle.cpp), without a GPU.

Tolerance: the reference adds the n values into a float one by one (uMean / uVariance, UMath.h:419-432, 512-526): its mean and its
standard deviation carry up to n * 2^-24 relative ((n - 1) roundings of the sum; three more for the deviation's square, quotient and root), as tests/bayes_checks.py argues for the posterior's sum.  That error is handed to the
model as (mean_tol, std_tol) and the model propagates it to every entry -- the same propagation the GPU tests use with the device's
bounds.  Entries whose selection `value > mean + stddev` that error leaves open are not compared."""
import numpy as np
import pytest

import oracle as O
from decision_inputs import exact_vector, launch_plan, near_cancel_vector, sparse_vector, stat_vector, statistics
from decision_model import Statistics, adjusted_value, chain_depth, f32


def _against_oracle(L, ratio):
    n = L.shape[0]
    st = statistics(L)
    rel = (n - 1) * 2.0 ** -24                       # a float sum of n values rounds n - 1 times; + the roundings of (v - mean)^2, / and sqrt
    a = st.adjust(ratio, mean_tol=rel * float(st.mean), std_tol=(rel + 3 * 2.0 ** -24) * float(st.stddev))
    exp = O.adjust_likelihood(np.concatenate([[0.0], L]).astype(np.float32), ratio)
    ok = a.decided
    err = np.abs(exp.astype(np.float64) - a.vector.astype(np.float64))
    assert (err[ok] <= a.tol[ok]).all(), (n, ratio, float((err[ok] - a.tol[ok]).max()))
    return a, exp, ok


@pytest.mark.parametrize("ratio", [0.0, 0.5])
@pytest.mark.parametrize("n", [1, 2, 3, 10, 257, 5000])
def test_statement_by_statement_against_the_oracle(n, ratio):
    for seed in range(3):
        L = stat_vector(n, max_at=(seed * 7) % n, seed=seed)
        a, exp, ok = _against_oracle(L, ratio)
        assert n < 257 or ok.mean() > 0.98                              # the comparison is not empty
        # what the float accumulation cannot move: entries that are not selected are exactly 1, zeros included
        assert (exp[1:][ok[1:] & ~a.selected] == 1.0).all() and (a.vector[1:][~a.selected] == 1.0).all()


@pytest.mark.parametrize("ratio", [0.0, 0.5])
def test_exact_sums_are_bit_equal_to_the_oracle(ratio):
    """Small integers: the reference's float sums are exact too, so both evaluations are the same IEEE operations."""
    for n in (3, 255, 5000):
        L, c = exact_vector(n)
        st = statistics(L)
        assert st.exact_sums and st.mean == 8 and st.stddev == 4 and st.mean_tol == 0 and st.std_tol == 0
        a = st.adjust(ratio)
        assert a.decided.all() and not a.selected.any()
        np.testing.assert_array_equal(a.vector, O.adjust_likelihood(np.concatenate([[0.0], L]).astype(np.float32), ratio))
        assert a.vector[0] == (3.0 if ratio == 0 else 2.0)


@pytest.mark.parametrize("ratio", [0.0, 0.5])
def test_sparse_vectors_against_the_oracle(ratio):
    for n in (1, 2, 300, 5000):
        for kind in ("one", "two", "none", "last_partial"):
            L = sparse_vector(n, kind)
            a = statistics(L).adjust(ratio)
            exp = O.adjust_likelihood(np.concatenate([[0.0], L]).astype(np.float32), ratio)
            if kind != "last_partial":                                 # at most two equal values: nothing to round
                assert a.decided.all()
                np.testing.assert_array_equal(a.vector, exp)
            else:
                _against_oracle(L, ratio)
    assert statistics(sparse_vector(9, "none")).adjust(ratio).vector.tolist() == [2.0] + [1.0] * 9


def test_the_best_candidate_and_the_tie_rule():
    L = np.array([0, 0.5, 0.25, 0.5, 0, 0.5, 0.1], np.float32)
    st = Statistics(L)
    assert st.best_slot == 5 and st.maxv == f32(0.5) and st.n_positive == 5            # of equal likelihoods the higher slot
    cons = np.array([1, 1, 1, 1, 1, 0, 1], bool)
    st = Statistics(L, cons)
    assert st.best_slot == 3 and st.n_positive == 4
    a = st.adjust(0.0)
    assert a.vector[1 + 5] == 0.0 and a.slot == 3 and a.likelihood == f32(0.5) and a.adjusted == a.vector[4]
    none = Statistics(np.zeros(4, np.float32)).adjust(0.0)
    assert none.slot == -1 and none.likelihood == 0 and none.adjusted == 0 and none.n_positive == 0


def test_bounds_are_functions_of_the_input():
    """More trips and the PER branch lengthen the chain; exact sums have no error; cancellation widens the bound on stddev."""
    assert chain_depth(1, 0, 16) == 1 + 6 + 3 + 0 + 6 + 15 and chain_depth(3, 4, 4) == 3 + 6 + 3 + 4 + 6 + 3
    assert launch_plan(600000)["chain"] > launch_plan(262144)["chain"] >= launch_plan(257)["chain"]
    a = statistics(stat_vector(5000, 17))
    b = statistics(near_cancel_vector(5000))
    assert 0 < a.std_tol / float(a.stddev) < b.std_tol / float(b.stddev) < 1e-3
    assert a.var_tol > 0 and statistics(exact_vector(5000)[0]).var_tol == 0
    # a float mean other than the model's own (the device's may be the neighbouring float): the variance is taken around it
    up = np.nextafter(a.own_mean, f32(1))
    c = statistics(a.L, mean=up)
    assert c.mean == up and c.var != a.var and abs(c.var - a.var) < 1e-6 * a.var


def test_decidedness():
    """An entry is decided when `value > mean + stddev` holds, or fails, for every (mean, stddev) inside the bounds."""
    L = stat_vector(5000, 11)
    st = statistics(L)
    assert st.adjust(0.0, mean_tol=0.0, std_tol=0.0).decided.all()
    mt = 1e-2 * float(st.mean)
    a = st.adjust(0.0, mean_tol=mt, std_tol=0.0)
    lo, hi = f32(f32(float(st.mean) - mt) + st.stddev), f32(f32(float(st.mean) + mt) + st.stddev)
    band = (L > lo) & (L <= hi)
    assert band.sum() > 5 and np.array_equal(~a.decided[1:], band)
    sel, out = adjusted_value(np.array([12, 4, 8, 0], np.float32), f32(8), f32(4), 0.0)
    assert not sel.any() and (out == 1).all()                          # EQUAL to the threshold is not above it
