"""CPU-only: every input of the guided matcher's GPU tests (tests/guided_match_inputs.py) really has the property it is there for, on the
model's output.  A generator that cannot produce its property is a bug in the generator."""
import numpy as np
import pytest

import guided_match_inputs as I
import guided_match_model as M


@pytest.mark.parametrize("dtype,dim", [("f32", 64), ("u8", 32), ("f32", 61), ("u8", 5)])
@pytest.mark.parametrize("size", I.GENERAL[:2], ids=lambda s: "x".join(map(str, s)))
def test_general_cases_hold_every_outcome(oracle, dtype, dim, size):
    pair = I.general_case(oracle, dtype, dim, *size)
    assert [x.shape[0] for x in pair[:3]] == [size[0], size[2], size[1]]
    for direction in (M.P2F, M.F2P):
        res = M.guided_pair(oracle, *pair, I.RADIUS, 0.8, M.RATIO, direction)
        assert M.outcomes(res, direction) == I.ALL_OUTCOMES, direction
    res = M.guided_pair(oracle, *pair, I.RADIUS, 0.8, M.RATIO, M.P2F)
    m, o = res["match"], res["owner"]
    lost = [c for c in range(m.size) if m[c] >= 0 and o[m[c]] != c]
    assert lost and all(o[m[c]] < c for c in lost)                        # the first-come rule drops corners, always in favour of a lower one
    cfr = pair[3]
    assert (np.diff(cfr) < 0).any() and np.unique(cfr).size == cfr.size < size[0]      # not monotone, a strict subset


def test_the_largest_general_case_crosses_1024(oracle):
    pair = I.general_case(oracle, "f32", 64, 1100, 1100, 1100)
    res = M.guided_pair(oracle, *pair, I.RADIUS, 0.8, M.RATIO, M.P2F)
    assert M.outcomes(res, M.P2F) == I.ALL_OUTCOMES
    assert (res["match"][1024:] >= 1024).any() and (res["match"][:1024] >= 1024).any() and (res["owner"][1024:] >= 0).any()


@pytest.mark.parametrize("dtype,dim", [("f32", 64), ("u8", 32)])
def test_window_cases_have_the_exact_counts(oracle, dtype, dim):
    """63, 64, 65, 128 and 129 candidates; among the wide windows the nearest candidate lies before the first drain in one, behind it in another"""
    for direction in (M.P2F, M.F2P):
        pair = I.window_case(oracle, dtype, dim, direction)
        res = M.guided_pair(oracle, *pair, I.RADIUS, 0.8, M.NEAREST, direction)
        assert res["count"].tolist() == [63, 64, 65, 128, 129] and (res["match"] >= 0).all()
        assert sorted(set(I.best_behind_first_drain(oracle, pair, direction))) == [False, True]


def test_the_grid_case_has_points_at_exactly_the_radius(oracle):
    pair = I.grid_pair("f32", 64, 1)
    d2 = M.window_d2(pair[2], pair[4])
    assert (d2 == np.float32(25.0)).sum() == 15                           # five per corner, at exactly the radius
    res = M.guided_pair(oracle, *pair, 5.0, 0.8, M.RATIO, M.P2F)
    assert res["count"].tolist() == [3, 3, 3]
    assert M.guided_pair(oracle, *pair, 5.0, 0.8, M.RATIO, M.F2P)["count"].tolist() == [0, 0, 0, 0, 0, 1, 1, 1] * 3


def test_the_no_fma_case_separates_the_two_arithmetics():
    pair = I.no_fma_case("f32", 64)
    assert I.fma_matters(pair) > 0
    r2 = np.float32(I.RADIUS) * np.float32(I.RADIUS)
    inside = M.window_d2(pair[2], pair[4]) < r2
    assert inside.sum() > 100 and (~inside).sum() > 100


@pytest.mark.parametrize("dtype,dim", [("f32", 64), ("u8", 32)])
def test_the_tie_cases_really_tie(oracle, dtype, dim):
    pair = I.tie_pair(dtype, dim, 2)
    for p, direction in ((pair, M.P2F), (I.swapped(pair), M.F2P)):
        ratio = M.guided_pair(oracle, *p, I.RADIUS, 1.0, M.RATIO, direction)
        positive, zero = I.ties(ratio)
        assert positive == 6 and zero == 6 and (ratio["match"] < 0).sum() >= 12
        near = M.guided_pair(oracle, *p, I.RADIUS, 1.0, M.NEAREST, direction)
        assert (near["match"] >= 0).sum() >= 12
        # the twins are two target rows: the lower one is reported
        t_desc = p[1] if direction == M.P2F else p[0][p[3]]
        for q in np.flatnonzero(near["count"] >= 2)[:12]:
            twin = [t for t in range(t_desc.shape[0]) if t != near["match"][q] and np.array_equal(t_desc[t], t_desc[near["match"][q]])]
            assert twin and min(twin) > near["match"][q]


def test_swapped_exchanges_the_roles(oracle):
    pair = I.general_case(oracle, "f32", 64, 33, 31, 65)
    a = M.guided_pair(oracle, *pair, I.RADIUS, 0.8, M.RATIO, M.P2F)
    b = M.guided_pair(oracle, *I.swapped(pair), I.RADIUS, 0.8, M.RATIO, M.F2P)
    for k in ("count", "match", "dist"):
        np.testing.assert_array_equal(a[k], b[k])


def test_one_row_case_and_nan_case(oracle):
    pair = I.one_row_pair("f32", 64, 4)
    res = M.guided_pair(oracle, *pair, I.RADIUS, 0.8, M.RATIO, M.P2F)
    assert (res["count"] == 1).all() and (res["match"] == 2).all() and res["owner"].tolist() == [-1, -1, 0]
    pair = I.nan_pair(oracle, "f32", 64)
    assert np.isnan(pair[2]).any(axis=1).sum() >= 40 and np.isnan(pair[4]).any(axis=1).sum() >= 60
    for direction in (M.P2F, M.F2P):
        res = M.guided_pair(oracle, *pair, I.RADIUS, 0.8, M.RATIO, direction)
        q_nan = np.isnan(pair[2] if direction == M.P2F else pair[4]).any(axis=1)
        t_nan = np.isnan(pair[4] if direction == M.P2F else pair[2]).any(axis=1)
        assert (res["count"][q_nan] == 0).all() and not np.isin(res["match"], np.flatnonzero(t_nan)).any()
        assert {"single", "accepted", "rejected"} <= M.outcomes(res, direction)


def test_tiny_pairs_hold_empty_sides_and_matches(oracle):
    pairs = I.many_tiny_pairs("f32", 64, 700, 77)
    assert pairs[3][2].shape[0] == 0 and pairs[5][1].shape[0] == 0 and sum(x.shape[0] for x in pairs[7][:3]) == 0
    exp = I.expected_batch(oracle, pairs, I.RADIUS, 0.8, M.RATIO, M.P2F)
    assert (exp["match"] >= 0).sum() > 100 and (exp["count"] >= 2).sum() > 100 and (exp["owner"] >= 0).sum() > 100
