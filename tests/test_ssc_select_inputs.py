"""What the generators of tests/ssc_select_inputs.py are named for, proved on the model without a GPU.  Every call of the model here runs
the reference's mask form and the pairwise form side by side and asserts that they select the same features."""
import numpy as np
import pytest

import ssc_select_inputs as I
import ssc_select_model as M


def _trace(name):
    f, mx = I.named(name)
    tr = {}
    kept = M.select_frame(f["response"], mx, M.BY_RESPONSE, f["image_size"], f["points"], trace=tr)
    assert len(f["response"]) > mx >= 2
    return f, mx, kept, tr


def test_exit_found():
    _f, mx, kept, tr = _trace("found")
    assert tr["exit"] == "found" and tr["kmin"] <= len(kept) <= tr["kmax"] <= mx and len(tr["widths"]) >= 4


def test_exit_with_too_few():
    _f, _mx, kept, tr = _trace("few")
    assert tr["exit"] == "few" and 0 < len(kept) < tr["kmin"] and len(tr["widths"]) >= 3
    assert tr["sizes"][-1] == len(kept)                                    # the LAST evaluated width's selection, not the best one
    assert max(tr["sizes"]) > tr["kmax"]                                   # the search has seen both sides


def test_exit_with_too_many_and_more_than_max_features():
    _f, mx, kept, tr = _trace("many_above_max")
    assert tr["exit"] == "many" and len(kept) > mx > tr["kmax"]


def test_exit_before_the_first_iteration():
    _f, _mx, kept, tr = _trace("empty")
    assert tr["exit"] == "empty" and kept == [] and tr["widths"] == [] and tr["low"] > tr["high"]


def test_a_search_that_reaches_width_1():
    _f, _mx, kept, tr = _trace("width_1")
    assert tr["widths"][-1] == 1 and len(tr["widths"]) >= 5 and len(kept) > 0


def test_all_features_in_one_pixel():
    f, _mx, kept, tr = _trace("one_pixel")
    assert len(kept) == 1 and tr["sizes"] == [1] * len(tr["widths"]) and len(tr["widths"]) >= 2
    assert kept[0] == M.order_of(f["response"])[0]


def test_ties_negative_responses_and_both_zeros():
    f, _mx, kept, _tr = _trace("ties")
    r = f["response"]
    bits = r.view(np.uint32)
    assert (bits == 0x80000000).any() and (bits == 0).any() and (r < 0).any() and len(set(r.tolist())) < 12
    order = M.order_of(r)
    zeros = [i for i in order if r[i] == 0.0]
    assert zeros == sorted(zeros) and {int(bits[i]) for i in zeros} == {0, 0x80000000}       # -0.0 and +0.0 are one value, ordered by index
    assert order.index(int(np.argmax(r))) == 0 and r[order[-1]] == r.min()                   # signed: the most negative response comes last
    assert kept == [i for i in order if i in set(kept)]


def test_points_on_all_four_borders():
    f, _mx, _kept, _tr = _trace("borders")
    cols, rows = f["image_size"]
    x, y = f["points"][:, 0], f["points"][:, 1]
    assert (x == 0).any() and (x == cols).any() and (y == 0).any() and (y == rows).any()
    assert ((x == cols) & (y == rows)).any() and (np.signbit(x) & (x == 0)).any()
    for width in (1, 2, 3, 7):                                             # x == cols and y == rows lie in the mask's last row and column
        c = width / 2.0
        assert M.cell_of((cols, rows), c) == (int(rows // c), int(cols // c))


@pytest.mark.parametrize("name", [n[0] for n in I.NAMED])
def test_both_orders_hold_the_same_features(name):
    f, mx = I.named(name)
    by_response = M.select_frame(f["response"], mx, M.BY_RESPONSE, f["image_size"], f["points"])
    keep_order = M.select_frame(f["response"], mx, M.KEEP_ORDER, f["image_size"], f["points"])
    assert keep_order == sorted(by_response) and len(set(by_response)) == len(by_response)
    assert M.select_frame(f["response"], mx, M.BY_RESPONSE, f["image_size"], f["points"], device=True) == by_response


def test_random_frames_reach_the_first_four_exits():
    """ordinary random frames of 3 to 400 features on the five image sizes: the exits occur, and the two forms agree on each of them"""
    seen = set()
    for seed in range(1, 40):
        rng = np.random.default_rng(seed)
        size = I.SIZES[seed % len(I.SIZES)]
        n = int(rng.integers(3, 400))
        mx = int(rng.integers(2, n))
        gen = (I.uniform_frame, I.integer_frame, I.clustered_frame)[seed % 3]
        f = gen(rng, n, size)
        tr = {}
        kept = M.select_frame(f["response"], mx, M.BY_RESPONSE, f["image_size"], f["points"], trace=tr)
        seen.add(tr["exit"] + ("_above" if len(kept) > mx else ""))
    assert {"found", "few", "empty", "many_above"} <= seen, seen
