"""CPU-only: every generator of tests/feature_select_inputs.py has, on the model, the property it is there for."""
import numpy as np
import pytest

import feature_select_inputs as I
import feature_select_model as M


def test_tied_frames_tie_across_signs_zeros_and_denormals():
    rng = np.random.default_rng(1)
    r = I.tied_frame(rng, 1000)["response"]
    mags = np.abs(r)
    assert len(set(mags.tolist())) <= 8 and (r < 0).any() and (r > 0).any()
    assert (np.signbit(r) & (r == 0)).any() and (~np.signbit(r) & (r == 0)).any()          # both zeros
    assert ((mags > 0) & (mags < np.finfo(np.float32).tiny)).any()                          # denormals
    # the order among equal magnitudes is the index alone: the selection differs from a sort that lets the lower index win
    kept = M.select_frame(r, 500, M.BY_RESPONSE)
    stable = sorted(range(1000), key=lambda i: (-abs(float(r[i])), i))[:500]
    assert kept != stable and sorted(abs(float(r[i])) for i in kept) == sorted(abs(float(r[i])) for i in stable)


@pytest.mark.parametrize("n,mx", [(300, 100), (1000, 500), (65, 64), (5000, 1000)])
def test_the_cut_falls_inside_a_group_of_equal_responses(n, mx):
    r = I.cut_in_tie_frame(np.random.default_rng(n), n, mx)["response"]
    full = M.strongest_first(r, list(range(n)))
    assert M.select_frame(r, mx, M.BY_RESPONSE) == full[:mx] and M.select_frame(r, mx, M.KEEP_ORDER) == sorted(full[:mx])
    assert abs(r[full[mx - 1]]) == abs(r[full[mx]])                                         # the last kept and the first dropped are equal
    assert full[mx - 1] > full[mx]                                                          # ... and the higher index is the one kept
    group = [i for i in range(n) if abs(r[i]) == abs(r[full[mx]])]
    assert (r[group] < 0).any() and (r[group] > 0).any() or len(group) < 4                  # both signs in the group (unless it is tiny)


@pytest.mark.parametrize("grid,size", I.GRIDS)
@pytest.mark.parametrize("mx", [16, 50, 200, 500])
def test_every_cell_state_occurs(grid, size, mx):
    rng = np.random.default_rng(mx)
    n = 1000
    f = I.grid_frame(rng, n, size, grid, mx)
    per_cell = mx // (grid[0] * grid[1])
    want = {"empty", "at", "over"} | ({"under"} if per_cell >= 2 else set())
    assert I.cell_states(f, grid, mx) == want
    kept = M.select_frame(f["response"], mx, M.KEEP_ORDER, grid, size, f["points"])        # nothing outside: the host rule applies
    assert kept == sorted(kept) and 0 < len(kept) < n
    g = I.grid_frame(rng, n, size, grid, mx, outside=8)
    assert "outside" in I.cell_states(g, grid, mx)
    with pytest.raises(M.Refused):
        M.select_frame(g["response"], mx, M.KEEP_ORDER, grid, size, g["points"])
    kept = M.select_frame(g["response"], mx, M.KEEP_ORDER, grid, size, g["points"], device=True)
    assert all(M.cell_of(g["points"][i], size, grid) is not None for i in kept)
    # points on a cell's first pixel and in its last fraction both occur
    frac = f["points"][:, 0] / (size[0] // grid[1])
    assert (frac == np.floor(frac)).any() and (frac - np.floor(frac) > 0.99).any()


def test_a_grid_can_select_more_or_fewer_than_max_features():
    rng = np.random.default_rng(3)
    f = I.grid_frame(rng, 1000, (640, 480), (4, 4), 500)
    assert len(M.select_frame(f["response"], 500, M.KEEP_ORDER, (4, 4), (640, 480), f["points"])) < 500      # an empty cell's share is lost
    assert len(M.select_frame(f["response"], 15, M.KEEP_ORDER, (4, 4), (640, 480), f["points"])) == 1000     # perCell == 0 keeps everything


@pytest.mark.parametrize("n", [1, 64, 500, 2049])
def test_expansion_inputs_hold_all_three_id_kinds(n):
    rng = np.random.default_rng(n)
    e = I.expansion_frame(rng, n, count=None if n > 1 else 1)
    assert len(set(e["index"].tolist())) == e["count"] and ((e["index"] >= 0) & (e["index"] < n)).all()
    if n >= 64:
        w = e["word_ids"]
        assert (w > 0).any() and (w < 0).any() and (w == 0).any()
        assert e["index"].tolist() != sorted(e["index"].tolist())
        with_first = M.expand_frame(n, e["index"], w, 9000)
        without = M.expand_frame(n, e["index"], w, 0)
        assert (with_first >= 9000).sum() == (w < 0).sum() and (without > 0).sum() == (w > 0).sum()
        assert (without < 0).sum() == n - (w > 0).sum() and sorted(-without[without < 0]) == list(range(1, n - int((w > 0).sum()) + 1))


def test_concat_and_batch_model():
    rng = np.random.default_rng(9)
    frames = [I.tied_frame(rng, n) for n in (0, 5, 0, 70)]
    resp, pts, off, size = I.concat(frames)
    assert off.tolist() == [0, 0, 5, 5, 75] and pts is None and size is None and resp.shape == (75,)
    count, index = M.select_batch(frames, 64)
    assert count.tolist() == [0, 5, 0, 64] and index[:5].tolist() == [0, 1, 2, 3, 4] and (index[5 + 64:] == -1).all()
