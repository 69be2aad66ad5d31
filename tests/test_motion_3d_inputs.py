"""Every input of tests/motion_3d_inputs.py has the property it exists for, shown with the NumPy model alone.  No GPU."""
import numpy as np
import pytest

import motion_3d_inputs as I
import motion_3d_model as M


def test_mixed_batch_has_the_sizes_duplicates_and_one_sided_ids():
    batch = I.mixed_batch()
    assert tuple(p["m"] for p in batch) == I.BATCH_SIZES
    for p in batch:
        ids, P, Q = M.correspondences(*I.frames(p))
        assert ids.tolist() == p["ids"].tolist() and len(ids) == p["m"]
        f, t = p["from_ids"].tolist(), p["to_ids"].tolist()
        assert any(f.count(i) == 2 and t.count(i) == 1 for i in set(f))             # twice in from, once in to
        assert any(t.count(i) == 2 and f.count(i) == 1 for i in set(t))             # once in from, twice in to
        assert len(set(f) - set(t)) >= 3 and len(set(t) - set(f)) >= 3              # ids of one side only
        assert p["from_ids"].shape[0] > p["m"] and (np.diff(p["from_ids"]) < 0).any()   # shuffled rows
    assert any((p["ids"] < 0).any() for p in batch)                                 # the rule has no sign test
    assert [m for m in I.BATCH_SIZES if m in (63, 64, 65, 255, 256, 257)] == [63, 64, 65, 255, 256, 257]   # around a wave and a workgroup


def test_the_batch_reaches_every_status_but_no_model():
    seen = set()
    for p in I.mixed_batch():
        seen.add(M.estimate(*I.frames(p), min_inliers=4, inlier_distance=0.1, iterations=300, refine_iterations=5, seed=1)["status"])
    assert {M.OK, M.FEW_CORRESPONDENCES} <= seen
    r = M.estimate(*I.frames(I.all_outlier_pair()), min_inliers=10, inlier_distance=0.1, iterations=300, refine_iterations=5, seed=1)
    assert r["counts"].max() < 10 and r["status"] in (M.BELOW_MIN_INLIERS, M.FEW_INLIERS)
    assert M.estimate(*I.frames(I.exact_pair(3)), min_inliers=3, iterations=1, refine_iterations=0, seed=I.seed_with_invalid_first(3, 1))["status"] == M.NO_MODEL


def test_exact_pair_ties_every_hypothesis():
    r = M.estimate(*I.frames(I.exact_pair(40)), min_inliers=3, inlier_distance=0.1, iterations=64, refine_iterations=0, seed=5)
    assert (r["counts"] == 40).all()
    np.testing.assert_array_equal(r["transform"], np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32))


def test_seed_with_invalid_first():
    for invalid in (1, 2):
        seed = I.seed_with_invalid_first(3, invalid)
        assert all(M.draw3(seed, h, 3) is None for h in range(invalid)) and M.draw3(seed, invalid, 3) is not None
        assert all(M.draw3(s, 0, 3) is not None for s in range(min(seed, 200)))      # it is the first such seed (checked up to 200)


def test_overflow_refit_pair():
    p = I.overflow_refit_pair()
    ids, P, Q = M.correspondences(*I.frames(p))
    assert len(ids) == p["m"] and np.isfinite(P).all() and np.isfinite(Q).all()
    assert np.isnan(M.fit_set(P, Q)).any()                                           # the fit of all of them overflows
    idx = np.array(M.draw3(1, 0, p["m"]))
    assert np.isfinite(M.fit3(P[idx][:, None], Q[idx][:, None])).all()               # a hypothesis does not
    r = M.estimate(*I.frames(p), min_inliers=3, inlier_distance=I.OVERFLOW_DISTANCE, iterations=20, refine_iterations=5, seed=1)
    assert (r["counts"] == p["m"]).all() and r["trace"] == ["empty"]


@pytest.mark.parametrize("name", sorted(I.REFINE_CASES))
def test_refine_cases_reach_their_branch(name):
    pair, kw = I.refine_case(name)
    assert I.REFINE_CASES[name][6] in M.estimate(*I.frames(pair), **kw)["trace"]


def test_fit_sets_are_well_conditioned():
    sets = I.fit_sets()
    assert len(sets) >= 20
    for P, Q in sets:
        assert len(P) >= 6 and np.sort(M.kabsch64(P, Q)[2])[1] / len(P) > I.SIGMA_FLOOR
    # what the floor is for: points on a line are refused
    line = np.outer(np.arange(8.0), [1.0, 2.0, 3.0]).astype(np.float32)
    assert not I.well_conditioned(line, line) and not I.well_conditioned(sets[0][0][:5], sets[0][1][:5])


def test_big_pair_is_beyond_the_staging():
    p = I.big_pair()
    assert p["from_ids"].shape[0] == 8192 and p["to_ids"].shape[0] == 8192
    assert len(M.correspondences(*I.frames(p))[0]) == 8000 > I.STAGE_CAP == 5248
    assert I.BATCH_SIZES[-1] < I.STAGE_CAP                                           # the mixed batch is on the staged path


# ---- the inputs of tests/test_gpu_motion_3d_shapes.py

def _estimate(pair, **kw):
    return M.estimate(*I.frames(pair), **kw)


def test_asymmetric_pairs_sort_two_lengths():
    pairs = I.asymmetric_pairs()
    sizes = [(p["from_ids"].shape[0], p["to_ids"].shape[0]) for p in pairs]
    assert tuple(sizes[:-1]) == I.ASYMMETRIC_SIZES and sizes[-1] == I.ASYMMETRIC_DISJOINT
    for (nf, nt), p in zip(sizes, pairs):
        assert I.sort_length(nf) != I.sort_length(nt)
        m = len(M.correspondences(*I.frames(p))[0])
        assert m == min(nf, nt, 60) or (nf, nt) == I.ASYMMETRIC_DISJOINT
        assert m >= 3 or min(nf, nt) < 3 or (nf, nt) == I.ASYMMETRIC_DISJOINT
    last = pairs[-1]
    assert not set(last["from_ids"].tolist()) & set(last["to_ids"].tolist()) and len(M.correspondences(*I.frames(last))[0]) == 0
    assert [I.sort_length(n) for n in (0, 1, 2, 3, 64, 65, 8192)] == [2, 2, 2, 4, 64, 128, 8192]


def test_duplicate_runs_straddle_the_blocks_and_take_no_part():
    pairs = I.duplicate_run_pairs()
    n = I.RUN_ROWS
    seen = {"from": set(), "to": set()}                                 # (boundary or end, length) per side, over all pairs
    for p in pairs:
        assert p["from_ids"].shape[0] == n and p["to_ids"].shape[0] == n
        matches = set(M.correspondences(*I.frames(p))[0].tolist())
        running = set()
        for side, other in (("from", "to"), ("to", "from")):
            runs = I.runs_of(p[side + "_ids"])
            ordered = np.sort(p[side + "_ids"])
            assert len(runs) == 4
            for start, length in runs.items():
                assert length in I.RUN_LENGTHS
                run_id = int(ordered[start])
                running.add(run_id)
                assert p[other + "_ids"].tolist().count(run_id) == 1   # once on the other side
                for b in I.RUN_BOUNDARIES:
                    if start <= b and b + 1 <= start + length - 1:      # covers the sorted positions b and b + 1
                        assert ordered[b] == ordered[b + 1] == run_id
                        seen[side].add((b, length))
                if start == 0:
                    seen[side].add(("first", length))
                if start + length == n:
                    seen[side].add(("last", length))
        assert len(running) == 8 and running == set(p["running"]) and not running & matches
        assert len(matches) == len(set(p["from_ids"].tolist())) - 8   # every other id is a correspondence
    want = {(b, l) for b in I.RUN_BOUNDARIES + ("first", "last") for l in I.RUN_LENGTHS}
    assert seen["from"] == want and seen["to"] == want                  # every length over every boundary and at both ends, on both sides


def test_extreme_ids():
    a, b, c = I.extreme_id_pairs()
    for p in (a, b, c):
        assert (p["from_ids"].shape[0], p["to_ids"].shape[0]) == I.EXTREME_ROWS
        assert all(n & (n - 1) for n in I.EXTREME_ROWS)                 # no power of two: padding keys follow the largest id
        assert set(I.EXTREME_IDS) <= set(p["from_ids"].tolist())
    m = M.correspondences(*I.frames(a))[0].tolist()
    assert m[0] == I.INT32_MIN and m[-1] == I.INT32_MAX and m == sorted(m) and {-1, 0, 1} <= set(m) and I.INT32_MIN + 1 not in m
    assert a["from_ids"].tolist().count(I.INT32_MAX) == 1 and a["to_ids"].tolist().count(I.INT32_MAX) == 1
    m = M.correspondences(*I.frames(b))[0].tolist()
    assert b["to_ids"].tolist().count(I.INT32_MAX) == 2 and b["from_ids"].tolist().count(I.INT32_MAX) == 1
    assert m[:2] == [I.INT32_MIN, I.INT32_MIN + 1] and I.INT32_MAX not in m and {-1, 0, 1} <= set(m)
    m = M.correspondences(*I.frames(c))[0].tolist()
    assert c["from_ids"].tolist().count(I.INT32_MAX) == 2 and c["to_ids"].tolist().count(I.INT32_MAX) == 1
    assert m[:2] == [I.INT32_MIN, I.INT32_MIN + 1] and I.INT32_MAX not in m and {-1, 0, 1} <= set(m)
    for p in (a, b, c):
        assert _estimate(p, min_inliers=3, inlier_distance=0.1, iterations=50, refine_iterations=2, seed=1)["status"] == M.OK


def test_predicate_pair_drops_every_third_by_one_cause():
    p = I.predicate_pair()
    n = I.PREDICATE_ROWS
    causes = I.predicate_causes()
    assert len(causes) == 22 and p["from_ids"].shape[0] == n and p["to_ids"].shape[0] == n
    assert sorted(p["from_ids"].tolist()) == sorted(p["to_ids"].tolist()) == p["ids"].tolist() and len(set(p["ids"].tolist())) == n
    ids = M.correspondences(*I.frames(p))[0]
    assert len(ids) == n - (n + 2) // 3 == 466 and ids.tolist() == p["ids"][~p["dropped"]].tolist()
    f_row = {int(i): p["from_xyz"][k] for k, i in enumerate(p["from_ids"])}
    t_row = {int(i): p["to_xyz"][k] for k, i in enumerate(p["to_ids"])}
    used = set()
    for k, i in enumerate(p["ids"].tolist()):
        x = np.concatenate([f_row[i], t_row[i]])
        bad = ~np.isfinite(x)
        zero = [not x[:3].any(), not x[3:].any()]
        if p["dropped"][k]:
            assert k % 3 == 0 and int(bad.sum()) + sum(zero) == 1       # exactly one cause
            side, v = causes[(k // 3) % 22]
            if isinstance(side, str):
                part = x[:3] if side == "from" else x[3:]
                assert zero[side == "to"] and (np.signbit(part) == np.signbit(np.float32(v))).all()
            else:
                assert bad[side] and (np.isnan(x[side]) if np.isnan(v) else x[side] == v)
            used.add((k // 3) % 22)
        else:
            assert not bad.any() and not any(zero)
            assert p["zeroed"][k] == (int((x == 0).sum()) == 1)         # a single zero coordinate drops nothing
    assert used == set(range(22)) and p["zeroed"].sum() > 50
    for lo in (0, 256, 512):                                            # dropped ones in each block of 256 of the sorted order
        assert p["dropped"][lo:lo + 256].any() and not p["dropped"][lo:lo + 256].all()


def test_stage_switch_pairs_stand_at_the_cap_and_one_above():
    at, above = I.stage_switch_pairs()
    for p in (at, above):
        assert (p["from_ids"].shape[0], p["to_ids"].shape[0]) == I.SWITCH_ROWS == (5400, 5300) and min(I.SWITCH_ROWS) > I.STAGE_CAP
    assert len(M.correspondences(*I.frames(at))[0]) == I.STAGE_CAP == 5248
    assert len(M.correspondences(*I.frames(above))[0]) == I.STAGE_CAP + 1
    assert (at["to_ids"] != above["to_ids"]).sum() == 1 and (at["from_ids"] == above["from_ids"]).all()     # the same rows but one id
    assert at["to_xyz"] is above["to_xyz"] and at["from_xyz"] is above["from_xyz"]
    r = _estimate(at, min_inliers=20, inlier_distance=0.1, iterations=32, refine_iterations=5, seed=8)
    assert r["status"] == M.OK and len(r["inliers"]) > 3000


def test_stride_pairs():
    small, five, large = I.stride_pairs()
    assert (small["from_ids"].shape[0], small["to_ids"].shape[0], len(M.correspondences(*I.frames(small))[0])) == (8192, 200, 150)
    assert (large["from_ids"].shape[0], large["to_ids"].shape[0], len(M.correspondences(*I.frames(large))[0])) == (8192, 5300, 5260)
    assert 5260 > I.STAGE_CAP > 150 and len(M.correspondences(*I.frames(five))[0]) == 5


def test_ties_across_chunks():
    assert I.TIE_ITERATIONS == (512, 513, 600, 65535) and 65535 % 256 == 255
    pair = I.exact_pair(40)
    r = _estimate(pair, min_inliers=3, inlier_distance=0.1, iterations=600, refine_iterations=0, seed=I.TIE_SEED)
    assert (r["counts"] == 40).all() and r["best"] == 0                 # every hypothesis of every chunk ties; the first valid one wins
    m, invalid, seed = I.TIE_INVALID_FIRST
    assert all(M.draw3(seed, h, m) is None for h in range(invalid)) and M.draw3(seed, invalid, m) is not None
    r = _estimate(I.exact_pair(m), min_inliers=3, inlier_distance=0.1, iterations=600, refine_iterations=0, seed=seed)
    valid = np.nonzero(r["counts"])[0]
    assert r["best"] == invalid == valid[0] and (r["counts"][valid] == m).all()
    for chunk in (0, 256):                                              # valid and invalid hypotheses in more than one chunk
        c = r["counts"][chunk:chunk + 256]
        assert (c == m).any() and (c == 0).any()


def test_the_late_winner_is_where_it_was_found():
    pair = I.late_winner_pair()
    assert len(M.correspondences(*I.frames(pair))[0]) == 40 and pair["planted"].sum() == 5
    w = I.LATE_POSITION
    assert I.find_late_winner(pair) == w
    counts = I.stream_counts(pair, w - I.LATE_GAP, I.LATE_GAP + 1)
    assert counts[-1] == 5 and counts[:-1].max() < 5


@pytest.mark.parametrize("h,iterations", I.LATE_CASES)
def test_late_winner_cases(h, iterations):
    r = _estimate(I.late_winner_pair(), **I.late_kw(h, iterations))
    assert r["best"] == h and r["counts"][h] == r["counts"].max() == 5 and (r["counts"][:h + 1] == 5).sum() == 1
    assert r["status"] == M.OK and len(r["inliers"]) == 5
    assert (h % 256, iterations) in ((255, 600), (0, 600), (87, 600), (0, 257))


@pytest.mark.parametrize("h", I.CUT_OFF)
def test_a_winner_beyond_the_iterations_is_cut_off(h):
    pair = I.late_winner_pair()
    whole = _estimate(pair, **I.late_kw(h, h + 1))
    cut = _estimate(pair, **I.late_kw(h, h))
    assert whole["best"] == h and whole["counts"][h] == 5
    assert cut["best"] != h and 0 < cut["counts"].max() < 5 and cut["best"] == int(np.argmax(cut["counts"]))
    assert (I.bits(cut["transform"]) != I.bits(whole["transform"])).any()


@pytest.mark.parametrize("seed", sorted(I.LATE_MEMBERS))
def test_members_change_behind_the_first_256(seed):
    r = _estimate(I.late_members_pair(seed), seed=seed, **I.LATE_MEMBERS_KW)
    assert "members_changed" in r["trace"] and r["first_differing"] == [I.LATE_MEMBERS[seed]] and I.LATE_MEMBERS[seed] >= 256
    assert len(r["inliers"]) > 256


def test_the_search_for_late_members():
    lo = min(I.LATE_MEMBERS)
    assert I.find_late_members(range(lo - 10, lo + 1)) == [(lo, [I.LATE_MEMBERS[lo]])]
    assert I.find_late_members(range(4, 5)) == []                       # members_changed at an index below 256 does not qualify
    r = _estimate(I.late_members_pair(4), seed=4, **I.LATE_MEMBERS_KW)
    assert r["first_differing"] and min(r["first_differing"]) < 256


def test_radix_select_cases():
    cases = I.select_cases()
    last = {}
    for name, (pair, kw) in cases.items():
        r = _estimate(pair, **kw)
        assert kw["refine_iterations"] == 0 and r["status"] == M.OK
        last[name] = np.sort(I.bits(r["last_d2"]))
        assert len(last[name]) == len(r["inliers"])
        assert r["variance"] == M.VARIANCE_FACTOR * np.float64(last[name][len(last[name]) >> 1:][:1].view(np.float32)[0])
    for name, n in I.SELECT_SIZES.items():                              # (a), (b)
        assert len(last[name]) == n
    assert len(last["all_zero"]) == 300 and not last["all_zero"].any()  # (c)
    d = last["majority_is_median"]                                      # (d)
    median = d[len(d) >> 1]
    assert median == I.bits(np.float32(0.0625))[0] and 2 * int((d == median).sum()) > len(d) and len(set(d.tolist())) == 3
    d = last["even_middle_differs"]                                     # (e)
    assert len(d) % 2 == 0 and d[(len(d) - 1) >> 1] != d[len(d) >> 1]
    d = last["low_byte"]                                                # (f)
    n = len(d)
    mid = d[n // 2 - 1:n // 2 + 2]
    assert n == 40 and len(set((mid >> 8).tolist())) == 1 and len(set((mid & 255).tolist())) == 3
    assert int((d >> 8 == mid[0] >> 8).sum()) == 4 + 3 + 4             # and more of that prefix on either side of them


def test_scratch_table_pair():
    pair = I.scratch_table_pair()
    refined, plain = I.scratch_table_kws()
    assert len(M.correspondences(*I.frames(pair))[0]) == 420 + I.SCRATCH_TABLE_EXACT > I.STAGE_CAP
    r = _estimate(pair, **refined)
    assert refined == dict(I.LATE_MEMBERS_KW, seed=I.SCRATCH_TABLE_SEED) and r["status"] == M.OK
    assert len(r["trace"]) >= 3 and "size_changed" in r["trace"] and r["trace"][-1] == "converged"      # several passes, the last compares the members
    assert len(r["inliers"]) > I.STAGE_CAP - 420
    r = _estimate(pair, **plain)
    d = np.sort(I.bits(r["last_d2"]))
    assert plain["refine_iterations"] == 0 and len(d) > I.STAGE_CAP and len(d) % 2 == 0 and d[(len(d) - 1) >> 1] != d[len(d) >> 1]


def test_wrapper_pairs_have_three_outcomes():
    kw = dict(I.WRAPPER_KW)
    kw["inlier_distance"] = kw.pop("inliers_distance")
    rs = [_estimate(p, **kw) for p in I.wrapper_pairs()]
    assert [r["status"] for r in rs] == [M.FEW_CORRESPONDENCES, M.BELOW_MIN_INLIERS, M.OK, M.OK]
    assert len(rs[1]["matches"]) >= kw["min_inliers"] > len(rs[1]["inliers"]) >= 3
    assert I.runs_of(I.wrapper_pairs()[3]["from_ids"]) and I.runs_of(I.wrapper_pairs()[3]["to_ids"])
