"""GPU tests of lcd_estimate_motion_3d and lcd_estimate_motion_3d_dev (rtabmap_amd/csrc/motion_3d.hip) where the kernel's own parts change
shape: the join (two sorts of different lengths, runs of duplicates over the block boundaries, the extreme ids beside the padding keys, the
predicate inside the compaction), the switch between coordinates in LDS and in the scratch, the hypothesis chunks (ties and a unique winner
across them, a winner beyond the iterations), the comparison of two index sets behind the first 256, the radix select, and the C++ wrapper.
The reference is tests/motion_3d_model.py; every comparison is exact, as in tests/test_gpu_motion_3d.py, whose helpers these tests use.
tests/test_motion_3d_inputs.py proves without a GPU that each input has the property it is here for."""
import numpy as np
import pytest

import motion_3d_inputs as I
import motion_3d_model as M
from test_gpu_motion_3d import check_both, model_of

pytestmark = pytest.mark.gpu

JOIN_KW = dict(min_inliers=3, inlier_distance=0.1, iterations=50, refine_iterations=2, seed=1)
SWITCH_KW = dict(min_inliers=20, inlier_distance=0.1, iterations=32, refine_iterations=5, seed=8)
_inputs = {}


def inputs(name, *args):
    """a generator's result, built once for the module (the model's results are cached per pair object)"""
    if (name,) + args not in _inputs:
        _inputs[(name,) + args] = getattr(I, name)(*args)
    return _inputs[(name,) + args]


@pytest.fixture(scope="module")
def eng():
    import rtabmap_amd
    e = rtabmap_amd.Engine("f32", 64)
    yield e
    assert e.vocab_count() == (0, 0) and e.sig_count() == (0, 0)
    e.close()


def test_the_join_in_one_batch(eng):
    """cases 1-4 in ONE call: sides of 0 .. 8192 rows against 0 .. 8192, runs of 2, 3 and 5 equal ids over the sorted positions 63/64, 255/256,
    511/512 and at both ends, INT32_MIN .. INT32_MAX (unique and doubled) in frames of 13 x 70 rows, and every cause of the predicate"""
    asym, runs, extreme, pred = inputs("asymmetric_pairs"), inputs("duplicate_run_pairs"), inputs("extreme_id_pairs"), inputs("predicate_pair")
    pairs = asym + runs + extreme + [pred]
    want = check_both(eng, pairs, "join", **JOIN_KW)
    n = want["n_matches"].tolist()
    assert n[:len(asym)] == [min(nf, nt, 60) for nf, nt in I.ASYMMETRIC_SIZES] + [0]
    assert n[-1] == 466 and n[-4:-1] == [10, 10, 10] and all(580 < v < 590 for v in n[len(asym):len(asym) + 6])
    status = want["status"].tolist()
    assert status[-4:] == [M.OK] * 4 and status[len(asym):len(asym) + 6] == [M.OK] * 6 and status[4:6] == [M.OK] * 2
    first = int(np.cumsum([0] + [p["from_ids"].shape[0] for p in pairs])[-5])          # the first extreme pair's region
    assert want["matches"][first] == I.INT32_MIN and want["matches"][first + 9] == I.INT32_MAX


@pytest.mark.parametrize("which", ("at_the_cap", "one_above", "both_beside_small_pairs"))
def test_the_switch_between_lds_and_scratch(eng, which):
    """5400 x 5300 rows with 5248 correspondences (the last count that is staged) and with 5249 (the first that is not)"""
    at, above = inputs("stage_switch_pairs")
    small = inputs("mixed_batch")[3:6]
    pairs = {"at_the_cap": [at], "one_above": [above], "both_beside_small_pairs": [small[0], at, small[1], above, small[2]]}[which]
    want = check_both(eng, pairs, which, **SWITCH_KW)
    big = [k for k, p in enumerate(pairs) if p is at or p is above]
    assert want["n_matches"][big].tolist() == [I.STAGE_CAP + (pairs[k] is above) for k in big]
    assert (want["status"][big] == M.OK).all() and (want["n_inliers"][big] > 3000).all()


def test_a_stride_that_is_not_the_row_count_in_either_layout(eng):
    """m = 150 of 8192 x 200 rows (staged, stride m), five correspondences, m = 5260 of 8192 x 5300 rows (scratch, stride n_from) in one call
    and again in the reverse order: both calls equal the model's results of the same three pairs, so a pair's outputs do not depend on where
    it stands"""
    pairs = inputs("stride_pairs")
    want = check_both(eng, pairs, "forward", **SWITCH_KW)
    assert want["n_matches"].tolist() == [150, 5, 5260] and want["status"].tolist() == [M.OK, M.FEW_CORRESPONDENCES, M.OK]
    back = check_both(eng, pairs[::-1], "reverse", **SWITCH_KW)      # the same model results (cached per pair), in the other order
    assert back["n_matches"].tolist() == [5260, 5, 150]


@pytest.mark.parametrize("iterations", I.TIE_ITERATIONS)
def test_a_tie_across_chunks_goes_to_the_first_valid_hypothesis(eng, iterations):
    """every valid hypothesis of every chunk holds all correspondences: hypothesis 0 wins, or -- under a seed whose first two hypotheses are
    invalid -- hypothesis 2; 65535 iterations end in a chunk of 255"""
    m, invalid, seed = I.TIE_INVALID_FIRST
    forty, three = inputs("tie_pairs")
    kw = dict(min_inliers=3, inlier_distance=0.1, iterations=iterations, refine_iterations=0)
    check_both(eng, [forty], "forty", seed=I.TIE_SEED, **kw)
    assert model_of(forty, seed=I.TIE_SEED, **kw)["best"] == 0
    check_both(eng, [three], "three", seed=seed, **kw)
    assert model_of(three, seed=seed, **kw)["best"] == invalid


@pytest.mark.parametrize("h,iterations", I.LATE_CASES)
def test_a_unique_winner_late_in_the_chunks(eng, h, iterations):
    pair = inputs("late_winner_pair")
    kw = I.late_kw(h, iterations)
    want = check_both(eng, [pair], "winner at %d of %d" % (h, iterations), **kw)
    assert model_of(pair, **kw)["best"] == h and want["n_inliers"][0] == 5 and want["status"][0] == M.OK


@pytest.mark.parametrize("h", I.CUT_OFF)
def test_a_hypothesis_beyond_the_iterations_never_wins(eng, h):
    """iterations = h: the winner would be the next hypothesis of a partial chunk"""
    pair = inputs("late_winner_pair")
    kw = I.late_kw(h, h)
    check_both(eng, [pair], "cut off at %d" % h, **kw)
    r = model_of(pair, **kw)
    assert r["best"] is not None and r["best"] < h and 0 < r["counts"].max() < 5


@pytest.mark.parametrize("seed", sorted(I.LATE_MEMBERS))
def test_two_index_sets_that_differ_only_behind_the_first_256(eng, seed):
    pair = inputs("late_members_pair", seed)
    kw = dict(I.LATE_MEMBERS_KW, seed=seed)
    want = check_both(eng, [pair], "members %d" % seed, **kw)
    r = model_of(pair, **kw)
    assert r["first_differing"] == [I.LATE_MEMBERS[seed]] and want["n_inliers"][0] > 256


def test_the_radix_select(eng):
    """selections of 3, 4, 255, 256 and 257 elements, all zero, mostly equal to the median, an even size with two different middle elements,
    and three middle elements that differ in their low byte only -- alone (each kernel launch with its own LDS carve) and in one batch"""
    cases = inputs("select_cases")
    for name, (pair, kw) in cases.items():
        want = check_both(eng, [pair], name, **kw)
        assert want["status"][0] == M.OK
    groups = {}
    for name, (pair, kw) in cases.items():
        groups.setdefault(tuple(sorted(kw.items())), []).append(pair)
    for kw, pairs in groups.items():
        if len(pairs) > 1:
            check_both(eng, pairs, "batch", **dict(kw))
    for name, n in I.SELECT_SIZES.items():
        assert len(model_of(cases[name][0], **cases[name][1])["last_d2"]) == n


def test_the_refinement_and_the_median_with_the_coordinates_in_the_scratch(eng):
    """5420 correspondences: the selection, the fits, the comparison of the members and the radix select read global memory"""
    pair = inputs("scratch_table_pair")
    for kw in I.scratch_table_kws():
        want = check_both(eng, [pair], "scratch table", **kw)
        assert want["status"][0] == M.OK and want["n_matches"][0] == 5420 and want["n_inliers"][0] >= 5000


def test_the_cpp_wrapper_over_a_dictionary_handle():
    """Motion3D::estimateMotion3DTo3D through VWDictionaryHip.estimate_motion_3d: the transform, the 6 x 6 covariance, the two id lists, and
    the dictionary that lends its handle untouched"""
    from rtabmap_amd.vwdictionary import VWDictionaryHip
    from rtabmap_amd import synth
    h = VWDictionaryHip(nndr=0.8, new_words_compared_together=True)
    h.add_new_words(synth.vocab_surf(50, seed=8), 1)
    h.update()
    before = (h.index_ids(), h.visual_words, h.indexed_words, h.not_indexed_words, h.total_active_references)
    assert before[1] > 40 and before[4] == 50
    kw = dict(I.WRAPPER_KW)
    model_kw = dict(kw, inlier_distance=kw["inliers_distance"])
    del model_kw["inliers_distance"]
    statuses = []
    for k, pair in enumerate(I.wrapper_pairs()):
        want = M.estimate(*I.frames(pair), **model_kw)
        statuses.append(want["status"])
        t, cov, matches, inliers = h.estimate_motion_3d((pair["from_ids"], pair["from_xyz"]), (pair["to_ids"], pair["to_xyz"]), **kw)
        assert (t is None) == (want["status"] != M.OK), k
        if t is not None:
            np.testing.assert_array_equal(I.bits(t), I.bits(want["transform"]), err_msg=str(k))
        np.testing.assert_array_equal(cov.view(np.uint64), (np.eye(6) * want["variance"]).view(np.uint64), err_msg=str(k))
        assert matches == want["matches"].tolist() and inliers == want["inliers"].tolist(), k
        # refused (iterations = 0): no transform, the identity, no ids
        t, cov, matches, inliers = h.estimate_motion_3d((pair["from_ids"], pair["from_xyz"]), (pair["to_ids"], pair["to_xyz"]), **dict(kw, iterations=0))
        assert t is None and matches == [] and inliers == []
        np.testing.assert_array_equal(cov, np.eye(6))
    assert statuses == [M.FEW_CORRESPONDENCES, M.BELOW_MIN_INLIERS, M.OK, M.OK]
    assert (h.index_ids(), h.visual_words, h.indexed_words, h.not_indexed_words, h.total_active_references) == before
    h.close()
