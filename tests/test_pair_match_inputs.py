"""CPU-only: every input of tests/test_gpu_pair_match_shapes.py has, on the MODEL alone (pair_match_model over the oracle), the property
it is there for -- so that a pass on the GPU means the code was taken where the case says it is.  An input without its property is
replaced by the next seed inside pair_match_inputs (capped; the builders raise when the cap is hit), never skipped."""
import numpy as np
import pytest

import pair_match_inputs as I
import pair_match_model as M

KINDS = [("f32", 64), ("u8", 32)]


def test_builders_give_the_shapes_they_are_asked_for():
    for dtype, dim, npdt in (("f32", 5, np.float32), ("u8", 33, np.uint8)):
        for nf, nt in ((0, 0), (0, 5), (5, 0), (1, 1), (1, 3), (2, 2), (33, 65)):
            f, t = I.interleaved_pair(dtype, dim, nf, nt, 1)
            assert f.shape == (nf, dim) and t.shape == (nt, dim) and f.dtype == npdt and t.dtype == npdt
            assert f.flags.c_contiguous and t.flags.c_contiguous
        f, t = I.collapsing_pair(dtype, dim, 3, 1100, 40)
        assert f.shape == (1100, dim) and t.shape == (40, dim) and len({r.tobytes() for r in f}) == 3
    f, t = I.interleaved_pair("f32", 64, 2049, 1100, 3)
    np.testing.assert_allclose(np.linalg.norm(f, axis=1), 1.0, rtol=1e-6)
    g, u = I.interleaved_pair("f32", 64, 2049, 1100, 3)
    assert np.array_equal(f, g) and np.array_equal(t, u)                   # a seed is an input
    pairs = I.many_small_pairs("u8", 32, 700, 5)
    sizes = np.array([(a.shape[0], b.shape[0]) for a, b in pairs])
    assert sizes.shape == (700, 2) and sizes.min() == 0 and sizes.max() == 40
    assert sizes[3, 0] == 0 and sizes[3, 1] > 0 and sizes[5, 1] == 0 and sizes[5, 0] > 0 and sizes[7].tolist() == [0, 0]
    assert len(set(map(tuple, sizes.tolist()))) > 300


def test_property_helpers_on_hand_made_results():
    ef = np.array([1, 2, 1, 3, 2], np.int32)
    assert I.shared_across(ef, 2) == 2 and I.shared_across(ef, 4) == 1 and I.shared_across(ef[:2], 1) == 0
    et = np.array([2, 4, 5, 4, 3, 5], np.int32)
    assert I.to_classes(ef, et).tolist() == [I.TOOK_FROM_WORD, I.CREATED, I.CREATED, I.TOOK_TO_WORD, I.TOOK_FROM_WORD, I.TOOK_TO_WORD]
    assert I.spans_boundaries(ef, et)                                       # no boundary, nothing to span
    ids = np.arange(1, 1031, dtype=np.int32)
    assert not I.spans_boundaries(ids, et)                                  # 1030 from-rows, all of them words of their own
    ids[1027] = 5
    assert I.spans_boundaries(ids, et)
    f = np.array([[1, 2], [3, 4], [1, 2]], np.float32)
    t = np.array([[9, 9], [3, 4], [9, 9], [7, 7]], np.float32)
    assert [x.tolist() for x in I.duplicate_rows(f, t)] == [[False, False, True], [False, True, True, False]]
    with pytest.raises(AssertionError):
        I.first_seed(lambda s: s, lambda x: False, 0, cap=3)
    assert I.first_seed(lambda s: s, lambda x: x == 12, 10, cap=3) == 12


@pytest.mark.parametrize("nf,nt", I.LARGE_SIZES)
@pytest.mark.parametrize("dtype,dim", KINDS)
def test_large_pairs_reach_across_the_workgroup_width(oracle, dtype, dim, nf, nt):
    f, t, (ef, et) = I.large_pair(oracle, dtype, dim, nf, nt)
    assert f.shape[0] == nf and t.shape[0] == nt and I.spans_boundaries(ef, et)
    cls = I.to_classes(ef, et)
    print("%s x %d, %d + %d: %d from-words, same-word from-row pairs across row 1024: %d; to-rows behind row 1024: %s"
          % (dtype, dim, nf, nt, np.unique(ef).size, I.shared_across(ef, 1024) if nf > 1024 else -1,
             [int((cls[1024:] == c).sum()) for c in (0, 1, 2)]))
    if nf > 1024:
        assert I.shared_across(ef, 1024) > 0
    if nf > 2048:
        assert ef[2048:].size == 1 and ef[2048] in ef[:2048]               # the one row behind row 2048 took an earlier row's word
    if nt > 1024:
        for part in (cls[:1024], cls[1024:2048]):
            assert all((part == c).any() for c in (I.TOOK_FROM_WORD, I.CREATED, I.TOOK_TO_WORD))
    if nt > 2048:
        assert (cls[2048:] != I.CREATED).any()
    # compared apart no two rows of a frame share a word: the from-frame is nf words whatever the rows are
    af, at = M.dictionary_pair(oracle, f, t, 0.8, False)
    assert af.tolist() == list(range(1, nf + 1)) and not (I.to_classes(af, at) == I.TOOK_TO_WORD).any()
    assert (I.to_classes(af, at)[-(nt // 4):] == I.TOOK_FROM_WORD).any()


@pytest.mark.parametrize("nf,nt", I.LIMIT_SIZES)
def test_pairs_at_the_row_limit_reach_across_every_multiple_of_the_width(oracle, nf, nt):
    f, t, (ef, et) = I.large_pair(oracle, "f32", 64, nf, nt)
    assert max(nf, nt) == 8192 and I.spans_boundaries(ef, et)
    if nf == 8192:
        assert all(I.shared_across(ef, b) > 0 for b in range(1024, 8192, 1024))
        assert ef[8128:].max() > ef[:8128].max() and np.isin(ef[8128:], ef[:8128]).any()    # the last 64 rows: new words and matches
    else:
        cls = I.to_classes(ef, et)
        assert all(len(set(cls[b:b + 1024].tolist())) == 3 for b in range(0, 8192, 1024))


@pytest.mark.parametrize("dtype,dim", KINDS)
def test_given_ids_decide_a_tie_across_row_1024(oracle, dtype, dim):
    f, t, ids, triples, (ef, et) = I.given_ids_pair(oracle, dtype, dim)
    assert ids.max() > 1000 * ids.size and (np.diff(ids) < 0).any() and np.unique(ids).size == ids.size
    won_by = set()
    for a, b, i in triples:
        assert a < 1024 <= b and np.array_equal(f[a], f[b]) and np.array_equal(t[i], f[a])
        assert et[i] == min(ids[a], ids[b])                                 # the lower ID, whichever side of row 1024 it is on
        won_by.add(bool(ids[b] < ids[a]))
    assert won_by == {True, False}
    assert np.array_equal(ef, ids) and et.max() > ids.max()


@pytest.mark.parametrize("nf,nt", I.RATIO_SIZES)
@pytest.mark.parametrize("dtype,dim", KINDS)
def test_the_four_ratios_give_four_results(oracle, dtype, dim, nf, nt):
    f, t, exp = I.ratio_pair(oracle, dtype, dim, nf, nt)
    assert I.ratios_tell_apart(f, t, exp)
    for c in (True, False):
        cat = [np.concatenate(exp[(r, c)]) for r in I.RATIOS]
        print(dtype, nf, nt, "together" if c else "apart", "rows that differ from nndr 0.8:", [int((x != cat[2]).sum()) for x in cat])
        assert all(not np.array_equal(cat[i], cat[j]) for i in range(4) for j in range(i))
    ef, et = exp[(1.0, True)]
    assert ef[:2].tolist() == [1, 2] and set(ef.tolist()) == {1, 2} and set(et.tolist()) <= {1, 2}
    ef, et = exp[(0.0, True)]
    dup_f, dup_t = I.duplicate_rows(f, t)
    assert dup_f.sum() >= 6 and dup_t.sum() >= 12
    assert np.unique(ef).size == np.unique(ef[~dup_f]).size == (~dup_f).sum()       # every row without an earlier twin is a word ...
    assert np.unique(ef).size < nf                                                   # ... and a twin met its word at distance 0
    assert (I.to_classes(ef, et)[~dup_t] == I.CREATED).all() and (I.to_classes(ef, et)[dup_t] != I.CREATED).any()


@pytest.mark.parametrize("dtype,dim", KINDS)
def test_collapsing_frames_sit_on_the_index_boundary(oracle, dtype, dim):
    """k distinct rows, 0 1 .. k-1 0 1 ..  Together: row 0 has no candidate and row 1 only one, so both are words whatever they hold; a
    later row sees its twin at distance 0 (0 > nndr * d is false) and takes the FIRST twin's word; a third distinct row is about as far
    from both words (ratio above 0.8) and becomes word 3.  Apart: no candidates at all, nf words."""
    for nf in (5, 1100):
        pat = np.arange(nf)
        want = {1: np.where(pat == 1, 2, 1), 2: pat % 2 + 1, 3: pat % 3 + 1}
        for k in (1, 2, 3):
            f, t = I.collapsing_pair(dtype, dim, k, nf, 40)
            ef, et = M.dictionary_pair(oracle, f, t, 0.8, True)
            assert ef.tolist() == want[k].tolist(), (k, nf)
            assert np.unique(ef).size == max(k, 2)                          # exactly two words: the smallest vocabulary that is searched
            base = np.unique(ef).size
            af, at = M.dictionary_pair(oracle, f, t, 0.8, False)
            assert af.tolist() == list(range(1, nf + 1))
            for j in range(k):                                              # the to-row that IS base row j: first twin's word, both ways
                i = [i for i in range(40) if np.array_equal(t[i], f[j])]
                assert i and (at[i] == j + 1).all() and (et[i] == j + 1).all()
            assert (et > base).any() and (at > nf).any()                    # fresh rows are new words behind the from-frame's
            if k == 1:
                # one distinct row, two words at the same place: a noisy copy is as far from one as from the other and is rejected
                twins = (t == f[0]).all(axis=1)                               # (a binary copy may come out without a flipped bit)
                assert np.array_equal(I.to_classes(ef, et) == I.TOOK_FROM_WORD, twins) and twins.sum() < 4
            else:
                assert (I.to_classes(ef, et) == I.TOOK_FROM_WORD).sum() > k
    f, t = I.collapsing_pair(dtype, dim, 1, 5, 40)
    assert M.dictionary_pair(oracle, f, t, 0.8, True)[0].tolist() == [1, 2, 1, 1, 1]


@pytest.mark.parametrize("nf,nt", I.LARGE_SIZES)
@pytest.mark.parametrize("dtype,dim", KINDS)
def test_cross_check_inputs_have_ties_and_both_outcomes(oracle, dtype, dim, nf, nt):
    f, t, D, (m, d) = I.tie_pair(oracle, dtype, dim, nf, nt)
    assert D.shape == (nt, nf) and M.tie_resolved_by_index(D) and I.cross_spans_boundaries(m, nf)
    assert (m >= 0).any() and (m < 0).any()
    if nf > 1024:
        assert (m >= 1024).any() and ((m >= 0) & (m < 1024)).any()          # from-rows on both sides of row 1024 are matched
    if nf >= 1024 + 12:
        # a to-row whose two nearest from-rows tie across row 1024 takes the one in front of it
        tied = [(i, np.flatnonzero(D[i] == D[i].min())) for i in range(nt)]
        assert any(j.size > 1 and j[0] < 1024 <= j[-1] and d[i] == D[i, j[0]] and m[i] in (-1, j[0]) for i, j in tied)
    if nt > 1024:
        assert (m[1024:] >= 0).any() and (m[1024:] < 0).any()


@pytest.mark.parametrize("dim", [61, 128])
def test_integer_rows_tie_exactly(oracle, dim):
    for nf, nt in ((33, 65), (65, 31)):
        f, t = I.integer_pair(dim, nf, nt, 50 + dim)
        assert f.dtype == np.float32 and np.array_equal(f, np.round(f)) and f.min() >= 0 and f.max() <= 4
        D = I.dist(oracle, t, f)
        assert np.array_equal(D, np.round(D)) and (D == 0).any() and (D == 3).any()       # twins, and rows one step away in three places
        m, _ = M.cross_check(D)
        assert M.tie_resolved_by_index(D) and (m >= 0).any() and (m < 0).any()
        s = np.sort(D, axis=1)
        assert ((s[:, 0] == s[:, 1]) & (s[:, 0] > 0)).any()                  # best and second-best tie at a distance that is not 0
        dup_f, dup_t = I.duplicate_rows(f, t)
        assert dup_f.sum() >= 2 and dup_t.sum() >= 4
        for compared in (True, False):
            ef, et = M.dictionary_pair(oracle, f, t, 0.8, compared)
            cls = I.to_classes(ef, et)
            assert (cls == I.TOOK_FROM_WORD).any() and (cls == I.CREATED).any()
            assert (np.unique(ef).size < nf) == compared


def test_small_pairs_in_the_kernel_cases_have_their_property(oracle):
    """the four pairs every handle of the distance-kernel case sees: sizes across both tile widths with matches and new words, one
    from-row (no index), exact duplicates (ties in both directions of the cross-check)"""
    for dtype, dim in (("f32", 3), ("f32", 61), ("u8", 8), ("u8", 33), ("u8", 128)):
        pairs = I.kernel_case_pairs(dtype, dim)
        assert [(f.shape[0], t.shape[0]) for f, t in pairs] == [(33, 65), (65, 31), (1, 3), (8, 11)]
        for f, t in pairs[:2]:
            ef, et = M.dictionary_pair(oracle, f, t, 0.8, True)
            cls = I.to_classes(ef, et)
            assert (cls == I.TOOK_FROM_WORD).any() and (cls == I.CREATED).any(), (dtype, dim)
        ef, et = M.dictionary_pair(oracle, *pairs[2], 0.8, True)
        assert ef.tolist() == [1] and et.tolist() == [2, 3, 2]                  # no index; the third row meets two twins
        D = I.dist(oracle, pairs[3][1], pairs[3][0])
        m, _ = M.cross_check(D)
        assert M.tie_resolved_by_index(D) and (m >= 0).any() and (m < 0).any()
