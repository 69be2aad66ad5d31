"""CPU-only: the model of the pair similarity (tests/similarity_model.py) is consistent with itself, the identity the sealed-bucket
kernel relies on holds, and the cross-compiled libraries export the feature's entry points."""
import ctypes

import numpy as np

import similarity_model as M


def _random_multiset(rng, n, n_words, frac_invalid):
    w = rng.integers(1, n_words + 1, n)
    bad = rng.random(n) < frac_invalid
    w[bad] = rng.integers(-5, 1, int(bad.sum()))          # ids <= 0: features without a word (0 included)
    return w.astype(np.int32)


def test_literal_walk_equals_closed_form():
    """(i) the restated findPairs / compareTo == (ii) sum of min over random multisets with duplicates, ids <= 0 and empty sides"""
    rng = np.random.default_rng(1)
    cases = []
    for _ in range(300):
        n_words = int(rng.integers(1, 30))
        a = _random_multiset(rng, int(rng.integers(0, 60)), n_words, float(rng.choice([0.0, 0.2, 1.0], p=[0.5, 0.4, 0.1])))
        b = _random_multiset(rng, int(rng.integers(0, 60)), n_words, float(rng.choice([0.0, 0.2, 1.0], p=[0.5, 0.4, 0.1])))
        cases.append((a, b))
    cases += [(np.zeros(0, np.int32), np.array([1, 2], np.int32)), (np.array([1, 2], np.int32), np.zeros(0, np.int32)),
              (np.array([-1, 0], np.int32), np.array([1, 1], np.int32)), (np.array([1, 2, 3, 4, 6, 6], np.int32), np.array([1, 1, 2, 4, 5, 6, 6], np.int32))]
    for a, b in cases:
        sim, pairs, valid = M.compare_to_literal(a, b)
        csim, cpairs, cvalid = M.similarity_closed_form(a, [b])
        assert pairs == cpairs[0] and valid == cvalid[0]
        assert np.float32(sim).tobytes() == csim[0].tobytes()
        # compareTo is symmetric in its words branch
        sim_r, pairs_r, _ = M.compare_to_literal(b, a)
        assert pairs_r == pairs and np.float32(sim_r).tobytes() == np.float32(sim).tobytes()
    # the example of EpipolarGeometry.h:120-121: five pairs
    assert M.compare_to_literal(cases[-1][0], cases[-1][1])[1] == 5
    assert M.pairs_closed_form(cases[-1][0], cases[-1][1]) == 5


def test_dense_sparse_cap_identity():
    """min(cq, cs) = min(cq, cell) + min(max(cq - 255, 0), excess) with cell = min(cs, 255), excess = max(cs - 255, 0): what a sealed
    bucket stores of a dense word's count, exhaustively for cq, cs in [0, 600]"""
    cq, cs = np.meshgrid(np.arange(601), np.arange(601), indexing="ij")
    cell, excess = np.minimum(cs, 255), np.maximum(cs - 255, 0)
    np.testing.assert_array_equal(np.minimum(cq, cell) + np.minimum(np.maximum(cq - 255, 0), excess), np.minimum(cq, cs))


def test_libraries_export_the_similarity_entry_points():
    import rtabmap_amd
    from rtabmap_amd import build as b
    rtabmap_amd.load()
    lib = ctypes.CDLL(rtabmap_amd.library_path())
    for s in ("lcd_similarity", "lcd_similarity_dev"):
        assert hasattr(lib, s), s
    host = ctypes.CDLL(b.build_host())
    for s in ("hmem_set_tfidf_likelihood_used", "hmem_compare_to"):
        assert hasattr(host, s), s
