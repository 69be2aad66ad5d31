"""GPU parity of the matrix-core 2-NN of 128- and 256-float rows (an LCD_F32 handle whose config writes LCD_KNN_BF16X3 or LCD_KNN_F16:
knn_wide_filter_kernel + knn_wide_rerank_kernel + knn_wide_rowpar_kernel, wide_filter_body.cuh) against the CPU oracle's linear scan: every
comparison is assert_array_equal on word ids AND distance bits, and the oracle's answer is computed before the engine exists.  The fall-back
cap (knn_last_fallback_queries <= q // 4 where a case names it) keeps the exact redo from hiding a broken filter."""
import os

import numpy as np
import pytest
import torch

from rtabmap_amd import synth

pytestmark = pytest.mark.gpu

NEW_KERNEL = "knn_wide_filter_kernel"
DIMS = [128, 256]
MODES = ["bf16", "f16"]
UNITS = 8                                                # lcd_set_option("filter_units"): several strips per workgroup at 3 000 rows
both = lambda f: pytest.mark.parametrize("dim", DIMS)(pytest.mark.parametrize("mode", MODES)(f))


def _engine(dim, mode, units=None, **kw):
    import rtabmap_amd
    eng = rtabmap_amd.Engine("f32", dim, knn_mode=mode, **kw)
    if units is not None:
        eng.set_option("filter_units", units)           # (also over a value the whole run was given)
    return eng


def _expect(oracle, vocab, ids, queries, removed=None):
    idx, d = oracle.knn2_linear(vocab, queries, removed=removed)
    return idx, (np.where(idx >= 0, ids[np.maximum(idx, 0)], 0).astype(np.int32), d)


def _plan(q, n_rows, dim, units):
    """[tiles per share of the rows, shares, query blocks, queries per block, qpad, record bytes / 4, tiles per strip, strips per share, workgroups
    along the rows (workgroup x takes shares x, x + workgroups, ...)]"""
    import ctypes as C
    import rtabmap_amd
    rtabmap_amd.load()
    lib = C.CDLL(rtabmap_amd.library_path())
    lib.lcd_debug_wide_mfma_plan.restype = C.c_int
    lib.lcd_debug_wide_mfma_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    out = (C.c_int * 9)()
    assert lib.lcd_debug_wide_mfma_plan(q, n_rows, dim, units, out) == 0
    return list(out)


def _check(eng, queries, exp, msg=""):
    """the engine's answer is the oracle's, bit for bit, and the launch that filtered was the matrix-core kernel's; returns the stats"""
    eng.profile_begin(2)
    got_ids, got_d = eng.knn2(queries)
    _, n, name = eng.profile_read()
    assert n == 1 and name.startswith(NEW_KERNEL), (n, name)
    np.testing.assert_array_equal(got_d, exp[1], err_msg=msg)
    np.testing.assert_array_equal(got_ids, exp[0], err_msg=msg)
    return eng.stats()


def _noisy_rows(rng, vocab, rows, sigma):
    return (vocab[rows] + sigma * rng.standard_normal((len(rows), vocab.shape[1])).astype(np.float32)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- 1. which kernel ran
def _kernel_of_a_search(dim, mode, n_rows, q):
    v = synth.vocab_surf(n_rows, seed=2, dim=dim)
    qs = synth.queries_surf(v, q, seed=3)
    eng = _engine(dim, mode)
    eng.vocab_append(v, np.arange(1, n_rows + 1, dtype=np.int32))
    d_q = torch.from_numpy(qs).cuda()
    d_w = torch.zeros((q, 2), dtype=torch.int32, device="cuda")
    d_d = torch.zeros((q, 2), dtype=torch.float32, device="cuda")
    eng.profile_begin(4)
    eng.knn2_dev(d_q.data_ptr(), q, d_w.data_ptr(), d_d.data_ptr())
    eng.synchronize()
    _, n, name = eng.profile_read()
    eng.close()
    return n, name


def test_which_kernel_ran():
    """Without this every other test here could pass on a silent fall-back to the scan."""
    n, name = _kernel_of_a_search(128, "bf16", 1000, 70)
    assert n == 1 and name.startswith(NEW_KERNEL), name
    assert _kernel_of_a_search(128, "f16", 1000, 70) == (1, NEW_KERNEL + " (fp16 operands)")
    assert _kernel_of_a_search(128, "bf16", 255, 70) == (1, "knn2_l2_kernel")        # below 256 rows: the exact scan, as at 64 floats
    assert _kernel_of_a_search(128, "default", 1000, 70) == (1, "knn2_l2_kernel")    # the default did not move
    assert _kernel_of_a_search(256, "valu", 1000, 70) == (1, "knn2_l2_kernel")
    assert _kernel_of_a_search(64, "bf16", 1000, 70) == (1, "knn_bf16_filter_kernel")   # 64 floats: the filter with the operand table, as before


# ---------------------------------------------------------------------------------------------------------------- 2. ragged sizes
@both
@pytest.mark.parametrize("n,q", [(256, 1), (257, 33), (1000, 64), (4097, 130), (9973, 65)])
def test_ragged_sizes(oracle, dim, mode, n, q):
    """the last rows of a tile and of a workgroup's share, the last queries of a group of 32 and of a wave"""
    v = synth.vocab_surf(n, seed=n, dim=dim)
    qs = synth.queries_surf(v, q, seed=q)
    ids = np.arange(1, n + 1, dtype=np.int32)
    _, exp = _expect(oracle, v, ids, qs)
    eng = _engine(dim, mode)
    eng.vocab_append(v, ids)
    st = _check(eng, qs, exp)
    print(dim, mode, n, q, "fallback", st["knn_last_fallback_queries"], "max err / eps", st["knn_max_err_ratio"])
    assert st["knn_last_fallback_queries"] <= q // 4
    assert 0.0 < st["knn_max_err_ratio"] < 1.0
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- 3. SIFT-like rows
def _sift_like(rng, n):
    """integer-valued components 0 .. 255, most of them small: |v|^2 ~ 10^5"""
    return np.minimum(np.floor(rng.exponential(20.0, (n, 128))), 255.0).astype(np.float32)


@pytest.mark.parametrize("mode", MODES)
def test_sift_like_rows(oracle, mode):
    rng = np.random.default_rng(128)
    n, q = 3000, 100
    v = _sift_like(rng, n)
    assert 5e4 < float((v.astype(np.float64) ** 2).sum(1).mean()) < 2e5
    qs = np.clip(_noisy_rows(rng, v, rng.integers(0, n, q), np.float32(4.0)), 0.0, 255.0).astype(np.float32)   # clipped noisy copies ...
    qs[70:] = _sift_like(rng, 30)                                                                              # ... plus fresh draws
    ids = np.arange(1, n + 1, dtype=np.int32)
    _, exp = _expect(oracle, v, ids, qs)
    eng = _engine(128, mode)
    eng.vocab_append(v, ids)
    st = _check(eng, qs, exp)
    print(mode, "fallback", st["knn_last_fallback_queries"], "max err / eps", st["knn_max_err_ratio"])
    assert st["knn_last_fallback_queries"] <= q // 4
    assert 0.0 < st["knn_max_err_ratio"] < 1.0
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- 4. ties
@both
def test_ties_lowest_row_wins(oracle, dim, mode):
    rng = np.random.default_rng(5 + dim)
    n, q = 3000, 120
    ids = np.arange(1, n + 1, dtype=np.int32)
    # every row has an exact duplicate 1 500 rows later
    v = synth.vocab_surf(n, seed=5, dim=dim)
    v[1500:] = v[:1500]
    qs = _noisy_rows(rng, v, rng.integers(0, n, q), np.float32(0.02))
    idx, exp = _expect(oracle, v, ids, qs)
    assert (exp[1][:, 0] == exp[1][:, 1]).all() and (idx[:, 1] == idx[:, 0] + 1500).all()
    eng = _engine(dim, mode)
    eng.vocab_append(v, ids)
    _check(eng, qs, exp)
    eng.close()
    # exact ties inside one group of four consecutive rows, across a 32-row tile seam, across a strip seam and across two workgroups' shares
    tpb, nb, _, _, _, _, strip, strips, wgs = _plan(q, n, dim, UNITS)
    assert (tpb, nb, strip, strips, wgs) == (12, 8, 8, 2, 8)         # a share is 12 tiles: a strip of 8 and one of 4; row 256 opens the second strip
    v = synth.vocab_surf(n, seed=6, dim=dim)
    qs = synth.queries_surf(v, q, seed=7)
    pairs = [(1204, 1206), (1205, 1207), (671, 672), (2047, 2048), (32 * strip - 1, 32 * strip), (32 * tpb + 32 * strip - 1, 32 * tpb + 32 * strip),
             (32 * tpb - 1, 32 * tpb), (32 * tpb * 3 - 1, 32 * tpb * 3), (40, 2990)]
    assert pairs[0][0] // 4 == pairs[0][1] // 4 and pairs[2][0] // 32 != pairs[2][1] // 32
    for i, (ra, rb) in enumerate(pairs):
        v[ra] = v[rb] = _noisy_rows(rng, qs, [i], np.float32(0.01))[0]
    idx, exp = _expect(oracle, v, ids, qs)
    for i, (ra, rb) in enumerate(pairs):
        assert idx[i].tolist() == [ra, rb] and exp[1][i, 0] == exp[1][i, 1]          # the planted rows are the two nearest and tie, by the oracle alone
    eng = _engine(dim, mode, units=UNITS)
    eng.vocab_append(v, ids)
    _check(eng, qs, exp)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- 5. tombstones and rebuild
@both
def test_tombstones_and_rebuild(oracle, dim, mode):
    n, q = 3000, 90
    v = synth.vocab_surf(n, seed=3, dim=dim)
    qs = synth.queries_surf(v, q, seed=4)
    ids = np.arange(10, n + 10, dtype=np.int32)
    idx0, exp0 = _expect(oracle, v, ids, qs)
    removed = np.zeros(n, np.uint8)
    removed[np.random.default_rng(9).choice(n, 500, replace=False)] = 1
    removed[idx0[:, 0]] = 1                                # every query's nearest row
    removed[640:672] = 1                                   # two whole aligned 32-row tiles
    removed[2048:2080] = 1
    _, exp1 = _expect(oracle, v, ids, qs, removed=removed)
    keep = removed == 0
    survivor = int(np.flatnonzero(keep)[1234])
    all_but_one = np.ones(n, np.uint8); all_but_one[survivor] = 0
    _, exp2 = _expect(oracle, v, ids, qs, removed=all_but_one)
    assert (exp2[0][:, 0] == ids[survivor]).all() and (exp2[0][:, 1] == 0).all() and (exp2[1][:, 1] == -1.0).all()
    _, exp3 = _expect(oracle, v[keep], ids[keep], qs)
    eng = _engine(dim, mode)
    eng.vocab_append(v, ids)
    _check(eng, qs, exp0)
    eng.vocab_remove(ids[removed == 1])
    _check(eng, qs, exp1)                                  # tombstoned rows are never returned
    gone = keep.copy(); gone[survivor] = False
    eng.vocab_remove(ids[gone])
    _check(eng, qs, exp2)                                  # all rows but one: (id, 0) and (d, -1)
    eng.close()
    # a rebuild compacts the rows: the same search over the survivors of the first removal
    eng = _engine(dim, mode)
    eng.vocab_append(v, ids)
    eng.vocab_remove(ids[removed == 1])
    eng.vocab_rebuild()
    assert eng.vocab_count() == (int(keep.sum()), int(keep.sum()))
    _check(eng, qs, exp3)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- 6. clusters
@both
def test_clusters_of_identical_rows_go_to_the_redo(oracle, dim, mode):
    """40 identical rows in one run and queries equal to them: no bound certifies a second neighbour among equals -- the exact redo answers"""
    n = 3000
    v = synth.vocab_surf(n, seed=61, dim=dim)
    v[1000:1040] = v[1000]
    ids = np.arange(1, n + 1, dtype=np.int32)
    qs = synth.queries_surf(v, 60, seed=62)
    qs[0] = v[1000]
    _, exp_one = _expect(oracle, v, ids, qs[:1])
    assert exp_one[0].tolist() == [[1001, 1002]] and exp_one[1].tolist() == [[0.0, 0.0]]
    eng = _engine(dim, mode)
    eng.vocab_append(v, ids)
    st = _check(eng, qs[:1], exp_one)
    assert st["knn_last_fallback_queries"] >= 1
    qs[:] = v[1000]                                        # 60 such queries at once
    _, exp = _expect(oracle, v, ids, qs)
    st = _check(eng, qs, exp)
    assert st["knn_last_fallback_queries"] >= 1
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- 7. range
@pytest.mark.parametrize("dim", DIMS)
def test_fp16_operands_beyond_halfs_range(oracle, dim):
    """components beyond 65504 cannot be fp16 operands: every query is rejected and redone exactly; scaled into range the filter certifies again"""
    n, q = 2000, 80
    unit = synth.vocab_surf(n, seed=71, dim=dim)
    uq = synth.queries_surf(unit, q, seed=72)
    scale = np.float32(2.0 ** 22)
    v, qs = (unit * scale).astype(np.float32), (uq * scale).astype(np.float32)
    assert float(np.abs(v).max()) > 65504.0 and float(np.abs(v).max(1).min()) > 65504.0 and float(np.abs(qs).max(1).min()) > 65504.0
    ids = np.arange(1, n + 1, dtype=np.int32)
    _, exp = _expect(oracle, v, ids, qs)
    eng = _engine(dim, "f16")
    eng.vocab_append(v, ids)
    st = _check(eng, qs, exp)
    assert st["knn_last_fallback_queries"] == q
    eng.close()
    _, exp = _expect(oracle, unit, ids, uq)
    eng = _engine(dim, "f16")
    eng.vocab_append(unit, ids)
    st = _check(eng, uq, exp)
    assert st["knn_last_fallback_queries"] <= q // 4
    eng.close()


@pytest.mark.parametrize("dim", DIMS)
def test_bf16_on_wide_range_rows(oracle, dim):
    """large and tiny components in one row (e^-6 .. e^6), mixed signs, non-unit norms, queries near, equal to and far from rows"""
    rng = np.random.default_rng(11 + dim)
    n, q = 2048, 129
    v = (rng.standard_normal((n, dim)) * np.exp(rng.uniform(-6, 6, (n, dim)))).astype(np.float32)
    qs = (v[rng.integers(0, n, q)] * (1 + rng.standard_normal((q, dim)).astype(np.float32) * np.float32(1e-3))).astype(np.float32)
    qs[:16] = v[:16]
    qs[16:32] = (rng.standard_normal((16, dim)) * 50).astype(np.float32)
    ids = np.arange(1, n + 1, dtype=np.int32)
    _, exp = _expect(oracle, v, ids, qs)
    eng = _engine(dim, "bf16")
    eng.vocab_append(v, ids)
    st = _check(eng, qs, exp)
    print(dim, "fallback", st["knn_last_fallback_queries"], "max err / eps", st["knn_max_err_ratio"])
    assert 0.0 < st["knn_max_err_ratio"] < 1.0
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- 8. query blocks and strips
SHAPES_8 = {(128, 500): [12, 8, 1, 8], (128, 512): [12, 8, 1, 8], (128, 513): [24, 4, 2, 4], (128, 1000): [24, 4, 2, 4],      # [tiles per share, shares, query
            (256, 500): [24, 4, 2, 4], (256, 512): [24, 4, 2, 4], (256, 513): [24, 4, 3, 2], (256, 1000): [24, 4, 4, 2]}      #  blocks, workgroups along the rows]


@both
@pytest.mark.parametrize("q", [500, 512, 513, 1000])
def test_query_blocks_and_strips(oracle, dim, mode, q):
    """planned for 8 compute units, 3 000 rows are shares of 12 or 24 tiles walked in strips of 8 (the last share and its last strip are ragged, the
    last tile has 24 rows), two shares per workgroup with three or four query blocks; 512 queries of 128 floats / 256 of 256 floats fill a block, 513
    open another one in which seven waves only convert tiles.  Query i is a noisy copy of row (37 i) mod n: a tile or a query group handled by the wrong wave cannot return the right rows"""
    n = 3000
    tpb, nb, qblocks, group_q, qpad, _, strip, strips, wgs = _plan(q, n, dim, UNITS)
    assert [tpb, nb, qblocks, wgs] == SHAPES_8[(dim, q)] and group_q == 65536 // dim
    n_tiles = (n + 31) // 32
    assert strips >= 2 and (n_tiles - (nb - 1) * tpb) % strip != 0 and n_tiles % tpb != 0 and n % 32 != 0      # several strips, ragged ends
    assert (qblocks >= 2) == (q > group_q)
    rng = np.random.default_rng(100 * dim + q)
    v = synth.vocab_surf(n, seed=q, dim=dim)
    src = (np.arange(q) * 37) % n
    qs = _noisy_rows(rng, v, src, np.float32(0.02))
    ids = np.arange(1, n + 1, dtype=np.int32)
    idx, exp = _expect(oracle, v, ids, qs)
    assert idx[:, 0].tolist() == src.tolist() and len(set(src.tolist())) == q          # every query has a nearest row of its own
    eng = _engine(dim, mode, units=UNITS)
    eng.vocab_append(v, ids)
    st = _check(eng, qs, exp)
    assert st["knn_last_fallback_queries"] <= q // 4
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- 9. word assignment
@both
def test_quantize_and_find_nn(oracle, dim, mode):
    from test_gpu_descriptor_sizes import _dictionary
    n = 1500
    v = synth.vocab_surf(n, seed=21, dim=dim)
    ids = np.arange(1, n + 1, dtype=np.int32)
    desc = synth.queries_surf(v, 120, seed=22)
    exp_words = _dictionary(oracle, v, ids).add_new_words(desc, 1)
    extra = synth.vocab_surf(40, seed=23, dim=dim)         # findNN's not-indexed words: they stay on the exact scan in every mode
    extra_ids = np.arange(n + 1, n + 41, dtype=np.int32)
    fq = np.vstack([synth.queries_surf(v, 80, seed=24), extra[::4]])
    res = {}
    for m in (mode, "valu"):
        eng = _engine(dim, m)
        eng.vocab_append(v, ids)
        eng.profile_begin(2)
        words, n_new = eng.quantize(desc)
        name = eng.profile_read()[2]
        assert name.startswith(NEW_KERNEL) if m == mode else name == "knn2_l2_kernel"
        found = eng.find_nn(fq, extra, extra_ids, incremental=True, nndr=0.8)
        res[m] = (words.tolist(), n_new, found.tolist())
        eng.close()
    assert res[mode] == res["valu"]
    got = np.array(res[mode][0])
    assert np.where(got < 0, n - got, got).tolist() == exp_words
    assert any(w > 0 for w in res[mode][0]) and res[mode][1] > 0 and any(w > n for w in res[mode][2])


@both
@pytest.mark.parametrize("auto_ids", [False, True], ids=["ids-given", "ids-auto"])
def test_frames_with_device_append(oracle, dim, mode, auto_ids):
    """lcd_frame_dev with append_new_words: the search is planned for an upper bound of the row count (a lagging mirror) and the rows behind the
    device's count carry row id 0; against the oracle's Memory::update over the growing dictionary"""
    from test_gpu_append_dev import _oracle_stream, _stream
    args = dict(n_words=1500, q=96, n_frames=12, seed=31 + dim, shape=("f32", dim))
    # the premise, from the oracle alone: some frame matches a word an EARLIER frame created (a row the device appended)
    _, _, _, _, first_new, expected, _ = _oracle_stream(oracle, args["n_words"], args["q"], args["n_frames"], args["seed"], shape=args["shape"])
    assert any(first_new[0] <= w < first_new[t] for t in range(len(expected)) for w in expected[t])
    assert _stream(oracle, False, knn_mode=mode, auto_ids=auto_ids, **args) > 0


# ---------------------------------------------------------------------------------------------------------------- 10. fuzz
def test_fuzz_in_the_modes(oracle):
    """random sizes around the tiles, the strips and the query groups, both row lengths and both arithmetics, plans for 1, 3 and 24 compute units
    and the device's, permuted ids, duplicates, tombstones.  LCD_FUZZ_ITERS raises the number of cases, as in test_gpu_fuzz.py"""
    from test_gpu_fuzz import EDGE_N, EDGE_Q
    iters = int(os.environ.get("LCD_FUZZ_ITERS", "12"))
    rng = np.random.default_rng(6)
    sizes = [n for n in EDGE_N if n >= 256]
    for it in range(iters):
        n, q = int(rng.choice(sizes)), int(rng.choice(EDGE_Q))
        dim, mode = int(rng.choice(DIMS)), str(rng.choice(MODES))
        units = int(rng.choice([-1, 1, 3, 24]))
        v = synth.vocab_surf(n, seed=1000 + it, dim=dim)
        qs = synth.queries_surf(v, q, seed=2000 + it)
        if rng.random() < 0.7:                           # duplicates: ties go to the lower row
            dup = int(rng.integers(0, n))
            v[rng.integers(0, n, 6)] = v[dup]
            qs[rng.integers(0, q)] = v[dup if q >= 8 else rng.integers(0, n)]     # (a query among seven equals may go to the redo: only where the cap admits one)
        ids = rng.permutation(np.arange(1, n + 1)).astype(np.int32) if rng.random() < 0.3 else np.arange(1, n + 1, dtype=np.int32)
        removed = None
        if rng.random() < 0.6:
            removed = np.zeros(n, np.uint8)
            removed[rng.choice(n, size=int(rng.integers(1, n // 3)), replace=False)] = 1
        _, exp = _expect(oracle, v, ids, qs, removed=removed)
        eng = _engine(dim, mode, units=units)
        eng.vocab_append(v, ids)
        if removed is not None:
            eng.vocab_remove(ids[removed == 1])
        msg = "case %d: n=%d q=%d dim=%d mode=%s units=%d plan=%s" % (it, n, q, dim, mode, units, _plan(q, n, dim, units))
        st = _check(eng, qs, exp, msg)
        assert st["knn_last_fallback_queries"] <= q // 4, msg
        eng.close()
