"""GPU parity of LCD_KNN_HAMMING_MFMA: the Hamming 2-NN of a u8 handle's main vocabulary computed on the i8 matrix cores
(knn_hamming_mfma.hip) against the CPU oracle's linear scan and against the exact vector-ALU scan of a second engine.  The distances
are integers and the kernel computes them exactly: every comparison is assert_array_equal on word ids and distances."""
import numpy as np
import pytest
import torch

from rtabmap_amd import synth

pytestmark = pytest.mark.gpu

MODE = "hamming_mfma"
NEW_KERNEL = "knn2_hamming_mfma_kernel"


def _engine(dtype, dim, **kw):
    import rtabmap_amd
    return rtabmap_amd.Engine(dtype, dim, **kw)


def _check(eng, oracle, vocab, ids, queries, removed=None):
    got_ids, got_d = eng.knn2(queries)
    metric = oracle.METRIC_HAMMING_CV if vocab.dtype == np.uint8 else None
    idx, d = oracle.knn2_linear(vocab, queries, removed=removed, metric=metric)
    exp_ids = np.where(idx >= 0, ids[np.maximum(idx, 0)], 0).astype(np.int32)
    np.testing.assert_array_equal(got_ids, exp_ids)
    np.testing.assert_array_equal(got_d, d)
    return got_ids, got_d


def _kernel_of_a_search(n_rows, q):
    v = synth.vocab_orb(n_rows, seed=2)
    qs = synth.queries_orb(v, q, seed=3)
    eng = _engine("u8", 32, knn_mode=MODE)
    eng.vocab_append(v, np.arange(1, n_rows + 1, dtype=np.int32))
    d_q = torch.from_numpy(qs).cuda()
    d_w = torch.zeros((q, 2), dtype=torch.int32, device="cuda")
    d_d = torch.zeros((q, 2), dtype=torch.float32, device="cuda")
    eng.profile_begin(4)
    eng.knn2_dev(d_q.data_ptr(), q, d_w.data_ptr(), d_d.data_ptr())
    eng.synchronize()
    ms, n, name = eng.profile_read()
    eng.close()
    return n, name


def test_which_kernel_ran():
    """Without this every other test here could pass on a silent fall-back to the scan."""
    n, name = _kernel_of_a_search(1000, 70)
    assert n == 1 and name == NEW_KERNEL
    n, name = _kernel_of_a_search(255, 70)               # below 256 rows the mode uses the exact scan, as the float matrix-core modes do
    assert n == 1 and name == "knn2_hamming_kernel"


@pytest.mark.parametrize("n,q", [(256, 1), (257, 33), (1000, 64), (4097, 130), (9973, 65)])
def test_ragged_sizes(oracle, n, q):
    """the last rows of a tile, a chunk and a workgroup's strip, and the last queries of a tile"""
    v = synth.vocab_orb(n, seed=n)
    qs = synth.queries_orb(v, q, seed=q)
    ids = np.arange(1, n + 1, dtype=np.int32)
    eng = _engine("u8", 32, knn_mode=MODE)
    eng.vocab_append(v, ids)
    _check(eng, oracle, v, ids, qs)
    eng.close()


@pytest.mark.parametrize("dim", [32, 64])
def test_full_distance_range(oracle, dim):
    """every row the bitwise complement of query 0 but one that equals it: distances 0 and 8 * dim (512 needs the tenth bit of the key) --
    a wrong offset or sign in the distance, or operands swapped, cannot survive this"""
    rng = np.random.default_rng(dim)
    qs = rng.integers(0, 256, (5, dim), dtype=np.uint8)
    v = np.repeat((~qs[:1]).astype(np.uint8), 300, axis=0)
    v[200] = qs[0]
    ids = np.arange(1, 301, dtype=np.int32)
    eng = _engine("u8", dim, knn_mode=MODE)
    eng.vocab_append(v, ids)
    got_ids, got_d = _check(eng, oracle, v, ids, qs)
    assert got_ids[0].tolist() == [201, 1] and got_d[0].tolist() == [0.0, 8.0 * dim]
    eng.close()


def test_ties_lowest_row_wins(oracle):
    rng = np.random.default_rng(5)
    v = rng.integers(0, 4, (6000, 32), dtype=np.uint8)
    v[3000:] = v[:3000]                                  # every row has an exact duplicate later on
    q = rng.integers(0, 4, (200, 32), dtype=np.uint8)
    ids = np.arange(1, 6001, dtype=np.int32)
    eng = _engine("u8", 32, knn_mode=MODE)
    eng.vocab_append(v, ids)
    got_ids, got_d = _check(eng, oracle, v, ids, q)
    assert (got_d[:, 0] == got_d[:, 1]).any() and (got_ids[:, 0] <= 3000).all()
    eng.close()


def test_tombstones_and_rebuild(oracle):
    n = 3000
    v = synth.vocab_orb(n, seed=3)
    q = synth.queries_orb(v, 150, seed=4)
    ids = np.arange(10, n + 10, dtype=np.int32)
    eng = _engine("u8", 32, knn_mode=MODE)
    eng.vocab_append(v, ids)
    got_ids, _ = _check(eng, oracle, v, ids, q)
    rng = np.random.default_rng(9)
    removed = np.zeros(n, np.uint8)
    removed[rng.choice(n, 700, replace=False)] = 1
    removed[640:672] = 1                                 # two whole aligned 32-row tiles
    removed[2048:2080] = 1
    removed[got_ids[:10, 0] - 10] = 1                    # the current nearest row of ten queries
    eng.vocab_remove(ids[removed == 1])
    _check(eng, oracle, v, ids, q, removed=removed)      # tombstoned rows are never returned
    keep = removed == 0
    # all rows but one: the second neighbour does not exist
    survivor = int(np.flatnonzero(keep)[1234])
    gone = keep.copy(); gone[survivor] = False
    eng.vocab_remove(ids[gone])
    all_but_one = np.ones(n, np.uint8); all_but_one[survivor] = 0
    one_ids, one_d = _check(eng, oracle, v, ids, q, removed=all_but_one)
    assert (one_ids[:, 0] == ids[survivor]).all() and (one_ids[:, 1] == 0).all() and (one_d[:, 1] == -1.0).all()
    eng.close()
    # a rebuild compacts the rows: the same search over the survivors of the first removal
    eng = _engine("u8", 32, knn_mode=MODE)
    eng.vocab_append(v, ids)
    eng.vocab_remove(ids[removed == 1])
    eng.vocab_rebuild()
    assert eng.vocab_count() == (int(keep.sum()), int(keep.sum()))
    _check(eng, oracle, v[keep], ids[keep], q)
    eng.close()


@pytest.mark.parametrize("dim", [8, 16, 24, 64, 33, 61])
def test_other_descriptor_sizes(oracle, dim):
    """rows of 2, 4, 6, 16 and 9 dwords, and rows the handle zero-pads on the device (33 -> 36, 61 -> 64 bytes): host rows in, as the
    padded handles are served"""
    rng = np.random.default_rng(dim)
    v = rng.integers(0, 256, (1500, dim), dtype=np.uint8)
    q = rng.integers(0, 256, (97, dim), dtype=np.uint8)
    q[:20] = v[rng.integers(0, 1500, 20)]                # some exact hits, some near ones
    flips = ((rng.random((20, dim)) < 0.1) * (1 << rng.integers(0, 8, (20, dim)))).astype(np.uint8)
    q[20:40] = v[rng.integers(0, 1500, 20)] ^ flips
    ids = np.arange(1, 1501, dtype=np.int32)
    eng = _engine("u8", dim, knn_mode=MODE)
    eng.vocab_append(v, ids)
    got = _check(eng, oracle, v, ids, q)
    eng.close()
    ref = _engine("u8", dim, knn_mode="valu")
    ref.vocab_append(v, ids)
    exp = ref.knn2(q)
    ref.close()
    np.testing.assert_array_equal(got[0], exp[0])
    np.testing.assert_array_equal(got[1], exp[1])


@pytest.mark.parametrize("auto_ids", [False, True])
def test_frames_with_device_append(oracle, auto_ids):
    """lcd_frame_dev on a u8 handle whose frames append their words on the device: the scan is planned for an upper bound of the row count and the
    rows behind the device's count carry row id 0; against the oracle's addNewWords over the growing dictionary"""
    from test_gpu_append_dev import _oracle_stream, _stream
    args = dict(n_words=1500, q=96, n_frames=20, seed=31, kind="orb")
    # the premise, from the oracle alone: some frame matches a word an EARLIER frame created (a row the device appended)
    _, _, _, _, first_new, expected, _ = _oracle_stream(oracle, args["n_words"], args["q"], args["n_frames"], args["seed"], args["kind"])
    assert any(first_new[0] <= w < first_new[t] for t in range(len(expected)) for w in expected[t])
    assert _stream(oracle, False, knn_mode=MODE, auto_ids=auto_ids, **args) > 100


def test_quantize_and_find_nn_match_the_scan(oracle):
    n = 2000
    v = synth.vocab_orb(n, seed=21)
    ids = np.arange(1, n + 1, dtype=np.int32)
    desc = synth.queries_orb(v, 120, seed=22)
    extra = synth.vocab_orb(40, seed=23)                 # findNN's not-indexed words: they stay on the exact scan in every mode
    extra_ids = np.arange(n + 1, n + 41, dtype=np.int32)
    fq = np.vstack([synth.queries_orb(v, 80, seed=24), extra[::4]])
    res = {}
    for mode in (MODE, "valu"):
        eng = _engine("u8", 32, knn_mode=mode)
        eng.vocab_append(v, ids)
        words, n_new = eng.quantize(desc)
        found = eng.find_nn(fq, extra, extra_ids, incremental=True, nndr=0.8)
        res[mode] = (words.tolist(), n_new, found.tolist())
        eng.close()
    assert res[MODE] == res["valu"]
    assert any(w > 0 for w in res[MODE][0]) and res[MODE][1] > 0 and any(w > n for w in res[MODE][2])


def test_f32_handle_with_the_mode(oracle):
    """on an LCD_F32 handle the value means LCD_KNN_DEFAULT"""
    v = synth.vocab_surf(300, seed=7)
    q = synth.queries_surf(v, 50, seed=8)
    ids = np.arange(1, 301, dtype=np.int32)
    eng = _engine("f32", 64, knn_mode=MODE)
    eng.vocab_append(v, ids)
    got = _check(eng, oracle, v, ids, q)
    eng.close()
    ref = _engine("f32", 64, knn_mode="default")
    ref.vocab_append(v, ids)
    exp = ref.knn2(q)
    ref.close()
    np.testing.assert_array_equal(got[0], exp[0])
    np.testing.assert_array_equal(got[1], exp[1])
