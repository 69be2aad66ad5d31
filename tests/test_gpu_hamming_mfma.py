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


def _check(eng, oracle, vocab, ids, queries, removed=None, expected=None):
    got_ids, got_d = eng.knn2(queries)
    if expected is not None:                             # (the oracle's answer, computed before the engine existed)
        np.testing.assert_array_equal(got_ids, expected[0])
        np.testing.assert_array_equal(got_d, expected[1])
        return got_ids, got_d
    metric = oracle.METRIC_HAMMING_CV if vocab.dtype == np.uint8 else None
    idx, d = oracle.knn2_linear(vocab, queries, removed=removed, metric=metric)
    exp_ids = np.where(idx >= 0, ids[np.maximum(idx, 0)], 0).astype(np.int32)
    np.testing.assert_array_equal(got_ids, exp_ids)
    np.testing.assert_array_equal(got_d, d)
    return got_ids, got_d


def _plan(q, n_rows, dim_bytes, units):
    """knn_hamming_mfma_plan as scan_partial makes it for a handle whose "filter_units" is `units`: [rows per workgroup, workgroups along the rows,
    query groups, rows of a chunk, qpad, partial bytes / 16]"""
    import ctypes as C
    import rtabmap_amd
    rtabmap_amd.load()
    lib = C.CDLL(rtabmap_amd.library_path())
    lib.lcd_debug_hamming_mfma_plan.restype = C.c_int
    lib.lcd_debug_hamming_mfma_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    out = (C.c_int * 6)()
    assert lib.lcd_debug_hamming_mfma_plan(q, n_rows, dim_bytes, units, out) == 0
    return list(out)


def _expect(oracle, vocab, ids, queries, removed=None):
    idx, d = oracle.knn2_linear(vocab, queries, removed=removed, metric=oracle.METRIC_HAMMING_CV)
    return idx, (np.where(idx >= 0, ids[np.maximum(idx, 0)], 0).astype(np.int32), d)


def _mode_engine(dim, units, mode=MODE):
    eng = _engine("u8", dim, knn_mode=mode)
    eng.set_option("filter_units", units)                # (also over a value the whole run was given)
    return eng


def _check_on_the_matrix_cores(eng, vocab, ids, queries, expected):
    """_check, and the launch that answered was the matrix-core kernel's"""
    eng.profile_begin(2)
    got = _check(eng, None, vocab, ids, queries, expected=expected)
    _, n, name = eng.profile_read()
    assert n == 1 and name == NEW_KERNEL
    return got


def _flip(row, bits):
    out = row.copy()
    for b in bits:
        out[b // 8] ^= np.uint8(1 << (b % 8))
    return out


def _noisy_copies(rng, vocab, rows, rate=0.04):
    """a noisy copy of each of `rows`: every bit flipped with probability `rate`"""
    flips = np.packbits(rng.random((len(rows), vocab.shape[1] * 8)) < rate, axis=1)
    return np.ascontiguousarray(vocab[rows] ^ flips)


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


@pytest.mark.parametrize("dim", [32, 64, 128, 4096])
def test_full_distance_range(oracle, dim):
    """every row the bitwise complement of query 0 but one that equals it: distances 0 and 8 * dim (512 needs the tenth bit of the key) --
    a wrong offset or sign in the distance, or operands swapped, cannot survive this.  Up to the longest row the handle admits (4096 bytes, 1024
    K steps of the runtime-K kernel): a live key reaches 127^2 * 2 * 32768, and a tombstoned complement row ends at 127^2 * (4 * 32768 + 1) =
    2 114 076 417, the top of the key's 32 bits -- it is never returned.  The scan of a second engine (which has not run past 64 bytes either)
    agrees bit for bit."""
    rng = np.random.default_rng(dim)
    qs = rng.integers(0, 256, (5, dim), dtype=np.uint8)
    v = np.repeat((~qs[:1]).astype(np.uint8), 300, axis=0)
    v[200] = qs[0]
    ids = np.arange(1, 301, dtype=np.int32)
    some = np.zeros(300, np.uint8); some[:25] = 1; some[100:125] = 1             # 50 dead complement rows, the first rows among them
    all_but_one = np.ones(300, np.uint8); all_but_one[200] = 0
    assert 127 * 127 * (4 * 8 * dim + 1) < 2 ** 31
    res = {}
    for mode in (MODE, "valu"):
        eng = _engine("u8", dim, knn_mode=mode)
        eng.vocab_append(v, ids)
        eng.profile_begin(2)
        got_ids, got_d = _check(eng, oracle, v, ids, qs)
        assert eng.profile_read()[1:] == (1, NEW_KERNEL if mode == MODE else "knn2_hamming_kernel")
        assert got_ids[0].tolist() == [201, 1] and got_d[0].tolist() == [0.0, 8.0 * dim]
        eng.vocab_remove(ids[some == 1])
        some_ids, some_d = _check(eng, oracle, v, ids, qs, removed=some)
        assert some_ids[0].tolist() == [201, 26] and some_d[0].tolist() == [0.0, 8.0 * dim]      # the first LIVE complement row
        eng.vocab_remove(ids[(all_but_one == 1) & (some == 0)])
        one_ids, one_d = _check(eng, oracle, v, ids, qs, removed=all_but_one)
        assert (one_ids == [201, 0]).all() and (one_d[:, 1] == -1.0).all() and one_d[0, 0] == 0.0
        res[mode] = [got_ids, got_d, some_ids, some_d, one_ids, one_d]
        eng.close()
    for a, b in zip(res[MODE], res["valu"]):
        np.testing.assert_array_equal(a, b)


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


# ---------------------------------------------------------------------------------------------------------------- where the launch plan changes shape
# Every case below first asserts, from lcd_debug_hamming_mfma_plan with its own q, rows, row length and units, that the plan has the shape the case
# was written for (chunks per strip, query groups, the clamp): a later change of the plan fails the case instead of moving it off its path.
UNITS = 8                                                # lcd_set_option("filter_units"): a multi-chunk plan at 3 000 rows


def _chunk_pipeline_case(rng, n, dim, q, rpb, chunk):
    """A vocabulary of n random rows with planted neighbours around the chunks of the strips of `rpb` rows, the queries that look for them (the rest:
    noisy copies of row (i * 37) % n), the tombstones of the second search, and what the oracle must answer: [query, tombstones?, rows]"""
    v = rng.integers(0, 256, (n, dim), dtype=np.uint8)
    qs = _noisy_copies(rng, v, (np.arange(q) * 37) % n)
    last0 = (n - 1) // rpb * rpb                         # the last strip, and its last, partial chunk
    tail0 = last0 + (n - 1 - last0) // chunk * chunk
    assert rpb >= 3 * chunk and 1 < n - tail0 < chunk and tail0 > last0 and last0 >= 6 * rpb
    removed = np.zeros(n, np.uint8)
    want = []

    def plant(qi, near):                                 # near: (row, bits that differ from the query)
        qs[qi] = rng.integers(0, 256, dim, dtype=np.uint8)
        for r, bits in near:
            v[r] = _flip(qs[qi], bits)

    # the two nearest rows in different chunks of one strip, in either order
    plant(0, [(rpb + 5, [0]), (rpb + 2 * chunk + 7, [1, 2])])
    want.append((0, False, [rpb + 5, rpb + 2 * chunk + 7]))
    plant(1, [(rpb + 2 * chunk + 9, [3]), (rpb + 3, [4, 5])])
    want.append((1, False, [rpb + 2 * chunk + 9, rpb + 3]))
    # both in the last, partial chunk of the last strip: its second row and the last row there is
    plant(2, [(n - 1, [6]), (tail0 + 1, [7, 8])])
    want.append((2, False, [n - 1, tail0 + 1]))
    # the last row of a chunk and the first row of the next at equal distance: the lower row wins (second to third chunk: the first LDS buffer again)
    plant(3, [(2 * rpb + chunk - 1, [0, 1, 2]), (2 * rpb + chunk, [3, 4, 5])])
    want.append((3, False, [2 * rpb + chunk - 1, 2 * rpb + chunk]))
    plant(4, [(2 * rpb + 2 * chunk, [0, 1, 2]), (2 * rpb + 2 * chunk - 1, [3, 4, 5])])
    want.append((4, False, [2 * rpb + 2 * chunk - 1, 2 * rpb + 2 * chunk]))
    # tombstones over one whole chunk, the query's nearest row in it: the answer is in the chunk behind it and in the next strip
    plant(5, [(3 * rpb + chunk + 11, [9]), (3 * rpb + 2 * chunk + 2, [10, 11]), (4 * rpb + 10, [12, 13, 14])])
    removed[3 * rpb + chunk:3 * rpb + 2 * chunk] = 1
    want.append((5, False, [3 * rpb + chunk + 11, 3 * rpb + 2 * chunk + 2]))
    want.append((5, True, [3 * rpb + 2 * chunk + 2, 4 * rpb + 10]))
    # a tombstone on the nearest row, which is the first of its chunk
    plant(6, [(5 * rpb + 2 * chunk, [15]), (5 * rpb + 2 * chunk + 1, [16, 17]), (5 * rpb + 1, [18, 19, 20])])
    removed[5 * rpb + 2 * chunk] = 1
    want.append((6, False, [5 * rpb + 2 * chunk, 5 * rpb + 2 * chunk + 1]))
    want.append((6, True, [5 * rpb + 2 * chunk + 1, 5 * rpb + 1]))
    return v, qs, removed, want


def _run_chunk_pipeline(oracle, n, dim, q, units, plan, with_an_engine=None):
    rpb, nb, groups, chunk = plan[:4]
    rng = np.random.default_rng(1000 * dim + q)
    v, qs, removed, want = _chunk_pipeline_case(rng, n, dim, q, rpb, chunk)
    ids = np.arange(1, n + 1, dtype=np.int32)
    idx0, exp0 = _expect(oracle, v, ids, qs)
    idx1, exp1 = _expect(oracle, v, ids, qs, removed=removed)
    for qi, dead, rows in want:                          # the planted rows are the two nearest, by the oracle alone
        assert (idx1 if dead else idx0)[qi].tolist() == rows, (qi, dead)
    assert exp0[1][3, 0] == exp0[1][3, 1] == 3 and exp0[1][4, 0] == exp0[1][4, 1] == 3      # the ties are ties
    eng = _mode_engine(dim, units)
    if with_an_engine:
        with_an_engine()
    eng.vocab_append(v, ids)
    _check_on_the_matrix_cores(eng, v, ids, qs, exp0)
    eng.vocab_remove(ids[removed == 1])
    _check_on_the_matrix_cores(eng, v, ids, qs, exp1)
    eng.close()


@pytest.mark.parametrize("dim,q,plan", [(32, 130, [192, 16, 1, 64]), (8, 130, [192, 16, 1, 64]), (16, 130, [192, 16, 1, 64]), (64, 300, [384, 8, 2, 32])])
def test_chunk_pipeline(oracle, dim, q, plan):
    """strips of 3 chunks (12 at 64 bytes, with two query groups): every chunk after the first is fetched and expanded into the other LDS buffer behind
    the products of the one before it, the third reuses the first buffer; the last strip ends in a partial chunk"""
    n = 3000
    assert _plan(q, n, dim, UNITS)[:4] == plan and plan[0] // plan[3] >= 3 and n % plan[0] % plan[3] != 0
    _run_chunk_pipeline(oracle, n, dim, q, UNITS, plan)


def test_chunk_pipeline_at_the_device_plan(oracle):
    """the same with no knob: a multi-chunk grid planned for the compute units the device has (365 strips of 192 rows on 256 units)"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    q, dim = 130, 32
    n = 2 * cus * 136 + 369                              # 137 rows and more per workgroup: strips of three chunks ...
    n -= (n - 113) % 192                                 # ... the last of 113 rows: a whole chunk and a partial one (70 001 rows on 256 units)
    plan = _plan(q, n, dim, cus)
    if cus == 256:
        assert n == 70001 and plan[:4] == [192, 365, 1, 64]
    assert plan[0] // plan[3] >= 3 and n % plan[0] % plan[3] != 0 and plan[1] >= 7

    def the_engine_plans_for_the_device():               # lcd_create has read the device's count: what a handle without the option plans for
        assert _plan(q, n, dim, -1) == plan
    _run_chunk_pipeline(oracle, n, dim, q, -1, plan, with_an_engine=the_engine_plans_for_the_device)


@pytest.mark.parametrize("dim,q,plan", [(32, 500, [192, 16, 1, 64]), (32, 512, [192, 16, 1, 64]), (32, 513, [384, 8, 2, 64]), (32, 577, [384, 8, 2, 64]),
                                        (32, 1000, [384, 8, 2, 64]), (64, 257, [384, 8, 2, 32]), (64, 300, [384, 8, 2, 32]), (24, 97, [384, 8, 2, 128]),
                                        (24, 65, [384, 8, 2, 128])])
def test_query_groups_and_tiles(oracle, dim, q, plan):
    """every wave with its full four query tiles and a ragged last one (500), a second query group (blockIdx.y = 1) of one tile on wave 0 while three
    waves only stage (513), of two tiles (577), a full one (1000); groups of 256 at 64 bytes and of 64 in the runtime-K kernel.  Query i is a noisy copy
    of row (i * 37) % n: a tile read or stored by the wrong wave cannot return the right rows"""
    n = 3000
    assert _plan(q, n, dim, UNITS)[:4] == plan
    rng = np.random.default_rng(100 * dim + q)
    v = rng.integers(0, 256, (n, dim), dtype=np.uint8)
    src = (np.arange(q) * 37) % n
    qs = _noisy_copies(rng, v, src)
    ids = np.arange(1, n + 1, dtype=np.int32)
    idx, exp = _expect(oracle, v, ids, qs)
    assert idx[:, 0].tolist() == src.tolist() and len(set(src.tolist())) == q      # every query has a nearest row of its own
    eng = _mode_engine(dim, UNITS)
    eng.vocab_append(v, ids)
    _check_on_the_matrix_cores(eng, v, ids, qs, exp)
    eng.close()


@pytest.mark.parametrize("dim,groups,chunk", [(32, 1, 64), (8, 1, 64), (24, 2, 128)])
def test_largest_row_offset_of_the_key(oracle, dim, groups, chunk):
    """planned for one compute unit, 33 000 rows are strips of MAX_BLOCK_ROWS = 16 128 rows (the clamp: 16 512 without it), the last of 744: the row
    offset inside the key reaches 16 127, one below KM = 127 * 127 where it would spill into the distance"""
    n, q, top = 33000, 70, 16127
    assert _plan(q, n, dim, 1)[:4] == [16128, 3, groups, chunk] and n - 2 * 16128 == 744
    rng = np.random.default_rng(dim)
    ids = np.arange(1, n + 1, dtype=np.int32)
    base = rng.integers(0, 256, (n, dim), dtype=np.uint8)
    near = np.concatenate([np.arange(16100, 16160), np.arange(32990, 33000)])     # noisy copies of the rows around the seam of two strips, and of the last rows
    qs0 = _noisy_copies(rng, base, near)
    assert len(qs0) == q

    # an exact duplicate on either side of the seam (offset 16 127, then offset 0 of the next strip), and row 0 as near as row 16 127
    va, qa = base.copy(), qs0.copy()
    va[top + 1] = va[top]
    qa[0] = va[top]
    qa[1] = _flip(va[top], [0, 1, 2])
    va[0] = _flip(qa[1], [3, 4, 5])
    idx, exp_a = _expect(oracle, va, ids, qa)
    assert idx[0].tolist() == [top, top + 1] and exp_a[1][0].tolist() == [0.0, 0.0]
    assert idx[1].tolist() == [0, top] and exp_a[1][1].tolist() == [3.0, 3.0]     # equal distance: offset 0 before offset 16 127
    eng = _mode_engine(dim, 1)
    eng.vocab_append(va, ids)
    _check_on_the_matrix_cores(eng, va, ids, qa, exp_a)
    eng.close()

    # row 16 127 at distance 2, row 0 at distance 3: the distance outranks the offset; then the same with row 16 127 dead
    vb, qb = base.copy(), qs0.copy()
    qb[0] = _flip(vb[top], [0, 1])
    vb[0] = _flip(qb[0], [2, 3, 4])
    vb[n - 1] = _flip(qb[0], [5, 6, 7, 8])
    removed = np.zeros(n, np.uint8); removed[top] = 1
    idx, exp_b = _expect(oracle, vb, ids, qb)
    idx_dead, exp_dead = _expect(oracle, vb, ids, qb, removed=removed)
    assert idx[0].tolist() == [top, 0] and exp_b[1][0].tolist() == [2.0, 3.0]
    assert idx_dead[0].tolist() == [0, n - 1] and exp_dead[1][0].tolist() == [3.0, 4.0]
    eng = _mode_engine(dim, 1)
    eng.vocab_append(vb, ids)
    _check_on_the_matrix_cores(eng, vb, ids, qb, exp_b)
    eng.vocab_remove(ids[removed == 1])
    _check_on_the_matrix_cores(eng, vb, ids, qb, exp_dead)
    eng.close()


def test_frame_of_600_descriptors_in_two_query_groups(oracle):
    """lcd_frame_dev in the mode (engine.hip's Hamming frame: the matrix-core scan, then knn2_merge_selfdist_hamming_kernel) with two query groups over
    strips of six chunks; same-frame duplicates 500 descriptors apart; against the oracle's addNewWords and against lcd_quantize on the same handle"""
    n, q = 3000, 600
    assert _plan(q, n, 32, UNITS)[:4] == [384, 8, 2, 64]
    v = synth.vocab_orb(n, seed=41)
    qs = synth.queries_orb(v, q, seed=42, frac_known=0.6)
    qs[500:540] = qs[0:40]                               # duplicates of matched and of fresh descriptors, in the other query group
    ids = np.arange(1, n + 1, dtype=np.int32)
    m = oracle.OracleVWDictionary(strategy=oracle.kNNBruteForce, nndr=0.8, new_words_compared_together=True)
    for i, r in zip(ids, v):
        m.add_word(int(i), r)
    m.update()
    exp = m.add_new_words(qs, 1)
    assert any(exp[i] > n and exp[500 + i] == exp[i] for i in range(40))        # a duplicate joins the word its first copy created ...
    assert any(0 < exp[i] <= n and exp[500 + i] == exp[i] for i in range(40))   # ... or matched
    assert any(w > n for w in exp[540:]) and any(w <= n for w in exp[540:])
    import rtabmap_amd
    eng = rtabmap_amd.Engine("u8", 32, sig_capacity=64, knn_mode=MODE)
    eng.set_option("filter_units", UNITS)
    eng.vocab_append(v, ids)
    got, n_new = eng.quantize(qs, incremental=True, new_words_compared=True, nndr=0.8)
    d = torch.from_numpy(qs).cuda()
    d_words = torch.zeros(q, dtype=torch.int32, device="cuda")
    eng.profile_begin(2)
    eng.frame_dev(d.data_ptr(), q, 0, 10.0, d_words.data_ptr(), 0, 0, incremental=True, new_words_compared=True, nndr=0.8)
    torch.cuda.synchronize()
    assert eng.profile_read()[1:] == (1, NEW_KERNEL)
    assert np.where(got < 0, n - got, got).tolist() == exp
    assert d_words.cpu().numpy().tolist() == got.tolist()
    assert n_new == len({e for e in exp if e > n})
    eng.close()


def test_frames_grow_the_vocabulary_across_a_strip_boundary(oracle):
    """frames of 520 descriptors (two query groups) that append their words on the device: 3 100 rows are 7 strips of 448; the row count the scan is
    planned for passes 3 136 (an eighth strip), then 3 584 (strips of 512)"""
    from test_gpu_append_dev import _oracle_stream, _stream
    args = dict(n_words=3100, q=520, n_frames=6, seed=57, kind="orb")
    _, _, _, _, first_new, expected, _ = _oracle_stream(oracle, args["n_words"], args["q"], args["n_frames"], args["seed"], args["kind"])
    rows = [f - 1 for f in first_new]                    # the rows in front of every frame (ids are handed out in row order)
    plans = [_plan(args["q"], r, 32, UNITS) for r in rows]
    assert rows[0] == 3100 and plans[0][:3] == [448, 7, 2] and plans[-1][2] == 2
    assert plans[-1][1] != plans[0][1] and plans[-1][0] > plans[0][0], plans
    assert any(first_new[0] <= w < first_new[t] for t in range(len(expected)) for w in expected[t])   # a frame matches a row the device appended
    assert _stream(oracle, False, knn_mode=MODE, options={"filter_units": UNITS}, **args) >= rows[-1] - rows[0]


def test_fuzz_in_the_mode(oracle):
    """random sizes around the tiles, the chunks and the largest strip, every kind of row length, plans for 1, 3 and 24 compute units and the device's,
    tombstones and duplicates.  LCD_FUZZ_ITERS raises the number of cases, as in test_gpu_fuzz.py"""
    import os
    from test_gpu_fuzz import EDGE_N, EDGE_Q
    iters = int(os.environ.get("LCD_FUZZ_ITERS", "12"))
    rng = np.random.default_rng(6)
    sizes = [n for n in EDGE_N if n >= 256] + [16127, 16128, 16129]
    for it in range(iters):
        n, q = int(rng.choice(sizes)), int(rng.choice(EDGE_Q))
        nbytes = int(rng.choice([8, 16, 24, 32, 61, 64, 128]))
        units = int(rng.choice([-1, 1, 3, 24]))
        v = rng.integers(0, 256, (n, nbytes), dtype=np.uint8)
        qs = _noisy_copies(rng, v, rng.integers(0, n, q), rate=0.1)
        if rng.random() < 0.7:                           # duplicates: ties go to the lower row
            v[rng.integers(0, n, 6)] = v[rng.integers(0, n)]
            qs[rng.integers(0, q)] = v[rng.integers(0, n)]
        ids = rng.permutation(np.arange(1, n + 1)).astype(np.int32) if rng.random() < 0.3 else np.arange(1, n + 1, dtype=np.int32)
        removed = None
        if rng.random() < 0.6:
            removed = np.zeros(n, np.uint8)
            removed[rng.choice(n, size=int(rng.integers(1, n // 3)), replace=False)] = 1
        _, exp = _expect(oracle, v, ids, qs, removed=removed)
        eng = _mode_engine(nbytes, units)
        eng.vocab_append(v, ids)
        if removed is not None:
            eng.vocab_remove(ids[removed == 1])
        eng.profile_begin(2)
        got_ids, got_d = eng.knn2(qs)
        assert eng.profile_read()[1:] == (1, NEW_KERNEL)
        msg = "case %d: n=%d q=%d nbytes=%d units=%d plan=%s" % (it, n, q, nbytes, units, _plan(q, n, nbytes, units))
        np.testing.assert_array_equal(got_d, exp[1], err_msg=msg)
        np.testing.assert_array_equal(got_ids, exp[0], err_msg=msg)
        eng.close()
