"""GPU tests of lcd_select_features / lcd_expand_word_ids and their _dev forms (rtabmap_amd/csrc/feature_select.hip) against
tests/feature_select_model.py.  Every comparison is exact."""
import numpy as np
import pytest
import torch

import feature_select_inputs as I
import feature_select_model as M

pytestmark = pytest.mark.gpu

LCD_ERR_INVALID, LCD_ERR_UNSUPPORTED = 1, 5
ORDERS = (M.KEEP_ORDER, M.BY_RESPONSE)


def _padded(dtype, dim):
    return dtype == "u8" and dim % 4 != 0


def _refused(status, call, *args, **kw):
    from rtabmap_amd import capi
    with pytest.raises(capi.LcdError) as err:
        call(*args, **kw)
    assert err.value.status == status, err.value


@pytest.mark.parametrize("dtype,dim", I.KINDS)
def test_both_entries_equal_the_model(dtype, dim):
    """every frame size in ONE batch (0, 1, around 64, 1024 and 2048, and 16384 features), heavy ties, max 1 / 64 / 500, both orders, rows and
    a payload of 12 or 28 bytes gathered; a padded handle's device entry refuses rows and serves the rest"""
    import rtabmap_amd
    rng = np.random.default_rng(dim)
    frames = [I.tied_frame(rng, n) for n in I.SIZES]
    n_all = sum(I.SIZES)
    rows = I.rows_of(rng, dtype, dim, n_all)
    aux = rng.integers(0, 256, (n_all, 12 if dim == 64 else 28), dtype=np.uint8)
    eng = rtabmap_amd.Engine(dtype, dim)
    for mx in (1, 64, 500):
        for order in ORDERS:
            what = "%s max %d" % (order, mx)
            I.assert_same(I.run_host(eng, frames, mx, order, rows=rows, aux=aux), frames, mx, order, rows=rows, aux=aux, what=what + " host")
            if _padded(dtype, dim):
                _refused(LCD_ERR_UNSUPPORTED, I.run_dev, eng, frames, mx, order, rows=rows, aux=aux)
                I.assert_same(I.run_dev(eng, frames, mx, order, aux=aux), frames, mx, order, aux=aux, device=True, what=what + " dev, no rows")
            else:
                I.assert_same(I.run_dev(eng, frames, mx, order, rows=rows, aux=aux), frames, mx, order, rows=rows, aux=aux, device=True, what=what + " dev")
    assert eng.vocab_count() == (0, 0) and eng.sig_count() == (0, 0)
    eng.close()


def test_max_of_n_minus_one_and_n_and_the_default_shapes():
    """max == n - 1 cuts one feature, max == n cuts nothing (and BY_RESPONSE then keeps the frame's order); 1000 -> 500 and 5000 -> 1000
    with the cut inside a group of equal responses, with all responses equal and with distinct ones; every optional pointer NULL"""
    import rtabmap_amd
    rng = np.random.default_rng(2)
    eng = rtabmap_amd.Engine("f32", 64)
    for n in (2, 64, 65, 1025, 2049, 16384):
        f = [I.tied_frame(rng, n)]
        for mx in (n - 1, n):
            for order in ORDERS:
                I.assert_same(I.run_dev(eng, f, mx, order), f, mx, order, device=True, what="n %d max %d %s" % (n, mx, order))
    for n, mx in ((1000, 500), (5000, 1000)):
        frames = [I.cut_in_tie_frame(rng, n, mx), I.all_equal_frame(n), I.distinct_frame(rng, n)]
        rows = I.rows_of(rng, "f32", 64, 3 * n)
        aux = rng.integers(0, 256, (3 * n, 32), dtype=np.uint8)            # a payload that is copied as 16-byte vectors
        for order in ORDERS:
            I.assert_same(I.run_dev(eng, frames, mx, order, rows=rows, aux=aux), frames, mx, order, rows=rows, aux=aux, device=True,
                          what="%d -> %d %s dev" % (n, mx, order))
            I.assert_same(I.run_host(eng, frames, mx, order), frames, mx, order, what="%d -> %d %s host" % (n, mx, order))
    eng.close()


@pytest.mark.parametrize("grid,size", I.GRIDS)
def test_grids(grid, size):
    """perCell 31 / 33, 12 / 13, 1 and 0; every cell state; a small frame that takes the whole-frame early exit although one of its points is
    outside the grid; on the device entry points outside the grid are never selected, the host entry refuses them"""
    import rtabmap_amd
    rng = np.random.default_rng(grid[1])
    eng = rtabmap_amd.Engine("f32", 64)
    for mx in (500, 200, 16, 15):
        frames = [I.grid_frame(rng, 1000, size, grid, mx), I.grid_frame(rng, 2049, size, grid, mx), I.grid_frame(rng, 10, size, grid, 16, outside=1)]
        assert len(frames[2]["response"]) == 11 <= mx and "outside" in I.cell_states(frames[2], grid, mx)
        if mx >= 200:
            assert {"empty", "under", "at", "over"} <= I.cell_states(frames[0], grid, mx)
        rows = I.rows_of(rng, "f32", 64, sum(len(f["response"]) for f in frames))
        I.assert_same(I.run_host(eng, frames, mx, grid=grid, rows=rows), frames, mx, grid=grid, rows=rows, what="host max %d" % mx)
        I.assert_same(I.run_dev(eng, frames, mx, grid=grid, rows=rows), frames, mx, grid=grid, rows=rows, device=True, what="dev max %d" % mx)
        wild = [I.grid_frame(rng, 1000, size, grid, mx, outside=8)]
        I.assert_same(I.run_dev(eng, wild, mx, grid=grid), wild, mx, grid=grid, device=True, what="dev, points outside, max %d" % mx)
        _refused(LCD_ERR_INVALID, I.run_host, eng, wild, mx, grid=grid)
    eng.close()


def test_nan_responses_on_the_device_entry():
    import rtabmap_amd
    rng = np.random.default_rng(4)
    f = I.tied_frame(rng, 300)
    f["response"][::7] = np.nan
    f["response"][3::11] = np.inf
    f["response"][5::13] = -np.nan
    eng = rtabmap_amd.Engine("f32", 64)
    for order in ORDERS:
        I.assert_same(I.run_dev(eng, [f], 60, order), [f], 60, order, device=True, what=order)
    _refused(LCD_ERR_INVALID, I.run_host, eng, [f], 60)
    eng.close()


@pytest.mark.parametrize("dtype,dim", [("f32", 64), ("u8", 32)])
def test_700_tiny_frames_in_one_call(dtype, dim):
    import rtabmap_amd
    rng = np.random.default_rng(7)
    frames = [I.tied_frame(rng, int(rng.integers(0, 9))) for _ in range(700)]
    n_all = sum(len(f["response"]) for f in frames)
    rows = I.rows_of(rng, dtype, dim, n_all)
    eng = rtabmap_amd.Engine(dtype, dim)
    for order in ORDERS:
        count = M.select_batch(frames, 3, order)[0]
        assert (count == 3).sum() > 100 and (count < 3).sum() > 100
        I.assert_same(I.run_dev(eng, frames, 3, order, rows=rows), frames, 3, order, rows=rows, device=True, what=order + " dev")
        I.assert_same(I.run_host(eng, frames, 3, order, rows=rows), frames, 3, order, rows=rows, what=order + " host")
    eng.close()


def test_scratch_is_counted_and_reused_between_unsynchronised_calls():
    """two device calls in a row without a synchronisation in between (the second takes the other job-table slot), a third that reuses the
    first slot; the host entry's staging is counted in lcd_stats.bytes_device"""
    import rtabmap_amd
    rng = np.random.default_rng(8)
    a = [I.tied_frame(rng, 65)]
    b = [I.tied_frame(rng, 1025), I.tied_frame(rng, 300), a[0]]
    eng = rtabmap_amd.Engine("f32", 64)
    bytes0 = eng.stats()["bytes_device"]
    staged = [I.stage_dev(f) for f in (a, b, a)]
    outs = [I.launch_dev(eng, st, 64) for st in staged]
    for o, f in zip(outs, (a, b, a)):
        I.assert_same(I.to_host(eng, o), f, 64, device=True)
    bytes1 = eng.stats()["bytes_device"]
    assert bytes1 > bytes0                                                 # the job table
    I.run_dev(eng, a, 64)
    assert eng.stats()["bytes_device"] == bytes1                           # ... reused
    I.assert_same(I.run_host(eng, b, 64), b, 64)
    assert eng.stats()["bytes_device"] > bytes1                            # the staged inputs and results
    eng.close()


def _expand_dev(eng, off, count, index, word_ids, first):
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()
    out = torch.full((int(off[-1]),), I.CANARY, dtype=torch.int32, device="cuda")
    d = [dev(x) for x in (count, index, word_ids, first)]
    torch.cuda.synchronize()
    eng.expand_word_ids_dev(off, d[0], d[1], d[2], out, d[3])
    eng.synchronize()
    return out.cpu().numpy()


def test_expansion_both_entries_equal_the_model():
    """frames of 0 .. 16384 features in one batch; count == 0 and count == n among them; ids, codes and zeros; with first ids, with first
    ids <= 0 and with a NULL array; on the device entry indices outside the frame and counts beyond it are skipped / clamped"""
    import rtabmap_amd
    rng = np.random.default_rng(10)
    sizes = [0, 1, 64, 65, 500, 1025, 2049, 16384, 300, 300]
    counts = [0, 1, None, None, None, None, None, None, 0, 300]
    ex = [I.expansion_frame(rng, n, c) for n, c in zip(sizes, counts)]
    off = np.cumsum([0] + sizes).astype(np.int64)
    count = np.array([e["count"] for e in ex], np.int32)
    index = np.full(int(off[-1]), -9, np.int32)
    word_ids = np.full(int(off[-1]), 77, np.int32)                        # behind a frame's count: never read
    for f, e in enumerate(ex):
        index[off[f]:off[f] + e["count"]] = e["index"]
        word_ids[off[f]:off[f] + e["count"]] = e["word_ids"]
    first = np.array([9000 + 100 * f for f in range(len(ex))], np.int32)
    first[4] = 0
    first[5] = -3
    eng = rtabmap_amd.Engine("f32", 64)
    for fi in (first, None):
        want = M.expand_batch(off, count, index, word_ids, fi)
        assert (want > 0).any() and (want < 0).any()
        np.testing.assert_array_equal(eng.expand_word_ids(off, count, index, word_ids, fi), want)
        np.testing.assert_array_equal(_expand_dev(eng, off, count, index, word_ids, fi), want)
    bad_index, bad_count = index.copy(), count.copy()
    bad_index[off[4]] = 500
    bad_index[off[4] + 1] = -1
    bad_count[6] = 5000
    bad_count[2] = -4
    index2 = bad_index.copy()
    index2[off[6] + count[6]:off[7]] = -1                                  # what the clamped count reads: outside, skipped
    np.testing.assert_array_equal(_expand_dev(eng, off, bad_count, index2, word_ids, first), M.expand_batch(off, bad_count, index2, word_ids, first, device=True))
    _refused(LCD_ERR_INVALID, eng.expand_word_ids, off, count, bad_index, word_ids, first)
    _refused(LCD_ERR_INVALID, eng.expand_word_ids, off, bad_count, index, word_ids, first)
    eng.close()


@pytest.mark.parametrize("pipeline", [False, True])
def test_select_frame_expand_end_to_end(oracle, pipeline):
    """eight frames of 160 features, 96 of them quantised: select_dev -> lcd_frame_dev (append_new_words, LCD_NEW_WORD_IDS_AUTO) -> expand_dev with
    the frame's own first id, the expansions issued lcd_pipeline_depth() frames late.  The expected ids are the oracle's addNewWords over the
    model's selected rows, expanded by the model; the vocabulary and the signatures equal those of a run that never called the new entries."""
    import rtabmap_amd
    from rtabmap_amd import capi, synth
    n_words, n_raw, q, T, n_sig = 2000, 160, 96, 8, 30
    rng = np.random.default_rng(21)
    vocab = synth.vocab_surf(n_words, seed=22)
    ids = np.arange(1, n_words + 1, dtype=np.int32)
    words = synth.zipf_words(n_sig, q, n_words, seed=23)
    words.reshape(-1)[-n_words:] = ids                                     # every word referenced: cleanUnusedWords drops none
    raw, resp, kept = [], [], []
    for t in range(T):
        d = vocab[rng.integers(0, n_words, n_raw)] + rng.standard_normal((n_raw, 64)).astype(np.float32) * np.float32(0.02)
        fresh = rng.random(n_raw) < 0.3
        d[fresh] = synth.vocab_surf(n_raw, seed=100 + t)[fresh]
        raw.append(np.ascontiguousarray(d, np.float32))
        resp.append(I.tied_frame(rng, n_raw)["response"])
        kept.append(np.array(M.select_frame(resp[t], q), np.int32))
    m = oracle.OracleMemory(strategy=oracle.kNNBruteForce, nndr=0.8, new_words_compared_together=True)
    for i, r in zip(ids, vocab):
        m.vwd.add_word(int(i), r)
    m.vwd.update()
    for s in range(n_sig):
        m.add_signature(words[s])
    expected, n_new = [], 0
    for t in range(T):
        first = m.vwd.last_word_id + 1
        _, w = m.update(raw[t][kept[t]])
        n_new += len(set(x for x in w if x >= first))
        expected.append(M.expand_frame(n_raw, kept[t], w))
    assert n_new > 50
    cap = n_sig + T + 4
    off = [0, n_raw]
    result = {}
    for with_select in (True, False):
        eng = rtabmap_amd.Engine("f32", 64, sig_capacity=cap, pipeline=pipeline)
        eng.vocab_append(vocab, ids)
        eng.sig_add_bulk(np.arange(1, n_sig + 1, dtype=np.int32), np.arange(0, (n_sig + 1) * q, q, dtype=np.int64), words.reshape(-1))
        eng.set_option("next_word_id", n_words + 1)
        depth = eng.pipeline_depth()
        assert depth == (3 if pipeline else 0)
        d_raw = [torch.from_numpy(x).cuda() for x in raw]
        d_resp = [torch.from_numpy(x).cuda() for x in resp]
        d_sel = [torch.from_numpy(np.ascontiguousarray(raw[t][kept[t]])).cuda() for t in range(T)]
        d_rows = torch.zeros((T, n_raw, 64), dtype=torch.float32, device="cuda")
        d_count = torch.zeros((T, 1), dtype=torch.int32, device="cuda")
        d_index = torch.zeros((T, n_raw), dtype=torch.int32, device="cuda")
        d_w = torch.zeros((T, n_raw), dtype=torch.int32, device="cuda")    # the frame writes q ids into its region
        d_all = torch.full((T, n_raw), I.CANARY, dtype=torch.int32, device="cuda")
        d_l = torch.zeros((T, cap), dtype=torch.float32, device="cuda")
        d_first = torch.zeros(T, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for t in range(T + depth):
            if t < T:
                if with_select:
                    eng.select_features_dev(d_resp[t], off, q, d_count[t], d_index[t], d_rows=d_raw[t], d_out_rows=d_rows[t])
                desc = d_rows[t] if with_select else d_sel[t]
                eng.frame_dev(desc.data_ptr(), q, n_sig + 1 + t, float(n_sig + 1 + t), d_w[t].data_ptr(), d_l[t].data_ptr(), cap,
                              first_new_word_id=capi.LCD_NEW_WORD_IDS_AUTO, append_new_words=True, d_first_new_word_id_ptr=d_first[t:].data_ptr())
            if with_select and t >= depth:                                 # frame t - depth's ids are final behind this frame's call
                if t == T:
                    eng.synchronize()                                      # no further frames: the owed stages are completed this way
                s = t - depth
                eng.expand_word_ids_dev(off, d_count[s], d_index[s], d_w[s], d_all[s], d_first[s:s + 1])
        eng.synchronize()
        result[with_select] = (d_w[:, :q].cpu().numpy(), eng.vocab_count(), eng.sig_count(), d_first.cpu().numpy())
        if with_select:
            assert d_count.cpu().numpy().reshape(-1).tolist() == [q] * T
            got = d_all.cpu().numpy()
            for t in range(T):
                np.testing.assert_array_equal(d_index[t, :q].cpu().numpy(), kept[t], err_msg="frame %d" % t)
                np.testing.assert_array_equal(got[t], expected[t], err_msg="frame %d" % t)
        eng.close()
    np.testing.assert_array_equal(result[True][0], result[False][0])
    np.testing.assert_array_equal(result[True][3], result[False][3])
    assert result[True][1] == result[False][1] == (n_words + n_new, n_words + n_new) and result[True][2] == result[False][2]


def test_memory_hip_selects_before_it_quantises(oracle):
    """MemoryHip::update with responses and points: Kp/MaxFeatures and the grid decide what is quantised; the ids equal the oracle's over
    the model's selection, expanded by the model; a frame that is not cut takes the plain path"""
    from rtabmap_amd.vwdictionary import MemoryHip
    from helpers import unit_rows
    rng = np.random.default_rng(31)
    for grid, size, mx in (((1, 1), (640, 480), 100), ((4, 4), (641, 482), 120)):
        h = MemoryHip(max_features=mx, grid_rows=grid[0], grid_cols=grid[1])
        m = oracle.OracleMemory(strategy=oracle.kNNBruteForce, nndr=0.8, new_words_compared_together=True)
        for t, n in enumerate((300, 80, 300, 300)):
            f = I.grid_frame(rng, n, size, (4, 4), mx)
            desc = unit_rows(n, 64, seed=40 + t % 3)                       # frames 0 and 3 share descriptors: words are found again
            kept = M.select_frame(f["response"], mx, M.KEEP_ORDER, grid, size, f["points"])
            assert (len(kept) < n) == (n > mx)
            _, w = m.update(np.ascontiguousarray(desc[kept]))
            sid, got = h.update_select(desc, f["response"], f["points"], size)
            assert sid == t + 1, h.select_error()
            assert got == M.expand_frame(n, kept, w).tolist(), (grid, t)
            assert h.get_ni(sid) == n
        bad = I.grid_frame(rng, 300, size, (4, 4), mx)
        bad["response"][5] = np.nan
        assert h.update_select(unit_rows(300, 64, seed=50), bad["response"], bad["points"], size)[0] == 0 and "NaN" in h.select_error()
        h.close()


def test_error_table():
    """every refusal of include/lcd.h's list; after each of them nothing was written and the handle still serves a call"""
    import rtabmap_amd
    from rtabmap_amd import capi
    import ctypes as C
    rng = np.random.default_rng(12)
    eng = rtabmap_amd.Engine("f32", 64)
    f = [I.tied_frame(rng, 100)]
    resp = f[0]["response"]
    pts = np.zeros((100, 2), np.float32)
    rows = I.rows_of(rng, "f32", 64, 100)
    sel = eng.select_features
    # limits
    big = np.zeros(16385, np.float32)
    _refused(LCD_ERR_UNSUPPORTED, sel, big, [0, 16385], 500)
    _refused(LCD_ERR_UNSUPPORTED, eng.expand_word_ids, [0, 16385], [0], np.zeros(16385, np.int32), np.zeros(16385, np.int32))
    _refused(LCD_ERR_UNSUPPORTED, sel, np.zeros(0, np.float32), np.zeros(65537, np.int64), 500)
    _refused(LCD_ERR_UNSUPPORTED, sel, resp, [0, 100], 50, grid=(33, 32), image_size=[(640, 480)], points=pts)
    # offsets
    _refused(LCD_ERR_INVALID, sel, resp, [1, 100], 50)
    _refused(LCD_ERR_INVALID, eng.expand_word_ids, [0, 60, 50, 100], [0, 0, 0], np.zeros(100, np.int32), np.zeros(100, np.int32))
    # order, aux_bytes, struct_size, grid
    _refused(LCD_ERR_INVALID, sel, resp, [0, 100], 50, order=2)
    _refused(LCD_ERR_INVALID, sel, resp, [0, 100], 50, aux=np.zeros((100, 6), np.uint8))
    _refused(LCD_ERR_INVALID, sel, resp, [0, 100], 50, aux=np.zeros((100, 68), np.uint8))
    _refused(LCD_ERR_INVALID, sel, resp, [0, 100], 50, grid=(0, 1))
    _refused(LCD_ERR_INVALID, sel, resp, [0, 100], 50, order=M.BY_RESPONSE, grid=(2, 2), image_size=[(640, 480)], points=pts)
    _refused(LCD_ERR_INVALID, sel, resp, [0, 100], 50, grid=(2, 2), image_size=[(640, 2)], points=pts)       # height <= grid_rows
    _refused(LCD_ERR_INVALID, sel, resp, [0, 100], 50, grid=(2, 2), image_size=[(640, 480)])                 # a grid without points
    _refused(LCD_ERR_INVALID, sel, resp, [0, 100], 50, grid=(2, 2), points=pts)                              # ... without image sizes
    off = np.array([0, 100], np.int64)
    count, index = np.full(1, I.CANARY, np.int32), np.full(100, I.CANARY, np.int32)
    a = capi.LcdSelectArgs(C.sizeof(capi.LcdSelectArgs) - 8, 1, 0, 50, 1, 1, 0, 0)
    a.offsets, a.response, a.out_count, a.out_index = off.ctypes.data, resp.ctypes.data, count.ctypes.data, index.ctypes.data
    assert eng.L.lcd_select_features(eng.h, C.byref(a)) == LCD_ERR_INVALID                                   # wrong struct_size
    a.struct_size = C.sizeof(capi.LcdSelectArgs)
    a.out_index = None
    assert eng.L.lcd_select_features(eng.h, C.byref(a)) == LCD_ERR_INVALID                                   # NULL output
    a.out_index, a.response = index.ctypes.data, None
    assert eng.L.lcd_select_features(eng.h, C.byref(a)) == LCD_ERR_INVALID                                   # NULL input
    a.response, a.rows = resp.ctypes.data, rows.ctypes.data
    assert eng.L.lcd_select_features(eng.h, C.byref(a)) == LCD_ERR_INVALID                                   # rows without out_rows
    e = capi.LcdExpandArgs(C.sizeof(capi.LcdExpandArgs) + 8, 1)
    assert eng.L.lcd_expand_word_ids(eng.h, C.byref(e)) == LCD_ERR_INVALID
    e.struct_size = C.sizeof(capi.LcdExpandArgs)
    e.offsets, e.count, e.index = off.ctypes.data, count.ctypes.data, index.ctypes.data
    assert eng.L.lcd_expand_word_ids(eng.h, C.byref(e)) == LCD_ERR_INVALID                                   # NULL word_ids / output
    assert (count == I.CANARY).all() and (index == I.CANARY).all()                                           # nothing was written
    # the device entries refuse the same before anything is enqueued
    d_resp = torch.from_numpy(big).cuda()
    d_count, d_index = torch.full((1,), I.CANARY, dtype=torch.int32, device="cuda"), torch.full((16385,), I.CANARY, dtype=torch.int32, device="cuda")
    _refused(LCD_ERR_UNSUPPORTED, eng.select_features_dev, d_resp, [0, 16385], 500, d_count, d_index)
    _refused(LCD_ERR_UNSUPPORTED, eng.expand_word_ids_dev, [0, 16385], d_count, d_index, d_index, d_index)
    _refused(LCD_ERR_INVALID, eng.select_features_dev, d_resp, [0, 100], 50, d_count, d_index, order=5)
    _refused(LCD_ERR_INVALID, eng.select_features_dev, d_resp, [0, 100], 50, d_count, None)
    eng.synchronize()
    assert (d_count.cpu().numpy() == I.CANARY).all() and (d_index.cpu().numpy() == I.CANARY).all()
    # n_frames == 0 is LCD_OK, and the handle still works
    assert sel(np.zeros(0, np.float32), [0], 5)[0].shape == (0,)
    I.assert_same(I.run_host(eng, f, 50, rows=rows), f, 50, rows=rows)
    I.assert_same(I.run_dev(eng, f, 50, rows=rows), f, 50, rows=rows, device=True)
    # 16384 features is the limit itself
    edge = [I.tied_frame(rng, 16384)]
    I.assert_same(I.run_dev(eng, edge, 500, M.BY_RESPONSE), edge, 500, M.BY_RESPONSE, device=True)
    eng.close()
