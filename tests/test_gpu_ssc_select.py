"""GPU tests of LCD_SELECT_SSC (Kp/SSC, the square covering) in lcd_select_features / lcd_select_features_dev
(rtabmap_amd/csrc/feature_select.hip) against tests/ssc_select_model.py.  Every comparison is exact: out_count, the whole out_index region
with its -1 tail, the gathered rows and the payload."""
import ctypes as C

import numpy as np
import pytest
import torch

import ssc_select_inputs as I
import ssc_select_model as M

pytestmark = pytest.mark.gpu

LCD_ERR_INVALID, LCD_ERR_UNSUPPORTED = 1, 5
ORDERS = (M.KEEP_ORDER, M.BY_RESPONSE)
LIMIT = M.MAX_SSC_FEATURES


def _refused(status, call, *args, **kw):
    from rtabmap_amd import capi
    with pytest.raises(capi.LcdError) as err:
        call(*args, **kw)
    assert err.value.status == status, err.value
    assert str(err.value)                                                  # a message
    return err.value


_MIXED = {}


def _mixed_batch():
    """max_features 60: n = 61, the sizes around the wave, the 256-thread workgroup and its switch at 2049, every generator's frame, and
    frames that are not cut in between; small and large images"""
    if not _MIXED:
        rng = np.random.default_rng(5)
        frames = []
        for k, n in enumerate((61, 63, 64, 65, 128, 129, 255, 256, 257, 2048, 2049)):
            gen = (I.uniform_frame, I.integer_frame, I.clustered_frame)[k % 3]
            frames.append(I.uniform_frame(rng, n, (640, 480)) if n >= 2048 else gen(rng, n, I.SIZES[2 + k % 3]))
            frames.append(I.uniform_frame(rng, (0, 1, 60, 17)[k % 4], (64, 48), tied=True))        # not cut
        for name in (nm[0] for nm in I.NAMED):
            frames.append(I.named(name)[0])
        _MIXED["frames"] = frames
    return _MIXED["frames"]


@pytest.mark.parametrize("dtype,dim", [("f32", 64), ("u8", 32)])
def test_one_batch_mixing_every_frame_size(dtype, dim):
    import rtabmap_amd
    frames = _mixed_batch()
    rng = np.random.default_rng(dim)
    n_all = sum(len(f["response"]) for f in frames)
    rows = I.rows_of(rng, dtype, dim, n_all)
    aux = rng.integers(0, 256, (n_all, 12), dtype=np.uint8)
    eng = rtabmap_amd.Engine(dtype, dim)
    for order in ORDERS:
        I.assert_same(I.run_dev(eng, frames, 60, order, rows=rows, aux=aux), frames, 60, order, rows=rows, aux=aux, device=True, what=order + " dev", key="mixed")
        I.assert_same(I.run_host(eng, frames, 60, order, rows=rows, aux=aux), frames, 60, order, rows=rows, aux=aux, device=True, what=order + " host", key="mixed")
    count = I.expected(frames, 60, M.KEEP_ORDER, True, key="mixed")[0]
    assert (count > 60).any() and (count == 0).any() and ((count > 0) & (count < 54)).any()
    # without the bit the same call is the plain selection: every cut frame keeps exactly max_features
    plain = I.run_dev(eng, frames, 60, M.KEEP_ORDER, ssc=False)
    assert all(c == min(len(f["response"]), 60) for c, f in zip(plain["count"], frames))
    assert eng.vocab_count() == (0, 0) and eng.sig_count() == (0, 0)
    eng.close()


@pytest.mark.parametrize("name", [nm[0] for nm in I.NAMED])
def test_every_generator_with_its_own_max(name):
    """each named frame with the max_features at which tests/test_ssc_select_inputs.py proves what it reaches, between two uncut frames"""
    import rtabmap_amd
    f, mx = I.named(name)
    rng = np.random.default_rng(9)
    frames = [I.uniform_frame(rng, min(mx, 40), (64, 48)), f, I.uniform_frame(rng, 2, (16, 16))]
    aux = rng.integers(0, 256, (sum(len(x["response"]) for x in frames), 12), dtype=np.uint8)
    eng = rtabmap_amd.Engine("f32", 64)
    for order in ORDERS:
        I.assert_same(I.run_dev(eng, frames, mx, order, aux=aux), frames, mx, order, aux=aux, device=True, what=order + " dev", key=name)
        I.assert_same(I.run_host(eng, frames, mx, order, aux=aux), frames, mx, order, aux=aux, device=True, what=order + " host", key=name)
    eng.close()


_AT_LIMIT = {}


def _limit_frame():
    if not _AT_LIMIT:
        _AT_LIMIT["f"] = I.uniform_frame(np.random.default_rng(11), LIMIT, (640, 480))
    return _AT_LIMIT["f"]


def test_a_frame_at_the_feature_limit():
    """8192 features cut to 1000: alone, and beside small frames; 8193 are refused by both entries, 8193 that are not cut are served"""
    import rtabmap_amd
    big = _limit_frame()
    rng = np.random.default_rng(12)
    small = [I.uniform_frame(rng, 70, (64, 48)), I.uniform_frame(rng, 1001, (640, 480))]
    eng = rtabmap_amd.Engine("f32", 64)
    I.assert_same(I.run_dev(eng, [big], 1000, M.BY_RESPONSE), [big], 1000, M.BY_RESPONSE, device=True, what="alone", key="limit")
    beside = [small[0], big, small[1]]
    for order in ORDERS:
        I.assert_same(I.run_dev(eng, beside, 1000, order), beside, 1000, order, device=True, what="beside " + order, key="limit beside")
    I.assert_same(I.run_host(eng, [big], 1000, M.KEEP_ORDER), [big], 1000, M.KEEP_ORDER, device=True, what="host", key="limit")
    over = I.uniform_frame(rng, LIMIT + 1, (640, 480))
    _refused(LCD_ERR_UNSUPPORTED, I.run_dev, eng, [over], 1000)
    _refused(LCD_ERR_UNSUPPORTED, I.run_host, eng, [over], 1000)
    got = I.run_dev(eng, [over], LIMIT + 1)                                # not cut: the limit is the plain one
    assert got["count"].tolist() == [LIMIT + 1] and (got["index"] == np.arange(LIMIT + 1)).all()
    eng.close()


def test_full_hd_clustered_frame_reaches_width_1():
    import rtabmap_amd
    f = I.clustered_frame(np.random.default_rng(13), 1000, (1920, 1080), clusters=3, spread=2.0)
    tr = {}
    kept = M.select_frame(f["response"], 500, M.BY_RESPONSE, f["image_size"], f["points"], device=True, trace=tr)
    assert tr["widths"][-1] == 1 and len(tr["widths"]) >= 6 and 0 < len(kept)
    eng = rtabmap_amd.Engine("f32", 64)
    for order in ORDERS:
        I.assert_same(I.run_dev(eng, [f], 500, order), [f], 500, order, device=True, what=order, key="full hd")
    eng.close()


def test_700_frames_in_one_call_and_batch_positions():
    """700 small frames, a third of them cut; the same frame at positions 0, 350 and 699 gives the same list"""
    import rtabmap_amd
    rng = np.random.default_rng(14)
    same = I.uniform_frame(rng, 40, (33, 17))
    frames = [I.uniform_frame(rng, int(rng.integers(0, 30)), I.SIZES[k % 3]) for k in range(700)]
    for k in (0, 350, 699):
        frames[k] = same
    rows = I.rows_of(rng, "u8", 32, sum(len(f["response"]) for f in frames))
    eng = rtabmap_amd.Engine("u8", 32)
    for order in ORDERS:
        got = I.run_dev(eng, frames, 12, order, rows=rows)
        I.assert_same(got, frames, 12, order, rows=rows, device=True, what=order, key="700")
        off = I.concat(frames)[2]
        lists = [got["index"][int(off[k]):int(off[k + 1])] for k in (0, 350, 699)]
        assert (lists[0] == lists[1]).all() and (lists[0] == lists[2]).all() and got["count"][0] == got["count"][350] == got["count"][699] > 0
    count = I.expected(frames, 12, M.KEEP_ORDER, True, key="700")[0]
    assert (count > 12).any() and (count == 0).any()
    eng.close()


def test_n_in_from_device_memory_cuts_a_region_short():
    """regions of 300 with n_in 300, 150, 61, 60 (not cut any more), 0, negative and above the region; a 2049 region with 100"""
    import rtabmap_amd
    rng = np.random.default_rng(15)
    regions = [300, 300, 300, 300, 300, 300, 300, 2049]
    n_in = [300, 150, 61, 60, 0, -3, 1000, 100]
    frames = [I.uniform_frame(rng, n, (64, 48)) for n in regions]
    rows = I.rows_of(rng, "f32", 64, sum(regions))
    eng = rtabmap_amd.Engine("f32", 64)
    for order in ORDERS:
        I.assert_same(I.run_dev(eng, frames, 60, order, rows=rows, n_in=n_in), frames, 60, order, rows=rows, device=True, n_in=n_in, what=order + " dev", key="n_in")
        I.assert_same(I.run_host(eng, frames, 60, order, rows=rows, n_in=n_in), frames, 60, order, rows=rows, device=True, n_in=n_in, what=order + " host", key="n_in")
    count = I.expected(frames, 60, M.KEEP_ORDER, True, n_in, key="n_in")[0]
    assert count[3] == 60 and count[4] == 0 and count[5] == 0 and 0 < count[6] != 60 and 0 < count[7] != 60 and count[0] != 60   # (1000 is clamped to the region)
    eng.close()


def test_three_unsynchronised_calls_with_the_largest_second():
    import rtabmap_amd
    rng = np.random.default_rng(16)
    a = [I.uniform_frame(rng, 100, (64, 48))]
    b = [I.uniform_frame(rng, 2049, (640, 480)), I.uniform_frame(rng, 300, (64, 48)), a[0]]
    c = [I.uniform_frame(rng, 65, (33, 17))]
    eng = rtabmap_amd.Engine("f32", 64)
    staged = [I.stage_dev(f) for f in (a, b, c)]
    outs = [I.launch_dev(eng, st, 60, M.BY_RESPONSE) for st in staged]
    for o, f, key in zip(outs, (a, b, c), ("three a", "three b", "three c")):
        I.assert_same(I.to_host(eng, o), f, 60, M.BY_RESPONSE, device=True, what=key, key=key)
    eng.close()


def test_device_entry_definitions_for_points_outside_the_mask_and_nan():
    """negative, NaN, infinite and too large coordinates and NaN responses: the device entry never selects a feature whose cell is outside
    the iteration's mask and orders NaN by its mapped bits; the host entry refuses both"""
    import rtabmap_amd
    rng = np.random.default_rng(17)
    f = I.uniform_frame(rng, 300, (64, 48), tied=True)
    wild = [(-0.5, 3.0), (3.0, -1e-40), (np.nan, 3.0), (3.0, np.inf), (-np.inf, 3.0), (64.6, 3.0), (3.0, 1e30), (-1e30, -1e30)]
    for k, w in enumerate(wild):
        f["points"][5 + 11 * k] = w
    g = dict(f, response=f["response"].copy(), points=I.uniform_frame(rng, 300, (64, 48))["points"])
    g["response"][::7] = np.nan
    g["response"][3::11] = -np.nan
    g["response"][5::13] = np.inf
    eng = rtabmap_amd.Engine("f32", 64)
    for order in ORDERS:
        got = I.run_dev(eng, [f, g], 60, order)
        I.assert_same(got, [f, g], 60, order, device=True, what=order, key="wild")
        chosen = set(got["index"][:got["count"][0]].tolist())
        assert not chosen & {5 + 11 * k for k in range(len(wild)) if k != 5}                  # (64.6 may share the last cell: the model decides)
    _refused(LCD_ERR_INVALID, I.run_host, eng, [f], 60)
    _refused(LCD_ERR_INVALID, I.run_host, eng, [g], 60)
    eng.close()


def test_error_table():
    """every refusal of include/lcd.h's list for the bit through both entries: the status, a message, no output byte written, and the handle
    serves a call afterwards; a handle of a sharded vocabulary refuses as it does without the bit"""
    import rtabmap_amd
    rng = np.random.default_rng(18)
    eng = rtabmap_amd.Engine("f32", 64)
    f = I.uniform_frame(rng, 100, (64, 48))
    resp, pts = f["response"], f["points"]
    d_resp, d_pts = torch.from_numpy(resp).cuda(), torch.from_numpy(pts).cuda()
    d_count = torch.full((1,), I.CANARY, dtype=torch.int32, device="cuda")
    d_index = torch.full((LIMIT + 1,), I.CANARY, dtype=torch.int32, device="cuda")
    d_big = torch.zeros(LIMIT + 1, dtype=torch.float32, device="cuda")
    d_big_pts = torch.zeros((LIMIT + 1, 2), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    host = lambda mx=50, size=((64, 48),), points=pts, grid=(1, 1), off=(0, 100), r=resp: eng.select_features(
        r, list(off), mx, image_size=None if size is None else list(size), points=points, grid=grid, ssc=True)
    dev = lambda mx=50, size=((64, 48),), points=d_pts, grid=(1, 1), off=(0, 100), r=d_resp: eng.select_features_dev(
        r, list(off), mx, d_count, d_index, image_size=None if size is None else list(size), d_points=points, grid=grid, ssc=True)
    table = [
        (LCD_ERR_INVALID, dict(grid=(2, 2))),                                                  # a grid above 1 x 1
        (LCD_ERR_INVALID, dict(mx=1)),                                                         # exp4 == 0
        (LCD_ERR_INVALID, dict(size=None)),                                                    # a cut frame without an image size
        (LCD_ERR_INVALID, dict(points=None)),                                                  # ... without points
        (LCD_ERR_INVALID, dict(size=((0, 48),))),
        (LCD_ERR_INVALID, dict(size=((64, -1),))),
        (LCD_ERR_UNSUPPORTED, dict(size=((16385, 48),))),
        (LCD_ERR_UNSUPPORTED, dict(size=((64, 16385),))),
    ]
    for status, kw in table:
        _refused(status, host, **kw)
        _refused(status, dev, **kw)
    _refused(LCD_ERR_UNSUPPORTED, host, mx=500, off=(0, LIMIT + 1), r=np.zeros(LIMIT + 1, np.float32), points=np.zeros((LIMIT + 1, 2), np.float32))
    _refused(LCD_ERR_UNSUPPORTED, dev, mx=500, off=(0, LIMIT + 1), r=d_big, points=d_big_pts)
    # what only the host entry can see: a NaN response, a coordinate outside [0, side]
    for bad in ((-0.25, 1.0), (1.0, 48.5), (np.nan, 1.0)):
        p = pts.copy()
        p[7] = bad
        _refused(LCD_ERR_INVALID, host, points=p)
    r = resp.copy()
    r[3] = np.nan
    _refused(LCD_ERR_INVALID, host, r=r)
    # nothing was written by any of them (the host entry's outputs through the C structure)
    from rtabmap_amd import capi
    off = np.array([0, 100], np.int64)
    count, index = np.full(1, I.CANARY, np.int32), np.full(100, I.CANARY, np.int32)
    size = np.array([[64, 48]], np.int32)
    for mx, grid, with_size in ((1, 1, True), (50, 2, True), (50, 1, False)):
        a = capi.LcdSelectArgs(C.sizeof(capi.LcdSelectArgs), 1, 0, mx, grid, grid, 0, capi.LCD_SELECT_SSC)
        a.offsets, a.response, a.points, a.out_count, a.out_index = off.ctypes.data, resp.ctypes.data, pts.ctypes.data, count.ctypes.data, index.ctypes.data
        a.image_size = size.ctypes.data if with_size else None
        assert eng.L.lcd_select_features(eng.h, C.byref(a)) == LCD_ERR_INVALID
    assert (count == I.CANARY).all() and (index == I.CANARY).all()
    eng.synchronize()
    assert (d_count.cpu().numpy() == I.CANARY).all() and (d_index.cpu().numpy() == I.CANARY).all()
    # the other bits of the flags word are ignored, with and without bit 0
    a = capi.LcdSelectArgs(C.sizeof(capi.LcdSelectArgs), 1, 0, 50, 1, 1, 0, 0x7ffffffe)
    a.offsets, a.response, a.out_count, a.out_index = off.ctypes.data, resp.ctypes.data, count.ctypes.data, index.ctypes.data
    assert eng.L.lcd_select_features(eng.h, C.byref(a)) == 0 and count[0] == 50
    # max_features == 1 and a missing image are fine without the bit and where no frame is cut; the handle still serves
    assert eng.select_features(resp, [0, 100], 1)[0].tolist() == [1]
    assert eng.select_features(resp, [0, 100], 100, ssc=True)[0].tolist() == [100]
    I.assert_same(I.run_host(eng, [f], 50), [f], 50, device=True, key="table")
    I.assert_same(I.run_dev(eng, [f], 50), [f], 50, device=True, key="table")
    assert eng.vocab_count() == (0, 0) and eng.sig_count() == (0, 0)
    eng.set_option("shard_append", 1)                                      # a handle of a sharded vocabulary
    _refused(LCD_ERR_UNSUPPORTED, host)
    _refused(LCD_ERR_UNSUPPORTED, dev)
    eng.close()


def _stream(eng, vocab, ids, words, raw, n_sig, q, between):
    """T frames through lcd_frame_dev (append_new_words) on a pipelined handle; between(t) is called in front of every frame"""
    from rtabmap_amd import capi
    T, cap = len(raw), n_sig + len(raw) + 4
    eng.vocab_append(vocab, ids)
    eng.sig_add_bulk(np.arange(1, n_sig + 1, dtype=np.int32), np.arange(0, (n_sig + 1) * q, q, dtype=np.int64), words.reshape(-1))
    eng.set_option("next_word_id", vocab.shape[0] + 1)
    d_raw = [torch.from_numpy(x).cuda() for x in raw]
    d_w = torch.zeros((T, q), dtype=torch.int32, device="cuda")
    d_l = torch.zeros((T, cap), dtype=torch.float32, device="cuda")
    d_first = torch.zeros(T, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for t in range(T):
        between(t)
        eng.frame_dev(d_raw[t].data_ptr(), q, n_sig + 1 + t, float(n_sig + 1 + t), d_w[t].data_ptr(), d_l[t].data_ptr(), cap,
                      first_new_word_id=capi.LCD_NEW_WORD_IDS_AUTO, append_new_words=True, d_first_new_word_id_ptr=d_first[t:].data_ptr())
    eng.synchronize()
    return d_w.cpu().numpy(), d_l.cpu().numpy().view(np.uint32), d_first.cpu().numpy(), eng.vocab_count(), eng.sig_count()


def test_calls_between_the_frames_of_a_pipelined_appending_stream():
    """SSC selections enqueued between the frames of a pipelined stream that appends its new words: the selections equal the model, and
    the stream's word ids, likelihoods, first ids and counts are bit for bit those of a stream without them"""
    import rtabmap_amd
    from rtabmap_amd import synth
    n_words, q, T, n_sig = 1500, 96, 6, 20
    rng = np.random.default_rng(19)
    vocab = synth.vocab_surf(n_words, seed=22)
    ids = np.arange(1, n_words + 1, dtype=np.int32)
    words = synth.zipf_words(n_sig, q, n_words, seed=23)
    raw = []
    for t in range(T):
        d = vocab[rng.integers(0, n_words, q)] + rng.standard_normal((q, 64)).astype(np.float32) * np.float32(0.02)
        fresh = rng.random(q) < 0.3
        d[fresh] = synth.vocab_surf(q, seed=100 + t)[fresh]
        raw.append(np.ascontiguousarray(d, np.float32))
    frames = [[I.uniform_frame(rng, 150 + 40 * t, (64, 48)), I.clustered_frame(rng, 90, (33, 17))] for t in range(T)]
    staged = []
    eng = rtabmap_amd.Engine("f32", 64, sig_capacity=n_sig + T + 4, pipeline=True)
    staged = [I.stage_dev(f) for f in frames]
    with_calls = _stream(eng, vocab, ids, words, raw, n_sig, q, lambda t: I.launch_dev(eng, staged[t], 60, ORDERS[t % 2]))
    for t in range(T):
        I.assert_same(I.to_host(eng, staged[t]), frames[t], 60, ORDERS[t % 2], device=True, what="frame %d" % t, key="stream %d" % t)
    eng.close()
    eng = rtabmap_amd.Engine("f32", 64, sig_capacity=n_sig + T + 4, pipeline=True)
    plain = _stream(eng, vocab, ids, words, raw, n_sig, q, lambda t: None)
    eng.close()
    for a, b in zip(with_calls[:3], plain[:3]):
        np.testing.assert_array_equal(a, b)
    assert with_calls[3:] == plain[3:] and with_calls[3][0] > n_words


def test_depth_ssc_select_frame_expand_chain(oracle):
    """four RGB-D frames: keypoints_3d_dev (3-D filter) -> select_features_dev (LCD_SELECT_SSC, n_in, the filter's compacted points, the
    3-D point as payload) -> lcd_frame_dev (append_new_words) -> expand_word_ids_dev (n_features), nothing read back in between; the number
    quantised is the model's.  The ids are the oracle's addNewWords over the rows the models keep and select, expanded by the model."""
    import rtabmap_amd
    from rtabmap_amd import capi, synth
    import feature_select_model as FM
    import keypoints_3d_inputs as KI
    import keypoints_3d_model as KM
    n_words, n_raw, mx, T, n_sig, q_sig = 2000, 320, 96, 4, 30, 96
    lo, hi = 1.5, 3.4
    rng = np.random.default_rng(21)
    vocab = synth.vocab_surf(n_words, seed=22)
    ids = np.arange(1, n_words + 1, dtype=np.int32)
    words = synth.zipf_words(n_sig, q_sig, n_words, seed=23)
    words.reshape(-1)[-n_words:] = ids
    raw, resp, pts, images, kept, sel, xyz = [], [], [], [], [], [], []
    for t in range(T):
        d = vocab[rng.integers(0, n_words, n_raw)] + rng.standard_normal((n_raw, 64)).astype(np.float32) * np.float32(0.02)
        fresh = rng.random(n_raw) < 0.3
        d[fresh] = synth.vocab_surf(n_raw, seed=100 + t)[fresh]
        raw.append(np.ascontiguousarray(d, np.float32))
        resp.append(I.tied_responses(rng, n_raw))
        im, p = KI.random_frame(rng, np.uint16 if t % 2 else np.float32, 64, 48, (1, 2)[t % 2], n_raw, border=False)
        images.append(im)
        pts.append(p)
        k, x = KM.frame(im, p, KM.FILTER_3D, lo, hi, device=True)
        assert mx < len(k) < n_raw
        kept.append(np.array(k, np.int32))
        xyz.append(x[k])
        sel.append(np.array(M.select_frame(resp[t][k], mx, M.KEEP_ORDER, (64, 48), p[k], device=True), np.int32))
        assert 0 < len(sel[t]) != mx
    m = oracle.OracleMemory(strategy=oracle.kNNBruteForce, nndr=0.8, new_words_compared_together=True)
    for i, r in zip(ids, vocab):
        m.vwd.add_word(int(i), r)
    m.vwd.update()
    for s in range(n_sig):
        m.add_signature(words[s])
    expected = []
    for t in range(T):
        _, w = m.update(raw[t][kept[t]][sel[t]])
        expected.append(np.concatenate([FM.expand_frame(len(kept[t]), sel[t], w), np.zeros(n_raw - len(kept[t]), np.int32)]))
    cap = n_sig + T + 4
    off = [0, n_raw]
    eng = rtabmap_amd.Engine("f32", 64, sig_capacity=cap)
    eng.vocab_append(vocab, ids)
    eng.sig_add_bulk(np.arange(1, n_sig + 1, dtype=np.int32), np.arange(0, (n_sig + 1) * q_sig, q_sig, dtype=np.int64), words.reshape(-1))
    eng.set_option("next_word_id", n_words + 1)
    st = [KI.stage_dev([images[t]], [pts[t]], response=resp[t], rows=raw[t]) for t in range(T)]
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    d_rows, d_xyz = z((T, n_raw, 64), torch.float32), z((T, n_raw, 3), torch.float32)
    d_count, d_index = z((T, 1), torch.int32), z((T, n_raw), torch.int32)
    d_w = z((T, n_raw), torch.int32)
    d_all = torch.full((T, n_raw), I.CANARY, dtype=torch.int32, device="cuda")
    d_l, d_first = z((T, cap), torch.float32), z((T,), torch.int32)
    torch.cuda.synchronize()
    for t in range(T):
        s = st[t]
        KI.launch_dev(eng, s, KM.FILTER_3D, lo, hi)
        eng.select_features_dev(s["response"], off, mx, d_count[t], d_index[t], image_size=[(64, 48)], d_points=s["points"], d_rows=s["rows"],
                                d_aux=s["xyz"], aux_bytes=12, d_out_rows=d_rows[t], d_out_aux=d_xyz[t], d_n_in=s["count"], ssc=True)
        eng.frame_dev(d_rows[t].data_ptr(), len(sel[t]), n_sig + 1 + t, float(n_sig + 1 + t), d_w[t].data_ptr(), d_l[t].data_ptr(), cap,
                      first_new_word_id=capi.LCD_NEW_WORD_IDS_AUTO, append_new_words=True, d_first_new_word_id_ptr=d_first[t:].data_ptr())
        eng.expand_word_ids_dev(off, d_count[t], d_index[t], d_w[t], d_all[t], d_first[t:t + 1], d_n_features=s["count"])
    eng.synchronize()
    got = d_all.cpu().numpy()
    for t in range(T):
        c = len(sel[t])
        assert int(d_count[t].cpu().numpy()[0]) == c, "frame %d" % t
        np.testing.assert_array_equal(d_index[t].cpu().numpy(), np.concatenate([sel[t], np.full(n_raw - c, -1, np.int32)]), err_msg="frame %d" % t)
        np.testing.assert_array_equal(KI.bits(d_xyz[t, :c].cpu().numpy()), KI.bits(xyz[t][sel[t]]), err_msg="frame %d" % t)
        np.testing.assert_array_equal(got[t], expected[t], err_msg="frame %d" % t)
    eng.close()


def test_memory_hip_with_kp_ssc(oracle):
    """MemoryHip::update with Kp/SSC: the covering decides what is quantised; a grid is refused as the entry refuses it"""
    import feature_select_model as FM
    from rtabmap_amd.vwdictionary import MemoryHip
    from helpers import unit_rows
    rng = np.random.default_rng(31)
    h = MemoryHip(max_features=100, ssc=True)
    m = oracle.OracleMemory(strategy=oracle.kNNBruteForce, nndr=0.8, new_words_compared_together=True)
    for t, n in enumerate((300, 80, 300)):
        f = I.uniform_frame(rng, n, (640, 480), tied=True)
        desc = unit_rows(n, 64, seed=40 + t % 2)
        kept = M.select_frame(f["response"], 100, M.KEEP_ORDER, f["image_size"], f["points"])
        _, w = m.update(np.ascontiguousarray(desc[kept]))
        sid, got = h.update_select(desc, f["response"], f["points"], f["image_size"])
        assert sid == t + 1, h.select_error()
        assert got == FM.expand_frame(n, kept, w).tolist(), t
    h.close()
    h = MemoryHip(max_features=100, grid_rows=2, grid_cols=2, ssc=True)
    f = I.uniform_frame(rng, 300, (640, 480))
    assert h.update_select(unit_rows(300, 64, seed=50), f["response"], f["points"], f["image_size"])[0] == 0 and "SSC" in h.select_error()
    h.close()
