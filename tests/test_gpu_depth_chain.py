"""GPU tests of the depth stage chained into selection, frame and expansion with nothing read back in between: lcd_keypoints_3d_dev ->
lcd_select_features_dev (n_in) -> lcd_frame_dev -> lcd_expand_word_ids_dev (n_features), and of the two new fields on their own."""
import numpy as np
import pytest
import torch

import feature_select_inputs as FS
import feature_select_model as FM
import keypoints_3d_inputs as I
import keypoints_3d_model as M

pytestmark = pytest.mark.gpu


def _select_with_n_in(frames, n_in, max_features, order):
    """the model: frame f is the first clamp(n_in[f], 0, region) features of its region; -1 to the end of the region"""
    count, index = [], []
    for f, k in zip(frames, n_in):
        region = len(f["response"])
        n = min(max(int(k), 0), region)
        kept = FM.select_frame(f["response"][:n], max_features, order, device=True)
        count.append(len(kept))
        index += kept + [-1] * (region - len(kept))
    return np.array(count, np.int32), np.array(index, np.int32)


@pytest.mark.parametrize("order", [FM.KEEP_ORDER, FM.BY_RESPONSE])
def test_n_in_decides_the_cut(order):
    """n_in above the region (clamped), of 0, negative, and on both sides of n > max_features in frames whose region is on the other side;
    rows and payload follow; both entries"""
    import rtabmap_amd
    rng = np.random.default_rng(2)
    regions = [300, 300, 300, 300, 64, 2049, 2049, 0, 65]
    n_in = [1000, 0, 100, 101, -5, 64, 2048, 7, 65]                       # max 100: clamped and cut, empty, not cut, cut by one, ...
    frames = [FS.tied_frame(rng, n) for n in regions]
    n_all = sum(regions)
    rows = FS.rows_of(rng, "f32", 64, n_all)
    aux = rng.integers(0, 256, (n_all, 12), dtype=np.uint8)
    count, index = _select_with_n_in(frames, n_in, 100, order)
    assert count.tolist() == [100, 0, 100, 100, 0, 64, 100, 0, 65]
    eng = rtabmap_amd.Engine("f32", 64)
    st = FS.stage_dev(frames, rows, aux)
    d_n = torch.tensor(n_in, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    eng.select_features_dev(st["resp"], st["off"], 100, st["count"], st["index"], order=order, d_rows=st["d_rows"], d_aux=st["d_aux"], aux_bytes=12,
                            d_out_rows=st["rows"], d_out_aux=st["aux"], d_n_in=d_n)
    got = FS.to_host(eng, st)
    resp, _, off, _ = FS.concat(frames)
    h_count, h_index, h_rows, h_aux = eng.select_features(resp, off, 100, order=order, rows=rows, aux=aux, n_in=n_in)
    for name, c, ix, r, x in (("dev", got["count"], got["index"], got["rows"], got["aux"]), ("host", h_count, h_index, h_rows, h_aux)):
        np.testing.assert_array_equal(c, count, err_msg=name)
        np.testing.assert_array_equal(ix, index, err_msg=name)
        for f in range(len(frames)):
            a, k = int(off[f]), int(count[f])
            np.testing.assert_array_equal(r[a:a + k], rows[a + index[a:a + k]], err_msg="%s rows of frame %d" % (name, f))
            np.testing.assert_array_equal(x[a:a + k], aux[a + index[a:a + k]], err_msg="%s aux of frame %d" % (name, f))
    eng.close()


def test_null_n_in_and_n_features_give_the_bytes_of_the_existing_path():
    """without the fields, and with them equal to the regions, every output byte is what the call gives today (the model of the existing tests)"""
    import rtabmap_amd
    rng = np.random.default_rng(3)
    frames = [FS.tied_frame(rng, n) for n in (300, 64, 0, 1025)]
    regions = [300, 64, 0, 1025]
    eng = rtabmap_amd.Engine("f32", 64)
    for order in (FM.KEEP_ORDER, FM.BY_RESPONSE):
        plain = FS.run_dev(eng, frames, 100, order)
        FS.assert_same(plain, frames, 100, order, device=True)
        st = FS.stage_dev(frames)
        d_n = torch.tensor(regions, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        eng.select_features_dev(st["resp"], st["off"], 100, st["count"], st["index"], order=order, d_n_in=d_n)
        same = FS.to_host(eng, st)
        np.testing.assert_array_equal(same["count"], plain["count"])
        np.testing.assert_array_equal(same["index"], plain["index"])
    ex = [FS.expansion_frame(rng, n) for n in regions]
    off = np.cumsum([0] + regions).astype(np.int64)
    count = np.array([e["count"] for e in ex], np.int32)
    index, word_ids = np.full(int(off[-1]), -9, np.int32), np.full(int(off[-1]), 77, np.int32)
    for f, e in enumerate(ex):
        index[off[f]:off[f] + e["count"]] = e["index"]
        word_ids[off[f]:off[f] + e["count"]] = e["word_ids"]
    want = FM.expand_batch(off, count, index, word_ids)
    np.testing.assert_array_equal(eng.expand_word_ids(off, count, index, word_ids), want)
    np.testing.assert_array_equal(eng.expand_word_ids(off, count, index, word_ids, n_features=regions), want)
    eng.close()


def test_n_features_numbers_the_frame_and_zeroes_the_rest():
    import rtabmap_amd
    rng = np.random.default_rng(4)
    regions = [300, 300, 64, 2049, 10]
    n_feat = [120, 0, 500, 2048, -1]
    off = np.cumsum([0] + regions).astype(np.int64)
    index, word_ids = np.full(int(off[-1]), -9, np.int32), np.full(int(off[-1]), 77, np.int32)
    count, want = [], []
    for f, (region, k) in enumerate(zip(regions, n_feat)):
        n = min(max(k, 0), region)
        e = FS.expansion_frame(rng, n)
        count.append(e["count"])
        index[off[f]:off[f] + e["count"]] = e["index"]
        word_ids[off[f]:off[f] + e["count"]] = e["word_ids"]
        want.append(np.concatenate([FM.expand_frame(n, e["index"], e["word_ids"]), np.zeros(region - n, np.int32)]))
    want = np.concatenate(want)
    count = np.array(count, np.int32)
    eng = rtabmap_amd.Engine("f32", 64)
    np.testing.assert_array_equal(eng.expand_word_ids(off, count, index, word_ids, n_features=n_feat), want)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()
    out = torch.full((int(off[-1]),), FS.CANARY, dtype=torch.int32, device="cuda")
    d = [dev(x) for x in (count, index, word_ids, n_feat)]
    torch.cuda.synchronize()
    eng.expand_word_ids_dev(off, d[0], d[1], d[2], out, d_n_features=d[3])
    eng.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    # a count beyond the device's frame is clamped to it: the entries behind are not read
    big = count.copy()
    big[0] = 300
    eng.expand_word_ids_dev(off, dev(big), d[1], d[2], out, d_n_features=d[3])
    eng.synchronize()
    index2 = index.copy()
    got = out.cpu().numpy()
    n0 = 120
    np.testing.assert_array_equal(got[:300], np.concatenate([FM.expand_frame(n0, index2[:n0], word_ids[:n0], device=True), np.zeros(180, np.int32)]))
    eng.close()


@pytest.mark.parametrize("pipeline", [False, True])
def test_depth_select_frame_expand_end_to_end(oracle, pipeline):
    """eight RGB-D frames of 320 features: keypoints_3d_dev (3-D filter, Kp/MinDepth 1.5, Kp/MaxDepth 3.4) -> select_features_dev(n_in, the
    3-D point as payload) -> lcd_frame_dev (append_new_words, LCD_NEW_WORD_IDS_AUTO) -> expand_word_ids_dev(n_features) with nothing read
    back in between, the expansions issued lcd_pipeline_depth() frames late.  The expected ids are the oracle's addNewWords over the rows the
    models keep and select, expanded by the model."""
    import rtabmap_amd
    from rtabmap_amd import capi, synth
    n_words, n_raw, q, T, n_sig = 2000, 320, 96, 8, 30
    lo, hi = 1.5, 3.4
    rng = np.random.default_rng(21)
    vocab = synth.vocab_surf(n_words, seed=22)
    ids = np.arange(1, n_words + 1, dtype=np.int32)
    words = synth.zipf_words(n_sig, q, n_words, seed=23)
    words.reshape(-1)[-n_words:] = ids
    raw, resp, pts, images, kept, sel, xyz = [], [], [], [], [], [], []
    for t in range(T):
        d = vocab[rng.integers(0, n_words, n_raw)] + rng.standard_normal((n_raw, 64)).astype(np.float32) * np.float32(0.02)
        fresh = rng.random(n_raw) < 0.3
        d[fresh] = synth.vocab_surf(n_raw, seed=100 + t)[fresh]
        raw.append(np.ascontiguousarray(d, np.float32))
        resp.append(FS.tied_frame(rng, n_raw)["response"])
        im, p = I.random_frame(rng, np.uint16 if t % 2 else np.float32, 64, 48, (1, 2, 4)[t % 3], n_raw, transform=I.TILT if t % 2 else None, border=False)
        images.append(im)
        pts.append(p)
        k, x = M.frame(im, p, M.FILTER_3D, lo, hi, device=True)
        assert q < len(k) < n_raw                                          # the depth filter drops some, the selection cuts the rest
        kept.append(np.array(k, np.int32))
        xyz.append(x[k])
        sel.append(np.array(FM.select_frame(resp[t][k], q), np.int32))
    m = oracle.OracleMemory(strategy=oracle.kNNBruteForce, nndr=0.8, new_words_compared_together=True)
    for i, r in zip(ids, vocab):
        m.vwd.add_word(int(i), r)
    m.vwd.update()
    for s in range(n_sig):
        m.add_signature(words[s])
    expected, n_new = [], 0
    for t in range(T):
        first = m.vwd.last_word_id + 1
        _, w = m.update(raw[t][kept[t]][sel[t]])
        n_new += len(set(x for x in w if x >= first))
        expected.append(np.concatenate([FM.expand_frame(len(kept[t]), sel[t], w), np.zeros(n_raw - len(kept[t]), np.int32)]))
    assert n_new > 50
    cap = n_sig + T + 4
    off = [0, n_raw]
    eng = rtabmap_amd.Engine("f32", 64, sig_capacity=cap, pipeline=pipeline)
    eng.vocab_append(vocab, ids)
    eng.sig_add_bulk(np.arange(1, n_sig + 1, dtype=np.int32), np.arange(0, (n_sig + 1) * q, q, dtype=np.int64), words.reshape(-1))
    eng.set_option("next_word_id", n_words + 1)
    depth = eng.pipeline_depth()
    assert depth == (3 if pipeline else 0)
    st = [I.stage_dev([images[t]], [pts[t]], response=resp[t], rows=raw[t]) for t in range(T)]
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    d_rows, d_xyz = z((T, n_raw, 64), torch.float32), z((T, n_raw, 3), torch.float32)
    d_count, d_index = z((T, 1), torch.int32), z((T, n_raw), torch.int32)
    d_w = z((T, n_raw), torch.int32)
    d_all = torch.full((T, n_raw), FS.CANARY, dtype=torch.int32, device="cuda")
    d_l, d_first = z((T, cap), torch.float32), z((T,), torch.int32)
    torch.cuda.synchronize()
    for t in range(T + depth):
        if t < T:
            s = st[t]
            I.launch_dev(eng, s, M.FILTER_3D, lo, hi)
            eng.select_features_dev(s["response"], off, q, d_count[t], d_index[t], d_rows=s["rows"], d_aux=s["xyz"], aux_bytes=12,
                                    d_out_rows=d_rows[t], d_out_aux=d_xyz[t], d_n_in=s["count"])
            eng.frame_dev(d_rows[t].data_ptr(), q, n_sig + 1 + t, float(n_sig + 1 + t), d_w[t].data_ptr(), d_l[t].data_ptr(), cap,
                          first_new_word_id=capi.LCD_NEW_WORD_IDS_AUTO, append_new_words=True, d_first_new_word_id_ptr=d_first[t:].data_ptr())
        if t >= depth:                                                     # frame t - depth's ids are final behind this frame's call
            if t == T:
                eng.synchronize()
            u = t - depth
            eng.expand_word_ids_dev(off, d_count[u], d_index[u], d_w[u], d_all[u], d_first[u:u + 1], d_n_features=st[u]["count"])
    eng.synchronize()
    assert d_count.cpu().numpy().reshape(-1).tolist() == [q] * T
    got = d_all.cpu().numpy()
    for t in range(T):
        assert int(st[t]["count"].cpu().numpy()[0]) == len(kept[t])
        np.testing.assert_array_equal(st[t]["index"].cpu().numpy()[:len(kept[t])], kept[t], err_msg="frame %d" % t)
        np.testing.assert_array_equal(d_index[t, :q].cpu().numpy(), sel[t], err_msg="frame %d" % t)
        np.testing.assert_array_equal(I.bits(d_xyz[t, :q].cpu().numpy()), I.bits(xyz[t][sel[t]]), err_msg="frame %d" % t)
        np.testing.assert_array_equal(got[t], expected[t], err_msg="frame %d" % t)
    assert eng.vocab_count() == (n_words + n_new, n_words + n_new)
    eng.close()


def test_memory_hip_runs_the_depth_stage_first(oracle):
    """MemoryHip::update with a depth image and cameras: Kp/MinDepth and Kp/MaxDepth decide which features exist, Kp/MaxFeatures which of them
    are quantised; ids, points and kept indices equal the models' and the oracle's"""
    from rtabmap_amd.vwdictionary import MemoryHip
    from helpers import unit_rows
    rng = np.random.default_rng(31)
    h = MemoryHip(max_features=100, min_depth=1.5, max_depth=3.4)
    m = oracle.OracleMemory(strategy=oracle.kNNBruteForce, nndr=0.8, new_words_compared_together=True)
    for t, (n, dtype, nc) in enumerate(((300, np.uint16, 2), (120, np.float32, 1), (300, np.uint16, 4), (300, np.float32, 2))):
        im, p = I.random_frame(rng, dtype, 64, 48, nc, n, transform=I.TILT if t % 2 else None, host_ok=True, border=t == 2)
        resp = FS.tied_frame(rng, n)["response"]
        desc = unit_rows(n, 64, seed=40 + t % 3)
        kept, xyz = M.frame(im, p, M.FILTER_3D, 1.5, 3.4)
        sel = FM.select_frame(resp[kept], 100)
        assert 0 < len(kept) < n
        _, w = m.update(np.ascontiguousarray(desc[kept][sel]))
        sid, ids, got_xyz, got_kept = h.update_depth(desc, resp, p, (64, 48), im["data"], im["cameras"], width=im["width"])
        assert sid == t + 1, h.select_error()
        assert got_kept.tolist() == kept
        np.testing.assert_array_equal(I.bits(got_xyz), I.bits(xyz[kept]))
        assert ids == FM.expand_frame(len(kept), sel, w).tolist(), t
        assert h.get_ni(sid) == len(kept)
    bad = np.array([[np.nan, 1.0]] * 3, np.float32)
    assert h.update_depth(unit_rows(3, 64, seed=50), np.ones(3, np.float32), bad, (64, 48), im["data"], im["cameras"])[0] == 0 and "keypoint" in h.select_error()
    h.close()
