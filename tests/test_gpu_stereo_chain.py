"""GPU tests of the stereo stage chained into selection, frame and expansion with nothing read back in between:
lcd_keypoints_3d_stereo_dev -> lcd_select_features_dev (n_in) -> lcd_frame_dev -> lcd_expand_word_ids_dev (n_features), against the models
and the oracle; n_in lies on both sides of the cut.  And MemoryHip's stereo stage over an engine."""
import numpy as np
import pytest
import torch

import feature_select_inputs as FS
import feature_select_model as FM
import stereo_flow_inputs as I
import stereo_flow_model as M

pytestmark = pytest.mark.gpu

LO, HI = 1.0, 4.0


def _frame(rng, t, n_raw):
    """a stereo frame of n_raw keypoints, some of them beyond the bounds test; in the odd frames most of them, so that fewer than the
    selection's maximum are left"""
    pr, p = I.random_frame(rng, 64, 48, n_raw, disparity=2.0 + 0.5 * t, transform=I.TILT if t % 3 == 1 else None, pad=3 if t % 3 == 2 else 0)
    p = np.stack([rng.uniform(10, 52, n_raw), rng.uniform(3, 44, n_raw)], 1).astype(np.float32)
    inside = 70 if t % 2 else n_raw - 30
    p[inside:, 0] = -40.0 - rng.uniform(0, 5, n_raw - inside).astype(np.float32)
    return pr, p


@pytest.mark.parametrize("pipeline", [False, True])
def test_stereo_select_frame_expand_end_to_end(oracle, pipeline):
    """six stereo frames of 320 features: keypoints_3d_stereo_dev (3-D filter, Kp/MinDepth 1, Kp/MaxDepth 4) -> select_features_dev(n_in, the
    3-D point as payload) -> lcd_frame_dev (append_new_words, LCD_NEW_WORD_IDS_AUTO) -> expand_word_ids_dev(n_features) with nothing read
    back in between, the expansions issued lcd_pipeline_depth() frames late.  The expected ids are the oracle's addNewWords over the rows the
    models keep and select, expanded by the model."""
    import rtabmap_amd
    from rtabmap_amd import capi, synth
    n_words, n_raw, q, T, n_sig = 2000, 320, 96, 6, 30
    rng = np.random.default_rng(21)
    vocab = synth.vocab_surf(n_words, seed=22)
    ids = np.arange(1, n_words + 1, dtype=np.int32)
    words = synth.zipf_words(n_sig, q, n_words, seed=23)
    words.reshape(-1)[-n_words:] = ids
    raw, resp, pts, pairs, kept, sel, xyz = [], [], [], [], [], [], []
    for t in range(T):
        d = vocab[rng.integers(0, n_words, n_raw)] + rng.standard_normal((n_raw, 64)).astype(np.float32) * np.float32(0.02)
        fresh = rng.random(n_raw) < 0.3
        d[fresh] = synth.vocab_surf(n_raw, seed=100 + t)[fresh]
        raw.append(np.ascontiguousarray(d, np.float32))
        resp.append(FS.tied_frame(rng, n_raw)["response"])
        pr, p = _frame(rng, t, n_raw)
        pairs.append(pr)
        pts.append(p)
        fr = M.frame(pr, p, None, M.FILTER_3D, LO, HI, device=True)
        k = fr["kept"]
        assert (0 < len(k) < q) if t % 2 else (q < len(k) < n_raw)         # n_in on both sides of the cut
        kept.append(np.array(k, np.int32))
        xyz.append(fr["xyz"][k])
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
    assert n_new > 30
    cap = n_sig + T + 4
    off = [0, n_raw]
    eng = rtabmap_amd.Engine("f32", 64, sig_capacity=cap, pipeline=pipeline)
    eng.vocab_append(vocab, ids)
    eng.sig_add_bulk(np.arange(1, n_sig + 1, dtype=np.int32), np.arange(0, (n_sig + 1) * q, q, dtype=np.int64), words.reshape(-1))
    eng.set_option("next_word_id", n_words + 1)
    depth = eng.pipeline_depth()
    st = [I.stage_dev([pairs[t]], [pts[t]], response=resp[t], rows=raw[t]) for t in range(T)]
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    d_rows, d_xyz = z((T, n_raw, 64), torch.float32), z((T, n_raw, 3), torch.float32)
    d_count, d_index = z((T, 1), torch.int32), z((T, n_raw), torch.int32)
    d_w = z((T, n_raw), torch.int32)
    d_all = torch.full((T, n_raw), FS.CANARY, dtype=torch.int32, device="cuda")
    d_l, d_first = z((T, cap), torch.float32), z((T,), torch.int32)
    n_sel = [len(s) for s in sel]
    torch.cuda.synchronize()
    for t in range(T + depth):
        if t < T:
            s = st[t]
            I.launch_dev(eng, s, None, M.FILTER_3D, LO, HI)
            eng.select_features_dev(s["response"], off, q, d_count[t], d_index[t], d_rows=s["rows"], d_aux=s["xyz"], aux_bytes=12,
                                    d_out_rows=d_rows[t], d_out_aux=d_xyz[t], d_n_in=s["count"])
            # the frame's size is the host's here: the oracle's frames are the models' selections
            eng.frame_dev(d_rows[t].data_ptr(), n_sel[t], n_sig + 1 + t, float(n_sig + 1 + t), d_w[t].data_ptr(), d_l[t].data_ptr(), cap,
                          first_new_word_id=capi.LCD_NEW_WORD_IDS_AUTO, append_new_words=True, d_first_new_word_id_ptr=d_first[t:].data_ptr())
        if t >= depth:                                                     # frame t - depth's ids are final behind this frame's call
            if t == T:
                eng.synchronize()
            u = t - depth
            eng.expand_word_ids_dev(off, d_count[u], d_index[u], d_w[u], d_all[u], d_first[u:u + 1], d_n_features=st[u]["count"])
    eng.synchronize()
    assert d_count.cpu().numpy().reshape(-1).tolist() == n_sel
    got = d_all.cpu().numpy()
    for t in range(T):
        assert int(st[t]["count"].cpu().numpy()[0]) == len(kept[t])
        np.testing.assert_array_equal(st[t]["index"].cpu().numpy()[:len(kept[t])], kept[t], err_msg="frame %d" % t)
        np.testing.assert_array_equal(d_index[t, :n_sel[t]].cpu().numpy(), sel[t], err_msg="frame %d" % t)
        np.testing.assert_array_equal(I.bits(d_xyz[t, :n_sel[t]].cpu().numpy()), I.bits(xyz[t][sel[t]]), err_msg="frame %d" % t)
        np.testing.assert_array_equal(got[t], expected[t], err_msg="frame %d" % t)
    assert eng.vocab_count() == (n_words + n_new, n_words + n_new)
    eng.close()


def test_memory_hip_runs_the_stereo_stage_first(oracle):
    """MemoryHip::update with a left and a right image and a stereo camera: the Stereo/* parameters, Kp/MinDepth and Kp/MaxDepth decide which
    features exist, Kp/MaxFeatures which of them are quantised; ids, points and kept indices equal the models' and the oracle's"""
    from rtabmap_amd.vwdictionary import MemoryHip
    from helpers import unit_rows
    rng = np.random.default_rng(31)
    h = MemoryHip(max_features=100, min_depth=LO, max_depth=HI)
    m = oracle.OracleMemory(strategy=oracle.kNNBruteForce, nndr=0.8, new_words_compared_together=True)
    for t, n in enumerate((300, 120, 300, 300)):
        pr, p = _frame(rng, t, n)
        resp = FS.tied_frame(rng, n)["response"]
        desc = unit_rows(n, 64, seed=40 + t % 3)
        fr = M.frame(pr, p, None, M.FILTER_3D, LO, HI)
        kept = fr["kept"]
        sel = FM.select_frame(resp[kept], 100)
        assert 0 < len(kept) < n
        _, w = m.update(np.ascontiguousarray(desc[kept][sel]))
        sid, ids, got_xyz, got_kept = h.update_stereo(desc, resp, p, (64, 48), pr["left"], pr["right"], pr["camera"], width=pr["width"])
        assert sid == t + 1, h.select_error()
        assert got_kept.tolist() == kept
        np.testing.assert_array_equal(I.bits(got_xyz), I.bits(fr["xyz"][kept]))
        assert ids == FM.expand_frame(len(kept), sel, w).tolist(), t
        assert h.get_ni(sid) == len(kept)
    bad = np.array([[np.nan, 1.0]] * 3, np.float32)
    assert h.update_stereo(unit_rows(3, 64, seed=50), np.ones(3, np.float32), bad, (64, 48), pr["left"], pr["right"], pr["camera"], width=pr["width"])[0] == 0
    assert "keypoint" in h.select_error()
    h.close()
