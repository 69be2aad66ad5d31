"""GPU tests of lcd_match_guided / lcd_match_guided_dev (rtabmap_amd/csrc/guided_match.hip) against tests/guided_match_model.py over the
oracle's distances.  Every comparison is exact: counts, indices and distance bits."""
import functools

import numpy as np
import pytest
import torch

import guided_match_inputs as I
import guided_match_model as M

pytestmark = pytest.mark.gpu

LCD_ERR_UNSUPPORTED = 5
COMBOS = [(d, n) for d in (M.P2F, M.F2P) for n in (M.RATIO, M.NEAREST)]


def _padded(dtype, dim):
    return dtype == "u8" and dim % 4 != 0


@functools.lru_cache(maxsize=None)
def _cases(dtype, dim):
    import oracle
    pairs = [I.general_case(oracle, dtype, dim, *s) for s in I.SIZES]
    return pairs, {c: I.expected_batch(oracle, pairs, I.RADIUS, 0.8, c[1], c[0]) for c in COMBOS}


@pytest.mark.parametrize("dtype,dim", I.KINDS)
def test_both_entries_equal_the_model(oracle, dtype, dim):
    """every size in ONE batch, the empty pairs among them; both directions x both nn types; out_dist NULL and non-NULL"""
    import rtabmap_amd
    from rtabmap_amd import capi
    pairs, exp = _cases(dtype, dim)
    assert M.outcomes(exp[(M.P2F, M.RATIO)], M.P2F) == I.ALL_OUTCOMES and M.outcomes(exp[(M.F2P, M.RATIO)], M.F2P) == I.ALL_OUTCOMES
    eng = rtabmap_amd.Engine(dtype, dim)
    for direction, nn_type in COMBOS:
        e = exp[(direction, nn_type)]
        what = "%s %s" % (direction, nn_type)
        I.assert_same(I.run_host(eng, pairs, nn_type=nn_type, direction=direction), e, what + " host")
        I.assert_same(I.run_host(eng, pairs, nn_type=nn_type, direction=direction, with_dist=False), e, what + " host, no dist")
        if _padded(dtype, dim):
            with pytest.raises(capi.LcdError) as err:
                I.run_dev(eng, pairs, nn_type=nn_type, direction=direction)
            assert err.value.status == LCD_ERR_UNSUPPORTED
            continue
        I.assert_same(I.run_dev(eng, pairs, nn_type=nn_type, direction=direction), e, what + " dev")
        I.assert_same(I.run_dev(eng, pairs, nn_type=nn_type, direction=direction, with_dist=False), e, what + " dev, no dist")
    # a pair alone equals its part of the batch
    k = I.SIZES.index((300, 280, 300))
    I.assert_same(I.run_host(eng, [pairs[k]]), I.expected_batch(oracle, [pairs[k]], I.RADIUS, 0.8, M.RATIO, M.P2F), "single pair")
    assert eng.vocab_count() == (0, 0) and eng.sig_count() == (0, 0)
    eng.close()


@pytest.mark.parametrize("dtype,dim", [("f32", 64), ("u8", 32)])
def test_700_tiny_pairs_in_one_call(oracle, dtype, dim):
    import rtabmap_amd
    pairs = I.many_tiny_pairs(dtype, dim, 700, 77)
    eng = rtabmap_amd.Engine(dtype, dim)
    for direction in (M.P2F, M.F2P):
        e = I.expected_batch(oracle, pairs, I.RADIUS, 0.8, M.RATIO, direction)
        assert (e["match"] >= 0).sum() > 100 and (e["count"] >= 2).sum() > 100
        I.assert_same(I.run_dev(eng, pairs, direction=direction), e, direction + " dev")
        I.assert_same(I.run_host(eng, pairs, direction=direction), e, direction + " host")
    eng.close()


def test_scratch_is_counted_and_reused_between_unsynchronised_calls(oracle):
    """two device calls in a row without a synchronisation in between (the second takes the other job-table slot), a third that reuses the
    first slot; the host entry's staging is counted in lcd_stats.bytes_device"""
    import rtabmap_amd
    a = [I.general_case(oracle, "f32", 64, 33, 31, 65)]
    b = [I.general_case(oracle, "f32", 64, 300, 280, 300), a[0]]
    ea, eb = (I.expected_batch(oracle, p, I.RADIUS, 0.8, M.RATIO, M.P2F) for p in (a, b))
    eng = rtabmap_amd.Engine("f32", 64)
    bytes0 = eng.stats()["bytes_device"]
    outs = []
    for pairs in (a, b, a):
        f, t, c, r, p, fo, to, co = I.concat(pairs)
        d = [torch.from_numpy(x).cuda() for x in (f, t, c, r, p)]
        o = [torch.full((c.shape[0],), -7, dtype=torch.int32, device="cuda") for _ in range(2)] + \
            [torch.full((c.shape[0], 2), -7.0, dtype=torch.float32, device="cuda"), torch.full((t.shape[0],), -7, dtype=torch.int32, device="cuda")]
        outs.append((d, o, (fo, to, co)))
    torch.cuda.synchronize()
    for d, o, offs in outs:
        eng.match_guided_dev(*d, *offs, *o)
    eng.synchronize()
    for (d, o, _), e in zip(outs, (ea, eb, ea)):
        I.assert_same(dict(count=o[0].cpu().numpy(), match=o[1].cpu().numpy(), dist=o[2].cpu().numpy(), owner=o[3].cpu().numpy()), e)
    assert eng.stats()["bytes_device"] > bytes0                            # the job table
    bytes1 = eng.stats()["bytes_device"]
    I.assert_same(I.run_host(eng, b), eb)
    assert eng.stats()["bytes_device"] > bytes1                            # the staged rows and results
    eng.close()


def test_pipelined_frame_stream_is_untouched_by_guided_matching(oracle):
    """A pipelined SURF handle runs an appending frame stream (words numbered on the device); lcd_match_guided_dev calls between the frames
    change no frame output, bit for bit, against a run without them, their own results equal the model, and the vocabulary, the signatures
    and the word numbering end up the same."""
    import rtabmap_amd
    from rtabmap_amd import capi, synth
    from pair_match_inputs import noisy

    def revisit(src):                                                     # noisy copies of an earlier frame's descriptors plus 30 % fresh ones
        out = noisy(rng, src[rng.integers(0, src.shape[0], q)])
        m = rng.random(q) < 0.3
        out[m] = synth.vocab_surf(q, seed=int(rng.integers(1 << 30)))[m]
        return np.ascontiguousarray(out)

    n_words, q, n_sig, T = 3000, 96, 40, 14
    rng = np.random.default_rng(11)
    vocab = synth.vocab_surf(n_words, seed=12)
    words = synth.zipf_words(n_sig, q, n_words, seed=13)
    ids = np.arange(1, n_words + 1, dtype=np.int32)
    history = [vocab[rng.integers(0, n_words, q)] for _ in range(2)]
    for t in range(T):
        history.append(revisit(history[int(rng.integers(len(history)))]))
    frames = [torch.from_numpy(h).cuda() for h in history[2:]]
    points = [I.uniform_points(rng, q) * np.float32(0.4) for _ in range(T)]          # a 256 x 192 image: about six candidates per window
    n_cor = 80
    guided = []                                                           # frame t - 1 projected into frame t
    for t in range(1, T):
        cfr = rng.permutation(q)[:n_cor].astype(np.int32)
        corners = (points[t][rng.integers(0, q, n_cor)] + rng.standard_normal((n_cor, 2)) * 3.0).astype(np.float32)
        guided.append((history[1 + t], history[2 + t], corners, cfr, points[t]))
    exp = [{d: I.expected_batch(oracle, [g], I.RADIUS, 0.8, M.RATIO, d) for d in (M.P2F, M.F2P)} for g in guided]
    assert all(M.outcomes(e[M.P2F], M.P2F) >= {"accepted", "rejected"} for e in exp) and any("contested" in M.outcomes(e[M.P2F], M.P2F) for e in exp)
    dev = [[torch.from_numpy(x).cuda() for x in g[2:]] for g in guided]
    cap = n_sig + T + 4
    out = {}
    for with_guided in (False, True):
        eng = rtabmap_amd.Engine("f32", 64, sig_capacity=cap, pipeline=True)
        eng.vocab_append(vocab, ids)
        eng.sig_add_bulk(np.arange(1, n_sig + 1, dtype=np.int32), np.arange(0, (n_sig + 1) * q, q, dtype=np.int64), words.reshape(-1))
        eng.set_option("next_word_id", n_words + 1)
        d_w = torch.zeros((T, q), dtype=torch.int32, device="cuda")
        d_l = torch.zeros((T, cap), dtype=torch.float32, device="cuda")
        d_first = torch.zeros(T, dtype=torch.int32, device="cuda")
        res = [{d: [torch.full((n,), -7, dtype=torch.int32, device="cuda") for _ in range(2)] +
                   [torch.full((n, 2), -7.0, dtype=torch.float32, device="cuda"), torch.full((q,), -7, dtype=torch.int32, device="cuda")]
                for d, n in ((M.P2F, n_cor), (M.F2P, q))} for _ in guided]
        torch.cuda.synchronize()
        for t in range(T):
            eng.frame_dev(frames[t].data_ptr(), q, n_sig + 1 + t, float(n_sig + 1 + t), d_w[t].data_ptr(), d_l[t].data_ptr(), cap,
                          first_new_word_id=capi.LCD_NEW_WORD_IDS_AUTO, append_new_words=True, d_first_new_word_id_ptr=d_first[t:].data_ptr())
            if with_guided and t >= 1:                                    # between the frames, nothing drained
                for d in (M.P2F, M.F2P):
                    eng.match_guided_dev(frames[t - 1], frames[t], *dev[t - 1], [0, q], [0, q], [0, n_cor], *res[t - 1][d], direction=d)
            if t % 4 == 3:
                eng.sig_remove(1 + t // 4)
        eng.synchronize()
        rows = eng.vocab_count()
        out[with_guided] = (d_w.cpu().numpy(), d_l.cpu().numpy(), d_first.cpu().numpy(), rows, eng.sig_count(), eng.vocab_read(0, rows[0])[1])
        if with_guided:
            for k, (r, e) in enumerate(zip(res, exp)):
                for d in (M.P2F, M.F2P):
                    o = r[d]
                    got = dict(count=o[0].cpu().numpy(), match=o[1].cpu().numpy(), dist=o[2].cpu().numpy(), owner=o[3].cpu().numpy() if d == M.P2F else None)
                    I.assert_same(got, e[d], "pair %d %s" % (k, d))
        eng.close()
    for k in (0, 1, 2, 5):
        np.testing.assert_array_equal(out[True][k], out[False][k])
    assert out[True][3] == out[False][3] and out[True][4] == out[False][4]
    assert out[False][3][0] > n_words + 100                               # the stream did append words
    assert (out[False][2][1:] > n_words).all()                            # ... and numbered them on the device


def test_match_frames_guided_of_the_host_mirror(oracle):
    """VWDictionaryHip::matchFramesGuided through the shim: the model's match under the reference's id bookkeeping, both directions, Vis/CorNNType
    1 and 5, with and without original ids -- and the dictionary that lends its handle keeps its words"""
    from rtabmap_amd.vwdictionary import VWDictionaryHip
    from helpers import unit_rows
    h = VWDictionaryHip(nndr=0.8, new_words_compared_together=True)
    first = h.add_new_words(unit_rows(50, 64, seed=8), 1)
    h.update()
    words = sorted(set(first))
    rng = np.random.default_rng(21)
    for size in [(33, 31, 65), (300, 280, 300), (5, 0, 5), (5, 5, 0), (0, 0, 5)]:
        frm, to, corners, cfr, pts = pair = I.general_case(oracle, "f32", 64, *size)
        orig_ids = (rng.permutation(frm.shape[0]) * 7 + 100).astype(np.int32)
        for to_projection in (False, True):
            for nn_type in (1, 5):
                res = M.guided_pair(oracle, *pair, 40.0, 0.8, M.NEAREST if nn_type == 5 else M.RATIO, M.F2P if to_projection else M.P2F)
                for orig in (None, orig_ids):
                    want = M.guided_word_ids(frm.shape[0], cfr, (res["match"] if to_projection else res["owner"]).tolist(), orig,
                                             None if to_projection else res["count"].tolist())
                    got = h.match_frames_guided(frm, to, corners, cfr, pts, win_size=40, nn_type=nn_type, nndr=0.8, match_to_projection=to_projection,
                                                original_from_ids=orig)
                    assert got == want, (size, to_projection, nn_type, orig is None)
                    if to.shape[0] and not to_projection:
                        assert len(set(got[1])) == len(got[1])             # projected-to-frame never shares an id
        if size == (300, 280, 300):
            shared = M.guided_word_ids(300, cfr, M.guided_pair(oracle, *pair, 40.0, 0.8, M.RATIO, M.F2P)["match"].tolist())[1]
            assert len(set(shared)) < len(shared)                          # frame-to-projected does
    assert h.index_ids() == words and h.visual_words == len(words)
    h.close()
