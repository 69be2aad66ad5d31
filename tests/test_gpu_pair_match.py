"""GPU tests of lcd_match_pairs / lcd_match_pairs_dev (rtabmap_amd/csrc/pair_match.hip) against tests/pair_match_model.py: the temporary
two-frame dictionary against the restated VWDictionary, the cross-check rule against its NumPy model over the oracle's distances.  Every
comparison is exact: ids, indices and distance bits."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import pair_match_model as M
from helpers import unit_rows

pytestmark = pytest.mark.gpu

KINDS = [("f32", 64), ("f32", 128), ("f32", 256), ("u8", 32), ("u8", 64)]
SIZES = [(0, 5), (5, 0), (1, 1), (1, 3), (2, 2), (31, 33), (64, 65), (257, 129), (300, 40)]
LCD_ERR_INVALID, LCD_ERR_UNSUPPORTED = 1, 5


def _fresh(rng, dtype, dim, n):
    if dtype == "u8":
        return rng.integers(0, 256, (n, dim), dtype=np.uint8)
    return unit_rows(n, dim, seed=int(rng.integers(1 << 30))) if n else np.zeros((0, dim), np.float32)


def _noisy(rng, dtype, rows):
    out = rows.copy()
    if dtype == "u8":
        out ^= np.packbits(rng.random((out.shape[0], out.shape[1] * 8)) < 0.02, axis=1)
    elif out.shape[0]:
        out += rng.standard_normal(out.shape).astype(np.float32) * np.float32(0.02)
        out /= np.linalg.norm(out, axis=1, keepdims=True)
    return out


def _pair(dtype, dim, nf, nt, seed):
    """the temporary-dictionary test's input: 3/4 noisy copies of from-rows (sigma 0.02, or 2 % bit flips) plus 1/4 fresh rows; the two
    one-from-row sizes have identical rows"""
    rng = np.random.default_rng(seed)
    frm = _fresh(rng, dtype, dim, nf)
    if nf == 1:
        return frm, np.ascontiguousarray(np.repeat(frm, nt, axis=0))
    n_copy = nt * 3 // 4 if nf else 0
    to = np.concatenate([_noisy(rng, dtype, frm[rng.integers(0, max(nf, 1), n_copy)]) if n_copy else frm[:0], _fresh(rng, dtype, dim, nt - n_copy)])
    return np.ascontiguousarray(frm), np.ascontiguousarray(to)


def _dup_pair(dtype, dim, seed):
    """exact duplicates inside `from` and inside `to`: best and second-best distance are both 0"""
    rng = np.random.default_rng(seed)
    b = _fresh(rng, dtype, dim, 9)
    return np.ascontiguousarray(b[[0, 1, 0, 2, 1, 3, 0, 4]]), np.ascontiguousarray(b[[0, 0, 5, 5, 1, 6, 2, 2, 2, 7, 5]])


def _tie_pair(dtype, dim, nf, nt, seed):
    """a few distinct rows repeated on both sides: ties in both directions of the cross-check"""
    rng = np.random.default_rng(seed)
    b = _fresh(rng, dtype, dim, 6)
    return np.ascontiguousarray(b[rng.integers(0, 5, nf)]), np.ascontiguousarray(b[rng.integers(1, 6, nt)])


@functools.lru_cache(maxsize=None)
def _pairs(dtype, dim):
    ps = [_pair(dtype, dim, nf, nt, 1000 + 17 * k + dim) for k, (nf, nt) in enumerate(SIZES)]
    ps.append(_dup_pair(dtype, dim, 77 + dim))
    return ps


@functools.lru_cache(maxsize=None)
def _dictionary_expected(dtype, dim, compared):
    import oracle
    return [M.dictionary_pair(oracle, f, t, 0.8, compared) for f, t in _pairs(dtype, dim)]


def _concat(pairs):
    fo = np.cumsum([0] + [f.shape[0] for f, _ in pairs]).astype(np.int64)
    to = np.cumsum([0] + [t.shape[0] for _, t in pairs]).astype(np.int64)
    return np.concatenate([f for f, _ in pairs]), np.concatenate([t for _, t in pairs]), fo, to


def _dev(eng, pairs, mode, ids=None, **kw):
    """the batch through lcd_match_pairs_dev, results read back"""
    f, t, fo, to = _concat(pairs)
    d_f, d_t = torch.from_numpy(f).cuda(), torch.from_numpy(t).cuda()
    d_ids = None if ids is None else torch.from_numpy(np.concatenate(ids).astype(np.int32)).cuda()
    if mode == "dictionary":
        o1 = torch.full((f.shape[0],), -7, dtype=torch.int32, device="cuda")
        o2 = torch.full((t.shape[0],), -7, dtype=torch.int32, device="cuda")
    else:
        o1 = torch.full((t.shape[0],), -7, dtype=torch.int32, device="cuda")
        o2 = torch.full((t.shape[0],), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    eng.match_pairs_dev(d_f, d_t, fo, to, o1, o2, mode, d_from_word_ids=d_ids, **kw)
    eng.synchronize()
    return o1.cpu().numpy(), o2.cpu().numpy(), fo, to


def _dist(oracle, to, frm):
    """D[to-row][from-row] with the engine's bits: squared L2 in the reference's order, Hamming over EVERY byte (cv::NORM_HAMMING; the
    oracle's default Hamming is rtflann's, which skips the bytes behind a multiple of 8 -- it matters for 61-byte rows only)"""
    if to.shape[0] == 0 or frm.shape[0] == 0:
        return np.zeros((to.shape[0], frm.shape[0]), np.float32)
    return oracle.dist_matrix(to, frm, metric=oracle.METRIC_HAMMING_CV if to.dtype == np.uint8 else None)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("compared", [True, False], ids=["together", "apart"])
@pytest.mark.parametrize("dtype,dim", KINDS)
def test_dictionary_mode_equals_the_temporary_dictionary(oracle, dtype, dim, compared):
    import rtabmap_amd
    pairs, exp = _pairs(dtype, dim), _dictionary_expected(dtype, dim, compared)
    # what the sizes are there for: one from-word leaves the to-frame without an indexed search (its rows are new words, or copies of
    # the first of them); the duplicates make from-rows share words only when new words are compared together
    assert exp[2][1].tolist() == [2] and exp[3][0].tolist() == [1]
    assert exp[3][1].tolist()[:2] == [2, 3] and (exp[3][1][2] == 4) == (not compared)
    assert (len(set(exp[-1][0].tolist())) < len(exp[-1][0])) == compared
    assert len(set(exp[7][0].tolist()) & set(exp[7][1].tolist())) > 40
    eng = rtabmap_amd.Engine(dtype, dim)
    for k, ((f, t), (ef, et)) in enumerate(zip(pairs, exp)):
        gf, gt = eng.match_pair(f, t, "dictionary", new_words_compared=compared)
        np.testing.assert_array_equal(gf, ef, err_msg="pair %d from" % k)
        np.testing.assert_array_equal(gt, et, err_msg="pair %d to" % k)
    # the same through one host batch and through the device entry
    f, t, fo, to = _concat(pairs)
    gf, gt = eng.match_pairs(f, t, fo, to, "dictionary", new_words_compared=compared)
    np.testing.assert_array_equal(gf, np.concatenate([e[0] for e in exp]))
    np.testing.assert_array_equal(gt, np.concatenate([e[1] for e in exp]))
    df, dt, _, _ = _dev(eng, pairs, "dictionary", new_words_compared=compared)
    np.testing.assert_array_equal(df, gf)
    np.testing.assert_array_equal(dt, gt)
    assert eng.vocab_count() == (0, 0) and eng.sig_count() == (0, 0)
    eng.close()


@pytest.mark.parametrize("dtype,dim", KINDS)
def test_dictionary_mode_with_given_from_ids(oracle, dtype, dim):
    """orignalWordsFromIds: sparse, unsorted ids with max >> n -- echoed, vocabulary rows in ascending id (the tie-break: the duplicate
    from-rows of the last pair meet at distance 0), the to-frame numbered from max + 1"""
    import rtabmap_amd
    pairs = [_pairs(dtype, dim)[k] for k in (0, 1, 3, 4, 5, 7, 9)]
    rng = np.random.default_rng(3 + dim)
    ids = [rng.permutation(np.arange(3, 3 + 9973 * max(f.shape[0], 1), 9973))[: f.shape[0]].astype(np.int32) for f, _ in pairs]
    assert ids[5].max() > 1000 * ids[5].size and (np.diff(ids[5]) < 0).any()
    exp = [M.dictionary_pair(oracle, f, t, 0.8, True, from_word_ids=i) for (f, t), i in zip(pairs, ids)]
    assert exp[-1][1][0] == min(ids[-1][[0, 2, 6]])                      # to-row 0 == from-rows 0, 2, 6: the lowest ID wins, not the lowest row
    assert exp[5][1].max() > ids[5].max()                                 # new words continue behind the highest given id
    eng = rtabmap_amd.Engine(dtype, dim)
    f, t, fo, to = _concat(pairs)
    gf, gt = eng.match_pairs(f, t, fo, to, "dictionary", from_word_ids=np.concatenate(ids))
    np.testing.assert_array_equal(gf, np.concatenate(ids))
    np.testing.assert_array_equal(gt, np.concatenate([e[1] for e in exp]))
    df, dt, _, _ = _dev(eng, pairs, "dictionary", ids=ids)
    np.testing.assert_array_equal(df, gf)
    np.testing.assert_array_equal(dt, gt)
    eng.close()


def _cross_inputs(dtype, dim):
    pairs = list(_pairs(dtype, dim))
    ties = []
    for k, (nf, nt) in enumerate(SIZES[3:], 3):
        for attempt in range(50):                                         # an input without the three properties is replaced, not skipped
            p = _tie_pair(dtype, dim, max(nf, 6), max(nt, 6), 500 + 31 * k + 1000 * attempt + dim)
            import oracle
            D = _dist(oracle, p[1], p[0])
            m, _ = M.cross_check(D)
            if (m >= 0).any() and (m < 0).any() and M.tie_resolved_by_index(D):
                break
        ties.append(p)
    return pairs, ties


@pytest.mark.parametrize("dtype,dim", KINDS)
def test_cross_check_mode_equals_the_model(oracle, dtype, dim):
    import rtabmap_amd
    pairs, ties = _cross_inputs(dtype, dim)
    for f, t in ties:                                                     # asserted here, on the model's output
        D = _dist(oracle, t, f)
        m, _ = M.cross_check(D)
        assert (m >= 0).any() and (m < 0).any() and M.tie_resolved_by_index(D)
    allp = pairs + ties
    exp = [M.cross_check(_dist(oracle, t, f)) for f, t in allp]
    eng = rtabmap_amd.Engine(dtype, dim)
    for k, ((f, t), (em, ed)) in enumerate(zip(allp, exp)):
        gm, gd = eng.match_pair(f, t, "cross_check")
        np.testing.assert_array_equal(gm, em, err_msg="pair %d" % k)
        np.testing.assert_array_equal(_bits(gd), _bits(ed), err_msg="pair %d" % k)
    dm, dd, _, _ = _dev(eng, allp, "cross_check")
    np.testing.assert_array_equal(dm, np.concatenate([e[0] for e in exp]))
    np.testing.assert_array_equal(_bits(dd), _bits(np.concatenate([e[1] for e in exp])))
    eng.close()


def test_padded_rows_through_the_host_entry(oracle):
    """61-byte rows (AKAZE) are stored zero-padded: the host entry pads them as it stages them, the device entry refuses the handle"""
    import rtabmap_amd
    from rtabmap_amd import capi
    pairs = [_pair("u8", 61, nf, nt, 40 + nf) for nf, nt in ((31, 33), (64, 65), (1, 3), (0, 5))] + [_dup_pair("u8", 61, 5)]
    eng = rtabmap_amd.Engine("u8", 61)
    f, t, fo, to = _concat(pairs)
    for compared in (True, False):
        gf, gt = eng.match_pairs(f, t, fo, to, "dictionary", new_words_compared=compared)
        exp = [M.dictionary_pair(oracle, a, b, 0.8, compared) for a, b in pairs]
        np.testing.assert_array_equal(gf, np.concatenate([e[0] for e in exp]))
        np.testing.assert_array_equal(gt, np.concatenate([e[1] for e in exp]))
    gm, gd = eng.match_pairs(f, t, fo, to, "cross_check")
    exp = [M.cross_check(_dist(oracle, b, a)) for a, b in pairs]
    assert not np.array_equal(oracle.dist_matrix(pairs[0][1], pairs[0][0]), _dist(oracle, pairs[0][1], pairs[0][0]))   # the last 5 bytes count
    np.testing.assert_array_equal(gm, np.concatenate([e[0] for e in exp]))
    np.testing.assert_array_equal(_bits(gd), _bits(np.concatenate([e[1] for e in exp])))
    with pytest.raises(capi.LcdError) as e:
        _dev(eng, pairs, "cross_check")
    assert e.value.status == LCD_ERR_UNSUPPORTED
    np.testing.assert_array_equal(eng.match_pairs(f, t, fo, to, "cross_check")[0], gm)      # the handle stays usable
    eng.close()


SEVEN = [(40, 33), (0, 9), (130, 70), (12, 0), (1, 1), (65, 64), (7, 200)]


@pytest.mark.parametrize("dtype,dim", [("f32", 64), ("u8", 32)])
def test_a_batch_equals_its_single_calls(dtype, dim):
    """seven pairs of different sizes, an empty `to` and an empty `from` among them, in one call"""
    import rtabmap_amd
    pairs = [_pair(dtype, dim, nf, nt, 900 + k) for k, (nf, nt) in enumerate(SEVEN)]
    eng = rtabmap_amd.Engine(dtype, dim)
    f, t, fo, to = _concat(pairs)
    for mode in ("dictionary", "cross_check"):
        single = [eng.match_pair(a, b, mode) for a, b in pairs]
        g1, g2 = eng.match_pairs(f, t, fo, to, mode)
        np.testing.assert_array_equal(g1, np.concatenate([s[0] for s in single]))
        np.testing.assert_array_equal(_bits(g2) if mode == "cross_check" else g2, np.concatenate([_bits(s[1]) if mode == "cross_check" else s[1] for s in single]))
        d1, d2, _, _ = _dev(eng, pairs, mode)
        np.testing.assert_array_equal(d1, g1)
        np.testing.assert_array_equal(_bits(d2) if mode == "cross_check" else d2, _bits(g2) if mode == "cross_check" else g2)
    assert g1[to[1]:to[2]].tolist() == [-1] * 9 and (g2[to[1]:to[2]] == -1.0).all()        # cross-check against an empty `from`
    eng.close()


def test_groups_and_scratch_growth_do_not_change_results():
    """"pair_match_budget" (tests) forces the batch into several groups of pairs; two device calls in a row without a synchronisation in
    between (the second reuses the scratch and the job-table slots of the first, and makes the scratch grow); the scratch is counted"""
    import rtabmap_amd
    pairs = [_pair("f32", 64, nf, nt, 300 + k) for k, (nf, nt) in enumerate(SEVEN)]
    big = pairs + [_pair("f32", 64, 200, 260, 399)] + pairs[::-1]
    ref = rtabmap_amd.Engine("f32", 64)
    exp = {m: ref.match_pairs(*_concat(pairs), m) for m in ("dictionary", "cross_check")}
    exp_big = ref.match_pairs(*_concat(big), "dictionary")
    ref.close()
    eng = rtabmap_amd.Engine("f32", 64)
    bytes0 = eng.stats()["bytes_device"]
    eng.set_option("pair_match_budget", 64 << 10)                          # 16 384 distances: most pairs are a group of their own
    f, t, fo, to = _concat(pairs)
    fb, tb, fob, tob = _concat(big)
    d = [torch.from_numpy(x).cuda() for x in (f, t, fb, tb)]
    o = [torch.full((n,), -7, dtype=torch.int32, device="cuda") for n in (f.shape[0], t.shape[0], fb.shape[0], tb.shape[0], t.shape[0])]
    od = torch.full((t.shape[0],), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    eng.match_pairs_dev(d[0], d[1], fo, to, o[0], o[1], "dictionary")
    eng.match_pairs_dev(d[2], d[3], fob, tob, o[2], o[3], "dictionary")   # larger: the scratch grows behind the first call's work
    eng.match_pairs_dev(d[0], d[1], fo, to, o[4], od, "cross_check")
    eng.synchronize()
    np.testing.assert_array_equal(o[0].cpu().numpy(), exp["dictionary"][0])
    np.testing.assert_array_equal(o[1].cpu().numpy(), exp["dictionary"][1])
    np.testing.assert_array_equal(o[2].cpu().numpy(), exp_big[0])
    np.testing.assert_array_equal(o[3].cpu().numpy(), exp_big[1])
    np.testing.assert_array_equal(o[4].cpu().numpy(), exp["cross_check"][0])
    np.testing.assert_array_equal(_bits(od.cpu().numpy()), _bits(exp["cross_check"][1]))
    assert eng.stats()["bytes_device"] > bytes0
    for m in ("dictionary", "cross_check"):                               # and the host entry under the same budget
        g = eng.match_pairs(f, t, fo, to, m)
        np.testing.assert_array_equal(g[0], exp[m][0])
        np.testing.assert_array_equal(_bits(g[1]), _bits(exp[m][1]))
    eng.close()


def test_pipelined_frame_stream_is_untouched_by_pair_matching():
    """A pipelined SURF handle runs an appending frame stream (words numbered on the device); lcd_match_pairs_dev calls between the frames
    change no frame output, bit for bit, against a run without them, their own results equal a plain handle's, and the vocabulary, the
    signatures and the word numbering end up the same."""
    import rtabmap_amd
    from rtabmap_amd import capi, synth

    def revisit(src):                                                     # noisy copies of an earlier frame's descriptors plus 30 % fresh ones
        out = _noisy(rng, "f32", src[rng.integers(0, src.shape[0], q)])
        m = rng.random(q) < 0.3
        out[m] = synth.vocab_surf(q, seed=int(rng.integers(1 << 30)))[m]
        return np.ascontiguousarray(out)

    n_words, q, n_sig, T = 3000, 96, 40, 14
    rng = np.random.default_rng(11)
    vocab = synth.vocab_surf(n_words, seed=12)
    words = synth.zipf_words(n_sig, q, n_words, seed=13)
    ids = np.arange(1, n_words + 1, dtype=np.int32)
    history = [vocab[rng.integers(0, n_words, q)] for _ in range(2)]
    frames = []
    for t in range(T):
        history.append(revisit(history[int(rng.integers(len(history)))]))
        frames.append(torch.from_numpy(history[-1]).cuda())
    pairs = [(history[2 + t], history[3 + t]) for t in range(T - 1)]
    plain = rtabmap_amd.Engine("f32", 64)
    exp = [(plain.match_pair(a, b, "dictionary"), plain.match_pair(a, b, "cross_check")) for a, b in pairs]
    plain.close()
    cap = n_sig + T + 4
    out = {}
    for with_pairs in (False, True):
        eng = rtabmap_amd.Engine("f32", 64, sig_capacity=cap, pipeline=True)
        eng.vocab_append(vocab, ids)
        eng.sig_add_bulk(np.arange(1, n_sig + 1, dtype=np.int32), np.arange(0, (n_sig + 1) * q, q, dtype=np.int64), words.reshape(-1))
        eng.set_option("next_word_id", n_words + 1)
        d_w = torch.zeros((T, q), dtype=torch.int32, device="cuda")
        d_l = torch.zeros((T, cap), dtype=torch.float32, device="cuda")
        d_first = torch.zeros(T, dtype=torch.int32, device="cuda")
        res = [[torch.full((q,), -7, dtype=torch.int32, device="cuda") for _ in range(3)] + [torch.full((q,), -7.0, dtype=torch.float32, device="cuda")]
               for _ in pairs]
        torch.cuda.synchronize()
        for t in range(T):
            eng.frame_dev(frames[t].data_ptr(), q, n_sig + 1 + t, float(n_sig + 1 + t), d_w[t].data_ptr(), d_l[t].data_ptr(), cap,
                          first_new_word_id=capi.LCD_NEW_WORD_IDS_AUTO, append_new_words=True, d_first_new_word_id_ptr=d_first[t:].data_ptr())
            if with_pairs and t >= 1:                                     # the verification of the hypothesis "frame t - 1": between the frames, nothing drained
                r = res[t - 1]
                eng.match_pairs_dev(frames[t - 1], frames[t], [0, q], [0, q], r[0], r[1], "dictionary")
                eng.match_pairs_dev(frames[t - 1], frames[t], [0, q], [0, q], r[2], r[3], "cross_check")
            if t % 4 == 3:
                eng.sig_remove(1 + t // 4)
        eng.synchronize()
        rows = eng.vocab_count()
        out[with_pairs] = (d_w.cpu().numpy(), d_l.cpu().numpy(), d_first.cpu().numpy(), rows, eng.sig_count(), eng.vocab_read(0, rows[0])[1])
        if with_pairs:
            for k, (r, (ed, ec)) in enumerate(zip(res, exp)):
                np.testing.assert_array_equal(r[0].cpu().numpy(), ed[0], err_msg="pair %d" % k)
                np.testing.assert_array_equal(r[1].cpu().numpy(), ed[1], err_msg="pair %d" % k)
                np.testing.assert_array_equal(r[2].cpu().numpy(), ec[0], err_msg="pair %d" % k)
                np.testing.assert_array_equal(_bits(r[3].cpu().numpy()), _bits(ec[1]), err_msg="pair %d" % k)
        eng.close()
    for k in (0, 1, 2, 5):
        np.testing.assert_array_equal(out[True][k], out[False][k])
    assert out[True][3] == out[False][3] and out[True][4] == out[False][4]
    assert out[False][3][0] > n_words + 100                               # the stream did append words
    assert (out[False][2][1:] > n_words).all()                            # ... and numbered them on the device


def test_errors_leave_nothing_written_and_the_handle_usable():
    import rtabmap_amd
    from rtabmap_amd import capi
    eng = rtabmap_amd.Engine("f32", 64)
    f, t = _pair("f32", 64, 20, 24, 1)
    good = eng.match_pair(f, t, "dictionary")
    ids = np.arange(1, 21, dtype=np.int32)

    def call(entry="lcd_match_pairs", n_pairs=1, fo=(0, 20), to=(0, 24), mode=0, flags=3, size=None, frm=f, dst=t, out_from=True, out_to=True,
             out_match=True, from_ids=None):
        fo_a, to_a = np.asarray(fo or [0], np.int64), np.asarray(to or [0], np.int64)
        of, ot, om = np.full(64, -7, np.int32), np.full(64, -7, np.int32), np.full(64, -7, np.int32)
        a = capi.LcdMatchArgs(C.sizeof(capi.LcdMatchArgs) if size is None else size, mode, n_pairs, flags, 0.8, 0)
        a.from_rows, a.to_rows = (None if frm is None else frm.ctypes.data), (None if dst is None else dst.ctypes.data)
        a.from_offsets, a.to_offsets = (None if fo is None else fo_a.ctypes.data), (None if to is None else to_a.ctypes.data)
        a.from_word_ids = None if from_ids is None else from_ids.ctypes.data
        a.out_from_word_ids, a.out_to_word_ids, a.out_to_match = (of.ctypes.data if out_from else None), (ot.ctypes.data if out_to else None), (om.ctypes.data if out_match else None)
        rc = getattr(eng.L, entry)(eng.h, C.byref(a))
        assert (of == -7).all() and (ot == -7).all() and (om == -7).all()       # nothing written
        return rc

    def usable():
        g = eng.match_pair(f, t, "dictionary")
        np.testing.assert_array_equal(g[0], good[0])
        np.testing.assert_array_equal(g[1], good[1])

    big = np.zeros((8193, 64), np.float32)
    cases = [
        (LCD_ERR_UNSUPPORTED, dict(frm=big, fo=(0, 8193))),                              # more than 8192 rows on one side
        (LCD_ERR_UNSUPPORTED, dict(dst=big, to=(0, 8193), mode=1)),
        (LCD_ERR_UNSUPPORTED, dict(n_pairs=65536, fo=None, to=None)),
        (LCD_ERR_INVALID, dict(fo=(1, 20))),                                             # offsets: not starting at 0, decreasing, missing
        (LCD_ERR_INVALID, dict(n_pairs=2, fo=(0, 20, 10), to=(0, 12, 24))),
        (LCD_ERR_INVALID, dict(to=None)),
        (LCD_ERR_INVALID, dict(out_from=False)),                                         # NULL where the mode needs an output
        (LCD_ERR_INVALID, dict(out_to=False)),
        (LCD_ERR_INVALID, dict(mode=1, out_match=False)),
        (LCD_ERR_INVALID, dict(frm=None)),
        (LCD_ERR_INVALID, dict(size=88)),                                                # wrong struct_size
        (LCD_ERR_INVALID, dict(mode=2)),
        (LCD_ERR_INVALID, dict(n_pairs=-1)),
        (LCD_ERR_INVALID, dict(flags=2)),                                                # a fixed dictionary
        (LCD_ERR_INVALID, dict(from_ids=np.where(ids == 5, 0, ids).astype(np.int32))),   # ids: not > 0, repeated
        (LCD_ERR_INVALID, dict(from_ids=np.where(ids == 5, 9, ids).astype(np.int32))),
    ]
    for want, kw in cases:
        assert call(**kw) == want, kw
        assert eng.L.lcd_last_error(eng.h)
        usable()
    assert call(n_pairs=0, fo=None, to=None) == 0                                        # no pairs: LCD_OK, nothing touched
    assert call(entry="lcd_match_pairs_dev", size=88) == LCD_ERR_INVALID
    usable()
    eng.close()


def test_match_frames_of_the_host_mirror(oracle):
    """VWDictionaryHip::matchFrames (RegistrationVis.cpp:1383-1504) over the dictionary's own long-lived handle: Vis/CorNNType 1 equals the
    temporary dictionary, type 5 the cross-check with the reference's id bookkeeping, with and without original ids -- and the dictionary
    that lends its handle keeps its words and its numbering"""
    from rtabmap_amd.vwdictionary import VWDictionaryHip
    pairs = [_pairs("f32", 64)[k] for k in (0, 1, 3, 5, 7, 9)]
    h = VWDictionaryHip(nndr=0.8, new_words_compared_together=True)
    own = unit_rows(50, 64, seed=8)
    o = oracle.OracleVWDictionary(strategy=oracle.kNNBruteForce, nndr=0.8, new_words_compared_together=True)
    first = h.add_new_words(own, 1)
    h.update()
    o_first = o.add_new_words(own, 1)
    o.update()
    words = sorted(set(first))
    assert first == o_first and h.index_ids() == words and len(words) > 40
    rng = np.random.default_rng(21)
    for k, (f, t) in enumerate(pairs):
        ef, et = M.dictionary_pair(oracle, f, t, 0.8, True)
        assert h.match_frames(f, t, nn_type=1) == (ef.tolist(), et.tolist()), k
        ids = (rng.permutation(f.shape[0]) * 7 + 100).astype(np.int32)
        ef, et = M.dictionary_pair(oracle, f, t, 0.8, True, from_word_ids=ids)
        assert h.match_frames(f, t, nn_type=3, original_from_ids=ids) == (ef.tolist(), et.tolist()), k
        m, _ = M.cross_check(_dist(oracle, t, f))
        for orig in (None, ids):
            fid = list(range(1, f.shape[0] + 1)) if orig is None else orig.tolist()
            last = fid[-1] if fid else 0
            tid = [fid[j] if j >= 0 else last + i + 1 for i, j in enumerate(m.tolist())]
            assert h.match_frames(f, t, nn_type=5, original_from_ids=orig) == (fid, tid), k
    assert h.index_ids() == words and h.visual_words == len(words)
    nxt = o.add_new_words(-own[:3], 2)
    assert max(nxt) > words[-1] and h.add_new_words(-own[:3], 2) == nxt    # the numbering went on where it stood
    o.close()
    h.close()
