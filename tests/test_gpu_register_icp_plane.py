"""GPU tests of lcd_register_icp_plane and lcd_register_icp_plane_dev (rtabmap_amd/csrc/register_icp_plane.hip) against
tests/register_icp_plane_model.py.  Every comparison is exact: every int, and every float and double bit for bit, through both entries."""
import numpy as np
import pytest
import torch

import register_icp_plane_inputs as I
import register_icp_plane_model as M
from register_icp_plane_device import (LCD_ERR_INVALID, LCD_ERR_UNSUPPORTED, SEARCHES, expected, assert_same, stage_dev, launch_dev, to_host, run_dev, run_host,
                                       check_both, refused as _refused)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import rtabmap_amd
    e = rtabmap_amd.Engine("f32", 64)
    yield e
    assert e.vocab_count() == (0, 0) and e.sig_count() == (0, 0)
    e.close()


def test_both_entries_equal_the_model_at_every_size(eng):
    """sides of 0, 1, 2, 3, 5, 6, 7, 255, 256, 257, 511, 512 and 513 rows in ONE batch; GRID, BRUTE and AUTO equal"""
    want = check_both(eng, I.size_batch(), searches=SEARCHES, **I.KW)
    assert {M.OK, M.EMPTY, M.NOT_CONVERGED} <= set(want["status"].tolist())
    assert {M.STOP_SINGULAR, M.STOP_FEW_CORRESPONDENCES} <= set(want["stop"].tolist())


def test_8192_rows_on_both_sides(eng):
    pair = I.pair(8192, 8192, 41, noise=0.003)
    kw = dict(I.KW, max_iterations=2)
    want = expected([pair], **kw)
    assert want["stop"][0] == M.STOP_ITERATIONS and want["branch"][0] == 0 and want["n_correspondences"][0] > 2000
    for search in SEARCHES:
        assert_same(run_dev(eng, [pair], search=search, **kw), want, "8192 dev, search %d" % search)
    assert_same(run_host(eng, [pair], **kw), want, "8192 host")
    small = I.size_batch()[14:17]
    batch = [small[0], pair, small[1], small[2]]
    assert_same(run_dev(eng, batch, **kw), expected(batch, **kw), "8192 beside small pairs")


def test_nan_normals_leave_the_loop_but_stay_in_the_ratio(eng):
    """rows 255, 256 and 511 of both sides carry a normal that is not finite -- legal on both entries: they take no part in branch 0, and the
    ratio's denominator still counts them"""
    pairs = [I.with_nan_normals(I.pair(600, 600, 7, noise=0.004)), I.pair(40, 50, 8), I.with_nan_normals(I.pair(513, 512, 9, noise=0.004))]
    want = check_both(eng, pairs, "NaN normals", searches=SEARCHES, **I.KW)
    assert (want["branch"] == 0).all() and (want["match"][[255, 256, 511]] == -1).all()
    assert I.bits(want["ratio"][0]) == I.bits(np.float32(want["n_correspondences"][0]) / np.float32(600))


def test_coordinates_that_are_not_finite(eng):
    """on the device entry such a row takes part in nothing; the host entry refuses"""
    p = I.pair(600, 600, 7, noise=0.004)
    q = I.changed(p)
    q["from_xyz"][[255, 256, 511], [0, 1, 2]] = [np.nan, np.inf, -np.inf]
    q["to_xyz"][[255, 511], [1, 2]] = [np.nan, np.inf]
    want = expected([q], device_entry=True, **I.KW)
    assert_same(run_dev(eng, [q], **I.KW), want, "non-finite coordinates")
    assert I.bits(want["ratio"][0]) == I.bits(np.float32(want["n_correspondences"][0]) / np.float32(598))
    _refused(LCD_ERR_INVALID, run_host, eng, [q], **I.KW)


@pytest.mark.parametrize("name", sorted(I.hand_cases()))
def test_the_hand_made_cases_through_the_device(eng, name):
    """corridor normals (complexity 0, no vectors), strategies 0, 1 and 2, the second value on either side of min_complexity, the 2 oi quirk,
    equal complexities, the gate with failing correspondences among the first `count`, counts of 0, 1 and 2, parallel normals
    (STOP_SINGULAR), force_3dof in both branches"""
    p, kw = I.hand_cases()[name]
    check_both(eng, [p], name, searches=SEARCHES, **kw)


def test_complexity_at_min_complexity_and_one_float_below(eng):
    p, kw, c = I.complexity_edge(M)
    at = check_both(eng, [p], **dict(kw, min_complexity=float(c)))
    below = check_both(eng, [p], **dict(kw, min_complexity=float(np.nextafter(c, np.float32(1)))))
    assert (at["branch"][0], below["branch"][0]) == (0, 1)


def test_the_gate_at_equality_and_one_ulp_either_side(eng):
    p, kw, d = I.gate_edge(M)
    n = [check_both(eng, [p], **dict(kw, min_normal_cos=float(v)))["n_correspondences"][0]
         for v in (np.nextafter(d, np.float32(-1)), d, np.nextafter(d, np.float32(1)))]
    assert n[0] > n[1] and n[1] >= n[2]                                    # at equality the correspondence fails: > is strict


def test_refusals_write_nothing(eng):
    pairs = I.size_batch()[14:16]
    fx, fn, fo, tx, tn, to, gs = I.concatenate(pairs)
    bad = [dict(max_iterations=0), dict(max_laser_scans=-1), dict(search=3), dict(max_correspondence_distance=0.0), dict(max_correspondence_distance=float("nan")),
           dict(max_correspondence_distance=1e200), dict(epsilon=-1.0), dict(correspondence_ratio=1.5), dict(min_complexity=-0.1), dict(min_complexity=1.5),
           dict(min_complexity=float("nan")), dict(low_complexity_strategy=3), dict(low_complexity_strategy=-1),
           dict(normal_gate=True, min_normal_cos=float("nan")), dict(normal_gate=True, min_normal_cos=float("inf"))]
    for kw in bad:
        st = stage_dev(pairs)
        _refused(LCD_ERR_INVALID, launch_dev, eng, st, **dict(I.KW, **kw))
        _refused(LCD_ERR_INVALID, run_host, eng, pairs, **dict(I.KW, **kw))
        got = to_host(eng, st)
        assert (got["status"] == -7).all() and (got["branch"] == -7).all() and (got["match"] == -7).all()
        assert np.isnan(got["transform"]).all() and np.isnan(got["complexity"]).all()
    _refused(LCD_ERR_INVALID, eng.register_icp_plane, fx, fn, fo, tx, tn, to, gs, struct_size=160, **I.KW)
    _refused(LCD_ERR_INVALID, eng.register_icp_plane, fx, None, fo, tx, tn, to, gs, **I.KW)
    _refused(LCD_ERR_INVALID, eng.register_icp_plane, fx, fn, fo, tx, None, to, gs, **I.KW)
    _refused(LCD_ERR_INVALID, eng.register_icp_plane, fx, fn, fo, tx, tn, to, None, **I.KW)
    _refused(LCD_ERR_INVALID, eng.register_icp_plane, fx, fn, fo[::-1].copy(), tx, tn, to, gs, **I.KW)
    big = I.raw(np.zeros((8193, 3)), np.zeros((8193, 3)), np.zeros((3, 3)), np.zeros((3, 3)))
    _refused(LCD_ERR_UNSUPPORTED, run_host, eng, [big], **I.KW)
    z = np.zeros((0, 3), np.float32)
    out = eng.register_icp_plane(z, z, [0], z, z, [0], np.zeros((0, 12), np.float32), **I.KW)
    assert out["status"].shape == (0,)
    # a min_normal_cos that is not finite is legal while the gate is off
    assert_same(run_host(eng, pairs, min_normal_cos=float("nan"), **I.KW), expected(pairs, **I.KW), "after the refusals")


def test_unsynchronised_back_to_back_calls_share_the_scratch(eng):
    """three device calls enqueued without a synchronisation in between, the largest second"""
    batch = I.size_batch()
    groups = [batch[:4], batch[14:], batch[4:8]]
    sts = [launch_dev(eng, stage_dev(g), **I.KW) for g in groups]
    for g, st in zip(groups, sts):
        assert_same(to_host(eng, st), expected(g, **I.KW))


def test_the_point_to_point_entry_is_unchanged_by_a_call_in_between(eng):
    """lcd_register_icp shares the scratch and the job table with the new entry: its results are its model's, before and after"""
    import register_icp_inputs as I0
    import register_icp_model as M0
    p = I0.pair(300, 280, False, 31, guess_off=True)
    want = M0.register(*I0.scans(p), **I0.KW)
    for _ in range(2):
        got = eng.register_icp(p["from_xyz"], [0, 300], p["to_xyz"], [0, 280], p["guess"][None], **I0.KW)
        np.testing.assert_array_equal(I.bits(got["transform"][0]), I.bits(want["transform"]))
        assert got["n_correspondences"][0] == want["n_correspondences"]
        run_host(eng, I.size_batch()[14:16], **I.KW)


def test_the_mirror_class_through_the_engine():
    """RegistrationIcpHip::computeTransformation with normals over a dictionary's engine: the plane rule's transform and the structural
    complexity for two 3-D scans, the point-to-point call for a 2-D scan or a scan without normals"""
    from rtabmap_amd import vwdictionary as V, synth
    import register_icp_model as M0
    p, _ = I.hand_cases()["plane_guess_far"]
    kw = dict(max_iterations=30, max_correspondence_distance=0.3, epsilon=0.0, correspondence_ratio=0.1)
    cos = float(np.cos(np.float64(np.float32(0.78))))
    want = M.register(*I.scans(p), normal_gate=True, min_normal_cos=cos, min_complexity=0.02, low_complexity_strategy=1, **kw)
    d = V.VWDictionaryHip(nndr=0.8, new_words_compared_together=True)
    d.add_new_words(synth.vocab_surf(50, seed=8), 1)
    d.update()
    t, info = d.register_icp_normals(*I.scans(p), max_translation=0.0, max_rotation=0.78, **kw)
    np.testing.assert_array_equal(I.bits(t), I.bits(want["transform"]))
    assert info["icp_correspondences"] == want["n_correspondences"] and I.bits(info["icp_structural_complexity"]) == I.bits(want["complexity"])
    low, lkw = I.hand_cases()["corridor_strategy_0"]
    t, info = d.register_icp_normals(*I.scans(low), max_translation=0.0, max_rotation=0.0, low_complexity_strategy=0, **kw)
    assert t is None and I.bits(info["icp_structural_complexity"]) == I.bits(M.register(*I.scans(low), **lkw)["complexity"])
    p2p = M0.register(p["from_xyz"], p["to_xyz"], p["guess"], **kw)
    for args in (dict(from_is_2d=True), dict(to_is_2d=True), dict(point_to_plane=False)):
        t, info = d.register_icp_normals(*I.scans(p), max_translation=0.0, max_rotation=0.0, **dict(kw, **args))
        np.testing.assert_array_equal(I.bits(t), I.bits(p2p["transform"]))
        assert info["icp_structural_complexity"] == 0
    t, _ = d.register_icp_normals(p["from_xyz"], None, p["to_xyz"], p["to_normals"], p["guess"], max_translation=0.0, max_rotation=0.0, **kw)
    np.testing.assert_array_equal(I.bits(t), I.bits(p2p["transform"]))
    d.close()


def test_pipelined_frame_stream_is_untouched_by_the_registration():
    """A pipelined SURF handle runs an appending frame stream; lcd_register_icp_plane_dev calls between the frames change no frame output, bit
    for bit, against a run without them, and their own results are the model's"""
    import rtabmap_amd
    from rtabmap_amd import capi, synth
    n_words, q, n_sig, T = 2000, 96, 30, 8
    rng = np.random.default_rng(11)
    vocab = synth.vocab_surf(n_words, seed=12)
    words = synth.zipf_words(n_sig, q, n_words, seed=13)
    ids = np.arange(1, n_words + 1, dtype=np.int32)
    frames = []
    for t in range(T):
        d = vocab[rng.integers(0, n_words, q)] + rng.standard_normal((q, 64)).astype(np.float32) * np.float32(0.02)
        fresh = rng.random(q) < 0.3
        d[fresh] = synth.vocab_surf(q, seed=100 + t)[fresh]
        frames.append(torch.from_numpy(np.ascontiguousarray(d, np.float32)).cuda())
    pairs = I.size_batch()[12:18]
    want = expected(pairs, **I.KW)
    cap = n_sig + T + 4
    out = {}
    for with_icp in (False, True):
        eng = rtabmap_amd.Engine("f32", 64, sig_capacity=cap, pipeline=True)
        eng.vocab_append(vocab, ids)
        eng.sig_add_bulk(np.arange(1, n_sig + 1, dtype=np.int32), np.arange(0, (n_sig + 1) * q, q, dtype=np.int64), words.reshape(-1))
        eng.set_option("next_word_id", n_words + 1)
        d_w = torch.zeros((T, q), dtype=torch.int32, device="cuda")
        d_l = torch.zeros((T, cap), dtype=torch.float32, device="cuda")
        d_first = torch.zeros(T, dtype=torch.int32, device="cuda")
        sts = [stage_dev(pairs) for _ in range(T)]
        for t in range(T):
            eng.frame_dev(frames[t].data_ptr(), q, n_sig + 1 + t, float(n_sig + 1 + t), d_w[t].data_ptr(), d_l[t].data_ptr(), cap,
                          first_new_word_id=capi.LCD_NEW_WORD_IDS_AUTO, append_new_words=True, d_first_new_word_id_ptr=d_first[t:].data_ptr())
            if with_icp:                                                # between the frames, nothing drained
                launch_dev(eng, sts[t], **I.KW)
        eng.synchronize()
        out[with_icp] = (d_w.cpu().numpy(), d_l.cpu().numpy(), d_first.cpu().numpy(), eng.vocab_count(), eng.sig_count())
        if with_icp:
            for st in sts:
                assert_same(to_host(eng, st), want, "between frames")
        eng.close()
    for a, b in zip(out[False][:3], out[True][:3]):
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))
    assert out[False][3:] == out[True][3:]
    assert out[True][3][0] > n_words
