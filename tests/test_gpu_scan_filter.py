"""GPU tests of lcd_filter_scans and lcd_filter_scans_dev (rtabmap_amd/csrc/scan_filter.hip) against tests/scan_filter_model.py.  Every
comparison is exact: every int, and every float bit for bit -- the NaN padding of the regions included --, through both entries.  Outputs are
canary-filled (7.0 / -7), so what a call left alone shows."""
import numpy as np
import pytest
import torch

import scan_filter_inputs as I
import scan_filter_model as M

pytestmark = pytest.mark.gpu

LCD_ERR_INVALID, LCD_ERR_UNSUPPORTED = 1, 5
INTS = ("count", "status", "stage_counts")
_model_cache = {}


def expected(name, scans, caps, device_entry=False, **kw):
    key = (name, device_entry, tuple(sorted(kw.items())))
    if key not in _model_cache:
        _model_cache[key] = M.filter_scans(scans, caps, device_entry=device_entry, **kw)
    return _model_cache[key]


def assert_same(got, want, what=""):
    for k in INTS:
        np.testing.assert_array_equal(got[k], want[k], err_msg="%s %s" % (what, k))
    np.testing.assert_array_equal(I.bits(got["xyz"]), I.bits(want["xyz"]), err_msg=what + " xyz")
    if want["normals"] is not None:
        np.testing.assert_array_equal(I.bits(got["normals"]), I.bits(want["normals"]), err_msg=what + " normals")


def stage_dev(scans, caps=None, normals=True):
    """the batch on the device, outputs canary-filled, uploaded and synchronised"""
    x, off, oo = I.concatenate(scans, caps)
    n, m = len(scans), int(oo[-1])
    out = dict(xyz=torch.full((max(m, 1), 3), 7.0, dtype=torch.float32, device="cuda"),
               normals=torch.full((max(m, 1), 3), 7.0, dtype=torch.float32, device="cuda") if normals else None,
               count=torch.full((n,), -7, dtype=torch.int32, device="cuda"), stage_counts=torch.full((n, 3), -7, dtype=torch.int32, device="cuda"),
               status=torch.full((n,), -7, dtype=torch.int32, device="cuda"))
    st = dict(x=torch.from_numpy(np.ascontiguousarray(x)).cuda() if x.shape[0] else None, off=off, oo=oo, out=out, m=m)
    torch.cuda.synchronize()
    return st


def launch_dev(eng, st, **kw):
    eng.filter_scans_dev(st["x"], st["off"], st["oo"], st["out"], **kw)
    return st


def to_host(eng, st):
    eng.synchronize()
    out = {k: (None if v is None else v.cpu().numpy()) for k, v in st["out"].items()}
    out["xyz"] = out["xyz"][:st["m"]]
    if out["normals"] is not None:
        out["normals"] = out["normals"][:st["m"]]
    return out


def with_normals(kw):
    return kw.get("normal_k", 0) > 0 or kw.get("normal_radius", 0) > 0


def run_dev(eng, scans, caps=None, **kw):
    return to_host(eng, launch_dev(eng, stage_dev(scans, caps, with_normals(kw)), **kw))


def run_host(eng, scans, caps=None, **kw):
    x, off, oo = I.concatenate(scans, caps)
    return eng.filter_scans(x, off, oo, **kw)


def check_both(eng, name, scans, caps=None, device_only=False, **kw):
    want = expected(name, scans, caps, device_entry=True, **kw)
    assert_same(run_dev(eng, scans, caps, **kw), want, name + " dev")
    if not device_only:                                                  # every row is finite: the host entry's rule is the same
        assert_same(run_host(eng, scans, caps, **kw), want, name + " host")
    return want


def _refused(status, call, *args, **kw):
    from rtabmap_amd import capi
    with pytest.raises(capi.LcdError) as err:
        call(*args, **kw)
    assert err.value.status == status, err.value


@pytest.fixture(scope="module")
def eng():
    import rtabmap_amd
    e = rtabmap_amd.Engine("f32", 64)
    yield e
    assert e.vocab_count() == (0, 0) and e.sig_count() == (0, 0)
    e.close()


@pytest.mark.parametrize("kw", [dict(), dict(voxel_size=0.2), dict(voxel_size=0.2, normal_k=5), dict(normal_radius=0.3), dict(downsampling_step=2, normal_k=8)],
                         ids=["plain", "voxel", "voxel_k5", "radius", "step2_k8"])
def test_both_entries_equal_the_model_at_every_size(eng, kw):
    """0, 1, 2, 3, 4, 5, 6, 255, 256, 257, 511, 512 and 513 rows in ONE batch with empty scans between"""
    want = check_both(eng, "sizes", I.size_batch(), **kw)
    assert {M.OK, M.EMPTY} <= set(want["status"].tolist())


@pytest.mark.parametrize("name", sorted(I.cases()))
def test_the_hand_made_cases_through_the_device(eng, name):
    """steps and ranges at their edges, rows that are not finite, the voxel grid's runs, signs and limits, K mode at every instantiation's edge,
    ties, duplicates, degenerate clouds, radius mode at d2 == r2, the flip at a dot product of 0, the ground rule, the capacities"""
    c = I.cases()[name]
    check_both(eng, name, c["scans"], c["caps"], c["device_only"], **c["kw"])


def test_the_ground_rule_at_equality_and_one_float_below(eng):
    scan, kw, up_equal, up_below = I.ground_edge(M)
    a = check_both(eng, "ground_equal", [scan], ground_normals_up=up_equal, **kw)
    b = check_both(eng, "ground_below", [scan], ground_normals_up=up_below, **kw)
    turned = (I.bits(a["normals"]) != I.bits(b["normals"])).any(axis=1)
    assert turned.any() and (a["xyz"][turned, 2] < 10).all()


def test_8192_rows_reach_the_normals_and_8193_do_not(eng):
    scan = I.spread(8193, 21)
    want = check_both(eng, "8192", [scan[:8192], I.cloud(300, 22)], normal_k=5)
    assert want["status"].tolist() == [M.OK, M.OK] and want["count"][0] == 8192
    want = check_both(eng, "8193", [scan, I.cloud(300, 22)], normal_k=5)
    assert want["status"].tolist() == [M.TOO_MANY_ROWS, M.OK] and want["stage_counts"][0].tolist() == [8193, 8193, 0]


def test_16384_sampled_rows_pass_and_16385_are_refused(eng):
    scan = I.spread(32770, 23)
    kw = dict(downsampling_step=2, voxel_size=0.5, normal_k=5)
    want = check_both(eng, "16384", [scan[:32769], I.cloud(300, 24)], **kw)
    assert want["status"].tolist() == [M.OK, M.OK] and want["stage_counts"][0, 0] == 16384 and want["stage_counts"][0, 1] <= 8192
    st = stage_dev([scan], None, True)
    _refused(LCD_ERR_UNSUPPORTED, launch_dev, eng, st, **kw)
    _refused(LCD_ERR_UNSUPPORTED, run_host, eng, [scan], **kw)
    got = to_host(eng, st)
    assert (got["status"] == -7).all() and (got["xyz"] == 7.0).all() and (got["normals"] == 7.0).all()


def test_refusals_write_nothing(eng):
    scans = [I.cloud(300, 31), I.cloud(40, 32)]
    x, off, oo = I.concatenate(scans)
    base = dict(voxel_size=0.2, normal_k=5)
    bad = [(LCD_ERR_INVALID, dict(normal_radius=0.3)), (LCD_ERR_INVALID, dict(normal_k=33)), (LCD_ERR_INVALID, dict(normal_k=-1)),
           (LCD_ERR_INVALID, dict(voxel_size=-0.1)), (LCD_ERR_INVALID, dict(normal_k=0, normal_radius=-1.0)), (LCD_ERR_INVALID, dict(ground_normals_up=-0.5)),
           (LCD_ERR_INVALID, dict(voxel_size=float("nan"))), (LCD_ERR_INVALID, dict(range_min=float("inf"))), (LCD_ERR_INVALID, dict(range_max=float("nan"))),
           (LCD_ERR_INVALID, dict(viewpoint=(0.0, float("inf"), 0.0))), (LCD_ERR_INVALID, dict(ground_normals_up=float("nan"))),
           (LCD_ERR_UNSUPPORTED, dict(is_2d=True))]
    for code, kw in bad:
        st = stage_dev(scans)
        _refused(code, launch_dev, eng, st, **dict(base, **kw))
        _refused(code, run_host, eng, scans, **dict(base, **kw))
        got = to_host(eng, st)
        assert (got["status"] == -7).all() and (got["count"] == -7).all() and (got["stage_counts"] == -7).all()
        assert (got["xyz"] == 7.0).all() and (got["normals"] == 7.0).all()
    _refused(LCD_ERR_INVALID, eng.filter_scans, x, off, oo, struct_size=112, **base)
    _refused(LCD_ERR_INVALID, eng.filter_scans, None, off, oo, **base)
    _refused(LCD_ERR_INVALID, eng.filter_scans, x, off, oo, with_normals=False, **base)
    _refused(LCD_ERR_INVALID, eng.filter_scans, x, off[::-1].copy(), oo, **base)
    _refused(LCD_ERR_INVALID, eng.filter_scans, x, off, oo[::-1].copy(), **base)
    _refused(LCD_ERR_INVALID, eng.filter_scans, x, off + 1, oo, **base)
    _refused(LCD_ERR_INVALID, eng.filter_scans, x, None, oo, **base)
    nan_row = x.copy()
    nan_row[7, 1] = np.nan
    _refused(LCD_ERR_INVALID, eng.filter_scans, nan_row, off, oo, **base)
    out = eng.filter_scans(np.zeros((0, 3), np.float32), [0], [0], **base)
    assert out["status"].shape == (0,)
    assert_same(run_host(eng, scans, **base), expected("after_refusals", scans, None, **base), "after the refusals")


def test_unsynchronised_back_to_back_calls_share_the_scratch(eng):
    """three device calls enqueued without a synchronisation in between, the largest second"""
    groups = [([I.cloud(300, 41)], dict(normal_k=5)), ([I.spread(4000, 42), I.cloud(513, 43)], dict(voxel_size=0.3, normal_k=9)),
              ([I.cloud(257, 44)], dict(voxel_size=0.2))]
    sts = [launch_dev(eng, stage_dev(g, None, with_normals(kw)), **kw) for g, kw in groups]
    for k, ((g, kw), st) in enumerate(zip(groups, sts)):
        assert_same(to_host(eng, st), expected("back_to_back_%d" % k, g, None, device_entry=True, **kw))


def test_the_filtered_regions_go_straight_into_the_plane_icp(eng):
    """two scans with regions of 1 024 rows are filtered; lcd_register_icp_plane_dev then takes out_offsets as the pair's offsets, nothing read
    back in between: the result equals the two models chained (the NaN rows of a region take part in nothing)"""
    import register_icp_plane_inputs as PI
    import register_icp_plane_model as PM
    from rtabmap_amd import capi
    p = PI.pair(900, 880, 5, noise=0.004)
    scans = [p["from_xyz"], p["to_xyz"]]
    kw = dict(voxel_size=0.15, normal_k=8)
    st = launch_dev(eng, stage_dev(scans, [1024, 1024]), **kw)
    out = {}
    for k, w, dt in capi.Engine.ICP_PLANE_OUT:
        tdt = {np.int32: torch.int32, np.float32: torch.float32, np.float64: torch.float64}[dt]
        out[k] = torch.full((1, w) if w else (1,), -7 if dt is np.int32 else float("nan"), dtype=tdt, device="cuda")
    out["match"] = torch.full((1024,), -7, dtype=torch.int32, device="cuda")
    o = st["out"]
    eng.register_icp_plane_dev(o["xyz"][:1024], o["normals"][:1024], [0, 1024], o["xyz"][1024:], o["normals"][1024:], [0, 1024], p["guess"][None], out, **PI.KW)
    got_f = to_host(eng, st)
    want_f = expected("chain", scans, [1024, 1024], device_entry=True, **kw)
    assert_same(got_f, want_f, "chain, filter")
    assert (want_f["status"] == M.OK).all() and 3 < want_f["count"].min() and want_f["count"].max() < 1024
    want = PM.register(want_f["xyz"][:1024], want_f["normals"][:1024], want_f["xyz"][1024:], want_f["normals"][1024:], p["guess"], device_entry=True, **PI.KW)
    for k in ("status", "stop", "iterations", "n_correspondences", "branch"):
        assert out[k].cpu().numpy()[0] == want[k], k
    for k in ("transform", "icp_transform", "correction", "ratio", "complexity"):
        np.testing.assert_array_equal(I.bits(out[k].cpu().numpy()[0]).reshape(-1), I.bits(want[k]).reshape(-1), err_msg=k)
    np.testing.assert_array_equal(out["match"].cpu().numpy(), want["match"])
    assert want["status"] == PM.OK


def test_the_mirror_class_filters_raw_scans_through_the_engine():
    """RegistrationIcpHip::computeTransformation over raw scans: the filter's sizes, the reference's maxLaserScans and the plane rule's transform"""
    import register_icp_plane_inputs as PI
    import register_icp_plane_model as PM
    from rtabmap_amd import vwdictionary as V, synth
    p = PI.pair(900, 880, 5, noise=0.004)
    f = [M.filter_scan(s, voxel_size=0.15, normal_k=8) for s in (p["from_xyz"], p["to_xyz"])]
    nf, nt = f[0]["count"], f[1]["count"]
    max_to = int(np.float32(500) * (np.float32(nt) / np.float32(880)))
    kw = dict(max_iterations=30, max_correspondence_distance=0.3, epsilon=0.0, correspondence_ratio=0.1)
    want = PM.register(f[0]["xyz"][:nf], f[0]["normals"][:nf], f[1]["xyz"][:nt], f[1]["normals"][:nt], p["guess"], max_laser_scans=max_to,
                       min_complexity=0.02, low_complexity_strategy=1, **kw)
    d = V.VWDictionaryHip(nndr=0.8, new_words_compared_together=True)
    d.add_new_words(synth.vocab_surf(50, seed=8), 1)
    d.update()
    t, info = d.register_icp_raw(p["from_xyz"], p["to_xyz"], p["guess"], to_max_points=500, voxel_size=0.15, point_to_plane_k=8, max_translation=0.0,
                                 max_rotation=0.0, **kw)
    assert (info["from_rows"], info["to_rows"], info["max_laser_scans"]) == (nf, nt, max_to)
    np.testing.assert_array_equal(I.bits(t), I.bits(want["transform"]))
    t, info = d.register_icp_raw(p["from_xyz"], p["to_xyz"], p["guess"], filters_enabled=1, voxel_size=0.15, point_to_plane_k=8, max_translation=0.0,
                                 max_rotation=0.0, **kw)
    assert (info["from_rows"], info["to_rows"], info["max_laser_scans"]) == (nf, 880, 880)
    d.close()


def test_pipelined_frame_stream_is_untouched_by_the_filter():
    """A pipelined SURF handle runs an appending frame stream; lcd_filter_scans_dev calls between the frames change no frame output, bit for
    bit, against a run without them, and their own results are the model's"""
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
    scans = [I.cloud(600, 51), I.cloud(0, 52), I.cloud(257, 53)]
    kw = dict(voxel_size=0.25, normal_k=5)
    want = expected("in_flight", scans, None, device_entry=True, **kw)
    cap = n_sig + T + 4
    out = {}
    for with_filter in (False, True):
        eng = rtabmap_amd.Engine("f32", 64, sig_capacity=cap, pipeline=True)
        eng.vocab_append(vocab, ids)
        eng.sig_add_bulk(np.arange(1, n_sig + 1, dtype=np.int32), np.arange(0, (n_sig + 1) * q, q, dtype=np.int64), words.reshape(-1))
        eng.set_option("next_word_id", n_words + 1)
        d_w = torch.zeros((T, q), dtype=torch.int32, device="cuda")
        d_l = torch.zeros((T, cap), dtype=torch.float32, device="cuda")
        d_first = torch.zeros(T, dtype=torch.int32, device="cuda")
        sts = [stage_dev(scans) for _ in range(T)]
        for t in range(T):
            eng.frame_dev(frames[t].data_ptr(), q, n_sig + 1 + t, float(n_sig + 1 + t), d_w[t].data_ptr(), d_l[t].data_ptr(), cap,
                          first_new_word_id=capi.LCD_NEW_WORD_IDS_AUTO, append_new_words=True, d_first_new_word_id_ptr=d_first[t:].data_ptr())
            if with_filter:                                             # between the frames, nothing drained
                launch_dev(eng, sts[t], **kw)
        eng.synchronize()
        out[with_filter] = (d_w.cpu().numpy(), d_l.cpu().numpy(), d_first.cpu().numpy(), eng.vocab_count(), eng.sig_count())
        if with_filter:
            for st in sts:
                assert_same(to_host(eng, st), want, "between frames")
        eng.close()
    for a, b in zip(out[False][:3], out[True][:3]):
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))
    assert out[False][3:] == out[True][3:]
    assert out[True][3][0] > n_words
