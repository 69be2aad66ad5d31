"""GPU tests of lcd_track_flow and lcd_track_flow_dev (rtabmap_amd/csrc/flow_track.hip) against tests/flow_track_model.py.  Every
comparison is exact: counts, indices, status, tracked corners, errors, NaN positions and all other bits; every output starts as a canary."""
import ctypes as C

import numpy as np
import pytest
import torch

import flow_track_inputs as I
import flow_track_model as M
import stereo_flow_inputs as SI
import stereo_flow_model as SM

pytestmark = pytest.mark.gpu

LCD_ERR_INVALID, LCD_ERR_UNSUPPORTED = 1, 5


def _refused(status, call, *args, **kw):
    from rtabmap_amd import capi
    with pytest.raises(capi.LcdError) as err:
        call(*args, **kw)
    assert err.value.status == status, err.value


def _both(eng, pairs, points, P, initials=None, aux=None, what=""):
    want = M.batch(pairs, points, P, initials, device=True)
    I.assert_same(I.run_dev(eng, pairs, points, P, initials, aux), pairs, points, P, initials, device=True, aux=aux, what=what + " dev", want=want, canary=I.CANARY)
    I.assert_same(I.run_host(eng, pairs, points, P, initials, aux), pairs, points, P, initials, aux=aux, what=what + " host", want=want)
    return want


def _batch(rng, width, height, win_w, win_h, sizes, max_level):
    """one pair per size; a pitch larger than the row every third pair"""
    pairs, points = [], []
    for k, n in enumerate(sizes):
        pr, pts, _ = I.random_pair(rng, width, height, n, win_w, win_h, pad=5 if k % 3 == 2 else 0, max_level=max_level)
        pairs.append(pr)
        points.append(pts)
    return pairs, points


@pytest.mark.parametrize("max_level", [0, 1, 5])
@pytest.mark.parametrize("width,height,win_w,win_h", I.SHAPES[:6])
def test_both_entries_equal_the_model(width, height, win_w, win_h, max_level):
    """pairs of 0, 1, 3, 4, 5, 63, 64, 65 and 1100 corners in ONE batch with a 16-byte payload; windows of 9, 64, 65, 256, 961 and 45 pixels;
    max_level 5 is cut short by every window here"""
    import rtabmap_amd
    rng = np.random.default_rng(width + win_w + max_level)
    P = M.params(win_width=win_w, win_height=win_h)
    pairs, points = _batch(rng, width, height, win_w, win_h, I.PAIR_SIZES, max_level)
    aux = rng.integers(0, 256, (sum(I.PAIR_SIZES), 16), dtype=np.uint8)
    eng = rtabmap_amd.Engine("f32", 64)
    want = _both(eng, pairs, points, P, aux=aux)
    assert sum(int(s.sum()) for s in want["status"]) > 300 and 300 < int(want["count"].sum()) < sum(I.PAIR_SIZES)
    assert eng.vocab_count() == (0, 0) and eng.sig_count() == (0, 0)
    eng.close()


def test_160_by_120_with_the_defaults_and_the_l1_error():
    import rtabmap_amd
    rng = np.random.default_rng(160)
    pairs, points = _batch(rng, 160, 120, 16, 16, [130, 65, 200], 3)
    eng = rtabmap_amd.Engine("f32", 64)
    _both(eng, pairs, points, M.params())
    _both(eng, pairs, points, M.params(use_min_eigenvals=0, error_threshold=2.0))
    eng.close()


def test_pairs_with_different_level_counts_share_their_images():
    """A->B with max_level 0, B->C with 3, A->B again with 2, C->A with 1, B->B: three distinct images, each built once to its highest level"""
    import rtabmap_amd
    rng = np.random.default_rng(21)
    tex = I.texture(rng, 64, 48)
    a, b = I.shifted_images(tex, 64, 48, (1.5, -0.75))
    _, c = I.shifted_images(tex, 64, 48, (2.75, 0.5))
    P = M.params(win_width=5, win_height=5)
    pairs = [M.pair(a, b, 64, 0), M.pair(b, c, 64, 3), M.pair(a, b, 64, 2), M.pair(c, a, 64, 1), M.pair(b, b, 64, 3)]
    points = [I.random_points(rng, n, 64, 48, 5, 5) for n in (70, 65, 64, 3, 40)]
    eng = rtabmap_amd.Engine("f32", 64)
    want = _both(eng, pairs, points, P)
    assert not np.array_equal(I.bits(want["track"][0][:64]), I.bits(M.run_pair(pairs[2], points[0][:64], P)["track"]))      # the level count matters
    eng.close()


def test_70_pairs_over_three_shared_images_and_an_empty_call():
    import rtabmap_amd
    rng = np.random.default_rng(7)
    tex = I.texture(rng, 64, 48)
    imgs = [I.shifted_images(tex, 64, 48, s, pad=p)[1] for s, p in (((0.0, 0.0), 0), ((1.25, 0.5), 0), ((2.5, -1.0), 0))]
    pools = I.random_points(rng, 200, 64, 48, 8, 8)
    pairs, points = [], []
    for f in range(70):
        k = int(rng.integers(0, 9))
        a = int(rng.integers(0, 200 - k))
        pairs.append(M.pair(imgs[f % 3], imgs[(f + 1) % 3], 64, f % 4))
        points.append(pools[a:a + k])
    P = M.params(win_width=8, win_height=8)
    eng = rtabmap_amd.Engine("f32", 64)
    want = _both(eng, pairs, points, P)
    assert (want["count"] == 0).sum() > 3 and (want["count"] > 2).sum() > 5
    assert eng.track_flow(np.zeros((0, 2), np.float32), [0], [])["count"].shape == (0,)
    st = I.stage_dev([], [])
    I.launch_dev(eng, st)
    got = I.run_dev(eng, pairs[:3], [np.zeros((0, 2), np.float32)] * 3, P)      # pairs without corners
    assert got["count"].tolist() == [0, 0, 0]
    eng.close()


def test_use_initial_mixed_with_pairs_that_do_not_use_it():
    import rtabmap_amd
    rng = np.random.default_rng(11)
    eng = rtabmap_amd.Engine("f32", 64)
    cases = I.initial_cases(rng)
    plain, pts, _ = I.random_pair(rng, 64, 48, 65, 8, 8, max_level=1)
    pairs = [cases[0]["pair"], plain, cases[1]["pair"], I.with_(cases[1]["pair"], use_initial=0)]
    points = [cases[0]["points"], pts, cases[1]["points"], cases[1]["points"]]
    initials = [cases[0]["initial"], None, cases[1]["initial"], None]
    want = _both(eng, pairs, points, cases[0]["P"], initials)
    assert not np.array_equal(I.bits(want["track"][2]), I.bits(want["track"][3]))             # the start positions matter
    _refused(LCD_ERR_INVALID, I.run_host, eng, pairs, points, cases[0]["P"], None)            # use_initial without initial
    _refused(LCD_ERR_INVALID, I.run_dev, eng, pairs, points, cases[0]["P"], None)
    eng.close()


def test_single_property_inputs():
    """the inputs whose properties tests/test_flow_track_model.py proves, each through both entries"""
    import rtabmap_amd
    eng = rtabmap_amd.Engine("f32", 64)
    for k, c in enumerate(I.all_cases(np.random.default_rng(5))):
        _both(eng, [c["pair"]], [c["points"]], c["P"], [c["initial"]], what="case %d" % k)
    eng.close()


def test_corners_the_reference_asserts_on():
    """NaN, inf, 1e20 and 2^31 among ordinary corners and among the start positions: the device entry gives them status 0, the track
    (NaN, NaN), err 0, does not keep them and is otherwise unaffected; the host entry refuses the call"""
    import rtabmap_amd
    rng = np.random.default_rng(3)
    eng = rtabmap_amd.Engine("f32", 64)
    P = M.params(win_width=8, win_height=8)
    pr, pts, ini = I.random_pair(rng, 64, 48, 100, 8, 8)
    order = rng.permutation(108)
    wild = np.concatenate([pts, I.wild_points()])[order]
    got = I.run_dev(eng, [pr], [wild], P)
    I.assert_same(got, [pr], [wild], P, device=True, canary=I.CANARY)
    bad = ~np.isfinite(wild).all(1) | (np.abs(wild) >= 2.0 ** 31).any(1)
    assert bad.sum() == 8 and (got["status"][bad] == 0).all() and np.isnan(got["track"][bad]).all() and (got["err"][bad] == 0).all()
    assert not set(np.flatnonzero(bad)) & set(got["index"][:got["count"][0]])
    _refused(LCD_ERR_INVALID, I.run_host, eng, [pr], [wild], P)
    pi = I.with_(pr, use_initial=1)
    start = np.concatenate([ini, I.wild_points()])[order]
    ok = np.concatenate([pts, pts[:8]])[order]
    got = I.run_dev(eng, [pi], [ok], P, [start])
    I.assert_same(got, [pi], [ok], P, [start], device=True, canary=I.CANARY)
    assert (got["status"][bad] == 0).all() and np.isnan(got["track"][bad]).all()
    _refused(LCD_ERR_INVALID, I.run_host, eng, [pi], [ok], P, [start])
    I.assert_same(I.run_host(eng, [pr], [ok], P, [start]), [pr], [ok], P, None)               # not read without use_initial
    eng.close()


@pytest.mark.parametrize("aux_bytes", [0, 4, 16, 64])
def test_payloads_and_every_optional_output_null_in_turn(aux_bytes):
    import rtabmap_amd
    rng = np.random.default_rng(aux_bytes)
    P = M.params(win_width=5, win_height=3)
    pairs, points = _batch(rng, 40, 24, 5, 3, [65, 130, 0, 64], 2)
    aux = rng.integers(0, 256, (65 + 130 + 64, aux_bytes), dtype=np.uint8) if aux_bytes else None
    eng = rtabmap_amd.Engine("f32", 64)
    want = M.batch(pairs, points, P, device=True)
    for optional in (("track", "status", "err"), ("status", "err"), ("track", "err"), ("track", "status"), ()):
        got = I.run_dev(eng, pairs, points, P, aux=aux, optional=optional)
        assert all(got[k] is None for k in ("track", "status", "err") if k not in optional)
        I.assert_same(got, pairs, points, P, device=True, aux=aux, what="dev %s" % (optional,), want=want, canary=I.CANARY)
        I.assert_same(I.run_host(eng, pairs, points, P, aux=aux, optional=optional), pairs, points, P, aux=aux, what="host %s" % (optional,), want=want)
    eng.close()


def test_unsynchronised_calls_and_the_scratch_shared_with_the_stereo_call():
    """two device calls back to back without a synchronisation, then the call between two lcd_keypoints_3d_stereo_dev calls: they take the
    job-table slots in turn and share d_small, which the stream orders"""
    import rtabmap_amd
    rng = np.random.default_rng(9)
    P = M.params(win_width=8, win_height=8)
    a = _batch(rng, 40, 24, 8, 8, [65], 1)
    b = _batch(rng, 160, 120, 8, 8, [130, 200, 64], 3)
    eng = rtabmap_amd.Engine("f32", 64)
    staged = [I.stage_dev(*x) for x in (b, a)]
    for st in staged:
        I.launch_dev(eng, st, P)
    for st, x in zip(staged, (b, a)):
        I.assert_same(I.to_host(eng, st), x[0], x[1], P, device=True, canary=I.CANARY)
    s_pairs, s_points = [], []
    for n in (130, 64):
        pr, pts = SI.random_frame(rng, 160, 120, n)
        s_pairs.append(pr)
        s_points.append(pts)
    s1, s2 = SI.stage_dev(s_pairs, s_points), SI.stage_dev(s_pairs[::-1], s_points[::-1])
    mid = I.stage_dev(*b)
    SI.launch_dev(eng, s1, None, SM.FILTER_3D, 1.0, 4.0)
    I.launch_dev(eng, mid, P)
    SI.launch_dev(eng, s2, None, SM.FILTER_3D, 1.0, 4.0)
    I.assert_same(I.to_host(eng, mid), b[0], b[1], P, device=True, canary=I.CANARY)
    SI.assert_same(SI.to_host(eng, s1), s_pairs, s_points, None, SM.FILTER_3D, 1.0, 4.0, device=True)
    SI.assert_same(SI.to_host(eng, s2), s_pairs[::-1], s_points[::-1], None, SM.FILTER_3D, 1.0, 4.0, device=True)
    eng.close()


class _Raw:
    """one pair of 100 corners through the C-ABI itself, every output canary-filled: host arrays for lcd_track_flow, tensors for
    lcd_track_flow_dev.  call(**changes) sets fields of lcd_track_flow_args (pair=..., params=... change the one pair / the parameters) for one
    call and returns (the status, whether every output still holds its canary)"""

    def __init__(self, eng, pr, pts, ini, aux, dev):
        from rtabmap_amd import capi
        self.eng, self.capi, self.dev, self.pr = eng, capi, dev, pr
        n = len(pts)
        self.off = np.array([0, n], np.int64)
        self.off3 = np.array([0, 60, 50, n], np.int64)
        self.huge = np.array([0, 2 ** 31], np.int64)
        self.off1 = np.array([1, n], np.int64)
        shapes = {"out_count": ((1,), np.int32), "out_index": ((n,), np.int32), "out_from": ((n, 2), np.float32), "out_to": ((n, 2), np.float32),
                  "out_aux": ((n, aux.shape[1]), np.uint8), "out_track": ((n, 2), np.float32), "out_status": ((n,), np.uint8), "out_err": ((n,), np.float32)}
        self.canary = {k: (0xA5 if dt == np.uint8 else I.CANARY) for k, (_, dt) in shapes.items()}
        host = {k: np.full(sh, self.canary[k], dt) for k, (sh, dt) in shapes.items()}
        ins = {"points": pts, "initial": ini, "aux": aux, "from": np.ascontiguousarray(pr["from"]), "to": np.ascontiguousarray(pr["to"])}
        if dev:
            self.out = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
            self.ins = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in ins.items()}
            torch.cuda.synchronize()
            self.ptr = lambda t: t.data_ptr()
        else:
            self.out, self.ins = host, {k: np.ascontiguousarray(v) for k, v in ins.items()}
            self.ptr = lambda a: a.ctypes.data
        self.fn = eng.L.lcd_track_flow_dev if dev else eng.L.lcd_track_flow

    def clean(self):
        self.eng.synchronize()
        return all(bool((v == self.canary[k]).all()) for k, v in self.out.items())

    def call(self, pair=None, params=None, n_pairs=1, null_args=False, null_params=False, **fields):
        capi = self.capi
        w = self.pr["width"]
        spec = {"from": self.ins["from"], "to": self.ins["to"], "width": w, "max_level": 3, "use_initial": 0, "from_pitch_bytes": self.pr["from"].shape[1],
                "to_pitch_bytes": self.pr["to"].shape[1], "height": self.pr["from"].shape[0]}
        spec.update(pair or {})
        arr = self.eng._flow_pairs([spec] * max(min(n_pairs, 3), 1), self.ptr)
        fp = capi.flow_params(params)
        a = capi.LcdTrackFlowArgs(C.sizeof(capi.LcdTrackFlowArgs), n_pairs, 0, 0)
        a.offsets, a.pairs, a.params, a.points = self.off.ctypes.data, arr, C.pointer(fp), self.ptr(self.ins["points"])
        for k in ("out_count", "out_index", "out_from", "out_to", "out_track", "out_status", "out_err"):
            setattr(a, k, self.ptr(self.out[k]))
        for k, v in fields.items():
            setattr(a, k, v)
        if null_params:
            a.params = None
        rc = self.fn(self.eng.h, None if null_args else C.byref(a))
        return rc, self.clean()


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_error_table_row_by_row(dev):
    """every refusal of include/lcd.h's list, on the entry named: the status, and nothing written to any canary-filled output; then the
    handle still serves the call.  The host entry's served call also shows that what lies behind a pair's count stays the caller's."""
    import rtabmap_amd
    rng = np.random.default_rng(12)
    eng = rtabmap_amd.Engine("f32", 64)
    pr, pts, ini = I.random_pair(rng, 64, 48, 100, pad=3)
    aux = rng.integers(0, 256, (100, 8), dtype=np.uint8)
    r = _Raw(eng, pr, pts, ini, aux, dev)
    nan = float("nan")
    invalid = [dict(struct_size=120), dict(null_args=True), dict(aux_bytes=6), dict(aux_bytes=68), dict(aux_bytes=-4), dict(null_params=True),
               dict(n_pairs=-1), dict(offsets=None), dict(offsets=r.off1.ctypes.data), dict(n_pairs=3, offsets=r.off3.ctypes.data),
               dict(out_count=None), dict(pairs=None), dict(points=None), dict(out_index=None), dict(out_from=None), dict(out_to=None),
               dict(aux_bytes=8, aux=r.ptr(r.ins["aux"])),                                        # aux without out_aux
               dict(pair=dict(use_initial=1))]                                                      # use_initial without initial
    invalid += [dict(params=c) for c in (dict(win_width=2), dict(win_width=32), dict(win_height=2), dict(win_height=33), dict(eps=nan),
                                         dict(min_eig_threshold=nan), dict(error_threshold=nan))]
    # width 16 and height 16: an image that is not larger than the 16 x 16 window
    invalid += [dict(pair=c) for c in ({"from": None}, {"to": None}, dict(max_level=-1), dict(max_level=9), dict(width=16), dict(height=16),
                                       dict(from_pitch_bytes=63), dict(to_pitch_bytes=10), dict(from_pitch_bytes=2 ** 31), dict(to_pitch_bytes=2 ** 31))]
    for row in invalid:
        rc, clean = r.call(**row)
        assert rc == LCD_ERR_INVALID and clean, row
    for row in (dict(n_pairs=65536), dict(offsets=r.huge.ctypes.data)):                             # the limits
        rc, clean = r.call(**row)
        assert rc == LCD_ERR_UNSUPPORTED and clean, row
    eng.set_option("shard_append", 1)                                                               # a handle of a sharded vocabulary
    rc, clean = r.call()
    eng.set_option("shard_append", 0)
    assert rc == LCD_ERR_UNSUPPORTED and clean
    rc, clean = r.call(n_pairs=0)                                                                   # n_pairs == 0: LCD_OK, nothing written
    assert rc == 0 and clean
    # the handle still works, payload and start positions included; behind the count every compacted output keeps the canary
    pi = I.with_(pr, use_initial=1)
    rc, clean = r.call(pair=dict(use_initial=1), aux_bytes=8, aux=r.ptr(r.ins["aux"]), out_aux=r.ptr(r.out["out_aux"]), initial=r.ptr(r.ins["initial"]))
    assert rc == 0 and not clean
    got = {k[4:]: (v.cpu().numpy() if dev else v) for k, v in r.out.items()}
    I.assert_same(got, [pi], [pts], M.params(), [ini], device=dev, aux=aux, canary=I.CANARY)
    assert 0 < got["count"][0] < 100
    eng.close()
