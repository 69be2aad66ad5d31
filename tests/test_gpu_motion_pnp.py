"""GPU tests of lcd_estimate_motion_pnp and lcd_estimate_motion_pnp_dev (rtabmap_amd/csrc/motion_pnp.hip) against tests/motion_pnp_model.py.
Every comparison is exact: transform bits, status, counts, ids over the whole region, variance bits, cosine bits, kind."""
import numpy as np
import pytest
import torch

import motion_pnp_inputs as I
import motion_pnp_model as M

pytestmark = pytest.mark.gpu

LCD_ERR_INVALID, LCD_ERR_UNSUPPORTED = 1, 5
KW = dict(min_inliers=6, reproj_error=2.0, iterations=300, refine_iterations=5, variance_median_ratio=4, max_variance=0.0, seed=3)
PER_PAIR = ("transform", "status", "n_matches", "n_inliers", "variance_lin", "angle_cos", "variance_kind")
_model_cache = {}


def model_of(pair, cam, guess, to_xyz, **kw):
    key = (id(pair), id(cam), None if guess is None else tuple(np.asarray(guess).tolist()), to_xyz, tuple(sorted(kw.items())))
    if key not in _model_cache:                                            # the pair and the camera are kept so that their ids stay their own
        _model_cache[key] = (pair, cam, M.estimate(*I.frames(pair, to_xyz), camera=I.model_camera(cam), guess=guess, **kw))
    return _model_cache[key][2]


def cameras_of(pairs, cam):
    return [cam] * len(pairs) if isinstance(cam, dict) else list(cam)


def expected(pairs, cam=I.CAMERA, guesses=None, to_xyz=True, **kw):
    """the model's results laid out as the call lays its outputs out"""
    n = len(pairs)
    cams = cameras_of(pairs, cam)
    out = dict(transform=np.zeros((n, 12), np.float32), status=np.zeros(n, np.int32), n_matches=np.zeros(n, np.int32), n_inliers=np.zeros(n, np.int32),
               variance_lin=np.zeros(n, np.float64), angle_cos=np.zeros(n, np.float64), variance_kind=np.zeros(n, np.int32), matches=[], inliers=[])
    for k, p in enumerate(pairs):
        r = model_of(p, cams[k], None if guesses is None else guesses[k], to_xyz, **kw)
        region = p["to_ids"].shape[0]
        out["transform"][k], out["status"][k], out["variance_lin"][k], out["angle_cos"][k] = r["transform"], r["status"], r["variance_lin"], r["angle_cos"]
        out["n_matches"][k], out["n_inliers"][k], out["variance_kind"][k] = len(r["matches"]), len(r["inliers"]), r["variance_kind"]
        for name in ("matches", "inliers"):
            out[name].append(np.concatenate([r[name], np.zeros(region - len(r[name]), np.int32)]).astype(np.int32))
    for name in ("matches", "inliers"):
        out[name] = np.concatenate(out[name] + [np.zeros(0, np.int32)])
    return out


def assert_same(got, want, what=""):
    for name in ("status", "n_matches", "n_inliers", "variance_kind", "matches", "inliers"):
        np.testing.assert_array_equal(got[name], want[name], err_msg=what + " " + name)
    np.testing.assert_array_equal(M.bits(got["transform"]), M.bits(want["transform"]), err_msg=what + " transform")
    for name in ("variance_lin", "angle_cos"):
        np.testing.assert_array_equal(np.ascontiguousarray(got[name]).view(np.uint64), want[name].view(np.uint64), err_msg=what + " " + name)


def stage_dev(pairs, to_xyz=True):
    """the batch on the device, outputs canary-filled, uploaded and synchronised"""
    c = I.concatenate(pairs, to_xyz)
    n, nt = len(pairs), c["to_ids"].shape[0]
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device="cuda")
    st = dict(fi=dev(c["from_ids"]), fx=dev(c["from_xyz"]), fo=c["from_offsets"], ti=dev(c["to_ids"]), tp=dev(c["to_points"]), tx=dev(c["to_xyz"]),
              to=c["to_offsets"], transform=full((n, 12), float("nan"), torch.float32), status=full((n,), -1, torch.int32),
              n_matches=full((n,), -1, torch.int32), n_inliers=full((n,), -1, torch.int32), variance_lin=full((n,), float("nan"), torch.float64),
              angle_cos=full((n,), float("nan"), torch.float64), variance_kind=full((n,), -1, torch.int32),
              matches=full((max(nt, 1),), -1, torch.int32), inliers=full((max(nt, 1),), -1, torch.int32))
    torch.cuda.synchronize()
    return st


def launch_dev(eng, st, cams, guesses=None, **kw):
    eng.estimate_motion_pnp_dev(st["fi"], st["fx"], st["fo"], st["ti"], st["tp"], st["to"], cams, st["transform"], st["status"], st["n_matches"],
                                st["n_inliers"], st["variance_lin"], st["angle_cos"], st["variance_kind"], st["matches"], st["inliers"],
                                d_to_xyz=st["tx"], guesses=guesses, **kw)
    return st


def to_host(eng, st):
    eng.synchronize()
    nt = int(st["to"][-1])
    out = {k: st[k].cpu().numpy() for k in PER_PAIR + ("matches", "inliers")}
    out["matches"], out["inliers"] = out["matches"][:nt], out["inliers"][:nt]
    return out


def run_dev(eng, pairs, cam=I.CAMERA, guesses=None, to_xyz=True, **kw):
    return to_host(eng, launch_dev(eng, stage_dev(pairs, to_xyz), cameras_of(pairs, cam), guesses, **kw))


def run_host(eng, pairs, cam=I.CAMERA, guesses=None, to_xyz=True, **kw):
    c = I.concatenate(pairs, to_xyz)
    return eng.estimate_motion_pnp(c["from_ids"], c["from_xyz"], c["from_offsets"], c["to_ids"], c["to_points"], c["to_offsets"], cameras_of(pairs, cam),
                                   to_xyz=c["to_xyz"], guesses=guesses, **kw)


def check_both(eng, pairs, what="", cam=I.CAMERA, guesses=None, to_xyz=True, **kw):
    want = expected(pairs, cam, guesses, to_xyz, **kw)
    assert_same(run_dev(eng, pairs, cam, guesses, to_xyz, **kw), want, what + " dev")
    assert_same(run_host(eng, pairs, cam, guesses, to_xyz, **kw), want, what + " host")
    return want


@pytest.fixture(scope="module")
def batch():
    return I.mixed_batch()


@pytest.mark.parametrize("refine", I.REFINE)
@pytest.mark.parametrize("iterations", I.ITERATIONS)
def test_both_entries_equal_the_model(batch, iterations, refine):
    """pairs of 0, 3, 4, 5, 6, 63, 64, 65, 255, 256, 257 and 1100 correspondences in ONE batch, inside frames with duplicates and one-sided ids"""
    import rtabmap_amd
    eng = rtabmap_amd.Engine("f32", 64)
    want = check_both(eng, batch, **dict(KW, min_inliers=4, iterations=iterations, refine_iterations=refine, seed=iterations + refine))
    assert want["n_matches"].tolist() == list(I.BATCH_SIZES)
    if iterations == 300:
        assert (want["status"][5:] == M.OK).all() and (want["status"][:2] == M.FEW_CORRESPONDENCES).all()
    assert eng.vocab_count() == (0, 0) and eng.sig_count() == (0, 0)
    eng.close()


@pytest.mark.parametrize("sized", (False, True))
@pytest.mark.parametrize("to_xyz", (False, True))
def test_covariance_branches_local_transform_and_max_variance(batch, to_xyz, sized):
    """with and without to_xyz, with and without an image size (kind 2 only without both), every second pair behind a local transform"""
    import rtabmap_amd
    eng = rtabmap_amd.Engine("f32", 64)
    cams = [I.camera(sized, local=k % 2 == 1) for k in range(len(batch))]
    _keep = _model_cache.setdefault(("cams", sized), cams)
    want = check_both(eng, batch, cam=_keep, to_xyz=to_xyz, **KW)
    assert set(want["variance_kind"][want["status"] == M.OK].tolist()) == {1 if (to_xyz or sized) else 2}
    if to_xyz or sized:                                                 # the rejection: a bound between the batch's variances
        lin = np.sort(want["variance_lin"][want["status"] == M.OK])
        bound = float(np.float32((lin[0] + lin[-1]) / 2))
        rej = check_both(eng, batch, cam=_keep, to_xyz=to_xyz, **dict(KW, max_variance=bound))
        assert (rej["status"] == M.VARIANCE_REJECTED).any() and (rej["status"] == M.OK).any()
        assert not rej["transform"][rej["status"] == M.VARIANCE_REJECTED].any()
    eng.close()


def test_all_outliers_everything_behind_the_camera_and_the_guess_as_winner(batch):
    import rtabmap_amd
    eng = rtabmap_amd.Engine("f32", 64)
    want = check_both(eng, [I.all_outlier_pair()], **dict(KW, min_inliers=10, seed=1))
    assert want["status"][0] != M.OK and not want["transform"].any()
    behind = I.behind_pair()
    want = check_both(eng, [behind], **dict(KW, min_inliers=4, iterations=1))
    assert want["status"][0] == M.NO_MODEL and want["n_matches"][0] == behind["m"] and want["n_inliers"][0] == 0
    # the guess is the true pose and one hypothesis runs beside it: candidate 0 holds every inlier and wins
    pairs = batch[5:9]
    cams = _model_cache.setdefault(("cams", "guess"), [I.camera(True, local=k % 2 == 1) for k in range(len(pairs))])
    guesses = np.stack([I.guess_of(I.true_model(p), c.get("local_transform")) for p, c in zip(pairs, cams)])
    want = check_both(eng, pairs, cam=cams, guesses=guesses, **dict(KW, iterations=1, refine_iterations=0))
    for p, c, g in zip(pairs, cams, guesses):
        r = model_of(p, c, g, True, **dict(KW, iterations=1, refine_iterations=0))
        assert r["best"] == 0 and r["counts"][0] >= int(p["inlier"].sum()) - 2
    assert (want["status"] == M.OK).all()
    for name in sorted(I.REFINE_CASES):
        pair, kw = I.refine_case(name)
        for refine in (kw["refine_iterations"],) + I.REFINE:
            check_both(eng, [pair], what=name, **dict(KW, **dict(kw, refine_iterations=refine)))
    seed = I.seed_with_invalid_first(4, 1)
    four = batch[2]
    assert check_both(eng, [four], **dict(KW, min_inliers=4, iterations=1, refine_iterations=0, seed=seed))["n_matches"][0] == 4
    eng.close()


@pytest.mark.parametrize("to_xyz", (False, True))
def test_the_staged_limit_on_either_side_of_its_edge(to_xyz):
    """the largest pair whose coordinates are staged in LDS and the smallest that reads them from the scratch"""
    import rtabmap_amd
    eng = rtabmap_amd.Engine("f32", 64)
    cap = I.STAGE_CAP[to_xyz]
    assert cap == (3360 if to_xyz else 5376)
    rng = np.random.default_rng(31)
    kw = dict(KW, iterations=40, refine_iterations=2)
    for m in (cap, cap + 1):
        pair = I.random_pair(rng, m, outliers=0.3, decoys=False)
        want = check_both(eng, [pair], to_xyz=to_xyz, what=str(m), **kw)
        assert want["n_matches"][0] == m and want["status"][0] == M.OK
    eng.close()


def test_a_pair_of_8192_rows_reads_its_coordinates_from_the_scratch(batch):
    """8192 x 8192 rows, 8000 correspondences: more than the kernel stages in LDS"""
    import rtabmap_amd
    eng = rtabmap_amd.Engine("f32", 64)
    big = I.big_pair()
    kw = dict(KW, min_inliers=20, iterations=64, refine_iterations=5, seed=8)
    want = check_both(eng, [big], **kw)
    assert want["status"][0] == M.OK and want["n_matches"][0] == 8000 > I.STAGE_CAP[False] and want["n_inliers"][0] > 1000
    small = batch[3:6]                                                   # beside small pairs, which the same launch stages
    mixed = [small[0], big, small[1], small[2]]
    assert_same(run_dev(eng, mixed, **kw), expected(mixed, **kw), "mixed with small pairs")
    eng.close()


def test_700_pairs_and_the_position_in_the_batch():
    """700 pairs in one call, made of ten distinct ones in turn: a pair's bits do not depend on where it stands"""
    import rtabmap_amd
    rng = np.random.default_rng(16)
    distinct = [I.random_pair(rng, m) for m in (0, 3, 5, 17, 33, 64, 65, 90, 130, 257)]
    pairs = [distinct[(k * 7 + k // 10) % 10] for k in range(700)]
    kw = dict(KW, min_inliers=5, iterations=40, refine_iterations=2, seed=21)
    eng = rtabmap_amd.Engine("f32", 64)
    want = expected(pairs, **kw)
    got = run_dev(eng, pairs, **kw)
    assert_same(got, want, "700 dev")
    assert_same(run_host(eng, pairs, **kw), want, "700 host")
    alone = run_dev(eng, [distinct[9]], **kw)
    k = next(k for k, p in enumerate(pairs) if p is distinct[9])
    np.testing.assert_array_equal(M.bits(alone["transform"][0]), M.bits(got["transform"][k]))
    eng.close()


def test_unsynchronised_back_to_back_calls_share_the_scratch(batch):
    """three device calls enqueued without a synchronisation in between, the largest second: its scratch and job table grow while the first
    launch is still in flight, and each call reads its own"""
    import rtabmap_amd
    eng = rtabmap_amd.Engine("f32", 64)
    groups = [batch[:6], batch[8:], batch[6:9]]
    assert sum(p["to_ids"].shape[0] for p in groups[1]) > 4 * sum(p["to_ids"].shape[0] for p in groups[0])
    sts = [launch_dev(eng, stage_dev(g), cameras_of(g, I.CAMERA), **KW) for g in groups]
    for g, st in zip(groups, sts):
        assert_same(to_host(eng, st), expected(g, **KW))
    eng.close()


def test_pipelined_frame_stream_is_untouched_by_motion_estimation(batch):
    """A pipelined SURF handle runs an appending frame stream; lcd_estimate_motion_pnp_dev calls between the frames change no frame output,
    bit for bit, against a run without them, and their own results are the model's"""
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
    pairs = batch[2:8]
    want = expected(pairs, **KW)
    cap = n_sig + T + 4
    out = {}
    for with_motion in (False, True):
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
            if with_motion:                                             # between the frames, nothing drained
                launch_dev(eng, sts[t], cameras_of(pairs, I.CAMERA), **KW)
        eng.synchronize()
        out[with_motion] = (d_w.cpu().numpy(), d_l.cpu().numpy(), d_first.cpu().numpy(), eng.vocab_count(), eng.sig_count())
        if with_motion:
            for st in sts:
                assert_same(to_host(eng, st), want, "between frames")
        eng.close()
    for a, b in zip(out[False][:3], out[True][:3]):
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))
    assert out[False][3:] == out[True][3:]
    assert out[True][3][0] > n_words


def test_the_chain_behind_the_depth_stage_and_the_matcher():
    """lcd_keypoints_3d_dev (both frames, every keypoint kept: a keypoint without depth carries NaNs) -> lcd_match_pairs_dev ->
    lcd_estimate_motion_pnp_dev with nothing read back in between: the from-frame gives its 3-D points, the to-frame its keypoints (and its
    points for the covariance).  The second frame is the first one's keypoints in another order over the same depth image, so the pose is
    the identity up to the fit's rounding."""
    import rtabmap_amd
    from rtabmap_amd import synth
    import keypoints_3d_inputs as KI
    import keypoints_3d_model as KM
    n = 400
    rng = np.random.default_rng(41)
    im, pts = KI.random_frame(rng, np.float32, 64, 48, 1, n, border=False)
    perm = rng.permutation(n)
    rows_a = synth.vocab_surf(n, seed=42)
    rows_b = np.ascontiguousarray(rows_a[perm] + rng.standard_normal((n, 64)).astype(np.float32) * np.float32(0.002))
    points = [pts, np.ascontiguousarray(pts[perm])]
    c0 = im["cameras"][0]
    cam = dict(fx=c0["fx"], fy=c0["fy"], cx=c0["cx"], cy=c0["cy"])
    eng = rtabmap_amd.Engine("f32", 64)
    st = KI.stage_dev([im, im], points)
    d_rows = torch.from_numpy(np.concatenate([rows_a, rows_b])).cuda()
    d_ids = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
    blank = dict(from_ids=np.zeros(n, np.int32), from_xyz=np.zeros((n, 3), np.float32), to_ids=np.zeros(n, np.int32),
                 to_points=np.zeros((n, 2), np.float32), to_xyz=np.zeros((n, 3), np.float32))
    res = stage_dev([blank])
    kw = dict(KW, min_inliers=20, iterations=100, reproj_error=1.0, seed=6)
    torch.cuda.synchronize()
    KI.launch_dev(eng, st, KM.KEEP_ALL, 0.5, 0.0)
    eng.match_pairs_dev(d_rows[:n], d_rows[n:], [0, n], [0, n], d_ids[:n], d_ids[n:], "dictionary")
    eng.estimate_motion_pnp_dev(d_ids[:n], st["xyz"][:n], [0, n], d_ids[n:], st["pts"][n:], [0, n], [cam], res["transform"], res["status"],
                                res["n_matches"], res["n_inliers"], res["variance_lin"], res["angle_cos"], res["variance_kind"], res["matches"],
                                res["inliers"], d_to_xyz=st["xyz"][n:], **kw)
    got = to_host(eng, dict(res, to=np.array([0, n])))
    xyz, ids = st["xyz"].cpu().numpy(), d_ids.cpu().numpy()
    pair = dict(from_ids=ids[:n], from_xyz=xyz[:n], to_ids=ids[n:], to_points=points[1], to_xyz=xyz[n:])
    _model_cache[("chain",)] = (pair, cam)
    want = expected([pair], cam, **kw)
    assert_same(got, want, "chain")
    assert want["status"][0] == M.OK and 100 < want["n_inliers"][0] <= want["n_matches"][0] <= n
    np.testing.assert_allclose(want["transform"][0], np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32), atol=1e-3)
    eng.close()


POINTERS = ("from_word_ids", "from_xyz", "to_word_ids", "to_points", "to_xyz", "out_transform", "out_status", "out_n_matches", "out_n_inliers",
            "out_variance_lin", "out_angle_cos", "out_variance_kind", "out_matches", "out_inliers")
OPTIONAL = ("to_xyz",)


def _table_buffers(pair, device):
    """one pair with canary-filled outputs, on the host or on the device -> dict(ptr = the address per pointer field, fo, to, outputs())"""
    c = I.concatenate([pair])
    n = c["to_ids"].shape[0]
    host = dict(from_word_ids=c["from_ids"], from_xyz=c["from_xyz"], to_word_ids=c["to_ids"], to_points=c["to_points"], to_xyz=c["to_xyz"],
                out_transform=np.full((1, 12), np.nan, np.float32), out_status=np.full(1, -1, np.int32), out_n_matches=np.full(1, -1, np.int32),
                out_n_inliers=np.full(1, -1, np.int32), out_variance_lin=np.full(1, np.nan, np.float64), out_angle_cos=np.full(1, np.nan, np.float64),
                out_variance_kind=np.full(1, -1, np.int32), out_matches=np.full(n, -1, np.int32), out_inliers=np.full(n, -1, np.int32))
    if device:
        held = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
        torch.cuda.synchronize()
        ptr = {k: v.data_ptr() for k, v in held.items()}
        outputs = lambda: {k: v.cpu().numpy() for k, v in held.items() if k.startswith("out_")}
    else:
        held = host
        ptr = {k: v.ctypes.data for k, v in held.items()}
        outputs = lambda: {k: v for k, v in held.items() if k.startswith("out_")}
    return dict(ptr=ptr, fo=c["from_offsets"], to=c["to_offsets"], held=held, outputs=outputs)


def _table_call(eng, entry, bufs, **over):
    """one raw call of `entry` with single fields of a good call replaced -> the status"""
    import ctypes as C
    from rtabmap_amd import capi
    kw = dict(struct_size=C.sizeof(capi.LcdMotionPnpArgs), n_pairs=1, min_inliers=4, iterations=10, refine_iterations=1, variance_median_ratio=4, seed=0,
              max_variance=0.0, reproj_error=2.0, fo=bufs["fo"], to=bufs["to"], null=(), camera=I.CAMERA, no_cameras=False)
    kw.update(over)
    a = capi.LcdMotionPnpArgs(kw["struct_size"], kw["n_pairs"], kw["min_inliers"], kw["iterations"], kw["refine_iterations"], kw["variance_median_ratio"],
                              kw["seed"], kw["max_variance"], kw["reproj_error"])
    for name in POINTERS:
        setattr(a, name, None if name in kw["null"] else bufs["ptr"][name])
    offs = [None if o is None else np.ascontiguousarray(o, dtype=np.int64) for o in (kw["fo"], kw["to"])]
    a.from_offsets, a.to_offsets = (None if o is None else o.ctypes.data for o in offs)
    cams = capi.Engine._pnp_cameras([kw["camera"]] * max(kw["n_pairs"], 1), max(kw["n_pairs"], 1))
    a.cameras = None if kw["no_cameras"] else C.cast(cams, C.c_void_p)
    return getattr(eng.L, entry)(eng.h, C.byref(a))


def _untouched(bufs):
    out = bufs["outputs"]()
    return all(np.isnan(out[k]).all() for k in ("out_transform", "out_variance_lin", "out_angle_cos")) and \
        all((out[k] == -1).all() for k in ("out_status", "out_n_matches", "out_n_inliers", "out_variance_kind", "out_matches", "out_inliers"))


def test_error_table(batch):
    """every row of the table, through both entries: the status, a message, and nothing written; then the handle serves a good call"""
    import rtabmap_amd
    eng = rtabmap_amd.Engine("f32", 64)
    pair = batch[4]
    nf, nt = pair["from_ids"].shape[0], pair["to_ids"].shape[0]
    ok = dict(KW, min_inliers=4, iterations=10, refine_iterations=1, seed=0)
    bad_fx = dict(I.CAMERA, fx=0.0)
    nan_fy = dict(I.CAMERA, fy=float("nan"))
    table = [(LCD_ERR_INVALID, dict(iterations=0)), (LCD_ERR_INVALID, dict(iterations=-3)), (LCD_ERR_UNSUPPORTED, dict(iterations=65536)),
             (LCD_ERR_INVALID, dict(reproj_error=0.0)), (LCD_ERR_INVALID, dict(reproj_error=-0.1)), (LCD_ERR_INVALID, dict(reproj_error=float("nan"))),
             (LCD_ERR_INVALID, dict(reproj_error=float("inf"))), (LCD_ERR_INVALID, dict(reproj_error=1e-60)), (LCD_ERR_INVALID, dict(reproj_error=1e30)),
             (LCD_ERR_INVALID, dict(refine_iterations=-1)), (LCD_ERR_INVALID, dict(min_inliers=0)),
             (LCD_ERR_INVALID, dict(variance_median_ratio=1)), (LCD_ERR_INVALID, dict(variance_median_ratio=0)),
             (LCD_ERR_INVALID, dict(max_variance=-1.0)), (LCD_ERR_INVALID, dict(max_variance=float("nan"))), (LCD_ERR_INVALID, dict(max_variance=float("inf"))),
             (LCD_ERR_INVALID, dict(struct_size=136)), (LCD_ERR_INVALID, dict(n_pairs=-1)), (LCD_ERR_UNSUPPORTED, dict(n_pairs=65536)),
             (LCD_ERR_INVALID, dict(fo=None)), (LCD_ERR_INVALID, dict(to=None)), (LCD_ERR_INVALID, dict(fo=[1, nf])), (LCD_ERR_INVALID, dict(to=[2, nt])),
             (LCD_ERR_INVALID, dict(n_pairs=2, fo=[0, nf, 3], to=[0, nt, nt])), (LCD_ERR_INVALID, dict(n_pairs=2, fo=[0, nf, nf], to=[0, nt, 4])),
             (LCD_ERR_UNSUPPORTED, dict(fo=[0, 8193])), (LCD_ERR_UNSUPPORTED, dict(to=[0, 8193])),
             (LCD_ERR_INVALID, dict(no_cameras=True)), (LCD_ERR_INVALID, dict(camera=bad_fx)), (LCD_ERR_INVALID, dict(camera=nan_fy))]
    table += [(LCD_ERR_INVALID, dict(null=(name,))) for name in POINTERS if name not in OPTIONAL]
    for entry, device in (("lcd_estimate_motion_pnp", False), ("lcd_estimate_motion_pnp_dev", True)):
        bufs = _table_buffers(pair, device)
        for want, over in table:
            assert _table_call(eng, entry, bufs, **over) == want, (entry, over)
            assert eng.L.lcd_last_error(eng.h), (entry, over)
            eng.synchronize()
            assert _untouched(bufs), (entry, over)
        assert _table_call(eng, entry, bufs, n_pairs=0, fo=None, to=None) == 0 and _untouched(bufs)      # no pairs: LCD_OK, nothing touched
        assert _table_call(eng, entry, bufs, null=OPTIONAL) == 0        # the handle stays usable: the good call, without to_xyz
        eng.synchronize()
        assert bufs["outputs"]()["out_n_matches"][0] == pair["m"]
    empty = {k: pair[k][:0] for k in ("from_ids", "from_xyz", "to_ids", "to_points", "to_xyz")}
    check_both(eng, [empty, pair, empty], **ok)                         # pairs without rows beside one with
    # a handle of a sharded vocabulary: refused by both entries, nothing written; the same handle serves the call once it is no such handle
    eng.set_option("shard_append", 1)
    for entry, device in (("lcd_estimate_motion_pnp", False), ("lcd_estimate_motion_pnp_dev", True)):
        bufs = _table_buffers(pair, device)
        assert _table_call(eng, entry, bufs) == LCD_ERR_UNSUPPORTED and eng.L.lcd_last_error(eng.h)
        eng.synchronize()
        assert _untouched(bufs), entry
    eng.set_option("shard_append", 0)
    check_both(eng, [pair], **ok)
    assert eng.vocab_count() == (0, 0) and eng.sig_count() == (0, 0)
    eng.close()


def test_the_reference_shaped_entry_through_the_dictionary(batch):
    """Motion2D::estimateMotion3DTo2D through VWDictionaryHip.estimate_motion_pnp: transform, the 6 x 6 covariance of all three branches, both
    id lists, a refused call, and the lending dictionary untouched"""
    from rtabmap_amd import synth
    from rtabmap_amd.vwdictionary import VWDictionaryHip
    h = VWDictionaryHip(nndr=0.8, new_words_compared_together=True)
    h.add_new_words(synth.vocab_surf(50, seed=8), 1)
    h.update()
    before = (h.index_ids(), h.visual_words, h.indexed_words, h.not_indexed_words, h.total_active_references)
    kinds = set()
    for k, sized, local, with_b, min_inliers in ((1, False, False, True, 4), (4, True, False, False, 6), (5, False, True, True, 6), (8, True, True, False, 6),
                                               (6, False, False, False, 6), (7, False, True, True, 60)):
        pair = batch[k]
        cam = I.camera(sized, local)
        guess = I.guess_of(I.true_model(pair), cam.get("local_transform")) if k == 8 else None
        kw = dict(KW, min_inliers=min_inliers, iterations=100, seed=k)
        want = M.estimate(*I.frames(pair, with_b), camera=I.model_camera(cam), guess=guess, **kw)
        call = lambda **over: h.estimate_motion_pnp((pair["from_ids"], pair["from_xyz"]), (pair["to_ids"], pair["to_points"]), pair["to_xyz"] if with_b else None,
                                                    camera=(cam["fx"], cam["fy"], cam["cx"], cam["cy"]), image_size=(cam.get("image_width", 0), cam.get("image_height", 0)),
                                                    local_transform=cam.get("local_transform"), guess=guess, **dict(kw, **over))
        t, cov, matches, inliers = call()
        assert (t is None) == (want["status"] != M.OK), k
        if t is not None:
            np.testing.assert_array_equal(M.bits(t), M.bits(want["transform"]), err_msg=str(k))
        diag = np.ones(6)
        if want["variance_kind"] == 1:
            diag[:3], diag[3:] = want["variance_lin"], 2.1981 * np.arccos(want["angle_cos"])
        elif want["variance_kind"] == 2:
            diag[:] = want["variance_lin"]
        kinds.add((want["status"], want["variance_kind"]))
        np.testing.assert_array_equal(cov[:3, :3].view(np.uint64), np.diag(diag[:3]).view(np.uint64), err_msg=str(k))
        np.testing.assert_allclose(cov[3:, 3:], np.diag(diag[3:]), rtol=1e-15, atol=0, err_msg=str(k))      # acos: the host library's against NumPy's
        assert not cov[:3, 3:].any() and not cov[3:, :3].any()
        assert matches == want["matches"].tolist() and inliers == want["inliers"].tolist(), k
        t, cov, matches, inliers = call(iterations=0)                  # refused: no transform, the identity, no ids
        assert t is None and matches == [] and inliers == []
        np.testing.assert_array_equal(cov, np.eye(6))
    assert {(M.FEW_CORRESPONDENCES, 0), (M.OK, 1), (M.OK, 2), (M.BELOW_MIN_INLIERS, 0)} <= kinds
    assert (h.index_ids(), h.visual_words, h.indexed_words, h.not_indexed_words, h.total_active_references) == before
    h.close()
