"""GPU tests of lcd_estimate_motion_3d and lcd_estimate_motion_3d_dev (rtabmap_amd/csrc/motion_3d.hip) against tests/motion_3d_model.py.
Every comparison is exact: transform bits, status, counts, ids over the whole region, variance bits."""
import numpy as np
import pytest
import torch

import motion_3d_inputs as I
import motion_3d_model as M

pytestmark = pytest.mark.gpu

LCD_ERR_INVALID, LCD_ERR_UNSUPPORTED = 1, 5
KW = dict(min_inliers=4, inlier_distance=0.1, iterations=300, refine_iterations=5, seed=3)
_model_cache = {}


def model_of(pair, **kw):
    key = (id(pair), tuple(sorted(kw.items())))
    if key not in _model_cache:
        _model_cache[key] = (pair, M.estimate(*I.frames(pair), **kw))       # the pair is kept so that its id stays its own
    return _model_cache[key][1]


def expected(pairs, **kw):
    """the model's results laid out as the call lays its outputs out"""
    n = len(pairs)
    out = dict(transform=np.zeros((n, 12), np.float32), status=np.zeros(n, np.int32), n_matches=np.zeros(n, np.int32),
               n_inliers=np.zeros(n, np.int32), variance=np.zeros(n, np.float64), matches=[], inliers=[])
    for k, p in enumerate(pairs):
        r = model_of(p, **kw)
        region = p["from_ids"].shape[0]
        out["transform"][k], out["status"][k], out["variance"][k] = r["transform"], r["status"], r["variance"]
        out["n_matches"][k], out["n_inliers"][k] = len(r["matches"]), len(r["inliers"])
        for name in ("matches", "inliers"):
            out[name].append(np.concatenate([r[name], np.zeros(region - len(r[name]), np.int32)]).astype(np.int32))
    for name in ("matches", "inliers"):
        out[name] = np.concatenate(out[name] + [np.zeros(0, np.int32)])
    return out


def assert_same(got, want, what=""):
    np.testing.assert_array_equal(got["status"], want["status"], err_msg=what + " status")
    np.testing.assert_array_equal(got["n_matches"], want["n_matches"], err_msg=what + " n_matches")
    np.testing.assert_array_equal(got["n_inliers"], want["n_inliers"], err_msg=what + " n_inliers")
    np.testing.assert_array_equal(got["matches"], want["matches"], err_msg=what + " matches")
    np.testing.assert_array_equal(got["inliers"], want["inliers"], err_msg=what + " inliers")
    np.testing.assert_array_equal(I.bits(got["transform"]), I.bits(want["transform"]), err_msg=what + " transform")
    np.testing.assert_array_equal(np.ascontiguousarray(got["variance"]).view(np.uint64), want["variance"].view(np.uint64), err_msg=what + " variance")


def stage_dev(pairs):
    """the batch on the device, outputs canary-filled, uploaded and synchronised"""
    fi, fx, fo, ti, tx, to = I.concatenate(pairs)
    n, nf = len(pairs), fi.shape[0]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    st = dict(fi=dev(fi), fx=dev(fx), fo=fo, ti=dev(ti), tx=dev(tx), to=to,
              transform=torch.full((n, 12), float("nan"), dtype=torch.float32, device="cuda"), status=torch.full((n,), -1, dtype=torch.int32, device="cuda"),
              n_matches=torch.full((n,), -1, dtype=torch.int32, device="cuda"), n_inliers=torch.full((n,), -1, dtype=torch.int32, device="cuda"),
              variance=torch.full((n,), float("nan"), dtype=torch.float64, device="cuda"),
              matches=torch.full((max(nf, 1),), -1, dtype=torch.int32, device="cuda"), inliers=torch.full((max(nf, 1),), -1, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    return st


def launch_dev(eng, st, **kw):
    eng.estimate_motion_3d_dev(st["fi"], st["fx"], st["fo"], st["ti"], st["tx"], st["to"], st["transform"], st["status"], st["n_matches"],
                               st["n_inliers"], st["variance"], st["matches"], st["inliers"], **kw)
    return st


def to_host(eng, st):
    eng.synchronize()
    nf = int(st["fo"][-1])
    out = {k: st[k].cpu().numpy() for k in ("transform", "status", "n_matches", "n_inliers", "variance", "matches", "inliers")}
    out["matches"], out["inliers"] = out["matches"][:nf], out["inliers"][:nf]
    return out


def run_dev(eng, pairs, **kw):
    return to_host(eng, launch_dev(eng, stage_dev(pairs), **kw))


def run_host(eng, pairs, **kw):
    return eng.estimate_motion_3d(*I.concatenate(pairs), **kw)


def check_both(eng, pairs, what="", **kw):
    want = expected(pairs, **kw)
    assert_same(run_dev(eng, pairs, **kw), want, what + " dev")
    assert_same(run_host(eng, pairs, **kw), want, what + " host")
    return want


def _refused(status, call, *args, **kw):
    from rtabmap_amd import capi
    with pytest.raises(capi.LcdError) as err:
        call(*args, **kw)
    assert err.value.status == status, err.value


@pytest.fixture(scope="module")
def batch():
    return I.mixed_batch()


@pytest.mark.parametrize("refine", I.REFINE)
@pytest.mark.parametrize("iterations", I.ITERATIONS)
def test_both_entries_equal_the_model(batch, iterations, refine):
    """pairs of 0, 2, 3, 5, 6, 63, 64, 65, 255, 256, 257 and 1100 correspondences in ONE batch, inside frames with duplicates and one-sided ids"""
    import rtabmap_amd
    eng = rtabmap_amd.Engine("f32", 64)
    want = check_both(eng, batch, min_inliers=4, inlier_distance=0.1, iterations=iterations, refine_iterations=refine, seed=iterations + refine)
    assert want["n_matches"].tolist() == list(I.BATCH_SIZES)
    if iterations == 300:
        assert (want["status"][5:] == M.OK).all() and (want["status"][:3] == M.FEW_CORRESPONDENCES).all()
    assert eng.vocab_count() == (0, 0) and eng.sig_count() == (0, 0)
    eng.close()


def test_all_outliers_ties_invalid_draws_and_the_refinement_branches():
    import rtabmap_amd
    eng = rtabmap_amd.Engine("f32", 64)
    want = check_both(eng, [I.all_outlier_pair()], min_inliers=10, inlier_distance=0.1, iterations=300, refine_iterations=5, seed=1)
    assert want["status"][0] != M.OK and not want["transform"].any()
    for name in sorted(I.REFINE_CASES):
        pair, kw = I.refine_case(name)
        for refine in (kw["refine_iterations"],) + I.REFINE:
            check_both(eng, [pair], what=name, **dict(kw, refine_iterations=refine))
    over = I.overflow_refit_pair()
    for refine in (0, 1, 5):
        want = check_both(eng, [over], what="overflow", min_inliers=3, inlier_distance=I.OVERFLOW_DISTANCE, iterations=20, refine_iterations=refine, seed=1)
        assert want["status"][0] == (M.FEW_INLIERS if refine else M.OK)
    seed = I.seed_with_invalid_first(3, 1)
    three, twelve = I.exact_pair(3), I.exact_pair(12)
    assert check_both(eng, [three, twelve], min_inliers=3, inlier_distance=0.1, iterations=1, refine_iterations=0, seed=seed)["status"][0] == M.NO_MODEL
    assert check_both(eng, [three, twelve], min_inliers=3, inlier_distance=0.1, iterations=2, refine_iterations=0, seed=seed)["status"].tolist() == [M.OK, M.OK]
    noisy = I.random_pair(np.random.default_rng(4), 6, outliers=0.0, noise=0.01, decoys=False)
    check_both(eng, [noisy], min_inliers=3, inlier_distance=0.2, iterations=30, refine_iterations=0, seed=2)      # a tie between different models
    half = I.exact_pair(12)
    half["to_xyz"][6:] = half["to_xyz"][6:] * np.float32(-3) + np.float32(40)
    assert check_both(eng, [half], min_inliers=7, inlier_distance=0.1, iterations=100, refine_iterations=5, seed=0)["status"][0] == M.BELOW_MIN_INLIERS
    eng.close()


def test_a_pair_of_8192_rows_reads_its_coordinates_from_the_scratch():
    """8192 x 8192 rows, 8000 correspondences: more than the kernel stages in LDS"""
    import rtabmap_amd
    eng = rtabmap_amd.Engine("f32", 64)
    big = I.big_pair()
    kw = dict(min_inliers=20, inlier_distance=0.1, iterations=64, refine_iterations=5, seed=8)
    want = check_both(eng, [big], **kw)
    assert want["status"][0] == M.OK and want["n_matches"][0] == 8000 > I.STAGE_CAP and want["n_inliers"][0] > I.STAGE_CAP
    # beside small pairs, which the same launch stages
    small = I.mixed_batch()[3:6]
    assert_same(run_dev(eng, [small[0], big, small[1], small[2]], **kw), expected([small[0], big, small[1], small[2]], **kw), "mixed with small pairs")
    eng.close()


def test_700_pairs_and_the_position_in_the_batch():
    """700 pairs in one call, made of ten distinct ones in turn: a pair's bits do not depend on where it stands"""
    import rtabmap_amd
    rng = np.random.default_rng(16)
    distinct = [I.random_pair(rng, m) for m in (0, 3, 5, 17, 33, 64, 65, 90, 130, 257)]
    pairs = [distinct[(k * 7 + k // 10) % 10] for k in range(700)]
    kw = dict(min_inliers=5, inlier_distance=0.1, iterations=40, refine_iterations=2, seed=21)
    eng = rtabmap_amd.Engine("f32", 64)
    want = expected(pairs, **kw)
    got = run_dev(eng, pairs, **kw)
    assert_same(got, want, "700 dev")
    assert_same(run_host(eng, pairs, **kw), want, "700 host")
    first = {}
    for k, p in enumerate(pairs):                                       # the same pair, the same bits, wherever it stands
        j = first.setdefault(id(p), k)
        assert I.bits(got["transform"][k]).tolist() == I.bits(got["transform"][j]).tolist() and got["variance"][k] == got["variance"][j]
    alone = run_dev(eng, [distinct[9]], **kw)
    k = next(k for k, p in enumerate(pairs) if p is distinct[9])
    np.testing.assert_array_equal(I.bits(alone["transform"][0]), I.bits(got["transform"][k]))
    eng.close()


def test_unsynchronised_back_to_back_calls_share_the_scratch():
    """three device calls enqueued without a synchronisation in between, the largest second: its scratch and job table grow while the first
    launch is still in flight, and each call reads its own"""
    import rtabmap_amd
    eng = rtabmap_amd.Engine("f32", 64)
    batch = I.mixed_batch()
    groups = [batch[:6], batch[8:], batch[6:9]]
    assert sum(p["from_ids"].shape[0] for p in groups[1]) > 4 * sum(p["from_ids"].shape[0] for p in groups[0])
    sts = [launch_dev(eng, stage_dev(g), **KW) for g in groups]
    for g, st in zip(groups, sts):
        assert_same(to_host(eng, st), expected(g, **KW))
    eng.close()


def test_pipelined_frame_stream_is_untouched_by_motion_estimation():
    """A pipelined SURF handle runs an appending frame stream; lcd_estimate_motion_3d_dev calls between the frames change no frame output,
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
    pairs = I.mixed_batch()[2:8]
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
                launch_dev(eng, sts[t], **KW)
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
    """lcd_keypoints_3d_dev (both frames, every keypoint kept: a keypoint without depth carries NaNs) -> lcd_match_pairs_dev -> lcd_estimate_motion_3d_dev
    with nothing read back in between: the matcher's ids are per row of each frame, as the depth stage's points are.  The second frame is
    the first one's keypoints in another order over the same depth image, so the motion is the identity, exactly."""
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
    eng = rtabmap_amd.Engine("f32", 64)
    st = KI.stage_dev([im, im], points)
    d_rows = torch.from_numpy(np.concatenate([rows_a, rows_b])).cuda()
    d_ids = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
    res = stage_dev([dict(from_ids=np.zeros(n, np.int32), from_xyz=np.zeros((n, 3), np.float32), to_ids=np.zeros(n, np.int32), to_xyz=np.zeros((n, 3), np.float32))])
    kw = dict(min_inliers=20, inlier_distance=0.05, iterations=100, refine_iterations=5, seed=6)
    torch.cuda.synchronize()
    KI.launch_dev(eng, st, KM.KEEP_ALL, 0.5, 0.0)
    eng.match_pairs_dev(d_rows[:n], d_rows[n:], [0, n], [0, n], d_ids[:n], d_ids[n:], "dictionary")
    eng.estimate_motion_3d_dev(d_ids[:n], st["xyz"][:n], [0, n], d_ids[n:], st["xyz"][n:], [0, n], res["transform"], res["status"], res["n_matches"],
                               res["n_inliers"], res["variance"], res["matches"], res["inliers"], **kw)
    got = to_host(eng, dict(res, fo=np.array([0, n])))
    xyz = st["xyz"].cpu().numpy()
    ids = d_ids.cpu().numpy()
    want_xyz = KM.frame(im, pts, KM.KEEP_ALL, 0.5, 0.0, device=True)[1]
    np.testing.assert_array_equal(I.bits(xyz[:n]), I.bits(want_xyz))
    f_ids, t_ids = eng.match_pair(rows_a, rows_b, "dictionary")
    np.testing.assert_array_equal(ids[:n], f_ids)
    np.testing.assert_array_equal(ids[n:], t_ids)
    pair = dict(from_ids=ids[:n], from_xyz=xyz[:n], to_ids=ids[n:], to_xyz=xyz[n:])
    want = expected([pair], **kw)
    assert_same(got, want, "chain")
    assert want["status"][0] == M.OK and 100 < want["n_inliers"][0] == want["n_matches"][0] <= n
    np.testing.assert_array_equal(want["transform"][0], np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32))
    eng.close()


POINTERS = ("from_word_ids", "from_xyz", "to_word_ids", "to_xyz", "out_transform", "out_status", "out_n_matches", "out_n_inliers", "out_variance",
            "out_matches", "out_inliers")


def _table_buffers(pair, device):
    """one pair with canary-filled outputs, on the host or on the device -> dict(ptr = the address per pointer field, fo, to, outputs())"""
    fi, fx, fo, ti, tx, to = I.concatenate([pair])
    n = fi.shape[0]
    host = dict(from_word_ids=fi, from_xyz=fx, to_word_ids=ti, to_xyz=tx, out_transform=np.full((1, 12), np.nan, np.float32),
                out_status=np.full(1, -1, np.int32), out_n_matches=np.full(1, -1, np.int32), out_n_inliers=np.full(1, -1, np.int32),
                out_variance=np.full(1, np.nan, np.float64), out_matches=np.full(n, -1, np.int32), out_inliers=np.full(n, -1, np.int32))
    if device:
        held = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
        torch.cuda.synchronize()
        ptr = {k: v.data_ptr() for k, v in held.items()}
        outputs = lambda: {k: v.cpu().numpy() for k, v in held.items() if k.startswith("out_")}
    else:
        held = host
        ptr = {k: v.ctypes.data for k, v in held.items()}
        outputs = lambda: {k: v for k, v in held.items() if k.startswith("out_")}
    return dict(ptr=ptr, fo=fo, to=to, held=held, outputs=outputs)


def _table_call(eng, entry, bufs, **over):
    """one raw call of `entry` with single fields of a good call replaced -> the status"""
    import ctypes as C
    from rtabmap_amd import capi
    kw = dict(struct_size=C.sizeof(capi.LcdMotion3dArgs), n_pairs=1, min_inliers=3, iterations=10, refine_iterations=1, seed=0, inlier_distance=0.1,
              fo=bufs["fo"], to=bufs["to"], null=())
    kw.update(over)
    a = capi.LcdMotion3dArgs(kw["struct_size"], kw["n_pairs"], kw["min_inliers"], kw["iterations"], kw["refine_iterations"], kw["seed"], kw["inlier_distance"])
    for name in POINTERS:
        setattr(a, name, None if name in kw["null"] else bufs["ptr"][name])
    offs = [None if o is None else np.ascontiguousarray(o, dtype=np.int64) for o in (kw["fo"], kw["to"])]
    a.from_offsets, a.to_offsets = (None if o is None else o.ctypes.data for o in offs)
    return getattr(eng.L, entry)(eng.h, C.byref(a))


def _untouched(bufs):
    out = bufs["outputs"]()
    return all(np.isnan(out[k]).all() for k in ("out_transform", "out_variance")) and \
        all((out[k] == -1).all() for k in ("out_status", "out_n_matches", "out_n_inliers", "out_matches", "out_inliers"))


def test_error_table():
    """every row of the table, through both entries: the status, a message, and nothing written; then the handle serves a good call"""
    import rtabmap_amd
    eng = rtabmap_amd.Engine("f32", 64)
    pair = I.exact_pair(5)
    ok = dict(min_inliers=3, inlier_distance=0.1, iterations=10, refine_iterations=1, seed=0)
    table = [(LCD_ERR_INVALID, dict(iterations=0)), (LCD_ERR_INVALID, dict(iterations=-3)), (LCD_ERR_UNSUPPORTED, dict(iterations=65536)),
             (LCD_ERR_INVALID, dict(inlier_distance=0.0)), (LCD_ERR_INVALID, dict(inlier_distance=-0.1)), (LCD_ERR_INVALID, dict(inlier_distance=float("nan"))),
             (LCD_ERR_INVALID, dict(inlier_distance=float("inf"))), (LCD_ERR_INVALID, dict(refine_iterations=-1)), (LCD_ERR_INVALID, dict(min_inliers=0)),
             (LCD_ERR_INVALID, dict(struct_size=128)), (LCD_ERR_INVALID, dict(n_pairs=-1)), (LCD_ERR_UNSUPPORTED, dict(n_pairs=65536)),
             (LCD_ERR_INVALID, dict(fo=None)), (LCD_ERR_INVALID, dict(to=None)), (LCD_ERR_INVALID, dict(fo=[1, 5])), (LCD_ERR_INVALID, dict(to=[2, 5])),
             (LCD_ERR_INVALID, dict(n_pairs=2, fo=[0, 5, 3], to=[0, 5, 5])), (LCD_ERR_INVALID, dict(n_pairs=2, fo=[0, 5, 5], to=[0, 5, 4])),
             (LCD_ERR_UNSUPPORTED, dict(fo=[0, 8193])), (LCD_ERR_UNSUPPORTED, dict(to=[0, 8193]))]
    table += [(LCD_ERR_INVALID, dict(null=(name,))) for name in POINTERS]
    for entry, device in (("lcd_estimate_motion_3d", False), ("lcd_estimate_motion_3d_dev", True)):
        bufs = _table_buffers(pair, device)
        for want, over in table:
            assert _table_call(eng, entry, bufs, **over) == want, (entry, over)
            assert eng.L.lcd_last_error(eng.h), (entry, over)
            eng.synchronize()
            assert _untouched(bufs), (entry, over)
        assert _table_call(eng, entry, bufs, n_pairs=0, fo=None, to=None) == 0 and _untouched(bufs)      # no pairs: LCD_OK, nothing touched
        assert _table_call(eng, entry, bufs) == 0                       # the handle stays usable: the good call
        eng.synchronize()
        assert bufs["outputs"]()["out_status"][0] == M.OK
    empty = dict(from_ids=pair["from_ids"][:0], from_xyz=pair["from_xyz"][:0], to_ids=pair["to_ids"][:0], to_xyz=pair["to_xyz"][:0])
    check_both(eng, [empty, pair, empty], **ok)                         # pairs without rows beside one with
    # a handle of a sharded vocabulary: refused by both entries, nothing written; the same handle serves the call once it is no such handle
    eng.set_option("shard_append", 1)
    for entry, device in (("lcd_estimate_motion_3d", False), ("lcd_estimate_motion_3d_dev", True)):
        bufs = _table_buffers(pair, device)
        assert _table_call(eng, entry, bufs) == LCD_ERR_UNSUPPORTED and eng.L.lcd_last_error(eng.h)
        eng.synchronize()
        assert _untouched(bufs), entry
    eng.set_option("shard_append", 0)
    check_both(eng, [pair], **ok)
    assert eng.vocab_count() == (0, 0) and eng.sig_count() == (0, 0)
    eng.close()
