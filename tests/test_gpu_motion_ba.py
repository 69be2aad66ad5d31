"""GPU tests of lcd_refine_motion_ba and lcd_refine_motion_ba_dev (rtabmap_amd/csrc/motion_ba.hip) against tests/motion_ba_model.py.  Every
comparison is exact: transform bits, status, counts, ids over the whole region, the bits of both costs and of both gate figures."""
import numpy as np
import pytest
import torch

import motion_ba_inputs as I
import motion_ba_model as M
import motion_pnp_inputs as PI

pytestmark = pytest.mark.gpu

LCD_ERR_INVALID, LCD_ERR_UNSUPPORTED = 1, 5
KW = dict(min_inliers=1, iterations=20, pixel_variance=1.0, robust_delta=8.0, max_inliers_mean_distance=0.0, min_inliers_distribution=0.0)
PER_PAIR = ("transform", "status", "n_inliers", "n_outliers", "chi2_before", "chi2_after", "lm_accepted", "inliers_mean_distance", "inliers_distribution")
_model_cache = {}


def model_of(pair, from_points, to_xyz, prior, baselines, **kw):
    key = (id(pair), from_points, to_xyz, prior, baselines, tuple(sorted(kw.items())))
    if key not in _model_cache:                                            # the pair is kept so that its id stays its own
        a, k = I.args(pair, from_points, to_xyz, **kw)
        k.update(prior_variance=prior, n_inliers=pair.get("n_inliers"))
        if baselines is not None:
            k["baselines"] = baselines
        _model_cache[key] = (pair, M.refine(*a, **k))
    return _model_cache[key][1]


def rows_of(v, n):
    """[n x 2] float64 of one tuple for every pair or of a row per pair; None stays None"""
    if v is None:
        return None
    a = np.asarray(v, np.float64)
    return np.tile(a, (n, 1)) if a.ndim == 1 else a.reshape(n, 2).copy()


def expected(pairs, from_points=True, to_xyz=True, prior=None, baselines=None, **kw):
    """the model's results laid out as the call lays its outputs out; prior / baselines: one tuple for every pair, or [n x 2] rows"""
    n = len(pairs)
    prior, baselines = rows_of(prior, n), rows_of(baselines, n)
    row = lambda rows, k: None if rows is None else tuple(float(v) for v in rows[k])
    out = dict(transform=np.zeros((n, 12), np.float32), status=np.zeros(n, np.int32), n_inliers=np.zeros(n, np.int32), n_outliers=np.zeros(n, np.int32),
               chi2_before=np.zeros(n, np.float64), chi2_after=np.zeros(n, np.float64), lm_accepted=np.zeros(n, np.int32),
               inliers_mean_distance=np.zeros(n, np.float32), inliers_distribution=np.zeros(n, np.float32), inliers=[])
    for k, p in enumerate(pairs):
        r = model_of(p, from_points, to_xyz, row(prior, k), row(baselines, k), **kw)
        for name in PER_PAIR:
            if name != "n_inliers":
                out[name][k] = r[name]
        out["n_inliers"][k] = len(r["inliers"])
        out["inliers"].append(np.concatenate([r["inliers"], np.zeros(p["to_ids"].shape[0] - len(r["inliers"]), np.int32)]).astype(np.int32))
    out["inliers"] = np.concatenate(out["inliers"] + [np.zeros(0, np.int32)])
    return out


def assert_same(got, want, what=""):
    for name in ("status", "n_inliers", "n_outliers", "lm_accepted", "inliers"):
        np.testing.assert_array_equal(got[name], want[name], err_msg=what + " " + name)
    for name in ("transform", "inliers_mean_distance", "inliers_distribution"):
        np.testing.assert_array_equal(np.ascontiguousarray(got[name]).view(np.uint32), want[name].view(np.uint32), err_msg=what + " " + name)
    for name in ("chi2_before", "chi2_after"):
        np.testing.assert_array_equal(np.ascontiguousarray(got[name]).view(np.uint64), want[name].view(np.uint64), err_msg=what + " " + name)


def call_kw(n, prior, baselines, kw):
    k = dict(kw)
    k["prior_variance"] = rows_of(prior, n)
    if baselines is None:
        k["default_baseline"] = I.BASELINE
    else:
        k["baselines"] = rows_of(baselines, n)
    return k


def run_host(eng, pairs, from_points=True, to_xyz=True, prior=None, baselines=None, **kw):
    c = I.concatenate(pairs, from_points, to_xyz)
    return eng.refine_motion_ba(c["from_ids"], c["from_xyz"], c["from_offsets"], c["to_ids"], c["to_points"], c["to_offsets"], c["inliers"], c["n_inliers"],
                                c["transforms"], c["cameras_from"], c["cameras_to"], from_points=c["from_points"], to_xyz=c["to_xyz"],
                                **call_kw(len(pairs), prior, baselines, kw))


def run_dev(eng, pairs, from_points=True, to_xyz=True, prior=None, baselines=None, **kw):
    """the batch on the device, outputs canary-filled"""
    c = I.concatenate(pairs, from_points, to_xyz)
    n, nt = len(pairs), c["to_ids"].shape[0]
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device="cuda")
    o = dict(transform=full((n, 12), float("nan"), torch.float32), status=full((n,), -1, torch.int32), inliers=full((max(nt, 1),), -1, torch.int32),
             n_inliers=full((n,), -1, torch.int32), n_outliers=full((n,), -1, torch.int32), chi2_before=full((n,), float("nan"), torch.float64),
             chi2_after=full((n,), float("nan"), torch.float64), lm_accepted=full((n,), -1, torch.int32),
             inliers_mean_distance=full((n,), float("nan"), torch.float32), inliers_distribution=full((n,), float("nan"), torch.float32))
    d = {k: dev(c[k]) for k in ("from_ids", "from_xyz", "from_points", "to_ids", "to_points", "to_xyz", "inliers", "n_inliers", "transforms")}
    torch.cuda.synchronize()
    eng.refine_motion_ba_dev(d["from_ids"], d["from_xyz"], c["from_offsets"], d["to_ids"], d["to_points"], c["to_offsets"], d["inliers"], d["n_inliers"],
                             d["transforms"], c["cameras_from"], c["cameras_to"], o["transform"], o["status"], o["inliers"], o["n_inliers"], o["n_outliers"],
                             o["chi2_before"], o["chi2_after"], o["lm_accepted"], o["inliers_mean_distance"], o["inliers_distribution"],
                             d_from_points=d["from_points"], d_to_xyz=d["to_xyz"], **call_kw(n, prior, baselines, kw))
    eng.synchronize()
    out = {k: v.cpu().numpy() for k, v in o.items()}
    out["inliers"] = out["inliers"][:nt]
    return out


def check_both(eng, pairs, what="", **kw):
    want = expected(pairs, **kw)
    assert_same(run_dev(eng, pairs, **kw), want, what + " dev")
    assert_same(run_host(eng, pairs, **kw), want, what + " host")
    return want


@pytest.fixture(scope="module")
def eng():
    import rtabmap_amd
    e = rtabmap_amd.Engine("f32", 64)
    yield e
    assert e.vocab_count() == (0, 0) and e.sig_count() == (0, 0)
    e.close()


@pytest.fixture(scope="module")
def counts():
    return I.count_pairs()


def test_both_entries_equal_the_model_at_every_count(eng, counts):
    """pairs of 1, 3, 4, 63, 64, 65, 255, 256, 257 and 1100 inliers in ONE batch, a tenth of them planted outliers, every third pair behind a
    local transform, with a prior"""
    want = check_both(eng, counts, prior=(1e-4, 4e-4), **KW)
    assert [len(p["inliers"]) for p in counts] == list(I.COUNTS)
    assert (want["status"] == M.OK).all() and want["n_outliers"][3:].all() and (want["lm_accepted"] > 0).all()
    assert (want["chi2_after"] <= want["chi2_before"]).all()


@pytest.mark.parametrize("n", (I.STAGE_CAP, I.STAGE_CAP + 1))
def test_the_switch_between_lds_and_scratch(eng, n):
    """the last number of points whose state is staged in LDS, and the first that is read from the scratch"""
    p = _model_cache.setdefault(("stage", n), I.seeded(400 + n, n, outliers=n // 20, extra=0))
    want = check_both(eng, [p], **KW)
    assert want["status"][0] == M.OK and want["n_outliers"][0] >= n // 20


def test_a_pair_of_8192_rows(eng):
    """the size limit: 8192 rows a side, 8000 of them inliers, read from the scratch"""
    p = _model_cache.setdefault("big", I.seeded(77, 8000, outliers=300, rows=8192))
    assert p["from_ids"].shape[0] == 8192 and p["to_ids"].shape[0] == 8192
    want = check_both(eng, [p], **KW)
    assert want["status"][0] == M.OK and want["n_outliers"][0] >= 300


@pytest.fixture(scope="module")
def statuses():
    return I.status_batch()


@pytest.mark.parametrize("reverse", (False, True))
def test_every_status_in_one_launch(eng, statuses, reverse):
    pairs, expect = statuses
    if reverse:
        pairs, expect = pairs[::-1], expect[::-1]
    want = check_both(eng, pairs, **dict(KW, **I.STATUS_KW))
    assert want["status"].tolist() == expect
    assert not want["transform"][want["status"] != M.OK].any() and want["transform"][want["status"] == M.OK].any()


@pytest.mark.parametrize("left_out", ("from_points", "to_xyz", "prior_variance", "baselines"))
def test_each_optional_array_left_out(eng, counts, left_out):
    """through the host form (and the device form): no from-side observations, mono to-edges, identity information, the default baseline"""
    kw = dict(from_points=left_out != "from_points", to_xyz=left_out != "to_xyz", prior=None if left_out == "prior_variance" else (2e-4, 1e-3),
              baselines=None if left_out == "baselines" else (0.12, 0.075))
    want = check_both(eng, counts[3:8], what=left_out, **dict(KW, **kw))
    assert (want["status"] == M.OK).all()


def test_a_baseline_that_is_not_positive_gives_mono_edges(eng, counts):
    want = check_both(eng, counts[3:6], baselines=(0.0, -1.0), **KW)
    assert (want["status"] == M.OK).all()


def test_no_kernel_no_iterations_and_the_gates_alone(eng, counts):
    check_both(eng, counts[3:6], **dict(KW, robust_delta=0.0))
    want = check_both(eng, counts[3:6], **dict(KW, iterations=0, max_inliers_mean_distance=100.0, min_inliers_distribution=1e-4))
    assert (want["lm_accepted"] == 0).all() and want["inliers_mean_distance"].all() and want["inliers_distribution"].all()
    np.testing.assert_array_equal(want["transform"], np.stack([p["transform"] for p in counts[3:6]]))


def test_between_calls_of_another_family(eng, counts):
    """lcd_estimate_motion_pnp in front and behind, so that the shared table slots and staging buffers change size between the calls"""
    rng = np.random.default_rng(5)
    for m in (700, 30):
        q = PI.random_pair(rng, m)
        c = PI.concatenate([q])
        r = eng.estimate_motion_pnp(c["from_ids"], c["from_xyz"], c["from_offsets"], c["to_ids"], c["to_points"], c["to_offsets"], [PI.CAMERA],
                                    to_xyz=c["to_xyz"], min_inliers=6, iterations=50)
        assert r["status"][0] == 0
        check_both(eng, counts[2:7] if m == 700 else counts[5:], "behind pnp %d" % m, **KW)


def test_refusals_write_nothing(eng, counts):
    pairs = counts[3:5]
    c = I.concatenate(pairs)
    base = dict(from_points=c["from_points"], to_xyz=c["to_xyz"], **KW)
    pos = [c["from_ids"], c["from_xyz"], c["from_offsets"], c["to_ids"], c["to_points"], c["to_offsets"], c["inliers"], c["n_inliers"], c["transforms"],
           c["cameras_from"], c["cameras_to"]]

    def refused(code, positional=None, **kw):
        with pytest.raises(RuntimeError) as e:
            eng.refine_motion_ba(*(positional or pos), **dict(base, **kw))
        assert ("LCD_ERR_INVALID" if code == LCD_ERR_INVALID else "LCD_ERR_UNSUPPORTED") in str(e.value), str(e.value)
    for kw in (dict(iterations=-1), dict(min_inliers=-1), dict(pixel_variance=0.0), dict(pixel_variance=float("nan")), dict(pixel_variance=1e-60),
               dict(robust_delta=-1.0), dict(robust_delta=float("inf")), dict(robust_delta=1e30), dict(max_inliers_mean_distance=-1.0),
               dict(min_inliers_distribution=float("nan")), dict(default_baseline=float("nan")), dict(baselines=[[0.1, float("inf")]] * 2),
               dict(prior_variance=[[1e-4, -1.0]] * 2), dict(prior_variance=[[float("nan"), 1.0]] * 2), dict(struct_size=240)):
        refused(LCD_ERR_INVALID, **kw)
    bad_cam = [dict(c["cameras_to"][0], fx=0.0), c["cameras_to"][1]]
    refused(LCD_ERR_INVALID, pos[:10] + [bad_cam])
    refused(LCD_ERR_INVALID, pos[:2] + [np.array([1, 5, 9], np.int64)] + pos[3:])
    refused(LCD_ERR_INVALID, pos[:5] + [c["to_offsets"][::-1].copy()] + pos[6:])
    refused(LCD_ERR_INVALID, pos[:6] + [None] + pos[7:])
    refused(LCD_ERR_INVALID, pos[:7] + [None] + pos[8:])
    refused(LCD_ERR_INVALID, pos[:8] + [None] + pos[9:])
    refused(LCD_ERR_UNSUPPORTED, iterations=65536)
    big = I.seeded(9, 10, rows=8193)
    cb = I.concatenate([big])
    refused(LCD_ERR_UNSUPPORTED, [cb["from_ids"], cb["from_xyz"], cb["from_offsets"], cb["to_ids"], cb["to_points"], cb["to_offsets"], cb["inliers"],
                                  cb["n_inliers"], cb["transforms"], cb["cameras_from"], cb["cameras_to"]], from_points=cb["from_points"], to_xyz=cb["to_xyz"])
    assert_same(run_host(eng, pairs, **KW), expected(pairs, **KW), "behind the refusals")


def test_no_pairs(eng):
    e = np.zeros(0, np.int32)
    out = eng.refine_motion_ba(e, np.zeros((0, 3), np.float32), np.zeros(1, np.int64), e, np.zeros((0, 2), np.float32), np.zeros(1, np.int64), e, e,
                               np.zeros((0, 12), np.float32), [], [])
    assert out["status"].shape[0] == 0
