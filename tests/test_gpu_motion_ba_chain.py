"""lcd_estimate_motion_pnp_dev -> lcd_refine_motion_ba_dev on one stream with nothing read back between them: the second call takes the first
one's out_inliers, out_n_inliers and out_transform where they lie in device memory.  The result equals the two models chained, bit for bit."""
import numpy as np
import pytest
import torch

import motion_ba_inputs as I
import motion_ba_model as M
import motion_pnp_inputs as PI
import motion_pnp_model as MP
from test_gpu_motion_ba import assert_same

pytestmark = pytest.mark.gpu

PNP_KW = dict(min_inliers=20, iterations=100, reproj_error=8.0, refine_iterations=1, variance_median_ratio=4, max_variance=0.0, seed=11)
BA_KW = dict(min_inliers=20, iterations=20, pixel_variance=1.0, robust_delta=8.0, max_inliers_mean_distance=0.0, min_inliers_distribution=0.0)


def test_the_pnp_and_the_adjustment_chained_on_the_device():
    import rtabmap_amd
    rng = np.random.default_rng(70)
    pairs = [I.pair(rng, m, outliers=m // 10, outlier_px=(4.0, 7.0)) for m in (40, 150, 10, 300)]       # the third has fewer correspondences than min_inliers
    cam = I.camera(True)
    c = I.concatenate(pairs)
    n, nt = len(pairs), c["to_ids"].shape[0]

    # ---- the two models chained
    want = dict(transform=np.zeros((n, 12), np.float32), status=np.zeros(n, np.int32), n_inliers=np.zeros(n, np.int32), n_outliers=np.zeros(n, np.int32),
                chi2_before=np.zeros(n, np.float64), chi2_after=np.zeros(n, np.float64), lm_accepted=np.zeros(n, np.int32),
                inliers_mean_distance=np.zeros(n, np.float32), inliers_distribution=np.zeros(n, np.float32), inliers=[])
    pnp_status = []
    for k, p in enumerate(pairs):
        first = MP.estimate(p["from_ids"], p["from_xyz"], p["to_ids"], p["to_points"], p["to_xyz"], camera=PI.model_camera(cam), **PNP_KW)
        pnp_status.append(first["status"])
        r = M.refine(p["from_ids"], p["from_xyz"], p["to_ids"], p["to_points"], first["inliers"], first["transform"], from_points=p["from_points"],
                     to_xyz=p["to_xyz"], camera_from=cam, camera_to=cam, baselines=(I.BASELINE, I.BASELINE), **BA_KW)
        for name in want:
            if name not in ("inliers", "n_inliers"):
                want[name][k] = r[name]
        want["n_inliers"][k] = len(r["inliers"])
        want["inliers"].append(np.concatenate([r["inliers"], np.zeros(p["to_ids"].shape[0] - len(r["inliers"]), np.int32)]).astype(np.int32))
    want["inliers"] = np.concatenate(want["inliers"])
    assert pnp_status == [MP.OK, MP.OK, MP.FEW_CORRESPONDENCES, MP.OK]
    assert want["status"].tolist() == [M.OK, M.OK, M.NO_INPUT, M.OK] and want["n_outliers"][3] > 0

    # ---- the two calls, one stream, one synchronisation at the end
    eng = rtabmap_amd.Engine("f32", 64)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device="cuda")
    d = {k: dev(c[k]) for k in ("from_ids", "from_xyz", "from_points", "to_ids", "to_points", "to_xyz")}
    mid = dict(transform=full((n, 12), float("nan"), torch.float32), status=full((n,), -1, torch.int32), n_matches=full((n,), -1, torch.int32),
               n_inliers=full((n,), -1, torch.int32), variance_lin=full((n,), float("nan"), torch.float64), angle_cos=full((n,), float("nan"), torch.float64),
               variance_kind=full((n,), -1, torch.int32), matches=full((nt,), -1, torch.int32), inliers=full((nt,), -1, torch.int32))
    o = dict(transform=full((n, 12), float("nan"), torch.float32), status=full((n,), -1, torch.int32), inliers=full((nt,), -1, torch.int32),
             n_inliers=full((n,), -1, torch.int32), n_outliers=full((n,), -1, torch.int32), chi2_before=full((n,), float("nan"), torch.float64),
             chi2_after=full((n,), float("nan"), torch.float64), lm_accepted=full((n,), -1, torch.int32),
             inliers_mean_distance=full((n,), float("nan"), torch.float32), inliers_distribution=full((n,), float("nan"), torch.float32))
    torch.cuda.synchronize()
    eng.estimate_motion_pnp_dev(d["from_ids"], d["from_xyz"], c["from_offsets"], d["to_ids"], d["to_points"], c["to_offsets"], [cam] * n, mid["transform"],
                                mid["status"], mid["n_matches"], mid["n_inliers"], mid["variance_lin"], mid["angle_cos"], mid["variance_kind"], mid["matches"],
                                mid["inliers"], d_to_xyz=d["to_xyz"], **PNP_KW)
    eng.refine_motion_ba_dev(d["from_ids"], d["from_xyz"], c["from_offsets"], d["to_ids"], d["to_points"], c["to_offsets"], mid["inliers"], mid["n_inliers"],
                             mid["transform"], [cam] * n, [cam] * n, o["transform"], o["status"], o["inliers"], o["n_inliers"], o["n_outliers"],
                             o["chi2_before"], o["chi2_after"], o["lm_accepted"], o["inliers_mean_distance"], o["inliers_distribution"],
                             d_from_points=d["from_points"], d_to_xyz=d["to_xyz"], default_baseline=I.BASELINE, **BA_KW)
    eng.synchronize()
    got = {k: v.cpu().numpy() for k, v in o.items()}
    assert_same(got, want, "chained")
    assert mid["status"].cpu().numpy().tolist() == pnp_status
    assert eng.vocab_count() == (0, 0) and eng.sig_count() == (0, 0)
    eng.close()
