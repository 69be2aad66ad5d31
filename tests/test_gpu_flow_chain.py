"""GPU test of the optical-flow registration chained on the device with nothing read back in between: lcd_track_flow_dev ->
lcd_keypoints_3d_dev on out_to -> lcd_estimate_motion_pnp_dev with the word ids and the from-side 3-D points out of out_aux, against the same
composition of the host models, bit for bit.  lcd_keypoints_3d and lcd_estimate_motion_pnp take their sizes from the host, so both run
over every pair's whole REGION: what lies behind out_count there is what the caller put (the canaries), and the models get the same."""
import numpy as np
import pytest
import torch

import flow_track_inputs as I
import flow_track_model as M
import keypoints_3d_model as K3
import motion_pnp_model as PM

pytestmark = pytest.mark.gpu

W, H, Z = 160, 120, 2.0
CAM = dict(fx=150.0, fy=150.0, cx=79.5, cy=59.5)
KW = dict(min_inliers=10, reproj_error=2.0, iterations=60, refine_iterations=1, variance_median_ratio=4, max_variance=0.0, seed=5)
PER_PAIR = ("transform", "status", "n_matches", "n_inliers", "variance_lin", "angle_cos", "variance_kind")


def _scene(rng, shift, n):
    """a fronto-parallel textured plane Z metres away seen before and after a sideways move of the camera: the image moves by `shift`"""
    a, b = I.shifted_images(I.texture(rng, W, H), W, H, shift)
    pts = np.stack([rng.uniform(-4, W + 4, n), rng.uniform(-4, H + 4, n)], 1).astype(np.float32)      # some corners leave or start outside
    xyz = np.stack([(pts[:, 0] - CAM["cx"]) * Z / CAM["fx"], (pts[:, 1] - CAM["cy"]) * Z / CAM["fy"], np.full(n, Z)], 1).astype(np.float32)
    ids = rng.permutation(n).astype(np.int32) + 1
    aux = np.ascontiguousarray(np.concatenate([ids[:, None].view(np.float32), xyz], 1)).view(np.uint8).reshape(n, 16)
    depth = (Z + 0.001 * np.arange(W, dtype=np.float32)[None, :] + np.zeros((H, 1), np.float32)).astype(np.float32)
    return M.pair(a, b, W, 3), pts, aux, depth


def test_track_flow_then_keypoints_3d_then_pnp_on_the_device():
    import rtabmap_amd
    rng = np.random.default_rng(77)
    sizes, shifts = (150, 65, 90), ((2.5, -1.25), (-1.0, 2.0), (0.75, 0.5))
    scenes = [_scene(rng, s, n) for s, n in zip(shifts, sizes)]
    pairs, points, auxs, depths = ([s[k] for s in scenes] for k in range(4))
    aux = np.concatenate(auxs)
    N = sum(sizes)
    P = M.params()
    # ---- the models, composed as the device composes the calls
    flow = M.batch(pairs, points, P, device=True)
    pts_all, off = I.concat(points)
    to = np.full((N, 2), I.CANARY, np.float32)
    out_aux = np.full((N, 16), 0xA5, np.uint8)
    for f in range(len(pairs)):
        a, kept = int(off[f]), flow["kept"][f]
        to[a:a + len(kept)] = flow["track"][f][kept]
        out_aux[a:a + len(kept)] = auxs[f][kept]
    assert all(20 < c < n for c, n in zip(flow["count"], sizes))
    images = [K3.image(d, [K3.camera(CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"])], W) for d in depths]
    k3 = K3.batch(images, [to[int(off[f]):int(off[f + 1])] for f in range(len(pairs))], K3.KEEP_ALL, 0.0, 0.0, device=True)
    words = out_aux.view(np.int32).reshape(N, 4)
    ids, from_xyz = np.ascontiguousarray(words[:, 0]), np.ascontiguousarray(words[:, 1:]).view(np.float32)
    want = []
    for f in range(len(pairs)):
        a, b = int(off[f]), int(off[f + 1])
        want.append(PM.estimate(ids[a:b], from_xyz[a:b], ids[a:b], to[a:b], k3["xyz"][f], camera=PM.Camera(CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], 0, 0, None), **KW))
    assert any(r["status"] == 0 and len(r["inliers"]) >= KW["min_inliers"] for r in want), [r["status"] for r in want]
    # ---- the device: three calls and two strided copies on one stream, one synchronisation at the end
    stream = torch.cuda.Stream()
    eng = rtabmap_amd.Engine("f32", 64, stream=stream.cuda_stream)
    with torch.cuda.stream(stream):
        st = I.stage_dev(pairs, points, aux=aux)
        d_depth = [torch.from_numpy(d).cuda() for d in depths]
        full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device="cuda")
        k_count, k_index, k_xyz = full((len(pairs),), I.CANARY, torch.int32), full((N,), I.CANARY, torch.int32), full((N, 3), I.CANARY, torch.float32)
        n = len(pairs)
        out = dict(transform=full((n, 12), float("nan"), torch.float32), status=full((n,), -1, torch.int32), n_matches=full((n,), -1, torch.int32),
                   n_inliers=full((n,), -1, torch.int32), variance_lin=full((n,), float("nan"), torch.float64), angle_cos=full((n,), float("nan"), torch.float64),
                   variance_kind=full((n,), -1, torch.int32), matches=full((N,), -1, torch.int32), inliers=full((N,), -1, torch.int32))
    stream.synchronize()
    k3_images = [dict(data=d, cameras=im["cameras"], width=W, n_cameras=1, type=1) for d, im in zip(d_depth, images)]
    with torch.cuda.stream(stream):
        I.launch_dev(eng, st, P)
        eng.keypoints_3d_dev(st["to"], off, k3_images, k_count, k_index, k_xyz, filter="keep_all")
        d_words = st["aux"].view(torch.int32).view(N, 4)
        d_ids, d_from_xyz = d_words[:, 0].contiguous(), d_words[:, 1:].contiguous().view(torch.float32)
        eng.estimate_motion_pnp_dev(d_ids, d_from_xyz, off, d_ids, st["to"], off, [CAM] * n, out["transform"], out["status"], out["n_matches"], out["n_inliers"],
                                    out["variance_lin"], out["angle_cos"], out["variance_kind"], out["matches"], out["inliers"], d_to_xyz=k_xyz, **KW)
    eng.synchronize()
    stream.synchronize()
    I.assert_same(I.to_host(eng, st), pairs, points, P, device=True, aux=aux, want=flow, canary=I.CANARY)
    got_xyz = k_xyz.cpu().numpy()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    for f in range(n):
        a, b = int(off[f]), int(off[f + 1])
        np.testing.assert_array_equal(I.bits(got_xyz[a:b]), I.bits(k3["xyz"][f]), err_msg="pair %d xyz" % f)
        r = want[f]
        np.testing.assert_array_equal(PM.bits(got["transform"][f]), PM.bits(np.asarray(r["transform"], np.float32)), err_msg="pair %d transform" % f)
        assert (got["status"][f], got["n_matches"][f], got["n_inliers"][f], got["variance_kind"][f]) == (r["status"], len(r["matches"]), len(r["inliers"]), r["variance_kind"]), f
        np.testing.assert_array_equal(got["matches"][a:a + len(r["matches"])], r["matches"], err_msg="pair %d matches" % f)
        np.testing.assert_array_equal(got["inliers"][a:a + len(r["inliers"])], r["inliers"], err_msg="pair %d inliers" % f)
        assert np.float64(got["variance_lin"][f]).view(np.uint64) == np.float64(r["variance_lin"]).view(np.uint64)
        assert np.float64(got["angle_cos"][f]).view(np.uint64) == np.float64(r["angle_cos"]).view(np.uint64)
    eng.close()
