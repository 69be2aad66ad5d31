"""The host mirror of lcd_filter_scans (rtabmap_amd/host/ScanFilter.cpp, the rule's header compiled for the CPU) against
tests/scan_filter_model.py, bit for bit; every refusal; the sweep count; and the rule's normals against an independent float64 pipeline.
No GPU."""
import numpy as np
import pytest

import register_icp_plane_inputs as PI
import scan_filter_inputs as I
import scan_filter_model as M

# The largest difference between pipeline64 run in float32 and in float64 over the accuracy scene's compared points, as measured when the rule
# was written; the bound on the rule's normals is 4 x what the test measures, and the test asserts the figure has not moved.
FP32_NOISE_MEASURED = {5: 3.58e-6, 10: 7.97e-7}


def mirror(scan, cap=None, **kw):
    from rtabmap_amd import vwdictionary as V
    return V.filter_scans_cpu(scan, capacity=cap, **kw)


def assert_same(a, b, what):
    assert (a["status"], a["count"]) == (b["status"], b["count"]), what
    np.testing.assert_array_equal(a["stage_counts"], b["stage_counts"], err_msg=what)
    np.testing.assert_array_equal(I.bits(a["xyz"]), I.bits(b["xyz"]), err_msg=what)
    assert (a["normals"] is None) == (b["normals"] is None), what
    if a["normals"] is not None:
        np.testing.assert_array_equal(I.bits(a["normals"]), I.bits(b["normals"]), err_msg=what)


@pytest.mark.parametrize("name", sorted(I.cases()))
def test_the_mirror_equals_the_model(name):
    c = I.cases()[name]
    caps = c["caps"] or [None] * len(c["scans"])
    for k, (s, cap) in enumerate(zip(c["scans"], caps)):
        assert_same(mirror(s, cap, device_entry=True, **c["kw"]), M.filter_scan(s, cap, device_entry=True, **c["kw"]), "%s scan %d" % (name, k))


def test_the_mirror_equals_the_model_at_every_size():
    for kw in (dict(), dict(voxel_size=0.2, normal_k=5), dict(normal_radius=0.3), dict(downsampling_step=2, normal_k=8)):
        for s in I.size_batch():
            assert_same(mirror(s, **kw), M.filter_scan(s, **kw), "%d rows %r" % (s.shape[0], kw))


def test_refusals():
    s = I.cloud(50, 1)
    base = dict(voxel_size=0.2, normal_k=5)
    bad = [(M.INVALID, dict(normal_radius=0.3)), (M.INVALID, dict(normal_k=33)), (M.INVALID, dict(normal_k=-1)), (M.INVALID, dict(voxel_size=-0.1)),
           (M.INVALID, dict(normal_k=0, normal_radius=-1.0)), (M.INVALID, dict(ground_normals_up=-0.5)), (M.INVALID, dict(voxel_size=float("nan"))),
           (M.INVALID, dict(range_min=float("inf"))), (M.INVALID, dict(range_max=float("nan"))), (M.INVALID, dict(viewpoint=(0.0, float("inf"), 0.0))),
           (M.INVALID, dict(normal_k=0, normal_radius=float("inf"))), (M.UNSUPPORTED, dict(is_2d=True))]
    for code, kw in bad:
        assert mirror(s, **dict(base, **kw)) == code, kw
        with pytest.raises(M.Refused) as err:
            M.filter_scan(s, **dict(base, **kw))
        assert err.value.code == code, kw
    big = np.zeros((16385, 3), np.float32)
    assert mirror(big) == M.UNSUPPORTED and mirror(big[:16384])["status"] == M.OK
    assert mirror(np.zeros((32770, 3), np.float32), downsampling_step=2) == M.UNSUPPORTED
    nan_row = s.copy()
    nan_row[7, 1] = np.nan
    assert mirror(nan_row) == M.INVALID and mirror(nan_row, device_entry=True)["count"] == 49
    assert mirror(s, range_min=-1.0, range_max=-2.0)["count"] == 50           # negative bounds are off
    assert mirror(s, is_2d=True, range_max=0.5)["status"] == M.OK             # 2-D without normals is served


def test_six_and_seven_sweeps_change_no_bit_of_any_normal():
    scans = [c["scans"][0] for n, c in sorted(I.cases().items()) if n.startswith(("k_", "radius_", "voxel_then", "ground"))]
    kws = [c["kw"] for n, c in sorted(I.cases().items()) if n.startswith(("k_", "radius_", "voxel_then", "ground"))]
    rng = np.random.default_rng(3)
    room = (PI.room(rng, 2000)[0] + rng.normal(0, 0.005, (2000, 3)) + np.array([-2, -1.5, -1.2])).astype(np.float32)
    scans.append(room)
    kws.append(dict(voxel_size=0.05, normal_k=5))
    for s, kw in zip(scans, kws):
        five = M.filter_scan(s, **kw)
        for sweeps in (6, 7):
            more = M.filter_scan(s, sweeps=sweeps, **kw)
            np.testing.assert_array_equal(I.bits(five["normals"]), I.bits(more["normals"]))


@pytest.mark.parametrize("k", [5, 10])
def test_normals_against_an_independent_float64_pipeline(k):
    """register_icp_plane_inputs.room, 6 000 points with 5 mm noise, shifted by (-2, -1.5, -1.2), leaf 0.05.  A point is left out when its
    neighbour set differs between the two pipelines or its float64 eigenvalue gap (l1 - l0) / l2 is below 0.05; at most 10 % may be left out.
    The bound on every entry of the rule's normals is 4 x the largest difference between the independent pipeline in float32 and in float64."""
    rng = np.random.default_rng(1)
    scan = (PI.room(rng, 6000)[0] + rng.normal(0, 0.005, (6000, 3)) + np.array([-2, -1.5, -1.2])).astype(np.float32)
    rule = M.filter_scan(scan, voxel_size=0.05, normal_k=k)
    p64, p32 = M.pipeline64(scan, 0.05, k), M.pipeline64(scan, 0.05, k, np.float32)
    n = p64["cloud"].shape[0]
    assert rule["stage_counts"][1] == n == p32["cloud"].shape[0] and rule["count"] == n
    assert np.abs(rule["xyz"][:n] - p64["cloud"]).max() < 1e-6
    nb_rule = np.sort(M.neighbours_k(rule["xyz"][:n], k), axis=1)
    stable = p64["gap"] >= 0.05
    use = stable & (nb_rule == p64["neighbours"]).all(axis=1)
    use32 = stable & (p32["neighbours"] == p64["neighbours"]).all(axis=1)
    left_out = 1.0 - use.mean()
    noise = np.abs(p32["normals"][use32].astype(np.float64) - p64["normals"][use32]).max()
    err = np.abs(rule["normals"][:n][use].astype(np.float64) - p64["normals"][use]).max()
    print("K = %d: %d voxels, %.2f %% left out, float32 noise of the independent pipeline %.3g, the rule's error %.3g" % (k, n, 100 * left_out, noise, err))
    assert left_out <= 0.10
    assert noise <= 1.25 * FP32_NOISE_MEASURED[k] and noise >= 0.5 * FP32_NOISE_MEASURED[k]
    assert err <= 4 * noise
