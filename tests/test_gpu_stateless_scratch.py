"""GPU test of the scratch the stateless calls share (rtabmap_amd/csrc/stateless_scratch.h, which lists them): all nine families --
lcd_match_pairs, lcd_match_guided, lcd_select_features, lcd_expand_word_ids, lcd_keypoints_3d, lcd_estimate_motion_3d,
lcd_estimate_motion_pnp, lcd_register_icp and lcd_register_icp_plane -- take the two pinned job-table slots in turn and stage their host
entries' data in the same four buffers.  Calls of DIFFERENT families follow each other here, each with a table of another size and
content, and every result is compared exactly with what the family's own test compares with: its model (tests/*_model.py), through the
helpers of its inputs module or of its test.  An optional array of each kind is left out once -- lcd_estimate_motion_pnp's to_xyz, the
cross-check's out_to_dist, a selection's rows and payload -- so a field that is null stays null through the host form."""
import numpy as np
import pytest
import torch

import feature_select_inputs as FI
import feature_select_model as FM
import guided_match_inputs as GI
import guided_match_model as GM
import keypoints_3d_inputs as KI
import keypoints_3d_model as KM
import motion_3d_inputs as M3I
import motion_pnp_inputs as MPI
import pair_match_inputs as PI
import pair_match_model as PM
import register_icp_inputs as RI
import register_icp_plane_inputs as RPI
import test_gpu_motion_3d as T3
import test_gpu_motion_pnp as TP
import test_gpu_register_icp as TR
import test_gpu_register_icp_plane as TRP

pytestmark = pytest.mark.gpu

DEPTH = (KM.FILTER_3D, 1.5, 3.0)
M3_KW = dict(min_inliers=4, inlier_distance=0.1, iterations=40, refine_iterations=2, seed=3)
PNP_KW = dict(TP.KW, min_inliers=4, iterations=40, refine_iterations=2)
ICP_KW = dict(RI.KW, search=TR.M.SEARCH_AUTO)
PLANE_KW = dict(RPI.KW, search=TRP.M.SEARCH_AUTO)
PNP_TO_XYZ = {"large": True, "small": False}                              # the smaller batch leaves the optional to_xyz out


def _pairs_concat(pairs):
    fo = np.cumsum([0] + [f.shape[0] for f, _ in pairs]).astype(np.int64)
    to = np.cumsum([0] + [t.shape[0] for _, t in pairs]).astype(np.int64)
    return np.concatenate([f for f, _ in pairs]), np.concatenate([t for _, t in pairs]), fo, to


def _dictionary(oracle, pairs):
    e = [PM.dictionary_pair(oracle, f, t, 0.8, True) for f, t in pairs]
    return np.concatenate([x[0] for x in e]), np.concatenate([x[1] for x in e])


def _expansion(rng, sizes):
    """-> (offsets, count, index, word_ids, first ids) of a batch of expansion frames"""
    ex = [FI.expansion_frame(rng, n) for n in sizes]
    off = np.cumsum([0] + list(sizes)).astype(np.int64)
    count = np.array([e["count"] for e in ex], np.int32)
    index = np.full(int(off[-1]), -9, np.int32)
    word_ids = np.full(int(off[-1]), 77, np.int32)                        # behind a frame's count: never read
    for f, e in enumerate(ex):
        index[off[f]:off[f] + e["count"]] = e["index"]
        word_ids[off[f]:off[f] + e["count"]] = e["word_ids"]
    return off, count, index, word_ids, np.array([9000 + 100 * f for f in range(len(ex))], np.int32)


def _depth_frames(rng, dtype, dim, sizes):
    """frames of these sizes over ONE 8 x 6 depth image (the host entry stages it once), with responses, rows and a 12-byte payload, and
    the model's answer"""
    im, pool = KI.random_frame(rng, np.uint16, 8, 6, 1, sum(sizes), host_ok=True)
    cuts = np.cumsum([0] + list(sizes))
    d = dict(images=[im] * len(sizes), points=[pool[a:b] for a, b in zip(cuts[:-1], cuts[1:])],
             kw=dict(response=rng.standard_normal(sum(sizes)).astype(np.float32), rows=FI.rows_of(rng, dtype, dim, sum(sizes)),
                     aux=rng.integers(0, 256, (sum(sizes), 12), dtype=np.uint8)))
    d["want"] = KM.batch(d["images"], d["points"], *DEPTH)                # no keypoint here is one the two entries differ on
    return d


def _inputs(oracle, dtype, dim):
    """per family a larger and a smaller batch with the model's answer; the pairs also one by one"""
    rng = np.random.default_rng(600 + dim)
    pair_a, pair_b = PI.interleaved_pair(dtype, dim, 65, 40, 610 + dim), PI.interleaved_pair(dtype, dim, 33, 31, 620 + dim)
    guided = {"large": [GI.general_pair(dtype, dim, 33, 31, 65, 630 + dim), GI.general_pair(dtype, dim, 20, 18, 30, 640 + dim)],
              "small": [GI.general_pair(dtype, dim, 12, 10, 17, 650 + dim)]}
    frames = {"large": [FI.tied_frame(rng, n) for n in (40, 55, 70)], "small": [FI.tied_frame(rng, 60)]}
    x = dict(pairs={"one": [pair_a], "large": [pair_a, pair_b], "small": [pair_b]}, guided=guided, frames=frames, max_features=50,
             rows={k: FI.rows_of(rng, dtype, dim, sum(len(f["response"]) for f in v)) for k, v in frames.items()},
             expand={"large": _expansion(rng, (50, 64)), "small": _expansion(rng, (30,))})
    x["pairs_exp"] = {k: _dictionary(oracle, v) for k, v in x["pairs"].items()}
    x["cross_exp"] = PM.cross_check(PI.dist(oracle, pair_b[1], pair_b[0]))
    x["guided_exp"] = {k: GI.expected_batch(oracle, v, GI.RADIUS, 0.8, GM.RATIO, GM.P2F) for k, v in guided.items()}
    x["expand_exp"] = {k: FM.expand_batch(*v) for k, v in x["expand"].items()}
    assert (FM.select_batch(frames["large"], 50)[0] == [40, 50, 50]).all()   # max_features cuts two of the three frames
    # the five families behind the selection: a batch of two frames or pairs of a few dozen rows, and a batch of one
    x["depth"] = {"large": _depth_frames(rng, dtype, dim, (45, 30)), "small": _depth_frames(rng, dtype, dim, (25,))}
    x["m3"] = {"large": [M3I.random_pair(rng, 30), M3I.random_pair(rng, 20)], "small": [M3I.random_pair(rng, 25)]}
    x["pnp"] = {"large": [MPI.random_pair(rng, 30), MPI.random_pair(rng, 20)], "small": [MPI.random_pair(rng, 25)]}
    x["icp"] = {"large": [RI.pair(40, 35, False, 660 + dim, noise=0.003), RI.pair(30, 45, True, 661 + dim, noise=0.003)],
                "small": [RI.pair(25, 20, False, 662 + dim, noise=0.003)]}
    x["plane"] = {"large": [RPI.pair(40, 35, 670 + dim, noise=0.003), RPI.pair(30, 45, 671 + dim, noise=0.003)],
                  "small": [RPI.pair(25, 20, 672 + dim, noise=0.003)]}
    x["m3_exp"] = {k: T3.expected(v, **M3_KW) for k, v in x["m3"].items()}
    x["pnp_exp"] = {k: TP.expected(v, to_xyz=PNP_TO_XYZ[k], **PNP_KW) for k, v in x["pnp"].items()}
    x["icp_exp"] = {k: TR.expected(v, **RI.KW) for k, v in x["icp"].items()}
    x["plane_exp"] = {k: TRP.expected(v, **RPI.KW) for k, v in x["plane"].items()}
    return x


def _host_entries(eng, x):
    """the nine host entries with the larger inputs, then all nine again with the smaller ones: every staging buffer is then used at a
    smaller size, with another call's bytes behind"""
    for size in ("large", "small"):
        f, t, fo, to = _pairs_concat(x["pairs"][size])
        gf, gt = eng.match_pairs(f, t, fo, to, "dictionary")
        np.testing.assert_array_equal(gf, x["pairs_exp"][size][0], err_msg=size + " pairs, from")
        np.testing.assert_array_equal(gt, x["pairs_exp"][size][1], err_msg=size + " pairs, to")
        GI.assert_same(GI.run_host(eng, x["guided"][size]), x["guided_exp"][size], size + " guided")
        FI.assert_same(FI.run_host(eng, x["frames"][size], x["max_features"], rows=x["rows"][size]), x["frames"][size], x["max_features"],
                       rows=x["rows"][size], what=size + " select")
        np.testing.assert_array_equal(eng.expand_word_ids(*x["expand"][size]), x["expand_exp"][size], err_msg=size + " expand")
        d = x["depth"][size]
        KI.assert_same(KI.run_host(eng, d["images"], d["points"], *DEPTH, **d["kw"]), d["images"], d["points"], *DEPTH, what=size + " depth",
                       want=d["want"], **d["kw"])
        T3.assert_same(T3.run_host(eng, x["m3"][size], **M3_KW), x["m3_exp"][size], size + " motion 3d")
        TP.assert_same(TP.run_host(eng, x["pnp"][size], to_xyz=PNP_TO_XYZ[size], **PNP_KW), x["pnp_exp"][size], size + " motion pnp")
        TR.assert_same(TR.run_host(eng, x["icp"][size], **ICP_KW), x["icp_exp"][size], size + " icp")
        TRP.assert_same(TRP.run_host(eng, x["plane"][size], **PLANE_KW), x["plane_exp"][size], size + " icp plane")
    f, t = x["pairs"]["small"][0]
    gm, gd = eng.match_pair(f, t, "cross_check")                          # the other mode, over what the dictionary calls left behind
    np.testing.assert_array_equal(gm, x["cross_exp"][0])
    np.testing.assert_array_equal(np.ascontiguousarray(gd, np.float32).view(np.uint32), x["cross_exp"][1].view(np.uint32))
    # a selection without rows and payload: the two optional inputs and their outputs stay null
    FI.assert_same(FI.run_host(eng, x["frames"]["small"], x["max_features"]), x["frames"]["small"], x["max_features"], what="select, no rows")


def test_calls_of_every_family_back_to_back(oracle):
    """One _dev call of each of the nine families and a match_pairs_dev that makes two groups (two table uploads) are enqueued with no
    synchronisation between them: eleven job tables through the two slots, each slot's next user a call of another family, every output
    canary-filled.  Then the host entries in turn, larger inputs first."""
    import rtabmap_amd
    x = _inputs(oracle, "f32", 64)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    canary = lambda n, dt=torch.int32: torch.full((n,), -7, dtype=dt, device="cuda")
    eng = rtabmap_amd.Engine("f32", 64)
    eng.set_option("pair_match_budget", 4)                                # one distance: every pair is a group of its own
    p1 = _pairs_concat(x["pairs"]["one"])
    p5 = _pairs_concat(x["pairs"]["large"])
    d1, d5 = [dev(a) for a in p1[:2]], [dev(a) for a in p5[:2]]
    o1, o5 = [canary(a.shape[0]) for a in p1[:2]], [canary(a.shape[0]) for a in p5[:2]]
    g = GI.concat(x["guided"]["large"])
    dg = [dev(a) for a in g[:5]]
    og = [canary(g[2].shape[0]), canary(g[2].shape[0]), torch.full((g[2].shape[0], 2), -7.0, dtype=torch.float32, device="cuda"), canary(g[1].shape[0])]
    st = FI.stage_dev(x["frames"]["large"], rows=x["rows"]["large"])
    e_off, e_count, e_index, e_words, e_first = x["expand"]["large"]
    de = [dev(a) for a in (e_count, e_index, e_words, e_first)]
    oe = canary(int(e_off[-1]))
    d = x["depth"]["large"]
    sk = KI.stage_dev(d["images"], d["points"], **d["kw"])
    s3, sp = T3.stage_dev(x["m3"]["large"]), TP.stage_dev(x["pnp"]["large"])
    si, sl = TR.stage_dev(x["icp"]["large"]), TRP.stage_dev(x["plane"]["large"])
    torch.cuda.synchronize()

    eng.match_pairs_dev(d1[0], d1[1], p1[2], p1[3], o1[0], o1[1], "dictionary")
    KI.launch_dev(eng, sk, *DEPTH)
    eng.match_guided_dev(*dg, *g[5:], *og)
    T3.launch_dev(eng, s3, **M3_KW)
    FI.launch_dev(eng, st, x["max_features"])
    TP.launch_dev(eng, sp, TP.cameras_of(x["pnp"]["large"], MPI.CAMERA), **PNP_KW)
    eng.expand_word_ids_dev(e_off, de[0], de[1], de[2], oe, de[3])
    TR.launch_dev(eng, si, **ICP_KW)
    eng.match_pairs_dev(d5[0], d5[1], p5[2], p5[3], o5[0], o5[1], "dictionary")
    TRP.launch_dev(eng, sl, **PLANE_KW)
    eng.synchronize()

    for got, exp, what in ((o1, x["pairs_exp"]["one"], "first call"), (o5, x["pairs_exp"]["large"], "two groups")):
        np.testing.assert_array_equal(got[0].cpu().numpy(), exp[0], err_msg=what + ", from")
        np.testing.assert_array_equal(got[1].cpu().numpy(), exp[1], err_msg=what + ", to")
    GI.assert_same(dict(count=og[0].cpu().numpy(), match=og[1].cpu().numpy(), dist=og[2].cpu().numpy(), owner=og[3].cpu().numpy()), x["guided_exp"]["large"])
    FI.assert_same(FI.to_host(eng, st), x["frames"]["large"], x["max_features"], rows=x["rows"]["large"], device=True)
    np.testing.assert_array_equal(oe.cpu().numpy(), x["expand_exp"]["large"])
    KI.assert_same(KI.to_host(eng, sk), d["images"], d["points"], *DEPTH, device=True, what="depth", want=d["want"], **d["kw"])
    T3.assert_same(T3.to_host(eng, s3), x["m3_exp"]["large"], "motion 3d")
    TP.assert_same(TP.to_host(eng, sp), x["pnp_exp"]["large"], "motion pnp")
    TR.assert_same(TR.to_host(eng, si), x["icp_exp"]["large"], "icp")
    TRP.assert_same(TRP.to_host(eng, sl), x["plane_exp"]["large"], "icp plane")
    _host_entries(eng, x)
    assert eng.vocab_count() == (0, 0) and eng.sig_count() == (0, 0)
    eng.close()


def test_host_entries_in_turn_on_a_padded_handle(oracle):
    """u8 x 61: rows are stored 64 bytes apart, so every host entry pads them on the way in and lcd_select_features and lcd_keypoints_3d
    un-pad them on the way out"""
    import rtabmap_amd
    x = _inputs(oracle, "u8", 61)
    eng = rtabmap_amd.Engine("u8", 61)
    _host_entries(eng, x)
    eng.close()
