"""lcd_verify_epipolar and lcd_verify_epipolar_dev against the NumPy model of the rule (epipolar_model.py), exactly -- ints and float bits -- with
every output canary-filled.  A pair's model result is computed once and shared (the cache is keyed by the pair and the call's parameters)."""
import numpy as np
import pytest

import epipolar_inputs as I
import epipolar_model as M

pytestmark = pytest.mark.gpu

KW = dict(match_count_min=8, iterations=60, ransac_threshold=3.0, seed=5)
_cache = {}


@pytest.fixture(scope="module")
def eng():
    import rtabmap_amd
    e = rtabmap_amd.Engine("f32", 64)
    yield e
    assert e.vocab_count() == (0, 0) and e.sig_count() == (0, 0)
    e.close()


def expected(pairs, **kw):
    """the model's results as a call lays them out"""
    n = sum(p["to_ids"].shape[0] for p in pairs)
    out = dict(fundamental=np.zeros((len(pairs), 9), np.float32), status=np.zeros(len(pairs), np.int32), n_pairs=np.zeros(len(pairs), np.int32),
               n_inliers=np.zeros(len(pairs), np.int32), matches=np.zeros(n, np.int32), inliers=np.zeros(n, np.int32))
    at = 0
    for k, p in enumerate(pairs):
        key = (id(p), tuple(sorted(kw.items())))
        if key not in _cache:
            _cache[key] = (p, M.verify(*I.frames(p), **kw))
        r = _cache[key][1]
        out["fundamental"][k], out["status"][k] = r["fundamental"], r["status"]
        out["n_pairs"][k], out["n_inliers"][k] = r["matches"].shape[0], r["inliers"].shape[0]
        out["matches"][at:at + r["matches"].shape[0]] = r["matches"]
        out["inliers"][at:at + r["inliers"].shape[0]] = r["inliers"]
        at += p["to_ids"].shape[0]
    return out


def run_host(eng, pairs, leave_out=(), **kw):
    return eng.verify_epipolar(*I.batch(pairs), leave_out=leave_out, **kw)


def run_dev(eng, pairs, leave_out=(), **kw):
    import torch
    fi, fp, fo, ti, tp, to = I.batch(pairs)
    dev = "cuda"
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    n, npairs = ti.shape[0], len(pairs)
    out = dict(fundamental=torch.full((max(npairs, 1), 9), float("nan"), device=dev), status=torch.full((max(npairs, 1),), -1, dtype=torch.int32, device=dev),
               n_pairs=torch.full((max(npairs, 1),), -1, dtype=torch.int32, device=dev), n_inliers=torch.full((max(npairs, 1),), -1, dtype=torch.int32, device=dev),
               matches=torch.full((max(n, 1),), -1, dtype=torch.int32, device=dev), inliers=torch.full((max(n, 1),), -1, dtype=torch.int32, device=dev))
    arg = {k: (None if k in leave_out else v) for k, v in out.items()}
    eng.verify_epipolar_dev(t(fi), t(fp), fo, t(ti), t(tp), to, arg["fundamental"], arg["status"], arg["n_pairs"], arg["n_inliers"], arg["matches"],
                            arg["inliers"], **kw)
    eng.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    for k in ("fundamental", "status", "n_pairs", "n_inliers"):
        res[k] = res[k][:npairs]
    res["matches"], res["inliers"] = res["matches"][:n], res["inliers"][:n]
    return res


def assert_same(got, want, what, leave_out=()):
    for k, w in want.items():
        g = got[k]
        if k in leave_out:                                              # the canary is still there
            assert (np.isnan(g).all() if g.dtype == np.float32 else (g == -1).all()), (what, k)
            continue
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        assert g.view(np.uint32).tobytes() == w.view(np.uint32).tobytes() if g.dtype == np.float32 else np.array_equal(g, w), (what, k, g, w)


def check_both(eng, pairs, what="", leave_out=(), **kw):
    kw = dict(KW, **kw)
    want = expected(pairs, **kw)
    assert_same(run_dev(eng, pairs, leave_out, **kw), want, what + " dev", leave_out)
    assert_same(run_host(eng, pairs, leave_out, **kw), want, what + " host", leave_out)
    return want


SIZES = (8, 9, 63, 64, 65, 255, 256, 257, 1100)


@pytest.fixture(scope="module")
def sized():
    return [I.scene(100 + m, m, outliers=0.3, extra=4) for m in SIZES]


def frame_only(n, seed):
    ids, pts = I.empty_frame(n, seed)
    return ids, pts


def small(nf, nt):
    a, b = frame_only(nf, 1), frame_only(nt, 2)
    return dict(from_ids=a[0], from_points=a[1], to_ids=b[0] + 5000, to_points=b[1])


def test_correspondence_counts_at_the_wave_and_workgroup_edges(eng, sized):
    """m = 8, 9, 63, 64, 65, 255, 256, 257 and 1 100 in one batch, and the same batch reversed"""
    want = check_both(eng, sized, "sizes")
    assert want["n_pairs"].tolist() == list(SIZES) and (want["status"][2:] == M.OK).all()   # (the pairs of 8 and 9 hold 30 % outliers)
    check_both(eng, sized[::-1], "sizes reversed")


@pytest.mark.parametrize("iterations", (1, 85, 86, 300))
def test_iteration_counts_on_either_side_of_a_chunk(eng, sized, iterations):
    """255 and 258 candidates lie on either side of a 256-candidate chunk"""
    check_both(eng, sized[2:6], "iterations %d" % iterations, iterations=iterations)


def test_small_and_empty_frames_first_in_the_middle_and_last(eng, sized):
    s = [small(0, 0), small(1, 2), sized[3], small(2, 0), small(0, 1), sized[1], small(2, 2), small(1, 0)]
    want = check_both(eng, s, "small frames")
    assert want["status"].tolist() == [M.FEW_PAIRS, M.FEW_PAIRS, M.OK, M.FEW_PAIRS, M.FEW_PAIRS, want["status"][5], M.FEW_PAIRS, M.FEW_PAIRS]
    empty_to = [dict(p, to_ids=p["to_ids"][:0], to_points=p["to_points"][:0]) for p in sized[:3]]
    check_both(eng, empty_to, "every to-frame empty")


def test_the_largest_frames(eng, sized):
    """One pair of 8 192 rows a side with 100 pairs, beside a small one in both orders.  Every pair this call accepts is staged in LDS (the
    carve holds 8 192 correspondences of four planes); 8 193 rows are refused (test_refusals_write_nothing)."""
    s = I.scene(77, 100, outliers=0.3, extra=8092)
    assert s["from_ids"].shape[0] == 8192 and s["to_ids"].shape[0] == 8192
    full = I.scene(78, 8192, outliers=0.5, extra=0)
    want = check_both(eng, [s, sized[0], full], "8192 rows", iterations=10)
    assert want["n_pairs"].tolist() == [100, 8, 8192]
    check_both(eng, [full, sized[0], s], "8192 rows reversed", iterations=10)


def test_more_pairs_than_compute_units(eng, sized):
    eight = sized[:8]
    want = check_both(eng, eight * 40, "320 pairs")
    assert want["status"].shape[0] == 320


def test_every_status_in_one_launch(eng):
    p = I.scene(3, 100)
    n = M.verify(*I.frames(p), **KW)["inliers"].shape[0]
    pairs = [p, I.with_m(7), I.all_equal(100), I.scene(9, 100, outliers=0.7)]
    want = check_both(eng, pairs, "statuses", match_count_min=n)
    assert want["status"].tolist() == [M.OK, M.FEW_PAIRS, M.NO_MODEL, M.FEW_INLIERS]
    want = check_both(eng, pairs, "statuses", match_count_min=n + 1)
    assert want["status"][0] == M.FEW_INLIERS and want["fundamental"][0].any()
    want = check_both(eng, [I.all_equal(), I.collinear(), I.c3_zero(), I.nan_keypoint(), I.id_cases()], "branches")
    assert want["status"].tolist() == [M.NO_MODEL] * 4 + [M.OK]


@pytest.mark.parametrize("leave_out", (("fundamental",), ("matches",), ("inliers",), ("fundamental", "matches", "inliers")))
def test_each_optional_output_left_out(eng, sized, leave_out):
    check_both(eng, sized[:5], "without %s" % (leave_out,), leave_out=leave_out)


def test_between_two_pnp_calls_the_shared_scratch_changes_nothing(eng, sized):
    import motion_pnp_inputs as P
    from test_gpu_motion_pnp import KW as PNP_KW, run_host as pnp_host
    batch = P.mixed_batch()[:6]
    before = pnp_host(eng, batch, P.CAMERA, None, True, **PNP_KW)
    check_both(eng, sized[:6], "between")
    after = pnp_host(eng, batch, P.CAMERA, None, True, **PNP_KW)
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k


LCD_ERR_INVALID, LCD_ERR_UNSUPPORTED = 1, 5
OPTIONAL = ("out_fundamental", "out_matches", "out_inliers")


def test_refusals_write_nothing(eng, sized):
    """every refusal, on the host entry through the raw argument struct: the code, and every output still holds its canary"""
    import ctypes as C
    from rtabmap_amd.capi import LcdEpipolarArgs
    pairs = sized[:2]
    fi, fp, fo, ti, tp, to = I.batch(pairs)
    nf, nt = int(fo[-1]), int(to[-1])

    def call(struct_size=None, n_pairs=2, fo_=fo, to_=to, null=(), **kw):
        kw = dict(KW, **kw)
        outs = dict(out_fundamental=np.full((2, 9), np.nan, np.float32), out_status=np.full(2, -1, np.int32), out_n_pairs=np.full(2, -1, np.int32),
                    out_n_inliers=np.full(2, -1, np.int32), out_matches=np.full(nt, -1, np.int32), out_inliers=np.full(nt, -1, np.int32))
        ins = dict(from_word_ids=fi, from_points=fp, to_word_ids=ti, to_points=tp)
        a = LcdEpipolarArgs(C.sizeof(LcdEpipolarArgs) if struct_size is None else struct_size, n_pairs, kw["match_count_min"], kw["iterations"],
                            kw["seed"], kw["ransac_threshold"])
        keep = [None if fo_ is None else np.ascontiguousarray(fo_, dtype=np.int64), None if to_ is None else np.ascontiguousarray(to_, dtype=np.int64)]
        a.from_offsets, a.to_offsets = (None if k is None else k.ctypes.data for k in keep)
        for name, arr in list(ins.items()) + list(outs.items()):
            setattr(a, name, None if name in null else arr.ctypes.data)
        rc = eng.L.lcd_verify_epipolar(eng.h, C.byref(a))
        clean = all(np.isnan(v).all() if v.dtype == np.float32 else (v == -1).all() for v in outs.values())
        return rc, clean

    table = [(LCD_ERR_INVALID, dict(iterations=0)), (LCD_ERR_INVALID, dict(iterations=-3)), (LCD_ERR_UNSUPPORTED, dict(iterations=65536)),
             (LCD_ERR_INVALID, dict(ransac_threshold=0.0)), (LCD_ERR_INVALID, dict(ransac_threshold=-0.1)), (LCD_ERR_INVALID, dict(ransac_threshold=float("nan"))),
             (LCD_ERR_INVALID, dict(ransac_threshold=float("inf"))), (LCD_ERR_INVALID, dict(ransac_threshold=1e-30)), (LCD_ERR_INVALID, dict(ransac_threshold=1e30)),
             (LCD_ERR_INVALID, dict(match_count_min=0)), (LCD_ERR_INVALID, dict(struct_size=120)), (LCD_ERR_INVALID, dict(n_pairs=-1)),
             (LCD_ERR_UNSUPPORTED, dict(n_pairs=65536)), (LCD_ERR_INVALID, dict(fo_=None)), (LCD_ERR_INVALID, dict(to_=None)),
             (LCD_ERR_INVALID, dict(fo_=[1, nf, nf])), (LCD_ERR_INVALID, dict(fo_=[0, nf, 3])), (LCD_ERR_INVALID, dict(to_=[0, nt, 4])),
             (LCD_ERR_UNSUPPORTED, dict(n_pairs=1, fo_=[0, 8193])), (LCD_ERR_UNSUPPORTED, dict(n_pairs=1, to_=[0, 8193]))]
    table += [(LCD_ERR_INVALID, dict(null=(name,))) for name in ("from_word_ids", "from_points", "to_word_ids", "to_points", "out_status", "out_n_pairs",
                                                                  "out_n_inliers")]
    for code, kw in table:
        rc, clean = call(**kw)
        assert rc == code and clean, (kw, rc, clean)
        assert eng.L.lcd_last_error(eng.h)
    import torch                                                          # the same through lcd_verify_epipolar_dev: the code, and the device outputs keep their canaries
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    d_in = [t(fi), t(fp), t(ti), t(tp)]
    for code, kw in ((LCD_ERR_INVALID, dict(iterations=0)), (LCD_ERR_UNSUPPORTED, dict(iterations=65536)), (LCD_ERR_INVALID, dict(ransac_threshold=0.0)),
                     (LCD_ERR_INVALID, dict(match_count_min=0)), (LCD_ERR_INVALID, dict(to_=[0, nt, 4])), (LCD_ERR_UNSUPPORTED, dict(to_=[0, nt, nt + 8193])),
                     (LCD_ERR_INVALID, dict(null_status=True))):
        d_out = [torch.full((2, 9), float("nan"), device="cuda")] + [torch.full((n,), -1, dtype=torch.int32, device="cuda") for n in (2, 2, 2, nt, nt)]
        k = dict(KW, **{a: b for a, b in kw.items() if a in KW})
        outs = list(d_out)
        if kw.get("null_status"):
            outs[1] = None
        from rtabmap_amd.capi import LcdError
        with pytest.raises(LcdError) as e:
            eng.verify_epipolar_dev(d_in[0], d_in[1], fo, d_in[2], d_in[3], kw.get("to_", to), *outs, **k)
        eng.synchronize()
        assert e.value.status == code, (kw, e.value)
        assert torch.isnan(d_out[0]).all() and all(bool((o == -1).all()) for o in d_out[1:]), kw
    eng.set_option("shard_append", 1)                                     # a handle of a sharded vocabulary
    rc, clean = call()
    eng.set_option("shard_append", 0)
    assert rc == LCD_ERR_UNSUPPORTED and clean
    rc, clean = call(n_pairs=0)                                           # n_pairs == 0: LCD_OK, nothing written
    assert rc == 0 and clean
    rc, clean = call()
    assert rc == 0 and not clean
    check_both(eng, pairs, "after the refusals")                          # the handle stays usable
