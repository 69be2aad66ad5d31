"""Inputs for the tests of lcd_keypoints_3d_stereo: textures with a known disparity, the single-property cases whose properties
tests/test_stereo_flow_inputs.py proves by the model, and the helpers that run both entries and compare them with the model bit for bit."""
import numpy as np

import stereo_flow_model as M

F = np.float32
CANARY = -7
TILT = [0.0, 0.0, 1.0, 0.05, -1.0, 0.0, 0.0, -0.1, 0.0, -1.0, 0.0, 0.3]      # the usual optical-to-base rotation, with a lever arm
FRAME_SIZES = [0, 1, 63, 64, 65, 1100]
# width, height, win_width, win_height
SHAPES = [(17, 5, 3, 3), (40, 24, 5, 3), (64, 48, 15, 3), (160, 120, 15, 3)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def texture(rng, width, height, margin=40, passes=2):
    """a smooth random texture [height x (width + 2 margin)] in float64, 0..255"""
    a = rng.standard_normal((height + 8, width + 2 * margin + 8))
    k = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
    for _ in range(passes):
        a = sum(k[i] * np.roll(a, i - 2, 0) for i in range(5))
        a = sum(k[i] * np.roll(a, i - 2, 1) for i in range(5))
    a = a[4:-4, 4:-4]
    return (a - a.min()) / (a.max() - a.min()) * 255.0


def shifted_pair(tex, width, disparity, margin=40, pad=0):
    """left = the texture's middle, right = the same scene seen `disparity` pixels to the left (right(x) = left(x + d)), resampled linearly.
    pad: extra columns of other bytes behind every row (a pitch above the row)"""
    x = np.arange(width) + margin
    left = tex[:, x]
    xs = x + disparity
    i = np.floor(xs).astype(int)
    t = xs - i
    right = tex[:, i] * (1 - t) + tex[:, i + 1] * t
    out = []
    for a in (left, right):
        u = np.full((a.shape[0], width + pad), 201, np.uint8)
        u[:, :width] = np.clip(np.rint(a), 0, 255).astype(np.uint8)
        out.append(u)
    return out


def camera_for(width, height, right_cx=None, transform=None):
    cx = (width - 1) / 2 + 0.25
    return M.camera(fx=float(width), fy=float(width) * 1.01, cx=cx, cy=(height - 1) / 2 - 0.125, baseline=0.12,
                    right_cx=cx + 1.5 if right_cx is None else right_cx, transform=transform)


def random_points(rng, n, width, height, win_w=15, win_h=3):
    """inside, around the border (some beyond the bounds test), a quarter on integers"""
    p = np.stack([rng.uniform(-win_w / 2 - 2, width + win_w / 2 + 2, n), rng.uniform(-win_h / 2 - 2, height + win_h / 2 + 2, n)], 1)
    inside = rng.random(n) < 0.7
    p[inside] = np.stack([rng.uniform(0, width - 1, n), rng.uniform(0, height - 1, n)], 1)[inside]
    whole = rng.random(n) < 0.25
    p[whole] = np.rint(p[whole])
    return p.astype(np.float32)


def wild_points():
    return np.array([[np.nan, 1], [1, np.nan], [np.inf, 2], [3, -np.inf], [1e20, 1], [2, -3e9], [2147483648.0, 0], [0, -2147483648.0]], np.float32)


def random_frame(rng, width, height, n, win_w=15, win_h=3, disparity=None, pad=0, right_cx=None, transform=None):
    d = float(rng.uniform(1.0, 6.0)) if disparity is None else disparity
    left, right = shifted_pair(texture(rng, width, height), width, d, pad=pad)
    return M.pair(left, right, camera_for(width, height, right_cx, transform), width), random_points(rng, n, width, height, win_w, win_h)


# ---- single-property cases: each returns dict(pair, points, P) and what test_stereo_flow_inputs.py proves about it
def level_count_cases(rng):
    """(pair, P, the number of levels): odd level sizes, and the stop rule met exactly -- the next level's height EQUAL to the window's"""
    out = []
    for w, h, want in ((17, 5, 1), (17, 9, 2), (19, 11, 2), (33, 25, 4), (35, 13, 3)):
        pr, _ = random_frame(rng, w, h, 0, 3, 3)
        out.append((pr, M.params(win_width=3, win_height=3, max_level=5), want))
    pr, _ = random_frame(rng, 64, 48, 0)
    out.append((pr, M.params(max_level=1), 2))                           # max_level stops it
    out.append((pr, M.params(max_level=0), 1))
    return out


def border_origin_case(rng, width=40, height=24, win_w=5, win_h=3):
    """level-0 window origins at -win and at cols - 1 / rows - 1 (inside the bounds test), and one step beyond each (status 0)"""
    pr, _ = random_frame(rng, width, height, 0, win_w, win_h, disparity=1.0)
    hx, hy = (win_w - 1) / 2, (win_h - 1) / 2
    xs = [-win_w + hx, -win_w + hx - 0.5, width - 1 + hx, width + hx, width - 1 + hx + 0.75]
    ys = [-win_h + hy, -win_h + hy - 0.5, height - 1 + hy, height + hy, height - 1 + hy + 0.75]
    pts = [(x, height / 2 + 0.25) for x in xs] + [(width / 2 + 0.5, y) for y in ys] + [(xs[0], ys[0]), (xs[2], ys[2]), (xs[0], ys[2])]
    return dict(pair=pr, points=np.array(pts, np.float32), P=M.params(win_width=win_w, win_height=win_h, max_level=0, min_disparity=0.0, min_eig_threshold=0.0))


def integer_case(rng):
    pr, _ = random_frame(rng, 64, 48, 0, disparity=3.0)
    pts = np.array([(x, y) for x in (10, 31, 50) for y in (5, 24, 40)], np.float32)
    return dict(pair=pr, points=pts, P=M.params(max_level=0))


def tie_case(rng):
    """a = 2^-15 at level 0: a * 16384 = 0.5 and (1 - a) * 16384 = 16383.5, both ties"""
    pr, _ = random_frame(rng, 40, 24, 0, 5, 3, disparity=2.0)
    pts = np.array([(x + 2.0 ** -15, y) for x in (6, 9, 14, 20, 27, 33) for y in (4, 11, 12, 19)], np.float32)
    return dict(pair=pr, points=pts, P=M.params(win_width=5, win_height=3, max_level=0))


def flat_case(rng):
    """a flat image: every sum is 0, so with min_eig_threshold = 0 the test D < FLT_EPSILON decides; with the default threshold minEig does"""
    flat = np.full((24, 40), 77, np.uint8)
    pr = M.pair(flat, flat.copy(), camera_for(40, 24), 40)
    pts = np.array([(10.5, 8.25), (20, 12)], np.float32)
    return dict(pair=pr, points=pts, P=M.params(win_width=5, win_height=3, max_level=1, min_eig_threshold=0.0))


def eigen_threshold_cases(rng):
    """the same frame with min_eig_threshold EQUAL to one keypoint's level-0 minEig (it passes) and one double above (it fails)"""
    pr, _ = random_frame(rng, 64, 48, 0, disparity=2.0)
    pt = np.array([[30.25, 20.5]], np.float32)
    P = M.params(max_level=0)
    trace = {}
    M.track(M.cached_levels(P, pr), P, pt[0], trace=trace)
    min_eig = [e for e in trace[0] if isinstance(e, tuple) and e[0] == "min_eig"][0][1]
    return [dict(pair=pr, points=pt, P=M.params(max_level=0, min_eig_threshold=float(min_eig))),
            dict(pair=pr, points=pt, P=M.params(max_level=0, min_eig_threshold=float(np.nextafter(min_eig, np.inf))))]


def exit_cases(rng):
    """the iteration cap (two iterations, eps 0), the eps exit (the defaults) and the oscillation exit (eps 0, 100 iterations)"""
    pr, pts = random_frame(rng, 64, 48, 40, disparity=2.3)
    pts = pts[:40]
    return dict(cap=dict(pair=pr, points=pts, P=M.params(iterations=2, eps=0.0)), eps=dict(pair=pr, points=pts, P=M.params()),
                oscillation=dict(pair=pr, points=pts, P=M.params(iterations=100, eps=0.0)))


def leaving_case(rng):
    """a right image that has nothing of the left one but a steep ramp: corrections are large, keypoints near the border leave the image --
    at level 0 (status 0), and at a higher level after which the next level goes on from the scaled position"""
    w, h = 96, 64
    left, _ = shifted_pair(texture(rng, w, h), w, 0.0)
    ramp = np.clip(np.arange(w)[None, :] * 2.5 + rng.integers(0, 3, (h, w)), 0, 255).astype(np.uint8)
    pr = M.pair(left, ramp, camera_for(w, h), w)
    pts = np.stack([rng.uniform(0, w - 1, 150), rng.uniform(0, h - 1, 150)], 1).astype(np.float32)
    return dict(pair=pr, points=pts, P=M.params(win_width=5, win_height=3, max_level=3, min_eig_threshold=0.0))


def disparity_gate_cases(rng):
    """one keypoint whose disparity d the model measures; then min_disparity = d (rejected), max_disparity = d (accepted); identical images
    (d = 0 against min_disparity = 0) and a scene shifted the other way (d < 0); with the L1 error and error_threshold = 0 the status
    stays set and d = 0 and d < 0 reach the projection"""
    pr, _ = random_frame(rng, 64, 48, 0, disparity=3.0)
    pt = np.array([[30.0, 20.0], [41.5, 30.25]], np.float32)
    fr = M.frame(pr, pt, M.params(min_disparity=0.0))
    assert fr["status"].all()
    d = (pt[:, 0] - fr["right"][:, 0]).astype(np.float32)
    same = M.pair(pr["left"], pr["left"].copy(), pr["camera"], 64)
    back, _ = random_frame(rng, 64, 48, 0, disparity=-2.0)
    out = [dict(pair=pr, points=pt, P=M.params(min_disparity=float(d[0]), max_disparity=128.0), d=d),
           dict(pair=pr, points=pt, P=M.params(min_disparity=0.0, max_disparity=float(d[0])), d=d),
           dict(pair=pr, points=pt, P=M.params(min_disparity=0.0, max_disparity=float(np.nextafter(d[0], F(-np.inf)))), d=d)]
    for other in (same, back):
        out.append(dict(pair=other, points=pt, P=M.params(min_disparity=0.0)))
        out.append(dict(pair=other, points=pt, P=M.params(min_disparity=0.0, use_min_eigenvals=0, error_threshold=0.0)))
    return out


def depth_bound_cases(rng):
    """Z on both depth bounds: min_depth = Z (the point falls: Z > min_depth is strict) and max_depth = Z (it stands); without right_cx and
    with a local transform"""
    out = []
    for kw in (dict(), dict(right_cx=0.0), dict(transform=TILT)):
        pr, _ = random_frame(rng, 64, 48, 0, disparity=3.0, **kw)
        pt = np.array([[30.0, 20.0], [12.5, 33.25], [50.0, 8.0]], np.float32)
        plain = dict(pr, camera=dict(pr["camera"], transform=None))
        z = float(M.frame(plain, pt)["xyz"][0, 2])
        assert np.isfinite(z)
        for lo, hi in ((0.0, 0.0), (z, 0.0), (0.0, z), (float(np.nextafter(F(z), F(0))), z)):
            out.append(dict(pair=pr, points=pt, P=M.params(), filter=M.FILTER_3D, min_depth=lo, max_depth=hi, z=z))
    return out


def error_mode_case(rng):
    pr, pts = random_frame(rng, 64, 48, 60, disparity=2.0)
    return [dict(pair=pr, points=pts, P=M.params(use_min_eigenvals=0, error_threshold=t)) for t in (50.0, 1.0, 0.25)]


def pitch_case(rng):
    pr, pts = random_frame(rng, 40, 24, 50, 5, 3, pad=7)
    return dict(pair=pr, points=pts, P=M.params(win_width=5, win_height=3))


def all_cases(rng):
    cases = [border_origin_case(rng), integer_case(rng), tie_case(rng), flat_case(rng), leaving_case(rng), pitch_case(rng)]
    cases += eigen_threshold_cases(rng) + list(exit_cases(rng).values()) + disparity_gate_cases(rng) + depth_bound_cases(rng) + error_mode_case(rng)
    cases += [dict(pair=pr, points=random_points(rng, 12, pr["width"], pr["left"].shape[0], 3, 3), P=P) for pr, P, _ in level_count_cases(rng)[:5]]
    return cases


# ---- running the entries
def concat(frames_points):
    off = np.cumsum([0] + [len(p) for p in frames_points]).astype(np.int64)
    pts = np.concatenate([np.asarray(p, np.float32).reshape(-1, 2) for p in frames_points]) if frames_points else np.zeros((0, 2), np.float32)
    return np.ascontiguousarray(pts), off


def api_images(pairs, data_of=lambda a: a):
    """the model's pairs as rtabmap_amd.Engine.keypoints_3d_stereo takes them"""
    return [dict(left=data_of(p["left"]), right=data_of(p["right"]), camera=p["camera"], width=p["width"]) for p in pairs]


def assert_same(got, pairs, frames_points, P=None, filter=M.KEEP_ALL, min_depth=0.0, max_depth=0.0, device=False, response=None, rows=None, aux=None,
                what="", want=None, tracks=True):
    """counts, the whole index list, the right corners and the status of every input keypoint and, for every frame, the first count entries
    of every compacted output: bit for bit.  want: the model's batch() where the caller has it already"""
    if want is None:
        want = M.batch(pairs, frames_points, P, filter, min_depth, max_depth, device)
    pts, off = concat(frames_points)
    np.testing.assert_array_equal(got["count"], want["count"], err_msg=what + " count")
    np.testing.assert_array_equal(got["index"], want["index"], err_msg=what + " index")
    for f in range(len(pairs)):
        a, kept, n = int(off[f]), want["kept"][f], len(frames_points[f])
        c = len(kept)
        tag = "%s frame %d" % (what, f)
        if tracks:
            np.testing.assert_array_equal(got["status"][a:a + n], want["status"][f], err_msg=tag + " status")
            np.testing.assert_array_equal(bits(got["right"][a:a + n]), bits(want["right"][f]), err_msg=tag + " right")
        np.testing.assert_array_equal(bits(got["xyz"][a:a + c]), bits(want["xyz"][f][kept]), err_msg=tag + " xyz")
        if filter == M.KEEP_ALL:
            continue
        np.testing.assert_array_equal(bits(got["points"][a:a + c]), bits(pts[a:a + n][kept]), err_msg=tag + " points")
        for src, name in ((response, "response"), (rows, "rows"), (aux, "aux")):
            if src is not None:
                x = np.ascontiguousarray(src[a:a + n][kept])
                np.testing.assert_array_equal(np.ascontiguousarray(got[name][a:a + c]).view(np.uint8), x.view(np.uint8), err_msg=tag + " " + name)


def stage_dev(pairs, frames_points, response=None, rows=None, aux=None, tracks=True):
    """the batch on the device, outputs canary-filled, uploaded and synchronised; an image shared by frames (the same array) is uploaded once"""
    import torch
    pts, off = concat(frames_points)
    n, nf = pts.shape[0], len(pairs)
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    cache = {}
    def data_of(a):
        if id(a) not in cache:
            cache[id(a)] = (a, torch.from_numpy(np.ascontiguousarray(a)).cuda())
        return cache[id(a)][1]
    canary = lambda shape, dt: torch.full(shape, CANARY, dtype=dt, device="cuda")
    st = dict(off=off, images=api_images(pairs, data_of), pts=dev(pts), resp=dev(response), d_rows=dev(rows), d_aux=dev(aux),
              aux_bytes=0 if aux is None else aux.shape[1], count=canary((nf,), torch.int32), index=canary((n,), torch.int32),
              xyz=canary((n, 3), torch.float32), points=canary((n, 2), torch.float32),
              response=None if response is None else canary((n,), torch.float32), rows=None if rows is None else torch.zeros_like(dev(rows)),
              aux=None if aux is None else torch.zeros_like(dev(aux)), right=canary((n, 2), torch.float32) if tracks else None,
              status=torch.full((n,), 249, dtype=torch.uint8, device="cuda") if tracks else None)
    torch.cuda.synchronize()
    return st


def launch_dev(eng, st, P=None, filter=M.KEEP_ALL, min_depth=0.0, max_depth=0.0):
    eng.keypoints_3d_stereo_dev(st["pts"], st["off"], st["images"], st["count"], st["index"], st["xyz"], params=P, filter=filter, min_depth=min_depth,
                                max_depth=max_depth, d_response=st["resp"], d_rows=st["d_rows"], d_aux=st["d_aux"], aux_bytes=st["aux_bytes"],
                                d_out_points=st["points"], d_out_response=st["response"], d_out_rows=st["rows"], d_out_aux=st["aux"],
                                d_out_right=st["right"], d_out_status=st["status"])
    return st


def to_host(eng, st):
    eng.synchronize()
    return {k: (None if st[k] is None else st[k].cpu().numpy()) for k in ("count", "index", "xyz", "points", "response", "rows", "aux", "right", "status")}


def run_dev(eng, pairs, frames_points, P=None, filter=M.KEEP_ALL, min_depth=0.0, max_depth=0.0, response=None, rows=None, aux=None, tracks=True):
    return to_host(eng, launch_dev(eng, stage_dev(pairs, frames_points, response, rows, aux, tracks), P, filter, min_depth, max_depth))


def run_host(eng, pairs, frames_points, P=None, filter=M.KEEP_ALL, min_depth=0.0, max_depth=0.0, response=None, rows=None, aux=None, tracks=True):
    pts, off = concat(frames_points)
    return eng.keypoints_3d_stereo(pts, off, api_images(pairs), params=P, filter=filter, min_depth=min_depth, max_depth=max_depth, response=response,
                                   rows=rows, aux=aux, right=tracks, status=tracks)
