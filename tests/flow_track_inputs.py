"""Inputs for the tests of lcd_track_flow: textures resampled at a known 2-D shift, the single-property cases whose properties
tests/test_flow_track_model.py proves by the model, and the helpers that run both entries and compare them with the model bit for bit."""
import numpy as np

import flow_track_model as M
import stereo_flow_inputs as SI

F = np.float32
CANARY = -7
bits = SI.bits
texture = SI.texture
random_points = SI.random_points
wild_points = SI.wild_points
PAIR_SIZES = [0, 1, 3, 4, 5, 63, 64, 65, 1100]
# width, height, win_width, win_height: 9, 64, 65, 256 (four full passes), 961 and 45 window pixels
SHAPES = [(17, 5, 3, 3), (40, 24, 8, 8), (40, 24, 5, 13), (64, 48, 16, 16), (64, 48, 31, 31), (64, 48, 15, 3), (160, 120, 16, 16)]


def shifted_images(tex, width, height, shift, margin=40, pad=0):
    """from = the texture's middle, to = the same scene moved by `shift` = (sx, sy): to(x + sx, y + sy) = from(x, y), resampled bilinearly.
    pad: extra columns of other bytes behind every row (a pitch above the row).  The texture has 8 spare rows: |sy| stays below 7"""
    sx, sy = shift
    x = np.arange(width) + margin
    y = np.arange(height) + 8
    big = np.pad(tex, ((8, 8), (0, 0)), mode="reflect")
    a = big[np.ix_(y, x)]
    xs, ys = x - sx, y - sy
    ix, iy = np.floor(xs).astype(int), np.floor(ys).astype(int)
    tx, ty = (xs - ix)[None, :], (ys - iy)[:, None]
    b = (big[np.ix_(iy, ix)] * (1 - tx) + big[np.ix_(iy, ix + 1)] * tx) * (1 - ty) + (big[np.ix_(iy + 1, ix)] * (1 - tx) + big[np.ix_(iy + 1, ix + 1)] * tx) * ty
    out = []
    for v in (a, b):
        u = np.full((height, width + pad), 201, np.uint8)
        u[:, :width] = np.clip(np.rint(v), 0, 255).astype(np.uint8)
        out.append(u)
    return out


def random_pair(rng, width, height, n, win_w=16, win_h=16, shift=None, pad=0, max_level=3, use_initial=0):
    """-> (pair, points, initial): the initial positions are the truth disturbed by up to a pixel"""
    s = (float(rng.uniform(-3.0, 3.0)), float(rng.uniform(-2.0, 2.0))) if shift is None else shift
    a, b = shifted_images(texture(rng, width, height), width, height, s, pad=pad)
    pts = random_points(rng, n, width, height, win_w, win_h)
    ini = (pts + np.array(s, np.float32) + rng.uniform(-1.0, 1.0, pts.shape).astype(np.float32)).astype(np.float32)
    return M.pair(a, b, width, max_level, use_initial), pts, ini


def with_(pr, **kw):
    """the same images under another max_level / use_initial"""
    return dict(pr, **kw)


# ---- single-property cases: each is dict(pair, points, initial, P); tests/test_flow_track_model.py proves what each one reaches
def case(pr, pts, P, initial=None):
    return dict(pair=pr, points=np.asarray(pts, np.float32).reshape(-1, 2), initial=initial, P=P)


def exit_cases(rng):
    """the iteration cap (two iterations, eps 0), the eps exit (the defaults) and the oscillation exit (eps 0, 100 iterations)"""
    pr, pts, _ = random_pair(rng, 64, 48, 40, 8, 8, shift=(2.3, -1.4))
    return dict(cap=case(pr, pts, M.params(win_width=8, win_height=8, iterations=2, eps=0.0)), eps=case(pr, pts, M.params(win_width=8, win_height=8)),
                oscillation=case(pr, pts, M.params(win_width=8, win_height=8, iterations=100, eps=0.0)))


def leaving_case(rng):
    """a to image that has nothing of the from image but a steep ramp: the corrections are large and corners near the border leave the
    image -- at level 0 (status 0) and at a higher level, after which the next level goes on from the scaled position"""
    w, h = 96, 64
    a, _ = shifted_images(texture(rng, w, h), w, h, (0.0, 0.0))
    ramp = np.clip(np.arange(w)[None, :] * 2.5 + np.arange(h)[:, None] * 1.5 + rng.integers(0, 3, (h, w)), 0, 255).astype(np.uint8)
    pts = np.stack([rng.uniform(0, w - 1, 150), rng.uniform(0, h - 1, 150)], 1).astype(np.float32)
    return case(M.pair(a, ramp, w, 3), pts, M.params(win_width=5, win_height=3, min_eig_threshold=0.0))


def eigen_gate_cases(rng):
    """min_eig_threshold EQUAL to one corner's level-0 minEig (it passes) and one double above (it fails: status 0); and a threshold between
    a corner's level-1 minEig and its larger level-0 minEig: the gate closes above level 0 only, the status stays set"""
    pr, pts, _ = random_pair(rng, 64, 48, 60, 5, 5, shift=(1.5, 0.5), max_level=1)
    pts = np.stack([rng.uniform(8, 55, 60), rng.uniform(8, 39, 60)], 1).astype(np.float32)
    P = M.params(win_width=5, win_height=5, min_eig_threshold=0.0)
    levels = M.cached_levels(P, pr)
    out, above = [], None
    for k, pt in enumerate(pts):
        trace = {}
        M.track(levels, P, pt, trace=trace)
        eig = {l: [e for e in trace[l] if isinstance(e, tuple) and e[0] == "min_eig"][0][1] for l in (0, 1)}
        if k == 0:
            out.append(case(pr, pt, M.params(win_width=5, win_height=5, min_eig_threshold=float(eig[0]))))
            out.append(case(pr, pt, M.params(win_width=5, win_height=5, min_eig_threshold=float(np.nextafter(eig[0], np.inf)))))
        if above is None and eig[1] < eig[0] and eig[1] > 0:
            above = case(pr, pt, M.params(win_width=5, win_height=5, min_eig_threshold=float(np.nextafter(eig[1], np.inf))))
    return out + [above]


def flat_case(rng):
    """a flat image: every sum is 0, so with min_eig_threshold = 0 the test D < FLT_EPSILON decides; with the default threshold minEig does"""
    flat = np.full((24, 40), 77, np.uint8)
    return [case(M.pair(flat, flat.copy(), 40, 1), [(10.5, 8.25), (20, 12)], M.params(win_width=5, win_height=3, min_eig_threshold=t)) for t in (0.0, 1e-4)]


def tie_case(rng):
    """a = 2^-15 at level 0: a * 16384 = 0.5 and (1 - a) * 16384 = 16383.5, both ties (half to even)"""
    pr, _, _ = random_pair(rng, 40, 24, 0, 5, 3, shift=(2.0, 1.0), max_level=0)
    pts = [(x + 2.0 ** -15, y + 2.0 ** -15) for x in (6, 9, 14, 20, 27, 33) for y in (4, 11, 12, 19)]
    return case(pr, pts, M.params(win_width=5, win_height=3))


def border_origin_case(rng, width=40, height=24, win_w=5, win_h=3):
    """level-0 window origins at -win and at cols - 1 / rows - 1 (inside the bounds test), and one step beyond each (status 0)"""
    pr, _, _ = random_pair(rng, width, height, 0, win_w, win_h, shift=(1.0, 0.5), max_level=0)
    hx, hy = (win_w - 1) / 2, (win_h - 1) / 2
    xs = [-win_w + hx, -win_w + hx - 0.5, width - 1 + hx, width + hx, width - 1 + hx + 0.75]
    ys = [-win_h + hy, -win_h + hy - 0.5, height - 1 + hy, height + hy, height - 1 + hy + 0.75]
    pts = [(x, height / 2 + 0.25) for x in xs] + [(width / 2 + 0.5, y) for y in ys] + [(xs[0], ys[0]), (xs[2], ys[2]), (xs[0], ys[2])]
    return case(pr, pts, M.params(win_width=win_w, win_height=win_h, min_eig_threshold=0.0))


def keep_bound_case(rng, width=40, height=24):
    """iterations = 0 leaves a tracked corner exactly where it starts, so the start positions put it ON the keep bounds: x == cols and
    y == rows (not kept), one float below (kept), 0 and -0.0 (kept), one float below 0 (not kept)"""
    pr, _, _ = random_pair(rng, width, height, 0, 5, 5, shift=(0.0, 0.0), max_level=0, use_initial=1)
    lo = float(np.nextafter(F(0), F(-1)))
    xs = [float(width), float(np.nextafter(F(width), F(0))), 0.0, -0.0, lo]
    ys = [float(height), float(np.nextafter(F(height), F(0))), 0.0, -0.0, lo]
    ini = [(x, 12.5) for x in xs] + [(20.25, y) for y in ys] + [(20.0, 12.0)]
    pts = [(20.0, 12.0)] * len(ini)
    return case(pr, pts, M.params(win_width=5, win_height=5, iterations=0, min_eig_threshold=0.0), np.array(ini, np.float32))


def error_mode_cases(rng):
    """use_min_eigenvals = 0: thresholds that keep everything and nothing, and error_threshold EQUAL to one corner's L1 error (not kept:
    the comparison is strict) and one float above it (kept)"""
    pr, pts, _ = random_pair(rng, 64, 48, 60, 8, 8, shift=(2.0, -1.0))
    P = M.params(win_width=8, win_height=8, use_min_eigenvals=0)
    fr = M.run_pair(pr, pts, P, device=True)
    k = int(np.flatnonzero((fr["status"] == 1) & (fr["err"] > 0))[0])
    e = fr["err"][k]
    one = pts[k:k + 1]
    return [case(pr, pts, dict(P, error_threshold=t)) for t in (20.0, 0.0)] + \
           [case(pr, one, dict(P, error_threshold=float(e))), case(pr, one, dict(P, error_threshold=float(np.nextafter(e, F(np.inf)))))]


def initial_cases(rng):
    """use_initial with max_level 0 and 2, and start positions outside the image (status 0 at level 0, or pulled back by the upper levels)"""
    out = []
    for ml in (0, 2):
        pr, pts, ini = random_pair(rng, 64, 48, 50, 8, 8, max_level=ml, use_initial=1)
        ini[::7] = ini[::7] + np.array([90.0, -70.0], np.float32)
        ini[3::11] = np.array([-40.0, 200.0], np.float32)
        out.append(case(pr, pts, M.params(win_width=8, win_height=8), ini))
    return out


def stop_precision_case(rng):
    """an eps whose square lies between delta.x^2 + delta.y^2 evaluated in float64 and in float32 for one iteration of one corner: the
    two evaluations of the stop test disagree there (found by the model; one float64 product and sum against the float32 ones)"""
    pr, _, _ = random_pair(rng, 64, 48, 0, 8, 8, shift=(1.3, -0.8), max_level=0)
    pts = np.stack([rng.uniform(10, 53, 80), rng.uniform(10, 37, 80)], 1).astype(np.float32)
    P = M.params(win_width=8, win_height=8, eps=0.0, iterations=6)
    levels = M.cached_levels(P, pr)
    for pt in pts:
        trace = {}
        M.track(levels, P, pt, trace=trace)
        for e in trace[0]:
            if not (isinstance(e, tuple) and e[0] == "delta"):
                continue
            dx, dy = e[1], e[2]
            s64 = np.float64(dx) * np.float64(dx) + np.float64(dy) * np.float64(dy)
            s32 = np.float64(dx * dx + dy * dy)
            if s64 == s32 or s64 > 1e-3:
                continue
            for t in (0.5, 0.25, 0.75, 0.1, 0.9):
                eps = float(np.sqrt(s64 + (s32 - s64) * t))
                if (s64 <= eps * eps) != (np.float32(s32) <= np.float32(eps * eps)):
                    return case(pr, pt, M.params(win_width=8, win_height=8, eps=eps, iterations=30))
    raise AssertionError("no corner found")


def pitch_case(rng):
    pr, pts, _ = random_pair(rng, 40, 24, 50, 5, 3, pad=7)
    return case(pr, pts, M.params(win_width=5, win_height=3))


def level_cut_case(rng):
    """max_level 5 on 40 x 24 with an 8 x 8 window: the window cuts the pyramid short at two levels"""
    pr, pts, _ = random_pair(rng, 40, 24, 40, 8, 8, max_level=5)
    return case(pr, pts, M.params(win_width=8, win_height=8))


def all_cases(rng):
    cases = list(exit_cases(rng).values()) + [leaving_case(rng)] + eigen_gate_cases(rng) + flat_case(rng) + [tie_case(rng), border_origin_case(rng)]
    return cases + [keep_bound_case(rng)] + error_mode_cases(rng) + initial_cases(rng) + [pitch_case(rng), level_cut_case(rng), stop_precision_case(rng)]


# ---- running the entries
concat = SI.concat


def api_pairs(pairs, data_of=lambda a: a):
    """the model's pairs as rtabmap_amd.Engine.track_flow takes them"""
    return [{"from": data_of(p["from"]), "to": data_of(p["to"]), "width": p["width"], "max_level": p["max_level"], "use_initial": p["use_initial"]} for p in pairs]


def concat_initial(pair_points, initials):
    """[N x 2] with zeros where a pair has no initial positions; None when no pair has any"""
    if initials is None or all(i is None for i in initials):
        return None
    return np.ascontiguousarray(np.concatenate([np.zeros((len(p), 2), np.float32) if i is None else np.asarray(i, np.float32).reshape(-1, 2)
                                                for p, i in zip(pair_points, initials)] + [np.zeros((0, 2), np.float32)]))


def assert_same(got, pairs, pair_points, P=None, initials=None, device=False, aux=None, what="", want=None, canary=None):
    """counts, the whole index list, the track, the status and the error of every input corner (where the output was asked for) and, for
    every pair, the first count entries of every compacted output: bit for bit.  canary: what the compacted outputs held before the call
    -- the entries behind a pair's count still hold it.  want: the model's batch() where the caller has it already"""
    if want is None:
        want = M.batch(pairs, pair_points, P, initials, device)
    pts, off = concat(pair_points)
    np.testing.assert_array_equal(got["count"], want["count"], err_msg=what + " count")
    np.testing.assert_array_equal(got["index"], want["index"], err_msg=what + " index")
    for f in range(len(pairs)):
        a, kept, n = int(off[f]), want["kept"][f], len(pair_points[f])
        c = len(kept)
        tag = "%s pair %d" % (what, f)
        if got.get("status") is not None:
            np.testing.assert_array_equal(got["status"][a:a + n], want["status"][f], err_msg=tag + " status")
        if got.get("track") is not None:
            np.testing.assert_array_equal(bits(got["track"][a:a + n]), bits(want["track"][f]), err_msg=tag + " track")
        if got.get("err") is not None:
            np.testing.assert_array_equal(bits(got["err"][a:a + n]), bits(want["err"][f]), err_msg=tag + " err")
        np.testing.assert_array_equal(bits(got["from"][a:a + c]), bits(pts[a:a + n][kept]), err_msg=tag + " from")
        np.testing.assert_array_equal(bits(got["to"][a:a + c]), bits(want["track"][f][kept]), err_msg=tag + " to")
        if aux is not None:
            np.testing.assert_array_equal(got["aux"][a:a + c], aux[a:a + n][kept], err_msg=tag + " aux")
        if canary is not None:
            assert (got["from"][a + c:a + n] == canary).all() and (got["to"][a + c:a + n] == canary).all(), tag + " written behind the count"
            assert aux is None or (got["aux"][a + c:a + n] == 0xA5).all(), tag + " aux written behind the count"


def stage_dev(pairs, pair_points, initials=None, aux=None, optional=("track", "status", "err")):
    """the batch on the device, outputs canary-filled, uploaded and synchronised; an image shared by pairs (the same array) is uploaded once"""
    import torch
    pts, off = concat(pair_points)
    ini = concat_initial(pair_points, initials)
    n, npairs = pts.shape[0], len(pairs)
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    cache = {}
    def data_of(a):
        if id(a) not in cache:
            cache[id(a)] = (a, torch.from_numpy(np.ascontiguousarray(a)).cuda())
        return cache[id(a)][1]
    canary = lambda shape, dt: torch.full(shape, CANARY, dtype=dt, device="cuda")
    st = {"off": off, "pairs": api_pairs(pairs, data_of), "pts": dev(pts), "ini": dev(ini), "d_aux": dev(aux), "aux_bytes": 0 if aux is None else aux.shape[1],
          "count": canary((npairs,), torch.int32), "index": canary((n,), torch.int32), "from": canary((n, 2), torch.float32), "to": canary((n, 2), torch.float32),
          "aux": None if aux is None else torch.full(aux.shape, 0xA5, dtype=torch.uint8, device="cuda"),
          "track": canary((n, 2), torch.float32) if "track" in optional else None,
          "status": torch.full((n,), 249, dtype=torch.uint8, device="cuda") if "status" in optional else None,
          "err": canary((n,), torch.float32) if "err" in optional else None}
    torch.cuda.synchronize()
    return st


def launch_dev(eng, st, P=None):
    eng.track_flow_dev(st["pts"], st["off"], st["pairs"], st["count"], st["index"], st["from"], st["to"], params=P, d_initial=st["ini"], d_aux=st["d_aux"],
                       aux_bytes=st["aux_bytes"], d_out_aux=st["aux"], d_out_track=st["track"], d_out_status=st["status"], d_out_err=st["err"])
    return st


def to_host(eng, st):
    eng.synchronize()
    return {k: (None if st[k] is None else st[k].cpu().numpy()) for k in ("count", "index", "from", "to", "aux", "track", "status", "err")}


def run_dev(eng, pairs, pair_points, P=None, initials=None, aux=None, optional=("track", "status", "err")):
    return to_host(eng, launch_dev(eng, stage_dev(pairs, pair_points, initials, aux, optional), P))


def run_host(eng, pairs, pair_points, P=None, initials=None, aux=None, optional=("track", "status", "err")):
    pts, off = concat(pair_points)
    return eng.track_flow(pts, off, api_pairs(pairs), params=P, initial=concat_initial(pair_points, initials), aux=aux,
                          track="track" in optional, status="status" in optional, err="err" in optional)
