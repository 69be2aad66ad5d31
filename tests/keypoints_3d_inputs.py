"""Inputs of the depth-stage tests: generators whose properties tests/test_keypoints_3d_inputs.py proves on the model, without a GPU, and
the helpers that run a batch through the engine's entries and compare it with the model exactly (NaN positions and all other bits)."""
import numpy as np

import keypoints_3d_model as M

F = np.float32
CANARY = -7
SHAPES = [(5, 4), (16, 12), (64, 48)]                     # width, height
FRAME_SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1100]
IDENTITY = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
TILT = [0.0, 0.0, 1.0, 0.05, -1.0, 0.0, 0.0, -0.1, 0.0, -1.0, 0.0, 0.3]      # the usual optical-to-base rotation, with a lever arm


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def up(v, k=1):
    """k float32 steps above v"""
    v = F(v)
    for _ in range(k):
        v = np.nextafter(v, F(np.inf))
    return v


def down(v, k=1):
    v = F(v)
    for _ in range(k):
        v = np.nextafter(v, F(-np.inf))
    return v


def cameras_for(sub_cols, rows, n, image_width=0, image_height=0, transform=None, zero_principal=False):
    """n pinhole models for sub-images of sub_cols x rows, slightly different from each other"""
    sx = image_width / sub_cols if image_width else 1.0
    sy = image_height / rows if image_height else 1.0
    out = []
    for c in range(n):
        cx, cy = (0.0, -1.0) if zero_principal else ((sub_cols / 2 - 0.37 + 0.11 * c) * sx, (rows / 2 - 0.41) * sy)
        out.append(M.camera((0.91 * sub_cols + c) * sx, (0.93 * sub_cols + c) * sy, cx, cy, image_width, image_height,
                            None if transform is None else [F(v) for v in transform]))
    return out


# ---------------------------------------------------------------------------------------------------------------- images
def surface(rng, dtype, width, height, holes=0.08, pad=0):
    """a smooth surface between 1 and 4 metres with 0.5 % noise (most neighbours lie within the 2 % band, some do not), `holes` of the pixels
    replaced by what is no measurement: u16 0 and 65535, f32 0, NaN, +inf and a negative depth.  pad > 0: that many more columns in the array
    than the image has (a pitch larger than the row), filled with valid depths that would change every window at the right edge."""
    yy, xx = np.mgrid[0:height, 0:width + pad]
    z = 2.5 + 1.4 * np.sin(xx * 0.31 + rng.random()) * np.cos(yy * 0.23 + rng.random())
    z = z * (1 + 0.005 * rng.standard_normal(z.shape))
    z[rng.random(z.shape) < 0.15] *= 1.03                  # outside the band
    hole = rng.random(z.shape) < holes
    hole[:, width:] = False
    kind = rng.integers(0, 4, z.shape)
    if dtype == np.uint16:
        d = np.clip(np.round(z * 1000), 1, 65534).astype(np.uint16)
        d[hole] = np.where(kind[hole] < 2, 0, 65535)
    else:
        d = z.astype(np.float32)
        d[hole] = np.array([0.0, np.nan, np.inf, -1.5], np.float32)[kind[hole]]
    return d


def isolated(rng, width, height, lo=1.0, hi=4.0):
    """an f32 image in which only the pixels with odd coordinates carry a depth: every window has its centre alone, so Z is the pixel itself"""
    d = np.zeros((height, width), np.float32)
    d[1::2, 1::2] = rng.uniform(lo, hi, d[1::2, 1::2].shape).astype(np.float32)
    return d


def odd_pixel_points(width, height):
    return np.array([(x, y) for y in range(1, height, 2) for x in range(1, width, 2)], np.float32)


# ---------------------------------------------------------------------------------------------------------------- keypoints
def border_points(width, height, n_cameras=1):
    """every corner and edge of every sub-image, on the pixel and at the fractions where the rounding and the clamp change: x + 0.5f exactly
    cols with x < cols (clamped), x == cols (rejected), a coordinate in (-1.5, -0.5) (pixel 0) and one at -1.5 (outside); the same for y"""
    cols = width // n_cameras
    xs, ys = [], [-1.5, -1.0, -0.75, -0.5, 0.0, 0.49, 0.5, 1.0, height / 2, height - 2.0, height - 1.5, height - 1.0, height - 0.75, height - 0.5,
                  float(down(height)), float(height), height + 0.5]
    for c in range(n_cameras):
        a = c * cols
        xs += [a - 1.5, a - 1.0, a - 0.75, a - 0.5, a + 0.0, a + 0.49, a + 0.5, a + 1.0, a + cols / 2, a + cols - 2.0, a + cols - 1.5, a + cols - 1.0,
               a + cols - 0.75, a + cols - 0.5, float(down(a + cols)), float(a + cols)]
    return np.array([(x, y) for x in xs for y in ys], np.float32)


def wild_points():
    """what the reference asserts on or leaves undefined: NaN, inf and 1e20 coordinates"""
    return np.array([(np.nan, 1.0), (1.0, np.nan), (np.inf, 1.0), (1.0, -np.inf), (1e20, 1.0), (1.0, -1e20), (3e9, 1.0), (-2147483648.0, 2.0)], np.float32)


def random_points(rng, n, width, height):
    """uniform over the image and a margin of two pixels around it, a third of them exactly on a pixel or on a half"""
    p = np.stack([rng.uniform(-2, width + 2, n), rng.uniform(-2, height + 2, n)], 1)
    snap = rng.random(n) < 0.33
    p[snap] = np.round(p[snap] * 2) / 2
    return p.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- single properties
def band_edge_case():
    """an f32 window whose centre is D and whose right neighbour lies at EXACTLY 0.02f * D from it (not counted: the test is strict); the
    same with the neighbour one float inside the band (counted) -> (image_exact, image_inside, point)"""
    for k in range(1, 4000):
        D = F(1.0) + F(k) * F(2.0 ** -10)
        e = F(0.02) * D
        d = D + e
        if d - D == e and down(d) - D < e:
            a = np.zeros((3, 3), np.float32)
            a[1, 1], a[1, 2] = D, d
            b = a.copy()
            b[1, 2] = down(d)
            return a, b, np.array([[1.0, 1.0]], np.float32)
    raise AssertionError("no exact band edge found")


def loop_order_case(rng):
    """an f32 3 x 3 window in which visiting vv before uu changes the float sum -> (image, point)"""
    for _ in range(10000):
        D = F(rng.uniform(1, 4))
        a = (D * (1 + rng.uniform(-0.015, 0.015, (3, 3)))).astype(np.float32)
        a[1, 1] = D
        im = M.image(a, cameras_for(3, 3, 1))
        if M.get_depth(im, 0, 3, F(1), F(1), "uv") != M.get_depth(im, 0, 3, F(1), F(1), "vu"):
            return a, np.array([[1.0, 1.0]], np.float32)
    raise AssertionError("no order-sensitive window found")


def seam_case(rng, dtype, n_cameras, sub_cols=6, rows=5):
    """keypoints on the first and the last column of every sub-image of an image without holes whose neighbours all lie within the band: the
    pixel across the seam is valid and would count, and the generator draws images until it would change every one of these results
    -> (image array, points)"""
    width = n_cameras * sub_cols
    pts = np.array([(c * sub_cols + dx, y) for c in range(n_cameras) for dx in (0.0, 0.25, sub_cols - 1.0, sub_cols - 0.6) for y in (0.0, 2.0, rows - 1.0)], np.float32)
    for _ in range(200):
        z = 2.0 * (1 + rng.uniform(-0.008, 0.008, (rows, width)))
        d = np.round(z * 1000).astype(np.uint16) if dtype == np.uint16 else z.astype(np.float32)
        im = M.image(d, cameras_for(sub_cols, rows, n_cameras))
        inner = [p for p in pts if 1.0 <= p[0] < width - 1.5]              # the image's own border has nothing beyond it
        if all(M.get_depth(im, 0, width, p[0], p[1]) != M.point_of(im, p)[0][2] for p in inner):
            return d, pts
    raise AssertionError("no image found whose seams all matter")


def fma_transform_case(rng, tries=4000):
    """a camera with a local transform and keypoints on isolated pixels such that fusing the products of transformPoint into its sums changes
    at least one coordinate of at least one point -> (image array, cameras, points)"""
    for _ in range(tries):
        d = isolated(rng, 8, 6)
        t = list(rng.uniform(-1, 1, 12).astype(np.float32))
        cams = cameras_for(8, 6, 1, transform=t)
        im = M.image(d, cams)
        pts = odd_pixel_points(8, 6)
        try:
            a = M.frame(im, pts)[1]
            b = M.frame(im, pts, fma=True)[1]
        except ValueError:
            continue
        if (bits(a) != bits(b)).any():
            return d, cams, pts
    raise AssertionError("no input found that tells a fused transformPoint from the rule")


def fma_dist_case(rng, tries=20000):
    """one keypoint and a bound for which d2 computed with fused products falls on the other side of the squared bound than the rule's d2:
    the rule keeps the keypoint, the fused variant drops it -> (image array, cameras, points, min_depth, max_depth)"""
    for _ in range(tries):
        d = isolated(rng, 4, 4, 1.0, 3.0)
        cams = cameras_for(4, 4, 1)
        im = M.image(d, cams)
        pts = np.array([[1.0, 1.0]], np.float32)
        p = M.frame(im, pts)[1][0]
        try:
            r, f = M.dist_sqr(p), M.dist_sqr(p, fma=True)
        except ValueError:
            continue
        if r == f:
            continue
        b = F(np.sqrt(r))
        if b * b != r or not p[2] <= b:
            continue
        lo, hi = (0.0, float(b)) if f > r else (float(b), 0.0)
        if hi == 0.0 and not p[2] > b:
            continue
        if M.frame(im, pts, M.FILTER_3D, lo, hi)[0] == [0] and M.frame(im, pts, M.FILTER_3D, lo, hi, fma=True)[0] == []:
            return d, cams, pts, lo, hi
    raise AssertionError("no input found that tells a fused d2 from the rule")


# ---------------------------------------------------------------------------------------------------------------- batches
def random_frame(rng, dtype, width, height, n_cameras, n, pad=0, image_size=None, transform=None, zero_principal=False, host_ok=False, border=True):
    """-> (image, points in the coordinates of the colour image): border_points (unless border is False) mixed with random_points.  host_ok: without the keypoints the reference asserts on (a keypoint at or
    behind the last camera's last column, or before the first camera's sub-image), which the host entry refuses"""
    sub = width // n_cameras
    iw, ih = image_size if image_size else (0, 0)
    im = M.image(surface(rng, dtype, width, height, pad=pad), cameras_for(sub, height, n_cameras, iw, ih, transform, zero_principal), width)
    sx, sy = (iw / sub if iw else 1.0), (ih / height if ih else 1.0)
    pts = random_points(rng, 2 * max(n, 0) + 8, width, height)               # more than needed: host_ok drops some
    if border:
        pts = np.concatenate([border_points(width, height, n_cameras), pts])
    pts = np.ascontiguousarray(pts * np.array([sx, sy], np.float32), np.float32)
    if host_ok:
        pts = pts[[M.point_of(im, p, device=True)[1] for p in pts]]
    pts = pts[rng.permutation(pts.shape[0])[:n]] if n else pts[:0]
    assert pts.shape[0] == n
    return im, np.ascontiguousarray(pts)


def concat(frames_points):
    off = np.cumsum([0] + [len(p) for p in frames_points]).astype(np.int64)
    pts = np.concatenate([np.asarray(p, np.float32).reshape(-1, 2) for p in frames_points]) if frames_points else np.zeros((0, 2), np.float32)
    return np.ascontiguousarray(pts), off


def api_images(images, data_of=lambda im: im["data"]):
    """the model's images as rtabmap_amd.Engine.keypoints_3d takes them"""
    return [dict(data=data_of(im), cameras=im["cameras"], width=im["width"], n_cameras=len(im["cameras"])) for im in images]


def assert_same(got, images, frames_points, filter, min_depth, max_depth, device=False, with_xyz=True, response=None, rows=None, aux=None, what="", want=None):
    """counts, the whole index list and, for every frame, the first count entries of every output: bit for bit.  want: the model's batch()
    where the caller has it already"""
    if want is None:
        want = M.batch(images, frames_points, filter, min_depth, max_depth, device, with_xyz)
    pts, off = concat(frames_points)
    np.testing.assert_array_equal(got["count"], want["count"], err_msg=what + " count")
    np.testing.assert_array_equal(got["index"], want["index"], err_msg=what + " index")
    for f in range(len(images)):
        a, kept = int(off[f]), want["kept"][f]
        c = len(kept)
        tag = "%s frame %d" % (what, f)
        if want["xyz"][f] is not None:
            np.testing.assert_array_equal(bits(got["xyz"][a:a + c]), bits(want["xyz"][f][kept]), err_msg=tag + " xyz")
        if filter == M.KEEP_ALL:
            continue
        np.testing.assert_array_equal(bits(got["points"][a:a + c]), bits(pts[a:a + len(frames_points[f])][kept]), err_msg=tag + " points")
        for src, name in ((response, "response"), (rows, "rows"), (aux, "aux")):
            if src is not None:
                x = np.ascontiguousarray(src[a:a + len(frames_points[f])][kept])
                np.testing.assert_array_equal(np.ascontiguousarray(got[name][a:a + c]).view(np.uint8), x.view(np.uint8), err_msg=tag + " " + name)


def stage_dev(images, frames_points, response=None, rows=None, aux=None, with_xyz=True):
    """the batch on the device, outputs canary-filled, uploaded and synchronised; an image shared by frames (the same array) is uploaded once"""
    import torch
    pts, off = concat(frames_points)
    n, nf = pts.shape[0], len(images)
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    cache = {}
    def data_of(im):
        if id(im["data"]) not in cache:
            d = im["data"]
            cache[id(im["data"])] = torch.from_numpy(np.ascontiguousarray(d.view(np.int16) if d.dtype == np.uint16 else d)).cuda()
        return cache[id(im["data"])]
    api = api_images(images, data_of)
    for a, im in zip(api, images):
        a["type"] = 0 if im["data"].dtype == np.uint16 else 1
    canary = lambda shape, dt: torch.full(shape, CANARY, dtype=dt, device="cuda")
    st = dict(off=off, images=api, pts=dev(pts), resp=dev(response), d_rows=dev(rows), d_aux=dev(aux), aux_bytes=0 if aux is None else aux.shape[1],
              count=canary((nf,), torch.int32), index=canary((n,), torch.int32), xyz=canary((n, 3), torch.float32) if with_xyz else None,
              points=canary((n, 2), torch.float32), response=None if response is None else canary((n,), torch.float32),
              rows=None if rows is None else torch.zeros_like(dev(rows)), aux=None if aux is None else torch.zeros_like(dev(aux)))
    torch.cuda.synchronize()
    return st


def launch_dev(eng, st, filter, min_depth, max_depth):
    eng.keypoints_3d_dev(st["pts"], st["off"], st["images"], st["count"], st["index"], st["xyz"], filter=filter, min_depth=min_depth, max_depth=max_depth,
                         d_response=st["resp"], d_rows=st["d_rows"], d_aux=st["d_aux"], aux_bytes=st["aux_bytes"], d_out_points=st["points"],
                         d_out_response=st["response"], d_out_rows=st["rows"], d_out_aux=st["aux"])
    return st


def to_host(eng, st):
    eng.synchronize()
    return {k: (None if st[k] is None else st[k].cpu().numpy()) for k in ("count", "index", "xyz", "points", "response", "rows", "aux")}


def run_dev(eng, images, frames_points, filter, min_depth, max_depth, response=None, rows=None, aux=None, with_xyz=True):
    return to_host(eng, launch_dev(eng, stage_dev(images, frames_points, response, rows, aux, with_xyz), filter, min_depth, max_depth))


def run_host(eng, images, frames_points, filter, min_depth, max_depth, response=None, rows=None, aux=None, with_xyz=True):
    pts, off = concat(frames_points)
    return eng.keypoints_3d(pts, off, api_images(images), filter=filter, min_depth=min_depth, max_depth=max_depth, response=response, rows=rows,
                            aux=aux, xyz=with_xyz)
