"""Inputs of the LCD_SELECT_SSC tests: generators whose properties tests/test_ssc_select_inputs.py proves on the model, without a GPU, and the
helpers that run a batch through the engine's entries and compare it with the model exactly."""
import numpy as np

import ssc_select_model as M

CANARY = -7
DENORMAL = np.float32(1e-45)
SIZES = [(16, 16), (33, 17), (64, 48), (100, 7), (640, 480)]


# ---------------------------------------------------------------------------------------------------------------- frames
def _frame(response, points, image_size):
    return dict(response=np.ascontiguousarray(response, np.float32), points=np.ascontiguousarray(points, np.float32).reshape(-1, 2),
                image_size=(int(image_size[0]), int(image_size[1])))


def distinct_responses(rng, n):
    """distinct, a third of them negative"""
    return ((rng.permutation(n) + 1) * np.where(rng.random(n) < 0.3, -1, 1)).astype(np.float32)


def tied_responses(rng, n):
    """a pool of 12 values with both signs, both zeros and denormals: heavy ties, and -0.0 == +0.0 ordered by index"""
    pool = np.array([0.0, -0.0, DENORMAL, -DENORMAL, 3 * DENORMAL, 0.5, -0.5, 1.0, 1.0, -1.0, 7.25, -1e30], np.float32)
    return pool[rng.integers(0, pool.shape[0], n)]


def uniform_frame(rng, n, image_size, tied=False):
    """points uniform over the image, its far edges included"""
    pts = rng.random((n, 2)) * np.array(image_size, np.float64)
    return _frame(tied_responses(rng, n) if tied else distinct_responses(rng, n), pts, image_size)


def integer_frame(rng, n, image_size):
    """points on the pixel grid, x == cols and y == rows among them"""
    pts = np.stack([rng.integers(0, image_size[0] + 1, n), rng.integers(0, image_size[1] + 1, n)], 1)
    return _frame(distinct_responses(rng, n), pts, image_size)


def clustered_frame(rng, n, image_size, clusters=4, spread=1.5):
    """points around a few centres: a covering that must shrink its squares to find enough of them"""
    size = np.array(image_size, np.float64)
    centres = rng.random((clusters, 2)) * size
    pts = centres[rng.integers(0, clusters, n)] + rng.standard_normal((n, 2)) * spread
    return _frame(distinct_responses(rng, n), np.clip(pts, 0.0, size), image_size)


def one_pixel_frame(rng, n, image_size):
    """every feature inside one pixel: whatever the width, one cell, one feature selected"""
    x, y = image_size[0] // 2, image_size[1] // 2
    pts = np.array([x, y], np.float64) + rng.random((n, 2)) * 0.125
    return _frame(tied_responses(rng, n), pts, image_size)


def border_frame(rng, n, image_size):
    """points on all four borders, the corners and x == cols, y == rows included; the rest uniform"""
    f = uniform_frame(rng, n, image_size, tied=True)
    cols, rows = image_size
    k = n // 8
    p = f["points"]
    p[0 * k:1 * k, 0] = 0.0
    p[1 * k:2 * k, 0] = cols
    p[2 * k:3 * k, 1] = 0.0
    p[3 * k:4 * k, 1] = rows
    p[4 * k:4 * k + 4] = [(0, 0), (cols, 0), (0, rows), (cols, rows)]
    p[4 * k + 4] = (-0.0, -0.0)                                           # inside: floor(-0.0 / c) is cell 0
    return f


# (name, generator, n, max_features, image size, seed): what tests/test_ssc_select_inputs.py proves each of them reaches
NAMED = [
    ("found", uniform_frame, 300, 100, (640, 480), 1),
    ("few", uniform_frame, 246, 63, (64, 48), 12),
    ("many_above_max", uniform_frame, 124, 59, (33, 17), 1),
    ("empty", uniform_frame, 204, 166, (16, 16), 1),
    ("width_1", clustered_frame, 400, 200, (640, 480), 1),
    ("one_pixel", one_pixel_frame, 90, 20, (64, 48), 1),
    ("ties", lambda rng, n, size: uniform_frame(rng, n, size, tied=True), 257, 64, (100, 7), 1),
    ("borders", border_frame, 200, 50, (33, 17), 1),
    ("integer", integer_frame, 400, 150, (64, 48), 1),
]


def named(name):
    """-> (frame, max_features)"""
    for nm, gen, n, mx, size, seed in NAMED:
        if nm == name:
            return gen(np.random.default_rng(seed), n, size), mx
    raise KeyError(name)


def rows_of(rng, dtype, dim, n):
    if dtype == "f32":
        return rng.standard_normal((n, dim)).astype(np.float32)
    return rng.integers(0, 256, (n, dim), dtype=np.uint8)


def concat(frames):
    """-> (response [N], points [N x 2], offsets [n_frames + 1], image_size [n_frames x 2])"""
    off = np.cumsum([0] + [len(f["response"]) for f in frames]).astype(np.int64)
    resp = np.concatenate([f["response"] for f in frames]).astype(np.float32)
    pts = np.concatenate([f["points"] for f in frames]).astype(np.float32).reshape(-1, 2)
    size = np.array([f["image_size"] for f in frames], np.int32).reshape(-1, 2)
    return resp, pts, off, size


# ---------------------------------------------------------------------------------------------------------------- running the engine
def run_host(eng, frames, max_features, order=M.KEEP_ORDER, rows=None, aux=None, n_in=None, ssc=True):
    resp, pts, off, size = concat(frames)
    count, index, out_rows, out_aux = eng.select_features(resp, off, max_features, order=order, image_size=size, points=pts, rows=rows, aux=aux,
                                                          n_in=n_in, ssc=ssc)
    return dict(count=count, index=index, rows=out_rows, aux=out_aux)


def stage_dev(frames, rows=None, aux=None, n_in=None):
    """the batch's inputs and canary-filled outputs on the device, uploaded and synchronised"""
    import torch
    resp, pts, off, size = concat(frames)
    n, nf = resp.shape[0], off.shape[0] - 1
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    st = dict(off=off, size=size, resp=dev(resp), pts=dev(pts), d_rows=dev(rows), d_aux=dev(aux), aux_bytes=0 if aux is None else aux.shape[1],
              n_in=None if n_in is None else dev(np.asarray(n_in, np.int32)),
              count=torch.full((nf,), CANARY, dtype=torch.int32, device="cuda"), index=torch.full((n,), CANARY, dtype=torch.int32, device="cuda"))
    st["rows"] = None if rows is None else torch.zeros_like(st["d_rows"])
    st["aux"] = None if aux is None else torch.zeros_like(st["d_aux"])
    torch.cuda.synchronize()
    return st


def launch_dev(eng, st, max_features, order=M.KEEP_ORDER, ssc=True):
    """lcd_select_features_dev on a staged batch: enqueued, not synchronised"""
    eng.select_features_dev(st["resp"], st["off"], max_features, st["count"], st["index"], order=order, image_size=st["size"], d_points=st["pts"],
                            d_rows=st["d_rows"], d_aux=st["d_aux"], aux_bytes=st["aux_bytes"], d_out_rows=st["rows"], d_out_aux=st["aux"],
                            d_n_in=st["n_in"], ssc=ssc)
    return st


def to_host(eng, out):
    eng.synchronize()
    return {k: (None if out[k] is None else out[k].cpu().numpy()) for k in ("count", "index", "rows", "aux")}


def run_dev(eng, frames, max_features, order=M.KEEP_ORDER, rows=None, aux=None, n_in=None, ssc=True):
    return to_host(eng, launch_dev(eng, stage_dev(frames, rows, aux, n_in), max_features, order, ssc))


_EXPECTED = {}


def expected(frames, max_features, order, device=False, n_in=None, key=None):
    """the model's (count, index) for a batch.  With a key the selection in response order is computed once per (key, max_features,
    device, n_in), shared by every test that names it and left unchanged; KEEP_ORDER is each frame's list in ascending index."""
    k = None if key is None else (key, max_features, device, None if n_in is None else tuple(int(v) for v in n_in))
    if k is None:
        return M.select_batch(frames, max_features, order, device, n_in)
    if k not in _EXPECTED:
        got = M.select_batch(frames, max_features, M.BY_RESPONSE, device, n_in)
        got[0].setflags(write=False)
        got[1].setflags(write=False)
        _EXPECTED[k] = got
    count, index = _EXPECTED[k]
    if order == M.BY_RESPONSE:
        return count, index
    index = index.copy()
    off = concat(frames)[2]
    for f in range(len(frames)):
        a, c = int(off[f]), int(count[f])
        index[a:a + c] = np.sort(index[a:a + c])
    return count, index


def assert_same(got, frames, max_features, order=M.KEEP_ORDER, rows=None, aux=None, device=False, n_in=None, what="", key=None):
    """counts and the whole index list (the -1 tails included) against the model; rows and payload gathered by the model's list"""
    count, index = expected(frames, max_features, order, device, n_in, key)
    np.testing.assert_array_equal(got["count"], count, err_msg=what + " count")
    np.testing.assert_array_equal(got["index"], index, err_msg=what + " index")
    off = concat(frames)[2]
    for src, dst, name in ((rows, got["rows"], " rows"), (aux, got["aux"], " aux")):
        if src is None:
            assert dst is None
            continue
        for f in range(len(frames)):
            a, c = int(off[f]), int(count[f])
            np.testing.assert_array_equal(dst[a:a + c], src[a + index[a:a + c]], err_msg="%s%s of frame %d" % (what, name, f))
