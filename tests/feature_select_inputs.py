"""Inputs of the feature-selection tests: generators whose properties tests/test_feature_select_inputs.py proves on the model, without a
GPU, and the helpers that run a batch through the engine's entries and compare it with the model exactly."""
import numpy as np

import feature_select_model as M

KINDS = [("f32", 64), ("f32", 128), ("u8", 32), ("u8", 61)]
# (grid rows, grid cols), (width, height): 640 x 480 divides by both grids, 641 x 482 by neither
GRIDS = [((4, 4), (640, 480)), ((3, 5), (640, 480)), ((4, 4), (641, 482)), ((3, 5), (641, 482))]
SIZES = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 16384]
DENORMAL = np.float32(1e-45)
CANARY = -7


# ---------------------------------------------------------------------------------------------------------------- frames
def tied_frame(rng, n):
    """responses drawn from a pool of 12 magnitudes with both signs, both zeros and denormals: heavy ties everywhere"""
    pool = np.array([0.0, -0.0, DENORMAL, -DENORMAL, 3 * DENORMAL, 0.5, -0.5, 1.0, 1.0, -1.0, 7.25, -1e30], np.float32)
    return dict(response=pool[rng.integers(0, pool.shape[0], n)])


def cut_in_tie_frame(rng, n, max_features):
    """distinct responses except a group of equal magnitudes (both signs) that straddles rank max_features"""
    r = (rng.permutation(n) + 1).astype(np.float32)
    order = np.argsort(-r)
    lo, hi = max(max_features - 3, 0), min(max_features + 3, n)
    r[order[lo:hi]] = r[order[lo]] * np.where(rng.random(hi - lo) < 0.5, -1, 1).astype(np.float32)
    return dict(response=r)


def all_equal_frame(n):
    return dict(response=np.full(n, 0.125, np.float32))


def distinct_frame(rng, n):
    return dict(response=(rng.permutation(n).astype(np.float32) + 1) * np.where(rng.random(n) < 0.3, -1, 1).astype(np.float32))


def grid_frame(rng, n, image_size, grid, max_features, outside=0):
    """n keypoints on the grid's cells such that every cell state occurs: cell 0 empty, cell 1 under perCell, cell 2 exactly perCell,
    cell 3 perCell + 1, the others random (many over).  Some points sit exactly on a cell's first pixel, some at its last fraction.
    outside > 0: that many further points lie outside the grid (below -cell size, in the remainder strip if there is one, or far away)."""
    rows, cols = grid
    row_size, col_size = image_size[1] // rows, image_size[0] // cols
    per_cell = max_features // (rows * cols)
    cells = [1] * max(per_cell - 1, 0) + [2] * per_cell + [3] * (per_cell + 1)
    assert n >= len(cells) and rows * cols > 4
    cells = np.array(cells + rng.integers(3, rows * cols, n - len(cells)).tolist())
    frac = rng.random((n, 2)) * 0.998
    frac[rng.random(n) < 0.1] = 0.0                                   # the cell's first pixel
    frac[rng.random(n) < 0.1] = 0.998
    x = ((cells % cols) + frac[:, 0]) * col_size
    y = ((cells // cols) + frac[:, 1]) * row_size
    pts = np.stack([x, y], 1).astype(np.float32)
    extra = []
    for k in range(outside):
        kind = k % 4
        if kind == 0:
            extra.append((-float(col_size) - 0.5, 3.0))
        elif kind == 1:
            extra.append((3.0, float(rows * row_size) + (0.5 if image_size[1] % rows else 1e6)))
        elif kind == 2:
            extra.append((float(cols * col_size), 3.0))
        else:
            extra.append((1e20, -1e20))
    if extra:
        pts = np.concatenate([pts, np.array(extra, np.float32)])
    perm = rng.permutation(pts.shape[0])
    f = tied_frame(rng, pts.shape[0])
    return dict(response=f["response"], points=np.ascontiguousarray(pts[perm]), image_size=tuple(image_size))


def cell_states(frame, grid, max_features):
    """the set of {"empty", "under", "at", "over", "outside"} that occur in the frame"""
    rows, cols = grid
    per_cell = max_features // (rows * cols)
    counts = {}
    states = set()
    for p in frame["points"]:
        c = M.cell_of(p, frame["image_size"], grid)
        if c is None:
            states.add("outside")
        else:
            counts[c] = counts.get(c, 0) + 1
    for r in range(rows):
        for c in range(cols):
            k = counts.get((r, c), 0)
            states.add("empty" if k == 0 else "under" if k < per_cell else "at" if k == per_cell else "over")
    return states


def expansion_frame(rng, n, count=None):
    """count distinct indices in random order; ids of all three kinds: existing words, the codes -1 .. -k of new words (each may repeat),
    and 0"""
    count = int(rng.integers(0, n + 1)) if count is None else count
    index = rng.permutation(n)[:count].astype(np.int32)
    kind = rng.integers(0, 3, count)
    n_new = max(1, count // 3)
    ids = np.where(kind == 0, rng.integers(1, 5000, count), np.where(kind == 1, -rng.integers(1, n_new + 1, count), 0)).astype(np.int32)
    return dict(index=index, word_ids=ids, count=count)


def rows_of(rng, dtype, dim, n):
    if dtype == "f32":
        return rng.standard_normal((n, dim)).astype(np.float32)
    return rng.integers(0, 256, (n, dim), dtype=np.uint8)


def concat(frames):
    """-> (response [N], points [N x 2] or None, offsets [n_frames + 1], image_size [n_frames x 2] or None)"""
    off = np.cumsum([0] + [len(f["response"]) for f in frames]).astype(np.int64)
    resp = np.concatenate([np.asarray(f["response"], np.float32) for f in frames]) if frames else np.zeros(0, np.float32)
    if frames and "points" in frames[0]:
        pts = np.concatenate([f["points"] for f in frames]).astype(np.float32).reshape(-1, 2)
        size = np.array([f["image_size"] for f in frames], np.int32).reshape(-1, 2)
    else:
        pts = size = None
    return resp, pts, off, size


# ---------------------------------------------------------------------------------------------------------------- running the engine
def run_host(eng, frames, max_features, order=M.KEEP_ORDER, grid=(1, 1), rows=None, aux=None):
    resp, pts, off, size = concat(frames)
    count, index, out_rows, out_aux = eng.select_features(resp, off, max_features, order=order, grid=grid, image_size=size, points=pts, rows=rows, aux=aux)
    return dict(count=count, index=index, rows=out_rows, aux=out_aux)


def stage_dev(frames, rows=None, aux=None):
    """the batch's inputs and canary-filled outputs on the device, uploaded and synchronised"""
    import torch
    resp, pts, off, size = concat(frames)
    n, nf = resp.shape[0], off.shape[0] - 1
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    st = dict(off=off, size=size, resp=dev(resp), pts=dev(pts), d_rows=dev(rows), d_aux=dev(aux), aux_bytes=0 if aux is None else aux.shape[1],
              count=torch.full((nf,), CANARY, dtype=torch.int32, device="cuda"), index=torch.full((n,), CANARY, dtype=torch.int32, device="cuda"))
    st["rows"] = None if rows is None else torch.zeros_like(st["d_rows"])
    st["aux"] = None if aux is None else torch.zeros_like(st["d_aux"])
    torch.cuda.synchronize()
    return st


def launch_dev(eng, st, max_features, order=M.KEEP_ORDER, grid=(1, 1)):
    """lcd_select_features_dev on a staged batch: enqueued, not synchronised"""
    eng.select_features_dev(st["resp"], st["off"], max_features, st["count"], st["index"], order=order, grid=grid, image_size=st["size"],
                            d_points=st["pts"], d_rows=st["d_rows"], d_aux=st["d_aux"], aux_bytes=st["aux_bytes"], d_out_rows=st["rows"],
                            d_out_aux=st["aux"])
    return st


def run_dev(eng, frames, max_features, order=M.KEEP_ORDER, grid=(1, 1), rows=None, aux=None):
    """the batch through lcd_select_features_dev, results read back"""
    return to_host(eng, launch_dev(eng, stage_dev(frames, rows, aux), max_features, order, grid))


def to_host(eng, out):
    eng.synchronize()
    return {k: (None if out[k] is None else out[k].cpu().numpy()) for k in ("count", "index", "rows", "aux")}


def assert_same(got, frames, max_features, order=M.KEEP_ORDER, grid=(1, 1), rows=None, aux=None, device=False, what=""):
    """counts and the whole index list (the -1 tails included) against the model; rows and payload gathered by the model's list"""
    count, index = M.select_batch(frames, max_features, order, grid, device)
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
