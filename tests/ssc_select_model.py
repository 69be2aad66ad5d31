"""The LCD_SELECT_SSC rule of lcd_select_features (include/lcd.h) in plain Python, written from the reference's text (util2d.cpp:2295-2366,
Features2d.cpp:304-355 and :420-446): float32 where the reference computes in float, Python floats where it computes in double, and the
reference's byte mask (`evaluate_mask`).  Beside it the pairwise reading the kernel uses (`evaluate_pairwise`): a feature is selected iff no
feature selected before it lies within 2 cells in both row and column.  `search` runs both and asserts that they agree.
`device=True` switches to the device entry's definitions: a NaN response is ordered by its mapped bits, and a feature whose cell lies
outside the mask of an iteration is not selected in it and covers nothing."""
import math

import numpy as np

KEEP_ORDER, BY_RESPONSE = "keep_order", "by_response"
MAX_SSC_FEATURES = 8192
MAX_IMAGE_SIDE = 16384
MASK_CELLS_LIMIT = 1 << 26                                                 # above it select_frame trusts the pairwise form alone
TOLERANCE = np.float32(0.1)


class Refused(Exception):
    """what the host entry answers with LCD_ERR_INVALID"""


def c_round(x):
    """C's round(): halves away from zero"""
    x = float(x)
    return math.copysign(math.floor(abs(x) + 0.5), x)


def mapped_bits(response):
    """b(i): the response's bits, -0.0 as +0.0, mapped monotonically to unsigned"""
    bits = np.ascontiguousarray(response, np.float32).view(np.uint32).astype(np.int64)
    bits = np.where(bits == 0x80000000, 0, bits)
    return np.where(bits >= 0x80000000, 0xFFFFFFFF - bits, bits | 0x80000000)


def order_of(response):
    """cv::sortIdx(.., SORT_DESCENDING) on the signed response, ties to the lower index (the engine's definition)"""
    b = mapped_bits(response)
    return sorted(range(len(b)), key=lambda i: (-int(b[i]), i))


def scalars(max_features, cols, rows):
    """-> (m, high, Kmin, Kmax) as util2d.cpp:2299-2319 computes them"""
    m = int(max_features - c_round(np.float32(max_features) * TOLERANCE))
    if m < 2:
        raise Refused("max_features == 1: exp4 == 0")
    exp1 = rows + cols + 2 * m
    exp2 = 4 * cols + 4 * m + 4 * rows * m + rows * rows + cols * cols - 2 * rows * cols + 4 * rows * cols * m
    exp3 = math.sqrt(exp2)
    exp4 = float(m - 1)
    sol1 = -c_round((exp1 + exp3) / exp4)
    sol2 = -c_round((exp1 - exp3) / exp4)
    high = int(sol1 if sol1 > sol2 else sol2)
    fm = np.float32(m)
    kmin = int(c_round(fm - fm * TOLERANCE))
    kmax = int(c_round(fm + fm * TOLERANCE))
    return m, high, kmin, kmax


def low_of(n, m):
    return max(1, int(math.floor(math.sqrt(float(n) / m))))


def cell_of(point, c):
    """(row, col) of util2d.cpp:2341-2342, or None where the quotient is no number or below zero"""
    qy, qx = float(point[1]) / c, float(point[0]) / c
    if not (math.isfinite(qy) and math.isfinite(qx)):
        return None
    return int(math.floor(qy)), int(math.floor(qx))


def _cells(points, sorted_idx, c, n_cell_rows, n_cell_cols):
    out = []
    for i in sorted_idx:
        rc = cell_of(points[i], c)
        out.append(rc if rc is not None and 0 <= rc[0] <= n_cell_rows and 0 <= rc[1] <= n_cell_cols else None)
    return out


def evaluate_mask(cells, n_cell_rows, n_cell_cols):
    """one iteration with the reference's covered mask (:2337-2352) -> positions in the sorted list"""
    covered = np.zeros((n_cell_rows + 1, n_cell_cols + 1), np.uint8)
    result = []
    for p, rc in enumerate(cells):
        if rc is None:
            continue
        row, col = rc
        if not covered[row, col]:
            result.append(p)
            covered[max(row - 2, 0):min(row + 2, n_cell_rows) + 1, max(col - 2, 0):min(col + 2, n_cell_cols) + 1] = 255
    return result


def evaluate_pairwise(cells):
    """one iteration as the kernel reads it: selected iff no earlier selected cell within 2 rows and 2 columns"""
    chosen = set()
    result = []
    for p, rc in enumerate(cells):
        if rc is None:
            continue
        row, col = rc
        if any((row + dr, col + dc) in chosen for dr in range(-2, 3) for dc in range(-2, 3)):
            continue
        chosen.add(rc)
        result.append(p)
    return result


def search(response, points, max_features, image_size, device=False, form="both", trace=None):
    """the binary search of :2325-2364 over a CUT frame -> the selected features in response order.  trace (a dict) receives the exit
    ("found", "few", "many", "empty"), the widths evaluated and the sizes they gave."""
    r = np.asarray(response, np.float32).reshape(-1)
    pts = np.asarray(points, np.float32).reshape(-1, 2)
    n = r.shape[0]
    cols, rows = int(image_size[0]), int(image_size[1])
    if cols < 1 or rows < 1:
        raise Refused("a cut frame's image side < 1")
    if not device:
        if np.isnan(r).any():
            raise Refused("NaN response")
        ok = (pts[:, 0] >= 0) & (pts[:, 0] <= cols) & (pts[:, 1] >= 0) & (pts[:, 1] <= rows)      # NaN compares false
        if not ok.all():
            raise Refused("a keypoint outside the image")
    m, high, kmin, kmax = scalars(max_features, cols, rows)
    low, high0 = low_of(n, m), high
    order = order_of(r)
    prev_width = -1
    result = []
    widths, sizes = [], []
    exit_ = None
    while True:
        width = low + int((high - low) / 2)                                # C truncation
        if width == prev_width or low > high:
            break
        c = width / 2.0
        n_cell_cols, n_cell_rows = int(math.floor(cols / c)), int(math.floor(rows / c))
        cells = _cells(pts, order, c, n_cell_rows, n_cell_cols)
        with_mask = form in ("both", "mask") and (n_cell_rows + 1) * (n_cell_cols + 1) <= MASK_CELLS_LIMIT
        if form != "mask" or not with_mask:
            result = evaluate_pairwise(cells)
        if with_mask:
            by_mask = evaluate_mask(cells, n_cell_rows, n_cell_cols)
            assert form == "mask" or by_mask == result, "the mask form and the pairwise form differ at width %d" % width
            result = by_mask
        widths.append(width)
        sizes.append(len(result))
        if kmin <= len(result) <= kmax:
            exit_ = "found"
            break
        if len(result) < kmin:
            high = width - 1
        else:
            low = width + 1
        prev_width = width
    if exit_ is None:
        exit_ = "empty" if not widths else ("few" if sizes[-1] < kmin else "many")
    if trace is not None:
        trace.update(exit=exit_, widths=widths, sizes=sizes, m=m, high=high0, kmin=kmin, kmax=kmax, low=low_of(n, m))
    return [order[p] for p in result]


def select_frame(response, max_features, order=KEEP_ORDER, image_size=None, points=None, device=False, form="both", trace=None):
    """-> the selected feature indices in output order (a list)"""
    n = len(response)
    if max_features == 1:
        raise Refused("max_features == 1")
    if max_features <= 0 or n <= max_features:
        return list(range(n))
    if image_size is None or points is None:
        raise Refused("a cut frame needs points and an image size")
    if max(image_size) > MAX_IMAGE_SIDE:
        raise Refused("image side above 16384")                           # (LCD_ERR_UNSUPPORTED in the entries)
    kept = search(response, points, max_features, image_size, device, form, trace)
    return kept if order == BY_RESPONSE else sorted(kept)


def select_batch(frames, max_features, order=KEEP_ORDER, device=False, n_in=None, form="both"):
    """frames: dicts with response, points and image_size -> (count [n_frames], index [N], -1 behind each frame's count)"""
    count, index = [], []
    for f, fr in enumerate(frames):
        region = len(fr["response"])
        n = region if n_in is None else min(max(int(n_in[f]), 0), region)
        kept = select_frame(fr["response"][:n], max_features, order, fr["image_size"], fr["points"][:n], device, form)
        count.append(len(kept))
        index += kept + [-1] * (region - len(kept))
    return np.array(count, np.int32), np.array(index, np.int32).reshape(-1)
