"""The rule of lcd_select_features / lcd_expand_word_ids (include/lcd.h) in NumPy and plain Python, written from the reference's text
(Features2d.cpp:293-516, Memory.cpp:5951-6059) and not from the engine's keys: a std::multimap over fabs(response) walked backwards is a
sort by (fabs(response), insertion index), descending.  `device=True` switches to the three definitions the device entries add: a NaN
response is ordered by its masked bits, a keypoint outside the grid is never selected, and an index outside its frame is skipped."""
import numpy as np

KEEP_ORDER, BY_RESPONSE = "keep_order", "by_response"
MAX_FEATURES_PER_FRAME = 16384


class Refused(Exception):
    """what the host entries answer with LCD_ERR_INVALID"""


def to_int(v):
    """int(v) toward zero, saturating, NaN -> 0"""
    v = float(v)
    if v != v:
        return 0
    if v >= 2147483648.0:
        return 2147483647
    if v <= -2147483648.0:
        return -2147483648
    return int(v)


def c_div(a, b):
    """C's integer division: toward zero"""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


def strongest_first(response, members, device=False):
    """`members` (feature indices) as the reverse walk of the multimap visits them"""
    r = np.asarray(response, np.float32)
    if np.isnan(r[members]).any():
        if not device:
            raise Refused("NaN response")
        bits = r.view(np.uint32) & np.uint32(0x7FFFFFFF)
        return sorted(members, key=lambda i: (int(bits[i]), i), reverse=True)
    return sorted(members, key=lambda i: (abs(float(r[i])), i), reverse=True)


def cell_of(point, image_size, grid):
    """(row, col) of Features2d.cpp:495-496, or None where the reference asserts"""
    rows, cols = grid
    row_size, col_size = image_size[1] // rows, image_size[0] // cols
    cr, cc = c_div(to_int(point[1]), row_size), c_div(to_int(point[0]), col_size)
    return (cr, cc) if 0 <= cr < rows and 0 <= cc < cols else None


def select_frame(response, max_features, order=KEEP_ORDER, grid=(1, 1), image_size=None, points=None, device=False):
    """-> the selected feature indices in output order (a list)"""
    r = np.asarray(response, np.float32).reshape(-1)
    n = r.shape[0]
    rows, cols = grid
    if rows * cols > 1 and order == BY_RESPONSE:
        raise Refused("no grid variant")
    if not device and np.isnan(r).any():
        raise Refused("NaN response")
    if max_features <= 0 or n <= max_features:
        return list(range(n))
    if rows * cols == 1:
        kept = strongest_first(r, list(range(n)), device)[:max_features]
        return kept if order == BY_RESPONSE else sorted(kept)
    if image_size[1] <= rows or image_size[0] <= cols:
        raise Refused("image not larger than the grid")
    per_cell = max_features // (rows * cols)
    members = {}
    for i in range(n):
        c = cell_of(points[i], image_size, grid)
        if c is None:
            if not device:
                raise Refused("keypoint outside the grid")
            continue
        members.setdefault(c, []).append(i)
    kept = []
    for m in members.values():
        kept += strongest_first(r, m, device)[:per_cell] if per_cell > 0 and len(m) > per_cell else m
    return sorted(kept)


def select_batch(frames, max_features, order=KEEP_ORDER, grid=(1, 1), device=False):
    """frames: dicts with response and, for a grid, points and image_size -> (count [n_frames], index [N], -1 behind each frame's count)"""
    count, index = [], []
    for f in frames:
        kept = select_frame(f["response"], max_features, order, grid, f.get("image_size"), f.get("points"), device)
        n = len(f["response"])
        count.append(len(kept))
        index += kept + [-1] * (n - len(kept))
    return np.array(count, np.int32), np.array(index, np.int32).reshape(-1)


def resolve(word_id, first_new_word_id):
    """an id > 0 stands, a code -(k+1) is first + k, everything else is 0 = no word"""
    if word_id > 0:
        return int(word_id)
    if word_id < 0 and first_new_word_id > 0:
        v = (int(first_new_word_id) + (-(int(word_id) + 1))) & 0xFFFFFFFF
        v = v - (1 << 32) if v >= (1 << 31) else v
        return v if v > 0 else 0
    return 0


def expand_frame(n, index, word_ids, first_new_word_id=0, device=False):
    """index[j] has word_ids[j] (all entries given are valid) -> one id per feature"""
    all_ids = [0] * n
    for i, w in zip(index, word_ids):
        if i < 0 or i >= n:
            if not device:
                raise Refused("index outside the frame")
            continue
        v = resolve(int(w), first_new_word_id)
        if v > 0:
            all_ids[int(i)] = v
    neg = -1
    for i in range(n):
        if all_ids[i] <= 0:
            all_ids[i] = neg
            neg -= 1
    return np.array(all_ids, np.int32).reshape(-1)


def expand_batch(offsets, count, index, word_ids, first_new_word_id=None, device=False):
    out = []
    for f in range(len(offsets) - 1):
        a, n = int(offsets[f]), int(offsets[f + 1] - offsets[f])
        c = int(count[f])
        if device:
            c = min(max(c, 0), n)
        elif c < 0 or c > n:
            raise Refused("count outside the frame")
        out.append(expand_frame(n, index[a:a + c], word_ids[a:a + c], 0 if first_new_word_id is None else int(first_new_word_id[f]), device))
    return np.concatenate(out) if out else np.zeros(0, np.int32)
