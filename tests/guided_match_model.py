"""NumPy model of lcd_match_guided (include/lcd.h has the rule; reference RegistrationVis.cpp:1078-1365 with the exact window instead of
the kd-tree's 32 checks) and of VWDictionaryHip::guidedWordIds.  The window is fp32 element-wise arithmetic -- NumPy rounds every operation,
which is rtflann's L2_Simple without fused multiply-add; the descriptor distances are the oracle's (oracle.dist_matrix), the bits lcd_knn2
returns.  Test infrastructure: nothing here is used by the product."""
import numpy as np

P2F, F2P = "projected_to_frame", "frame_to_projected"
RATIO, NEAREST = "ratio", "nearest"


def window_d2(q_pts, t_pts):
    """[nq x nt] fp32: fl(fl(dx * dx) + fl(dy * dy))"""
    q, t = np.asarray(q_pts, np.float32).reshape(-1, 2), np.asarray(t_pts, np.float32).reshape(-1, 2)
    with np.errstate(invalid="ignore", over="ignore"):
        dx = q[:, None, 0] - t[None, :, 0]
        dy = q[:, None, 1] - t[None, :, 1]
        return dx * dx + dy * dy


def window_d2_fused(q_pts, t_pts):
    """what a fused multiply-add would give: dx * dx + fl(dy * dy) evaluated exactly (float64 holds the sum of two fp32 products of this
    size) and rounded once"""
    q, t = np.asarray(q_pts, np.float32).reshape(-1, 2), np.asarray(t_pts, np.float32).reshape(-1, 2)
    dx = (q[:, None, 0] - t[None, :, 0]).astype(np.float64)
    dy = q[:, None, 1] - t[None, :, 1]
    return (dx * dx + (dy * dy).astype(np.float64)).astype(np.float32)


def windows(q_pts, t_pts, radius, chunk=1024):
    """[nq x nt] bool: d2 < radius * radius (fp32 product, strict; NaN is in no window)"""
    q = np.asarray(q_pts, np.float32).reshape(-1, 2)
    r2 = np.float32(radius) * np.float32(radius)
    out = np.zeros((q.shape[0], np.asarray(t_pts).reshape(-1, 2).shape[0]), bool)
    for i in range(0, q.shape[0], chunk):
        out[i:i + chunk] = window_d2(q[i:i + chunk], t_pts) < r2
    return out


def descriptor_dist(oracle, q_row, t_rows):
    """distances of one query row to the target rows, the engine's bits: squared L2 in the reference's order, Hamming over every byte"""
    return oracle.dist_matrix(np.ascontiguousarray(q_row.reshape(1, -1)), np.ascontiguousarray(t_rows),
                              metric=oracle.METRIC_HAMMING_CV if t_rows.dtype == np.uint8 else None)[0]


def guided_pair(oracle, frm, to, corners, corner_from_row, to_points, radius, nndr, nn_type=RATIO, direction=P2F):
    """-> dict(count, match, dist [nq x 2], owner [nt] or None): one pair by the rule of include/lcd.h.  A corner whose from-row is out of
    range is no candidate (lcd_match_guided_dev's treatment; lcd_match_guided refuses it)."""
    corners = np.asarray(corners, np.float32).reshape(-1, 2)
    to_points = np.asarray(to_points, np.float32).reshape(-1, 2)
    cfr = np.asarray(corner_from_row, np.int64).reshape(-1)
    nf, nt, nc = frm.shape[0], to.shape[0], corners.shape[0]
    ok = (cfr >= 0) & (cfr < nf)
    cpts = corners.copy()
    cpts[~ok] = np.nan
    cdesc = frm[np.where(ok, cfr, 0)] if nf else np.zeros((nc, to.shape[1]), to.dtype)
    if direction == P2F:
        q_pts, q_desc, t_pts, t_desc = cpts, cdesc, to_points, to
    else:
        q_pts, q_desc, t_pts, t_desc = to_points, to, cpts, cdesc
    nq = q_pts.shape[0]
    W = windows(q_pts, t_pts, radius)
    count = W.sum(axis=1).astype(np.int32)
    match = np.full(nq, -1, np.int32)
    dist = np.full((nq, 2), -1.0, np.float32)
    for q in range(nq):
        idx = np.flatnonzero(W[q])
        if idx.size == 1:
            match[q] = idx[0]
        elif idx.size >= 2:
            d = descriptor_dist(oracle, q_desc[q], t_desc[idx])
            order = np.argsort(d, kind="stable")                          # candidates ascend by index: the lowest index wins ties
            d1, d2 = np.float32(d[order[0]]), np.float32(d[order[1]])
            dist[q] = (d1, d2)
            if nn_type == NEAREST or d1 < np.float32(nndr) * d2:
                match[q] = idx[order[0]]
    owner = None
    if direction == P2F:
        owner = np.full(nt, -1, np.int32)
        for c in range(nq):                                               # addedWordsTo: first come, first served
            if match[c] >= 0 and owner[match[c]] < 0:
                owner[match[c]] = c
    return dict(count=count, match=match, dist=dist, owner=owner)


def guided_word_ids(n_from, corner_from_row, to_corner, original_from_ids=None, corner_count=None):
    """VWDictionaryHip::guidedWordIds: (from ids, to ids, projected ids).  to_corner = owner (projected-to-frame) or match
    (frame-to-projected) per to-row."""
    cfr = [int(x) for x in corner_from_row]
    orig = original_from_ids is not None and len(original_from_ids) > 0     # !orignalWordsFromIds.empty()
    ids = [int(x) for x in original_from_ids] if orig else list(range(n_from))
    new_to = max(ids) + 1 if orig else n_from
    to_ids = []
    for c in to_corner:
        if 0 <= c < len(cfr) and 0 <= cfr[c] < n_from:
            to_ids.append(ids[cfr[c]])
        else:
            to_ids.append(new_to)
            new_to += 1
    proj = [] if corner_count is None else [ids[cfr[c]] for c in range(len(cfr)) if corner_count[c] > 0 and 0 <= cfr[c] < n_from]
    return ids, to_ids, proj


def outcomes(res, direction):
    """the kinds of query in a result: {"empty", "single", "accepted", "rejected", "contested"}"""
    kinds = set()
    c, m = res["count"], res["match"]
    if (c == 0).any():
        kinds.add("empty")
    if (c == 1).any():
        kinds.add("single")
    if ((c >= 2) & (m >= 0)).any():
        kinds.add("accepted")
    if ((c >= 2) & (m < 0)).any():
        kinds.add("rejected")
    chosen = m[m >= 0]
    if chosen.size and np.unique(chosen).size < chosen.size:
        kinds.add("contested")                                            # a target chosen by two queries
    return kinds
