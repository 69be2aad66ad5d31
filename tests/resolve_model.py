"""The addNewWords decision loop in numpy (no GPU): what resolve_body.cuh must compute, and which of its routes each descriptor takes.

Inputs of both evaluations: the frame's two indexed neighbours per descriptor (`idx_id` [q, 2] word ids, 0 = invalid; `idx_d` [q, 2]
float32 distances, negative = invalid), the frame's self-distance matrix `sd` [q, q] float32, `nndr`, and `together`
(Kp/NewWordsComparedTogether).

sequential(): the reference's statements as resolve_kernels.hip cites them (VWDictionary.cpp:1089-1219), descriptor after descriptor:
  * the indexed candidates are pushed first, cut at the first invalid one (:1092-1137);
  * then the two nearest among the words that descriptors j < i of this call created, lowest j on equal distance (:1140-1160);
  * std::multimap<float, int>: equal keys keep insertion order (:1091);
  * new iff fewer than two candidates or c0.d > nndr * c1.d, the product rounded to float32 (:1163);
  * new words are numbered in descriptor order (:1185).
jacobi(): the evaluation the kernel performs -- candidate bits dist(j, i) < thr(i) (cand_threshold(), knn2_kernels.hip), sweep 0 from the
indexed candidates alone, then sweeps over the new-word mask until one changes nothing -- with the census of what each descriptor does on
the device: its candidate count cn, its route, the last sweep that changed its decision; per frame the sweeps, `straight`, fast / plain body.

Word ids: > 0 an indexed word, -(k + 1) the k-th new word of the frame (the device's encoding).

The switches are deliberately WRONG variants (tests/test_resolve_model.py shows that the designed inputs tell each from the rule):
  higher_j_on_ties     equal distances among same-frame words go to the higher j
  new_before_indexed   a same-frame word displaces an indexed candidate at equal distance
  nndr_ge              c0.d >= nndr * c1.d
  nonstrict_bit        candidate bit dist(j, i) <= thr(i)
  j_le_i               the bit row is masked to j <= i
  half_sweeps          at most q // 2 sweeps
A variant may change the census (cn, the winner c0) without changing a word id: where the rule makes the answer independent of it --
a same-frame word AT the second indexed distance, an equal-distance pair that the NNDR test rejects either way -- that is all there is
to see, and the census is what the test compares."""
import numpy as np

INF32 = np.float32(np.inf)
ROUTES = ("none", "list_1", "list_2", "list_3", "list_4", "bitrow_reg_hit", "bitrow_reg_skip", "bitrow_mem_hit", "bitrow_mem_skip")
FAST_MAX_Q = 1024                  # RBLOCK * KPT: resolve_body_fast up to here, resolve_body<NT> behind
REG_ROW_MAX_BW = 16                # bit rows of up to 16 words (512 descriptors) are kept in registers
LIST_MAX = 4                       # compact (j, distance) list entries per descriptor
STRAIGHT_MIN_Q = 8


def _valid(idx_id, idx_d, i, j):
    return idx_d[i, j] >= 0.0 and idx_id[i, j] != 0


def _push(c, d, cid, before_equal=False):
    """std::multimap insertion restricted to the two smallest entries (cand_push): an equal key goes BEHIND what is there"""
    pos = len(c)
    for k, (dk, _) in enumerate(c):
        if d < dk or (before_equal and d == dk):
            pos = k
            break
    c.insert(pos, (np.float32(d), cid))


def _indexed(idx_id, idx_d, i):
    c = []
    for j in range(2):
        if not _valid(idx_id, idx_d, i, j):
            break
        _push(c, idx_d[i, j], int(idx_id[i, j]))
    return c


def _is_new(c, nndr, ge=False):
    if len(c) < 2:
        return True
    rhs = np.float32(np.float32(nndr) * np.float32(c[1][0]))          # one float32 product, not contracted, not double
    return bool(c[0][0] >= rhs) if ge else bool(c[0][0] > rhs)


def _finish(reject, win):
    """new words numbered in descriptor order; a descriptor that matched a same-frame word takes that word's number"""
    rank = np.cumsum(reject) - 1
    ids = []
    for i in range(len(reject)):
        if reject[i]:
            ids.append(-(int(rank[i]) + 1))
        else:
            w = win[i]
            ids.append(w if w > 0 else -(int(rank[-w - 1]) + 1))
    return ids, int(np.sum(reject))


def sequential(idx_id, idx_d, sd, nndr, together=True):
    q = idx_id.shape[0]
    reject = np.zeros(q, bool)
    win = [0] * q
    for i in range(q):
        c = _indexed(idx_id, idx_d, i)
        if together:
            js = np.flatnonzero(reject[:i])
            for k in np.lexsort((js, sd[js, i]))[:2]:                  # by distance, then by j
                _push(c, sd[js[k], i], -(int(js[k]) + 1))
        reject[i] = _is_new(c, nndr)
        win[i] = c[0][1] if c else 0
    return _finish(reject, win)


def thresholds(idx_id, idx_d):
    """cand_threshold(): the second indexed neighbour's distance when both neighbours are valid, else +inf"""
    q = idx_id.shape[0]
    thr = np.full(q, INF32, np.float32)
    for i in range(q):
        if _valid(idx_id, idx_d, i, 0) and _valid(idx_id, idx_d, i, 1):
            thr[i] = idx_d[i, 1]
    return thr


def jacobi(idx_id, idx_d, sd, nndr, together=True, lists=True, higher_j_on_ties=False, new_before_indexed=False, nndr_ge=False,
           nonstrict_bit=False, j_le_i=False, half_sweeps=False):
    """-> (ids, n_new, census).  lists: the producer left compact lists and counts (the matrix-core filter's re-rank); without them every
    descriptor reads cn = 5 and walks its bit row."""
    q = idx_id.shape[0]
    thr = thresholds(idx_id, idx_d)
    sd = np.asarray(sd, np.float32)
    bits = (sd.T <= thr[:, None]) if nonstrict_bit else (sd.T < thr[:, None])           # bits[i, j] = dist(j, i) < thr(i)
    below = np.tri(q, q, 0 if j_le_i else -1, dtype=bool)                               # j < i
    row = bits & below
    cn = row.sum(axis=1).astype(int) if together else np.zeros(q, int)
    base = [_indexed(idx_id, idx_d, i) for i in range(q)]
    reject = np.array([_is_new(c, nndr, nndr_ge) for c in base], bool)                  # sweep 0
    win = [c[0][1] if c else 0 for c in base]
    last_change = np.zeros(q, int)
    hit = np.zeros(q, bool)
    sweeps = 0
    if together:
        members = [np.flatnonzero(row[i]) for i in range(q)]
        limit = q // 2 if half_sweeps else q + 1
        for sweep in range(1, limit + 1):
            sweeps = sweep
            nxt, nwin = reject.copy(), list(win)
            for i in range(q):
                if cn[i] == 0:
                    continue
                new = [(np.float32(sd[j, i]), (-j if higher_j_on_ties else j), j) for j in members[i] if reject[j]]
                c = list(base[i])
                if new:
                    hit[i] = True
                for d, _, j in sorted(new)[:2]:
                    _push(c, d, -(int(j) + 1), before_equal=new_before_indexed)
                nxt[i] = _is_new(c, nndr, nndr_ge)
                nwin[i] = c[0][1] if c else 0
            changed = nxt != reject
            last_change[changed] = sweep
            reject, win = nxt, nwin
            if not changed.any():
                break
    ids, n_new = _finish(reject, win)
    bw = (q + 63) // 64 * 2
    fast = q <= FAST_MAX_Q
    route = []
    for i in range(q):
        c = int(cn[i]) if (lists and fast) else (LIST_MAX + 1 if together else 0)
        if c == 0:
            route.append("none")
        elif c <= LIST_MAX:
            route.append("list_%d" % c)
        elif fast and bw <= REG_ROW_MAX_BW:
            route.append("bitrow_reg_hit" if hit[i] else "bitrow_reg_skip")
        else:
            route.append("bitrow_mem_hit" if hit[i] else "bitrow_mem_skip")
    census = dict(cn=cn, route=route, last_change=last_change, win=win, sweeps=sweeps, bw=bw, body="fast" if fast else "plain",
                  straight=bool(lists and together and fast and bw <= REG_ROW_MAX_BW and q >= STRAIGHT_MIN_Q))
    return ids, n_new, census


# ------------------------------------------------------------------------------------------------ the model's inputs from rows
_POPCOUNT = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(axis=1).astype(np.uint8)


def distances(a, b, hamming=False):
    """exact distances [len(a), len(b)] as float32: squared L2 of integer coordinates (every partial sum an integer below 2^24, so any
    summation order gives these bits) or Hamming distance of byte rows"""
    if hamming:
        return _POPCOUNT[np.bitwise_xor(a[:, None, :], b[None, :, :])].sum(axis=2, dtype=np.int64).astype(np.float32)
    a64, b64 = a.astype(np.int64), b.astype(np.int64)
    d = (a64 * a64).sum(1)[:, None] + (b64 * b64).sum(1)[None, :] - 2 * (a64 @ b64.T)
    return d.astype(np.float32)


def neighbours(vocab, ids, frame, hamming=False):
    """the two nearest indexed words of every descriptor, ties to the lower row; no search below two live words (VWDictionary.cpp:1015)"""
    q = frame.shape[0]
    idx_id, idx_d = np.zeros((q, 2), np.int32), np.full((q, 2), -1.0, np.float32)
    if vocab.shape[0] >= 2 and q:
        d = distances(frame, vocab, hamming)
        order = np.lexsort((np.broadcast_to(np.arange(vocab.shape[0]), d.shape), d), axis=1)[:, :2]
        idx_id = np.asarray(ids, np.int32)[order]
        idx_d = np.take_along_axis(d, order, axis=1)
    return idx_id, idx_d


def model_inputs(vocab, ids, frame, hamming=False):
    idx_id, idx_d = neighbours(vocab, ids, frame, hamming)
    return idx_id, idx_d, distances(frame, frame, hamming)
