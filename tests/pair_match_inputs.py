"""Inputs of the pair matcher's shape tests (tests/test_gpu_pair_match_shapes.py), NumPy only, and the properties each input is there
for, stated over the MODEL's output (pair_match_model over the oracle): tests/test_pair_match_inputs.py asserts them without a GPU, the
GPU file asserts them again on the expected output it compares the engine with.

An input that lacks its property is replaced by the next seed (first_seed), never skipped; the number of seeds is capped."""
import numpy as np

import pair_match_model as M

RBLOCK = 1024                                                  # threads of pair_match_kernel's one workgroup per pair (resolve_body.cuh)
LARGE_SIZES = [(1000, 1000), (1025, 1023), (2049, 1100), (1030, 2050)]
LIMIT_SIZES = [(8192, 40), (40, 8192)]                         # MAX_SIDE: the decision loop's LDS masks are full
RATIO_SIZES = [(300, 260), (1025, 1023)]
RATIOS = [0.0, 0.6, 0.8, 1.0]
SEED_CAP = 20


# ---------------------------------------------------------------------------------------------------------------- rows
def fresh(rng, dtype, dim, n):
    """n fresh descriptors: unit-norm Gaussian floats or uniform random bytes"""
    if dtype == "u8":
        return rng.integers(0, 256, (n, dim), dtype=np.uint8)
    v = rng.standard_normal((n, dim)).astype(np.float32)
    if n:
        v /= np.linalg.norm(v, axis=1, keepdims=True)
    return np.ascontiguousarray(v, np.float32)


def noisy(rng, rows):
    """what a detector gives at the same place again: sigma 0.02 per component, renormalised (float); 2 % of the bits flipped (binary)"""
    out = rows.copy()
    if out.shape[0] == 0:
        return out
    if out.dtype == np.uint8:
        out ^= np.packbits(rng.random((out.shape[0], out.shape[1] * 8)) < 0.02, axis=1)
        return out
    out += rng.standard_normal(out.shape).astype(np.float32) * np.float32(0.02)
    out /= np.linalg.norm(out, axis=1, keepdims=True)
    return out


def interleaved_pair(dtype, dim, nf, nt, seed):
    """`from`: nf // 2 fresh rows and noisy copies of them, SHUFFLED; `to`: half noisy copies of from-rows, one eighth noisy copies of other
    to-rows, the rest fresh, SHUFFLED.  Rows that belong together lie anywhere in their frame, on both sides of every multiple of the
    workgroup's width -- and copies WITHIN a frame are what makes rows of one frame share a word at all (random 256-bit rows never do)."""
    rng = np.random.default_rng(seed)
    nb = nf // 2 if nf >= 2 else nf
    base = fresh(rng, dtype, dim, nb)
    frm = np.concatenate([base, noisy(rng, base[rng.integers(0, max(nb, 1), nf - nb)])])[rng.permutation(nf)]
    n_copy = nt // 2 if nf else 0
    n_self = nt // 8
    first = np.concatenate([noisy(rng, frm[rng.integers(0, max(nf, 1), n_copy)]), fresh(rng, dtype, dim, nt - n_copy - n_self)])
    to = np.concatenate([first, noisy(rng, first[rng.integers(0, max(first.shape[0], 1), n_self)])])[rng.permutation(nt)] if nt else first
    return np.ascontiguousarray(frm), np.ascontiguousarray(to)


def plant_duplicates(frm, to, seed, n=6, boundary=None):
    """Exact duplicates at random places: n times from[b] = from[a] and to[i] = from[a] (a to-row with two from-rows at distance 0),
    n times to[i2] = to[i1].  With `boundary`, a < boundary <= b: the tie lies across it.  Returns (from, to, [(a, b, i), ...])."""
    rng = np.random.default_rng(seed)
    frm, to = frm.copy(), to.copy()
    nf, nt = frm.shape[0], to.shape[0]
    assert nf >= 4 * n and nt >= 4 * n and (boundary is None or n <= boundary <= nf - n)
    if boundary is None:
        p = rng.permutation(nf)[: 2 * n]
        a, b = np.minimum(p[:n], p[n:]), np.maximum(p[:n], p[n:])
    else:
        a, b = rng.permutation(boundary)[:n], boundary + rng.permutation(nf - boundary)[:n]
    rows = rng.permutation(nt)[: 3 * n]
    i, i1, i2 = rows[:n], rows[n:2 * n], rows[2 * n:]
    frm[b] = frm[a]
    to[i2] = to[i1]
    to[i] = frm[a]
    return np.ascontiguousarray(frm), np.ascontiguousarray(to), list(zip(a.tolist(), b.tolist(), i.tolist()))


def graded(rng, a, b):
    """rows on the way from rows `a` to rows `b`, 30 % to 50 % of it: distance to a / distance to b spreads over (3/7)^2 .. 1 (squared L2)
    or 3/7 .. 1 (Hamming) -- the rows a ratio test decides differently at different ratios (a noisy copy passes all of them, a fresh row none)"""
    t = rng.uniform(0.3, 0.5, (a.shape[0], 1))
    if a.dtype == np.uint8:
        return a ^ ((a ^ b) & np.packbits(rng.random((a.shape[0], a.shape[1] * 8)) < t, axis=1))
    return (a + t.astype(np.float32) * (b - a)).astype(np.float32)


def with_graded_rows(frm, to, seed):
    """a quarter of the to-rows, and an eighth of the from-rows (in the frame's second half), replaced by graded() mixes of two from-rows"""
    rng = np.random.default_rng(seed)
    frm, to = frm.copy(), to.copy()
    nf, nt = frm.shape[0], to.shape[0]
    rows = nf // 2 + rng.permutation(nf - nf // 2)[: nf // 8]
    frm[rows] = graded(rng, frm[rng.integers(0, nf // 2, rows.size)], frm[rng.integers(0, nf // 2, rows.size)])
    rows = rng.permutation(nt)[: nt // 4]
    to[rows] = graded(rng, frm[rng.integers(0, nf, rows.size)], frm[rng.integers(0, nf, rows.size)])
    return np.ascontiguousarray(frm), np.ascontiguousarray(to)


def integer_pair(dim, nf, nt, seed):
    """f32 rows with entries 0..3, as an unnormalised histogram descriptor (raw SIFT) has them: every distance is a small integer, so
    best and second-best tie exactly all the time and nndr * d is a product of exactly representable values; plus exact duplicates on
    both sides and rows that differ from another by +-1 in three places"""
    rng = np.random.default_rng(seed)
    frm = rng.integers(0, 4, (nf, dim)).astype(np.float32)
    to = rng.integers(0, 4, (nt, dim)).astype(np.float32)

    def nudged(rows):
        out = rows.copy()
        for r in out:
            c = rng.permutation(dim)[:3]
            r[c] += np.where(r[c] == 0, 1, rng.choice([-1, 1], 3)).astype(np.float32)
        return out

    if nf >= 8:
        frm[nf // 2] = frm[1]                                             # duplicates inside `from`
        frm[nf - 1] = frm[2]
        frm[nf // 3:nf // 3 + 2] = nudged(frm[3:5])
    if nf >= 8 and nt >= 12:
        k = nt // 4
        to[:k] = nudged(frm[rng.integers(0, nf, k)])                      # near a from-row
        to[k:k + 3] = frm[[1, 2, 5]]                                      # equal to a from-row (rows 1 and 2 exist twice)
        to[nt - 1] = to[k + 4]                                            # duplicates inside `to`
        to[nt - 2] = nudged(to[k + 5:k + 6])[0]
    assert frm.min() >= 0 and to.min() >= 0
    return np.ascontiguousarray(frm), np.ascontiguousarray(to)


def collapsing_pair(dtype, dim, k, nf, nt):
    """`from`: k distinct rows, nf rows in all (0, 1, .., k - 1, 0, 1, ..): compared together the frame collapses into max(k, 2) words (a
    second row is a word whatever it is: it meets one candidate only), apart it is nf words of which only k differ.  `to`: the k rows,
    noisy copies of them, fresh rows."""
    rng = np.random.default_rng(1009 * k + 31 * dim + nf)
    base = fresh(rng, dtype, dim, k)
    frm = base[np.arange(nf) % k]
    n_copy = (nt - k) // 2
    to = np.concatenate([base, noisy(rng, base[rng.integers(0, k, n_copy)]), fresh(rng, dtype, dim, nt - k - n_copy)])[rng.permutation(nt)]
    return np.ascontiguousarray(frm), np.ascontiguousarray(to)


def kernel_case_pairs(dtype, dim):
    """what every handle of the distance-kernel case is given: (33, 65) and (65, 31) cross TILE_A = 32 and TILE_B = 64 in both roles; one
    from-row with three copies of it (no index); the duplicate pattern of tests/test_gpu_pair_match.py (best and second-best both 0)"""
    rng = np.random.default_rng(4000 + dim + 500 * (dtype == "u8"))
    one = fresh(rng, dtype, dim, 1)
    b = fresh(rng, dtype, dim, 9)
    return [interleaved_pair(dtype, dim, 33, 65, 4100 + dim), interleaved_pair(dtype, dim, 65, 31, 4200 + dim),
            (one, np.ascontiguousarray(np.repeat(one, 3, axis=0))),
            (np.ascontiguousarray(b[[0, 1, 0, 2, 1, 3, 0, 4]]), np.ascontiguousarray(b[[0, 0, 5, 5, 1, 6, 2, 2, 2, 7, 5]]))]


def many_small_pairs(dtype, dim, n_pairs, seed):
    """n_pairs pairs with 0..40 rows on each side; pair 3 has no from-rows, pair 5 no to-rows, pair 7 neither"""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(0, 41, (n_pairs, 2))
    assert n_pairs > 7
    sizes[3, 0] = 0
    sizes[5, 1] = 0
    sizes[7] = 0
    sizes[[3, 5], [1, 0]] = np.maximum(sizes[[3, 5], [1, 0]], 1)
    return [interleaved_pair(dtype, dim, int(nf), int(nt), seed + 1 + p) for p, (nf, nt) in enumerate(sizes)]


# ---------------------------------------------------------------------------------------------------------------- properties
def first_seed(build, ok, seed0, cap=SEED_CAP):
    """build(seed) for seed0, seed0 + 1, ..: the first input for which ok(input) holds; fails when `cap` seeds gave none"""
    for seed in range(seed0, seed0 + cap):
        x = build(seed)
        if ok(x):
            return x
    raise AssertionError("no input with the wanted property among %d seeds from %d" % (cap, seed0))


def shared_across(ids, b):
    """number of row pairs (i < b <= j) with the same word"""
    lo_w, lo_n = np.unique(ids[:b], return_counts=True)
    hi_w, hi_n = np.unique(ids[b:], return_counts=True)
    _, i, j = np.intersect1d(lo_w, hi_w, return_indices=True)
    return int((lo_n[i] * hi_n[j]).sum())


TOOK_FROM_WORD, CREATED, TOOK_TO_WORD = 0, 1, 2


def to_classes(ef, et):
    """per to-row of a dictionary result: it took a word of the from-frame, created one, or took one that an EARLIER to-row created"""
    cls = np.full(et.shape[0], TOOK_TO_WORD, np.int8)
    cls[np.unique(et, return_index=True)[1]] = CREATED                       # first occurrence of an id
    cls[np.isin(et, ef)] = TOOK_FROM_WORD
    return cls


def spans_boundaries(ef, et):
    """The "together" result of a large pair reaches across every multiple of RBLOCK that a side passes.  Across row 1024: from-rows on
    both sides share words, and the to-rows on EACH side contain all three classes.  Across row 2048 the sizes of the tests leave one or
    two rows behind the boundary, which cannot hold three classes: there, the from-rows share a word across it as well, the to-rows in
    front of it hold all three classes and a to-row behind it takes a word that existed before it (from either frame)."""
    nf, nt = ef.shape[0], et.shape[0]
    cls = to_classes(ef, et)
    for b in range(RBLOCK, max(nf, nt), RBLOCK):
        if nf > b and shared_across(ef, b) == 0:
            return False
        if nt > b:
            if len(set(cls[:b].tolist())) < 3:
                return False
            behind = set(cls[b:].tolist())
            if (len(behind) < 3) if nt - b >= 16 else not (behind - {CREATED}):
                return False
    return True


def cross_spans_boundaries(m, nf):
    """a cross-check result keeps and drops to-rows on both sides of row 1024, and matches from-rows on both sides of it (where there are such)"""
    nt = m.shape[0]
    if nf > RBLOCK and not ((m >= RBLOCK).any() and ((m >= 0) & (m < RBLOCK)).any()):
        return False
    for part in ([m[:RBLOCK], m[RBLOCK:]] if nt > RBLOCK else [m]):
        if not ((part >= 0).any() and (part < 0).any()):
            return False
    return True


def _key(dtype, dim, nf, nt):
    return 7000 + 1000 * (dtype == "u8") + 13 * nf + 7 * nt + dim


_large = {}


def large_pair(oracle, dtype, dim, nf, nt):
    """interleaved_pair at a size past one workgroup's width whose "together" result spans the boundaries -> (from, to, that result)"""
    k = (dtype, dim, nf, nt)
    if k not in _large:
        def build(seed):
            f, t = interleaved_pair(dtype, dim, nf, nt, seed)
            return f, t, M.dictionary_pair(oracle, f, t, 0.8, True)
        _large[k] = first_seed(build, lambda x: spans_boundaries(*x[2]), _key(*k))
    return _large[k]


_given = {}


def given_ids_pair(oracle, dtype, dim, nf=2049, nt=1100):
    """the large pair with eight exact duplicates ACROSS row 1024 of `from`, each met by a to-row, and sparse unsorted ids: the vocabulary
    is in ascending id, so the twin with the lower id wins wherever it lies -> (from, to, ids, [(a, b, to-row)], model result).  Both
    orders occur among the eight."""
    k = (dtype, dim, nf, nt)
    if k not in _given:
        def build(seed):
            f, t, _ = large_pair(oracle, dtype, dim, nf, nt)
            f, t, triples = plant_duplicates(f, t, seed, 8, RBLOCK)
            ids = np.random.default_rng(seed + 1).permutation(np.arange(3, 3 + 9973 * nf, 9973))[:nf].astype(np.int32)
            return f, t, ids, triples, M.dictionary_pair(oracle, f, t, 0.8, True, from_word_ids=ids)
        _given[k] = first_seed(build, lambda x: len({bool(x[2][b] < x[2][a]) for a, b, _ in x[3]}) == 2, _key(*k) + 300)
    return _given[k]


def dist(oracle, to, frm):
    """D[to-row][from-row] with the engine's bits: squared L2 in the reference's order, Hamming over EVERY byte (cv::NORM_HAMMING)"""
    if to.shape[0] == 0 or frm.shape[0] == 0:
        return np.zeros((to.shape[0], frm.shape[0]), np.float32)
    return oracle.dist_matrix(to, frm, metric=oracle.METRIC_HAMMING_CV if to.dtype == np.uint8 else None)


_ties = {}


def tie_pair(oracle, dtype, dim, nf, nt):
    """the cross-check's large input: an interleaved pair with exact duplicates (across row 1024 of `from` where twelve rows or more lie
    behind it), so that the lower-index rule decides in both directions, and near copies of from-rows behind row 1024; kept and dropped
    matches on both sides of row 1024 of `to`, matched from-rows on both sides of row 1024 -> (from, to, D, (match, dist))"""
    k = (dtype, dim, nf, nt)
    if k not in _ties:
        def build(seed):
            f, t = interleaved_pair(dtype, dim, nf, nt, seed)
            f, t, trip = plant_duplicates(f, t, seed + 1, 6, RBLOCK if nf >= RBLOCK + 12 else None)
            if nf > RBLOCK:                                               # near copies of from-rows behind row 1024 (not of the planted twins)
                rng = np.random.default_rng(seed + 2)
                r = np.setdiff1d(np.arange(RBLOCK, nf), [b for _, b, _ in trip])[:6]
                t[rng.permutation(nt)[: r.size]] = noisy(rng, f[r])
            D = dist(oracle, t, f)
            return f, t, D, M.cross_check(D)
        _ties[k] = first_seed(build, lambda x: M.tie_resolved_by_index(x[2]) and cross_spans_boundaries(x[3][0], nf), _key(*k) + 500)
    return _ties[k]


def duplicate_rows(frm, to):
    """(from-rows equal to an earlier from-row, to-rows equal to a from-row or to an earlier to-row)"""
    def codes(a):
        return np.unique(np.ascontiguousarray(a).view(np.uint8).reshape(a.shape[0], -1), axis=0, return_inverse=True)[1].reshape(-1)
    c = codes(np.concatenate([frm, to]))
    cf, ct = c[: frm.shape[0]], c[frm.shape[0]:]
    dup_f = np.ones(cf.shape[0], bool)
    dup_f[np.unique(cf, return_index=True)[1]] = False
    dup_t = np.ones(ct.shape[0], bool)
    dup_t[np.unique(ct, return_index=True)[1]] = False
    return dup_f, dup_t | np.isin(ct, cf)


_ratio = {}


def ratio_pair(oracle, dtype, dim, nf, nt):
    """an interleaved pair with graded rows and planted exact duplicates whose results under the four ratios differ pairwise, in both ways of comparing
    new words -> (from, to, {(nndr, compared): (from ids, to ids)})"""
    k = (dtype, dim, nf, nt)
    if k not in _ratio:
        def build(seed):
            f, t = with_graded_rows(*interleaved_pair(dtype, dim, nf, nt, seed), seed + 2)
            f, t, _ = plant_duplicates(f, t, seed + 1, 6)
            return f, t, {(r, c): M.dictionary_pair(oracle, f, t, r, c) for r in RATIOS for c in (True, False)}
        _ratio[k] = first_seed(build, lambda x: ratios_tell_apart(*x), _key(*k) + 900)
    return _ratio[k]


def ratios_tell_apart(frm, to, exp):
    """what the four ratios are there for: different results under each of them; at 0.0 only an exact duplicate can match (and some do); at
    1.0 only "fewer than two candidates" rejects: compared together the from-frame is exactly two words and no to-row is new"""
    dup_f, dup_t = duplicate_rows(frm, to)
    for c in (True, False):
        cat = [np.concatenate(exp[(r, c)]) for r in RATIOS]
        if any(np.array_equal(cat[i], cat[j]) for i in range(4) for j in range(i)):
            return False
        ef, et = exp[(0.0, c)]
        new_f = np.zeros(ef.shape[0], bool)
        new_f[np.unique(ef, return_index=True)[1]] = True
        new_t = to_classes(ef, et) == CREATED
        if not (new_f[~dup_f].all() and new_t[~dup_t].all() and not new_t.all() and (c is False or not new_f.all())):
            return False
    ef, et = exp[(1.0, True)]
    return np.unique(ef).tolist() == [1, 2] and np.isin(et, [1, 2]).all()
