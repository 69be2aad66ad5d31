"""Designed frames for the addNewWords decision loop (resolve_body.cuh): each generator returns (vocab, ids, frame, nndr) and
tests/test_resolve_inputs.py proves with tests/resolve_model.py which route, sweep and seam it reaches.

Every coordinate is a small integer (|x| <= 10: exact as bf16 and fp16 operand), so every squared distance and every partial sum of one
is an integer far below 2^24 -- the same bits in any summation order: the oracle's, the exact scan's, the self-distance kernels', the
matrix-core filters'.  That is what makes the model's census a statement about the device.

Geometry (64 floats; the 128-float handle pads with zeros).  Coordinates 16..63 carry 96 GROUP centres +-10 e_a, pairwise 200 or 400 apart.
A group is three vocabulary rows c, c + 4 e_0, c + 6 e_1 (16, 36 and 52 apart).  Coordinates 2..15 are zero in every group row, so a
descriptor row + x with x in those coordinates is |x|^2 farther from every row of the vocabulary than `row` is: the order and the gaps of its
indexed neighbours stay what they are.
  * a SITE c + 9 e_k (k in 2..7) sees its group at 81, 97, 117: rejected by the NNDR test at 0.8 and at 0.5, with the candidate threshold at 97 --
    "far from every indexed word" with three certified neighbours.  Designed descriptors are a site plus local coordinates in 8..15;
  * filler descriptors (cn == 0): row +- 6 e_(8 + t) matches its row (36 against 52 or 72) and is at least its threshold away from every other
    one; centre +- 9 e_k is an isolated new word (threshold 97, the nearest other descriptor at 117);
  * twelve hand-placed words around the sites of group 5 give the NNDR test its exact 2 : 4, 3 : 4, 4 : 5 and 7 : 10.
Groups 0..7 are kept for the designed pieces, the filler descriptors use groups 8..95.  The vocabulary is the 12 hand-placed words followed by the 288
group rows, ids 1..300; cut to its first 200 rows it is below the matrix-core filter's 256 and every mode runs the exact scan."""
import functools

import numpy as np

DIM = 64
N_GROUPS = 96
N_HAND = 12
N_ROWS = N_HAND + 3 * N_GROUPS
FILL_GROUP0 = 8
MAX_ABS = 10                                   # asserted by the test: the largest coordinate


def e(k, v=1):
    x = np.zeros(DIM, np.int64)
    x[k] = v
    return x


def centre(g):
    return e(16 + g // 2, 10 if g % 2 == 0 else -10)


def group_rows(g):
    c = centre(g)
    return [c, c + e(0, 4), c + e(1, 6)]


def site(g, k=0, sign=1):
    return centre(g) + e(2 + k, 9 * sign)


def _hand_words():
    s = [site(5, k) for k in range(6)]
    return [s[0] + e(8) + e(9), s[0] + e(10, 2),                                   # 2 and 4 from site 0
            s[1] + e(8) + e(9) + e(10), s[1] + e(11, 2),                           # 3 and 4 from site 1
            s[2] + e(8) + e(9), s[2] + e(10, 2) + e(11, 3),                        # 2 and 13 from site 2; 6 and 9 from site 2 + 2 e_10
            s[3] + e(8) + e(9) + e(10), s[3] + e(11, 2) + e(12, 3),                # 3 and 13 from site 3; 7 and 9 from site 3 + 2 e_11
            s[4] + e(8, 2), s[4] + e(9, 2) + e(10),                                # 4 and 5 from site 4
            s[5] + e(8, 2) + e(9) + e(10) + e(11), s[5] + e(12, 3) + e(13)]        # 7 and 10 from site 5


def _f32(rows):
    return np.ascontiguousarray(np.array(rows, np.int64).reshape(-1, DIM), dtype=np.float32)


@functools.lru_cache(maxsize=None)
def _vocab_all():
    rows = _hand_words()
    for g in range(N_GROUPS):
        rows += group_rows(g)
    v = _f32(rows)
    v.setflags(write=False)
    return v


def vocabulary(n_rows=N_ROWS):
    """-> (rows [n_rows, 64] float32, ids 1..n_rows); read-only, shared"""
    ids = np.arange(1, n_rows + 1, dtype=np.int32)
    ids.setflags(write=False)
    return _vocab_all()[:n_rows], ids


@functools.lru_cache(maxsize=None)
def vocabulary_with_identical_rows():
    """rows 150..190 (41 group rows the designed pieces never touch) become copies of group 6's centre: 42 identical rows, more than a
    row block keeps -- no query near them can be certified"""
    v = _vocab_all().copy()
    v[150:191] = _f32([centre(6)])
    v.setflags(write=False)
    return v


# ------------------------------------------------------------------------------------------------ filler descriptors, cn == 0
@functools.lru_cache(maxsize=None)
def _fill_lists():
    matched, isolated = [], []
    for s in (1, -1):
        for t in range(3):
            for g in range(FILL_GROUP0, N_GROUPS):
                matched.append(group_rows(g)[t] + e(8 + t, 6 * s))
    for s in (1, -1):
        for k in range(6):
            for g in range(FILL_GROUP0, N_GROUPS):
                isolated.append(centre(g) + e(2 + k, 9 * s))
    return matched, isolated


def fill(n):
    """n descriptors without a same-frame candidate: alternately one that matches an indexed word and one isolated new word"""
    matched, isolated = _fill_lists()
    assert n <= 2 * len(matched)
    return [(matched if i % 2 == 0 else isolated)[i // 2] for i in range(n)]


def place(q, pieces):
    """a frame of q descriptors: the blocks of `pieces` [(first position, rows)] where they say, filler descriptors everywhere else"""
    out = [None] * q
    for pos, rows in pieces:
        for k, r in enumerate(rows):
            assert out[pos + k] is None
            out[pos + k] = r
    rest = iter(fill(sum(1 for r in out if r is None)))
    return [r if r is not None else next(rest) for r in out]


def _input(rows, nndr=0.8, n_rows=N_ROWS, vocab=None):
    v, ids = vocabulary(n_rows)
    if vocab is not None:
        v = vocab
    return v, ids, _f32(rows), nndr


# ------------------------------------------------------------------------------------------------ the designed pieces
@functools.lru_cache(maxsize=None)
def snake(k, n=8):
    """k vertices of the n-cube on an induced path: consecutive vertices differ in one coordinate, all other pairs in at least two (depth-first
    search, deterministic)"""
    path, used = [0], {0}

    def ok(v):
        return v not in used and sum(1 for b in range(n) if (v ^ (1 << b)) in used) == 1

    def grow():
        if len(path) == k:
            return True
        for b in range(n):
            v = path[-1] ^ (1 << b)
            if ok(v):
                path.append(v); used.add(v)
                if grow():
                    return True
                path.pop(); used.discard(v)
        return False

    assert grow()
    return tuple(path)


def chain_rows(k, g=0):
    """site + (+-7 in each of the coordinates 8..15) along a snake: every vertex is 392 from the site, a step is 196, two steps 392.  The site's
    group is at 473, 489, 509.  Behind a new word the next descriptor matches it (196 <= 0.8 * 392); behind a matched one the nearest new word is
    two steps back and 392 > 0.8 * 473 makes the descriptor new: the sequential answer alternates, and the Jacobi evaluation settles one descriptor
    per sweep."""
    out = []
    for v in snake(k):
        x = site(g)
        for b in range(8):
            x = x + e(8 + b, 7 if (v >> b) & 1 else -7)
        out.append(x)
    return out


def cluster_rows(m, g=2):
    """site, site + e_8, site + e_9, ..., then site - e_8, ...: the first is new, every other one is 1 from it and 2 or 4 from the rest; the
    i-th has i candidates"""
    assert m <= 17
    out = [site(g)]
    for i in range(1, m):
        out.append(site(g) + e(8 + (i - 1) % 8, 1 if i <= 8 else -1))
    return out


def popular_rows(c, g=1):
    """copies of group g's centre, each one unit off in one coordinate: 1 from their word, 17 from its neighbour, 2 or 4 from each other"""
    steps = [(k, s) for k in range(2, 16) for s in (1, -1)] + [(k, 1) for k in range(20, 64)]
    assert c <= len(steps)
    return [centre(g) + e(k, s) for k, s in steps[:c]]


def chain(k, q=None):
    """k = q: the chain alone; else the chain at the end of a frame of q descriptors"""
    return _input(chain_rows(k) if q is None else place(q, [(q - k, chain_rows(k))]))


def cluster(m):
    return _input(cluster_rows(m))


def popular(c, q=None):
    return _input(popular_rows(c) if q is None else place(q, [(q - c, popular_rows(c))]))


def later_only():
    """descriptor 0 matches its word (49 against 65); the two behind it are new words 4 and 8 away from it -- inside its threshold, above it in the frame"""
    c = centre(3)
    return _input([c + e(8, 7), c + e(8, 9), c + e(8, 9) + e(9, 2)])


def ties(case):
    if case == "lower_j":
        # no vocabulary, nndr = 1: descriptors 0 and 1 are new (fewer than two candidates); 2 and 3 are 8 from both and go to the lower j
        v, ids, frame, _ = _input([e(8, 2), e(8, -2), e(9, 2), e(9, -2), e(8, 2) + e(9)], n_rows=0)
        return v, ids, frame, 1.0
    c = centre(4)
    if case == "indexed_first":
        # X = c + 7 e_8: 49 from its word, 65 from the next.  N (new: 98 against 114) is 49 from X: the indexed word stays c0, 49 > 0.8 * 49: X is new
        return _input([c + e(8, 7) + e(9, 7), c + e(8, 7)])
    if case == "second_excluded":
        # N (new: 114 against 130) is exactly 65 from X: no candidate bit, and X matches its word as it does alone
        return _input([c + e(8, 7) + e(9, 8) + e(10), c + e(8, 7)])
    raise ValueError(case)


def nndr_edge(case):
    s = [site(5, k) for k in range(6)]
    if case == "half":
        # 2 : 4 accepted at equality, 3 : 4 rejected -- c1 an indexed word (sites 0, 1), c1 a same-frame new word (sites 2, 3)
        return _input([s[0], s[1], s[2] + e(10, 2), s[2], s[3] + e(11, 2), s[3]], nndr=0.5)
    if case == "point8":
        return _input([s[4]], nndr=0.8)              # 4 against float32(0.8f * 5) = 4: accepted
    if case == "point7":
        return _input([s[5]], nndr=0.7)              # 7 against float32(0.7f * 10) = 7: accepted; the exact product 6.99999988 would reject
    raise ValueError(case)


EMPTY_FRAMES = {"chain": lambda: chain_rows(40), "cluster": lambda: cluster_rows(7), "popular": lambda: popular_rows(40),
                "later_only": lambda: [r for r in later_only()[2].astype(np.int64)]}


def empty_dictionary(frame, n_words):
    """a designed frame against no vocabulary (n_words = 0) or one live word (n_words = 1): no indexed search, every candidate bit set"""
    return _input(EMPTY_FRAMES[frame](), n_rows=n_words)


SEAMS = (32, 64, 256, 512, 1024)


def seams(b, pattern):
    """the pattern with descriptors on either side of position b - 1 | b, in a frame of b + 16"""
    q = b + 16
    if pattern == "cluster":
        rows = cluster_rows(6)
        return _input(place(q, [(b - 1, rows[:1]), (b, rows[1:3]), (b + 8, rows[3:])]))   # the new word below the seam, its matches above it
    if pattern == "chain":
        return _input(place(q, [(b - 3, chain_rows(6))]))
    if pattern == "ties":
        c = centre(4)
        return _input(place(q, [(b - 1, [c + e(8, 7) + e(9, 7)]), (b, [c + e(8, 7)])]))
    raise ValueError(pattern)


SIZES = (1, 7, 8, 64, 65, 512, 513, 1024, 1025)


def sizes(q):
    """q >= 64: a cluster of 10 from position 3 and a chain of 8 at the end, filler descriptors between them.  Below that the frame holds what fits: one isolated
    descriptor; a cluster of 6 and one filler; a chain of 8."""
    if q == 1:
        return _input(fill(2)[1:])
    if q == 7:
        return _input(cluster_rows(6) + fill(1))
    if q == 8:
        return _input(chain_rows(8))
    return _input(place(q, [(3, cluster_rows(10)), (q - 8, chain_rows(8))]))


def redo():
    """a cluster on the run of identical rows: 9 (10) from 42 rows at once, nothing to certify -- every one of the seven goes to the exact redo, which
    must leave the same candidate bits, lists and counts as the re-rank would have"""
    x = centre(6) + e(8, 3)
    rows = [x] + [x + e(9 + i) for i in range(6)]
    return _input(place(16, [(4, rows)]), vocab=vocabulary_with_identical_rows())


def all_inputs():
    """name -> generator of every input the CPU proofs and the GPU test run"""
    out = {"chain40": lambda: chain(40), "chain20_in_513": lambda: chain(20, 513), "chain20_in_1025": lambda: chain(20, 1025)}
    for m in range(2, 8):
        out["cluster%d" % m] = functools.partial(cluster, m)
    out["popular40"] = lambda: popular(40)
    out["popular40_in_600"] = lambda: popular(40, 600)
    out["later_only"] = later_only
    for c in ("lower_j", "indexed_first", "second_excluded"):
        out["ties_" + c] = functools.partial(ties, c)
    for c in ("half", "point8", "point7"):
        out["nndr_" + c] = functools.partial(nndr_edge, c)
    for f in EMPTY_FRAMES:
        for n in (0, 1):
            out["empty%d_%s" % (n, f)] = functools.partial(empty_dictionary, f, n)
    for b in SEAMS:
        for p in ("cluster", "chain", "ties"):
            out["seam%d_%s" % (b, p)] = functools.partial(seams, b, p)
    for q in SIZES:
        out["size%d" % q] = functools.partial(sizes, q)
    return out


def widen(rows, dim):
    """the same rows as `dim` floats, zeros behind the 64: every distance is unchanged"""
    out = np.zeros((rows.shape[0], dim), np.float32)
    out[:, :DIM] = rows
    return out


# ================================================================================================ Hamming analogues (u8 handles, 32 bytes)
# Hamming distances are integers on every path, so nothing has to be certified and the filler may be random.  One anchor pair carries the designed
# pieces: word A and word A2 = A with bits 200 and 201 flipped.  A descriptor A ^ F, F a set of f bits below 200, has A at f and A2 at f + 2 (every
# other row of the vocabulary is a random code, ~128 away): it matches A iff f <= 0.8 (f + 2), i.e. f <= 8, and its candidate threshold is f + 2.
U8_BYTES = 32
_U8_SEED = 20240611


def _bits(positions):
    x = np.zeros(U8_BYTES, np.uint8)
    for p in positions:
        x[p >> 3] ^= np.uint8(1 << (p & 7))
    return x


@functools.lru_cache(maxsize=None)
def _u8_codes():
    """random codes: [0] the anchor A, [1..4] the centres of the four NNDR pairs, [5..] filler rows"""
    rng = np.random.default_rng(_U8_SEED)
    c = rng.integers(0, 256, (N_ROWS, U8_BYTES), dtype=np.uint8)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _u8_vocab_all():
    c = _u8_codes()
    a, (b0, b1, b2, b3) = c[0], c[1:5]
    hand = [a, a ^ _bits([200, 201]),
            b0 ^ _bits([0, 1]), b0 ^ _bits([2, 3, 4, 5]),                            # 2 and 4 from b0
            b1 ^ _bits([0, 1, 2]), b1 ^ _bits([3, 4, 5, 6]),                         # 3 and 4 from b1
            b2 ^ _bits([0, 1]), b2 ^ _bits(range(2, 15)),                            # 2 and 13 from b2; 6 and 9 from b2 ^ bits 2..5
            b3 ^ _bits([0, 1, 2]), b3 ^ _bits(range(3, 16))]                         # 3 and 13 from b3; 7 and 9 from b3 ^ bits 3..6
    v = np.ascontiguousarray(np.concatenate([np.array(hand, np.uint8), c[10:]]))
    assert v.shape == (N_ROWS, U8_BYTES)
    v.setflags(write=False)
    return v


def u8_vocabulary(n_rows=N_ROWS):
    ids = np.arange(1, n_rows + 1, dtype=np.int32)
    ids.setflags(write=False)
    return _u8_vocab_all()[:n_rows], ids


def _u8_near_a(positions):
    return _u8_codes()[0] ^ _bits(positions)


def u8_filler(n, seed):
    """alternately a filler word with three random bits flipped (it matches) and a fresh random code (a new word, now and then with a same-frame candidate)"""
    rng = np.random.default_rng(_U8_SEED + seed)
    v = _u8_vocab_all()
    out = []
    for i in range(n):
        if i % 2 == 0:
            out.append(v[10 + int(rng.integers(0, N_ROWS - 10))] ^ _bits(rng.choice(256, 3, replace=False).tolist()))
        else:
            out.append(rng.integers(0, 256, U8_BYTES, dtype=np.uint8))
    return out


def u8_chain_rows(k, first_bit=0):
    """A ^ (twelve consecutive bits from 4 i): 12 and 14 from the anchors (new on its own), 8 from its neighbours in the chain (8 <= 0.8 * 12: it matches a new
    word in front of it), 16 or 24 from the rest (at or beyond the threshold 14): new, matched, new, ... and one descriptor settled per sweep"""
    assert first_bit + 4 * (k - 1) + 12 <= 200
    return [_u8_near_a(range(first_bit + 4 * i, first_bit + 4 * i + 12)) for i in range(k)]


def u8_cluster_rows(m):
    return [_u8_near_a(range(12))] + [_u8_near_a(list(range(12)) + [20 + i]) for i in range(m - 1)]


def u8_popular_rows(c):
    return [_u8_near_a([p]) for p in range(c)]


def _u8_input(rows, nndr=0.8, n_rows=N_ROWS):
    v, ids = u8_vocabulary(n_rows)
    return v, ids, np.ascontiguousarray(np.array(rows, np.uint8).reshape(-1, U8_BYTES)), nndr


def _u8_at_end(q, rows, seed):
    return u8_filler(q - len(rows), seed) + rows


def u8_all_inputs():
    c = _u8_codes()
    x7 = list(range(7))
    out = {"chain40": lambda: _u8_input(u8_chain_rows(40)),
           "chain20_in_513": lambda: _u8_input(_u8_at_end(513, u8_chain_rows(20), 1)),
           "chain20_in_1025": lambda: _u8_input(_u8_at_end(1025, u8_chain_rows(20), 2)),
           "popular40": lambda: _u8_input(u8_popular_rows(40)),
           "popular40_in_600": lambda: _u8_input(_u8_at_end(600, u8_popular_rows(40), 3)),
           # the fused merge keeps the first 512 distances of a row in registers and loops again behind them: a cluster across 511 | 512
           "seam512_cluster": lambda: _u8_input(u8_filler(511, 4) + u8_cluster_rows(6) + u8_filler(11, 5)),
           "later_only": lambda: _u8_input([_u8_near_a(x7), _u8_near_a(x7 + [30, 31]), _u8_near_a(x7 + [30, 31, 32, 33])]),
           "ties_lower_j": lambda: _u8_input([_bits([0, 1]), _bits([2, 3]), _bits([4, 5]), _bits([6, 7]), _bits([0, 1, 8])], nndr=1.0, n_rows=0),
           "ties_indexed_first": lambda: _u8_input([_u8_near_a(x7 + list(range(40, 47))), _u8_near_a(x7)]),
           "ties_second_excluded": lambda: _u8_input([_u8_near_a(x7 + list(range(40, 49))), _u8_near_a(x7)]),
           "nndr_half": lambda: _u8_input([c[1], c[2], c[3] ^ _bits([2, 3, 4, 5]), c[3], c[4] ^ _bits([3, 4, 5, 6]), c[4]], nndr=0.5)}
    for m in range(2, 8):
        out["cluster%d" % m] = functools.partial(lambda m: _u8_input(u8_cluster_rows(m)), m)
    for b in SEAMS:                                                # the word created at b - 1, its matches from b on
        if b != 512:
            out["seam%d_cluster" % b] = functools.partial(lambda b: _u8_input(u8_filler(b - 1, 10 + b) + u8_cluster_rows(6) + u8_filler(11, 11 + b)), b)
    for q in SIZES:                                                # as sizes(): what fits below 64, a cluster of 10 from position 3 and a chain of 8 at the end from there on
        if q == 1:
            out["size1"] = lambda: _u8_input(u8_filler(2, 20)[1:])
        elif q == 7:
            out["size7"] = lambda: _u8_input(u8_cluster_rows(6) + u8_filler(1, 21))
        elif q == 8:
            out["size8"] = lambda: _u8_input(u8_chain_rows(8))
        else:
            out["size%d" % q] = functools.partial(lambda q: _u8_input(u8_filler(3, 30 + q) + u8_cluster_rows(10) + u8_filler(q - 21, 31 + q) + u8_chain_rows(8, 40)), q)   # (the chain 24 away from the cluster)
    for n in (0, 1):
        out["empty%d_chain" % n] = functools.partial(lambda n: _u8_input(u8_chain_rows(40), n_rows=n), n)
        out["empty%d_popular" % n] = functools.partial(lambda n: _u8_input(u8_popular_rows(40), n_rows=n), n)
    return out
