"""GPU parity of the TF-IDF scoring at the sealed inverted index's encoding limits (rtabmap_amd/csrc/tfidf.h, score_body.cuh).

Every case plants signatures whose postings must take one route of a sealed bucket -- the word-major directory's 5-bit fields and
their saturation, dense rows and their saturated cells, dense ids that do not fit a bucket's allocation, the dense-id budget, the
extra trips / passes of the scorer for large frames, retirement and recycled postings keys, the documented maxima -- and combines
  * the oracle: the restated Memory::computeLikelihood at the parity bound of tests/test_gpu_likelihood.py, same arg-max;
  * a sensitivity guard: the same scores in float64 with the route's postings edited away (helpers.tfidf_f64) must move by more
    than 100 x RTOL, so that a lost or doubled posting on that route cannot hide inside the tolerance;
  * bit identity wherever tfidf.h's arithmetic claim (one exact int64 sum of count x Q5.26 idf, rounded once) makes results equal:
    across score_block 256 / 512 / 1024, registration paths, dense / sparse splits and twin signatures;
  * evidence that the route ran: lcd_profile_score_work's counters and lcd_get_stats."""
import numpy as np
import pytest
import torch  # noqa: F401  (before liblcd_hip.so is loaded: one HIP runtime per process, rtabmap_amd/capi.py)

from helpers import max_rel_change, min_word_visibility, signatures_from_postings, spread_slots, tfidf_f64
from rtabmap_amd import synth

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-4, 1e-7
GUARD = 100 * RTOL
BLOCKS = (256, 512, 1024)
R = 256                       # slots per bucket (TF_R)
LCD_ERR_UNSUPPORTED = 5


def _like3(eng, q, ids, N):
    """lcd_likelihood once per scoring workgroup size: the three must agree bit for bit."""
    outs = []
    for b in BLOCKS:
        eng.set_option("score_block", b)
        outs.append(eng.likelihood(q, ids, N))
    eng.set_option("score_block", 512)
    np.testing.assert_array_equal(outs[0], outs[1])
    np.testing.assert_array_equal(outs[2], outs[1])
    return outs[1]


class _Index:
    """The same signatures in a HIP engine and in the C++ oracle (word ids 1..n_words known to both), and their word lists."""

    def __init__(self, oracle, n_words, vocab=False):
        import rtabmap_amd
        self.eng = rtabmap_amd.Engine("f32", 64)
        self.m = oracle.OracleMemory(strategy=oracle.kNNBruteForce)
        self.n_words = n_words
        for w in range(1, n_words + 1):
            self.m.vwd.add_word(w, np.zeros(1, np.float32))
        if vocab:   # vocabulary rows (their keys are handed out in id order, and a removed row's key is recycled)
            self.eng.vocab_append(synth.vocab_surf(n_words, seed=7), np.arange(1, n_words + 1, dtype=np.int32))
        self.sigs, self.ids, self.live = [], [], []

    def add_words(self, ids):
        for w in ids:
            self.m.vwd.add_word(int(w), np.zeros(1, np.float32))
        self.n_words = max(self.n_words, int(max(ids)))

    def _note(self, sid, words):
        self.sigs.append(np.asarray(words, np.int32))
        self.ids.append(sid)
        self.live.append(True)

    def add(self, words):
        words = np.asarray(words, np.int32)
        sid = self.m.add_signature(words)
        self.eng.sig_add(sid, words)
        self._note(sid, words)

    def add_bulk(self, lists):
        sids = [self.m.add_signature(np.asarray(w, np.int32)) for w in lists]
        off = np.zeros(len(lists) + 1, np.int64)
        off[1:] = np.cumsum([len(w) for w in lists])
        self.eng.sig_add_bulk(np.array(sids, np.int32), off, np.concatenate([np.asarray(w, np.int32) for w in lists]))
        for sid, w in zip(sids, lists):
            self._note(sid, w)

    def retire(self, k):
        self.m.forget(int(self.ids[k]))
        self.eng.sig_remove(int(self.ids[k]))
        self.live[k] = False

    def N(self):
        return float(self.m.num_signatures())

    def live_ids(self):
        return np.array([s for s, a in zip(self.ids, self.live) if a], np.int32)

    def check(self, q, ids=None):
        """oracle parity (and the three workgroup sizes bit for bit); returns (ids, scores)"""
        q = np.asarray(q, np.int32)
        ids = self.live_ids() if ids is None else np.asarray(ids, np.int32)
        oid, exp = self.m.compute_likelihood(q, ids)
        assert oid.size == ids.size
        got = _like3(self.eng, q, oid, self.N())
        np.testing.assert_allclose(got, exp, rtol=RTOL, atol=ATOL)
        if exp.max() > 0:
            top = np.sort(exp)[::-1]
            if top.size < 2 or top[0] - top[1] > 2 * RTOL * top[0]:
                assert int(np.argmax(got)) == int(np.argmax(exp))
            else:                                           # a near-tie: the engine's pick must score as the oracle's best does
                assert got[int(np.argmax(exp))] >= got.max() * (1 - RTOL)
        # the guards' float64 yardstick is the same sum as the oracle's
        ref, _ = tfidf_f64(self.sigs, q, self.live)
        pos = {s: i for i, s in enumerate(self.ids)}
        np.testing.assert_allclose(ref[[pos[int(s)] for s in oid]], exp, rtol=RTOL, atol=ATOL)
        return oid, got

    def guard(self, q, edited, live=None):
        """the route's fault, applied to the input, must show: at least one score moves by more than GUARD"""
        live = self.live if live is None else live
        base, _ = tfidf_f64(self.sigs, q, live)
        moved, _ = tfidf_f64(edited, q, live)
        assert max_rel_change(base, moved) > GUARD

    def close(self):
        self.eng.close()
        self.m.close()


def _drop(sigs, words, rows=None):
    """the signatures with every posting of `words` lost (only in signature indices `rows` when given); ni stays what it was"""
    words = np.asarray(sorted(words))
    rows = range(len(sigs)) if rows is None else set(rows)
    return [np.where(np.isin(s, words), -1, s).astype(np.int32) if k in rows else s for k, s in enumerate(sigs)]


def _clamp255(sigs):
    """the signatures with every count above 255 cut to 255 (a lost excess); ni stays what it was"""
    out = []
    for s in sigs:
        u, c = np.unique(s, return_counts=True)
        cut = np.repeat(u, np.minimum(c, 255))
        out.append(np.concatenate([cut, np.full(s.size - cut.size, -1)]).astype(np.int32) if (c > 255).any() else s)
    return out


def _fill(n):
    """n signatures without words (ni = 1): they fill slots"""
    return [np.array([-1], np.int32) for _ in range(n)]


# ------------------------------------------------------------------------------------------------------------ A. directory fields
P = (0, 5, 6, 11, 12, 29, 30, 31)      # a block's field boundaries: 6 fields per dword, positions 5/6, 11/12, 29/30/31


def _a_counts():
    """postings of word 32 b + p + 1 in bucket 1: block 0 / 1 packed (29 / 30 at the boundaries, smaller neighbours on both sides),
    block 2 saturated at every boundary, blocks 3 / 4 one saturated word (positions 12 / 0) among fields that fit"""
    c = np.zeros((5, 32), int)
    for p in range(32):
        c[0, p] = 0 if p in (3, 20) else 1 + (p * 7) % 12
        c[1, p] = 13 + p % 17
        c[2, p] = 1 + (p * 3) % 27
        c[3, p] = 1 + p % 9
        c[4, p] = 2 + p % 20
    for i, p in enumerate(P):
        c[0, p] = 29 + i % 2
        c[1, p] = 30 - i % 2
        c[2, p] = 31
        c[3, p] = 31 if p == 12 else 29 + i % 2
    c[4, 0], c[4, 31] = 31, 30
    return c


def _a_signatures():
    c = _a_counts()
    n_words = c.size
    post = []
    for b in range(5):
        for p in range(32):
            w = 32 * b + p + 1
            for i, s in enumerate(spread_slots(c[b, p], w)):
                post.append((w, s, 3 if (w + i) % 11 == 0 else 1 + ((w + i) % 5 == 0)))
    # slot 0 lists every word in id order (key = id - 1: the planted block positions), bucket 1 holds the planted postings,
    # slot 512 seals it
    sigs = [np.arange(1, n_words + 1, dtype=np.int32)] + _fill(R - 1) + signatures_from_postings(post) + _fill(1)
    return c, sigs


@pytest.mark.parametrize("path", ["bulk", "one_by_one"])
def test_a_directory_fields(oracle, path):
    c, sigs = _a_signatures()
    sat_blocks = [b for b in range(5) if c[b].max() > 30]
    assert sat_blocks == [2, 3, 4] and (c[3] > 30).sum() == 1 and (c[4] > 30).sum() == 1 and c.max() < 32
    ix = _Index(oracle, c.size)
    if path == "bulk":
        ix.add_bulk(sigs)
    else:
        for s in sigs:
            ix.add(s)
    st = ix.eng.stats()
    assert st["dense_words"] == 0 and st["buckets_sealed"] == 2
    planted = [32 * b + p + 1 for b in range(5) for p in P]
    ix.guard(np.arange(1, c.size + 1), _drop(ix.sigs, planted, rows=range(R, 2 * R)))
    q_all = np.arange(1, c.size + 1, dtype=np.int32)
    _, got = ix.check(q_all)
    prof = ix.eng.profile_score_work()
    present = int((c > 0).sum())
    assert prof["directory_lookups"] == 2 * c.size                 # bucket 0 and bucket 1, every word sparse
    assert prof["directory_hits"] == c.size + present               # bucket 0: slot 0 holds every word
    assert prof["sparse_postings"] == c.size + int(c.sum())
    assert prof["dense_row_bytes"] == 0
    for b in range(5):                                              # one block at a time, then only its boundary words
        ix.check(np.arange(32 * b + 1, 32 * b + 33, dtype=np.int32))
        ix.check(np.array([32 * b + p + 1 for p in P], np.int32))
    ix.check(np.array(planted[::-1] + [-1, 0, 5, 5], np.int32))
    # the two registration paths seal the same postings: the same bits
    if path == "bulk":
        ix2 = _Index(oracle, c.size)
        for s in sigs:
            ix2.add(s)
        np.testing.assert_array_equal(_like3(ix2.eng, q_all, ix2.live_ids(), ix2.N()), got)
        ix2.close()
    ix.close()


# ------------------------------------------------------------------------------------------------------ B. saturated dense cells
EXCESS = (254, 255, 256, 257, 511, 1000, 8192)


def _b_signatures():
    X, Y, Wd, V = 1, 2, 3, 50
    pool = np.arange(101, 181)
    b0 = []
    for s in range(R):
        w = [int(pool[(s * 7 + j * 31) % 80]) for j in range(3)]
        if s % 5 == 0:
            w += [V] * (1 + s % 3)
        b0.append(np.array(sorted(w), np.int32))
    b1 = []
    ycnt = {9: 255, 13: 254, 17: 200}
    for s in range(R):
        cx = EXCESS[s] if s < len(EXCESS) else 1 + s % 3
        if cx == 8192:                                              # a blank wall quantised to one word: TF_MAX_WORDS of it
            b1.append(np.full(8192, X, np.int32))
            continue
        w = [X] * cx + [int(pool[(s * 11 + j * 17) % 80]) for j in range(2)]
        if s % 4 == 1:
            w += [Y] * ycnt.get(s, 1 + s % 5)
        if s % 6 == 0:
            w += [Wd]
        b1.append(np.array(sorted(w), np.int32))
    return b0 + b1 + _fill(1)


@pytest.mark.parametrize("path", ["bulk", "one_by_one"])
def test_b_saturated_dense_cells(oracle, path):
    """counts 254 .. 8192 of a dense word (row cell 255, the excess a sparse posting of the same bucket) next to dense words whose
    counts fit (255 itself among them: no excess, nothing in the sparse part), in a bucket with the excess flag and one without"""
    X, Y, V = 1, 2, 50
    sigs = _b_signatures()
    ix = _Index(oracle, 180)
    if path == "bulk":
        ix.add_bulk(sigs)
    else:
        for s in sigs:
            ix.add(s)
    assert ix.eng.stats()["dense_words"] == 4                       # V (bucket 0), X, Y and word 3 (bucket 1)
    q_all = np.array([1, 2, 3, 50] + list(range(101, 181)), np.int32)
    ix.guard(q_all, _clamp255(ix.sigs))
    _, got = ix.check(q_all)
    for q in ([X], [Y], [V], [X, Y, V, 3], [X, 101, 150]):
        ix.check(np.array(q, np.int32))
    ix.eng.likelihood(np.array([X], np.int32), ix.live_ids(), ix.N())
    p = ix.eng.profile_score_work()
    assert p["dense_words"] == 1 and p["dense_row_bytes"] >= R
    assert p["directory_hits"] == 1 and p["sparse_postings"] == 5    # the excess of 256, 257, 511, 1000 and 8192
    ix.eng.likelihood(np.array([Y], np.int32), ix.live_ids(), ix.N())
    p = ix.eng.profile_score_work()
    assert p["directory_lookups"] >= 1 and p["directory_hits"] == 0  # looked up in the flagged bucket, nothing there
    ix.eng.likelihood(np.array([V], np.int32), ix.live_ids(), ix.N())
    p = ix.eng.profile_score_work()
    assert p["dense_row_bytes"] == 2 * R                            # a row in both buckets ...
    assert p["directory_lookups"] == 1 and p["directory_hits"] == 0  # ... looked up only where the bucket has excess postings
    if path == "bulk":
        ix2 = _Index(oracle, 180)
        for s in sigs:
            ix2.add(s)
        np.testing.assert_array_equal(_like3(ix2.eng, q_all, ix2.live_ids(), ix2.N()), got)
        ix2.close()
    ix.close()


# --------------------------------------------------------------------------------------------------- C. allocation headroom
def _bucket(words, n_post, key, extra=None):
    """256 signatures in which every word of `words` has n_post postings (counts 1-3); extra(s) -> more words of signature s"""
    post = []
    for w in words:
        for i, s in enumerate(spread_slots(n_post, int(w) + key)):
            post.append((int(w), s, 1 + ((int(w) + i) % 4 == 0) + ((int(w) + i) % 9 == 0)))
    sigs = signatures_from_postings(post)
    if extra is not None:
        sigs = [np.sort(np.concatenate([s, np.asarray(extra(k), np.int32)])).astype(np.int32) for k, s in enumerate(sigs)]
    return sigs


def test_c_headroom_bulk_two_seal_batches(oracle):
    """one lcd_sig_add_bulk over 65 full buckets: the first batch of 64 seals with D_alloc = its dense ids + 32; bucket 64 (second
    batch, same D_alloc) creates 100 dense ids, 68 of which do not fit: sparse there with 64 postings each; dense in bucket 65"""
    b0 = _bucket(range(1, 41), 40, 0, extra=lambda s: [301 + (s * 7) % 100])   # 40 dense ids from the first bucket
    mid = [np.array([301 + (s * 7 + b) % 100], np.int32) for b in range(1, 64) for s in range(R)]
    b64 = _bucket(range(101, 201), 64, 7)
    b65 = _bucket(range(101, 201), 64, 91)
    ix = _Index(oracle, 400)
    ix.add_bulk(b0 + mid + b64 + b65[:1])
    for s in b65[1:] + _fill(1):
        ix.add(s)
    st = ix.eng.stats()
    assert st["dense_words"] == 140 and st["buckets_sealed"] == 66
    q = np.arange(101, 201, dtype=np.int32)
    ix.guard(q, _drop(ix.sigs, range(133, 201), rows=range(64 * R, 65 * R)))
    ix.check(q)
    p = ix.eng.profile_score_work()
    assert p["directory_hits"] == 68 and p["sparse_postings"] == 68 * 64
    assert p["directory_lookups"] == 64 * 100 + 68                  # buckets 0-63: ids past their D; bucket 64: the 68 that did not fit
    assert p["dense_row_bytes"] == (32 + 100) * R
    ix.check(np.arange(1, 401, dtype=np.int32))
    ix.check(np.concatenate([np.arange(1, 41), np.arange(150, 170)]).astype(np.int32))
    ix.close()


def test_c_headroom_incremental(oracle):
    """one signature at a time: the first seal allocates 1024 rows for 1100 new dense ids (76 stay sparse with 40 postings), a later
    seal 128 rows more than it knows of for 200 new ones (72 stay sparse); the next buckets hold all of them as rows"""
    A, B = np.arange(1, 1101), np.arange(1101, 1301)
    sigs = _bucket(A, 40, 0) + _bucket(A, 40, 3) + _bucket(B, 40, 0) + _bucket(B, 40, 5)
    rng = np.random.default_rng(3)
    sigs += [np.sort(rng.integers(1, 1301, 60)).astype(np.int32) for _ in range(10)]
    ix = _Index(oracle, 1300)
    for s in sigs:
        ix.add(s)
    st = ix.eng.stats()
    assert st["dense_words"] == 1300 and st["buckets_sealed"] == 4
    q = np.arange(1, 1301, dtype=np.int32)
    ix.guard(q, _drop(ix.sigs, range(1025, 1101), rows=range(0, R)))
    ix.guard(q, _drop(ix.sigs, range(1229, 1301), rows=range(2 * R, 3 * R)))
    ix.check(q)
    p = ix.eng.profile_score_work()
    first2 = len(set(sigs[2 * R].tolist()))                         # keys handed out before bucket 1 sealed: inside its directory
    assert p["directory_hits"] == 76 + 72 and p["sparse_postings"] == (76 + 72) * 40
    assert p["directory_lookups"] == 76 + first2 + 72
    for k in range(4):
        ix.check(np.sort(rng.choice(1300, 300 + 200 * k, replace=False) + 1).astype(np.int32))
    ix.close()


# ------------------------------------------------------------------------------------------------------------- D. dense budget
def _d_signatures():
    n = 4200                                                        # > TF_DENSE_MAX words with 32 postings in each bucket
    per = [[] for _ in range(2 * R)]
    for w in range(1, n + 1):
        for i in range(32):
            s = (w + 8 * i) % R
            per[s].extend([w] * (1 + ((w * s) % 3 == 0)))
            per[R + s].extend([w] * (1 + ((w + s) % 4 == 0)))
    return n, [np.array(p, np.int32) for p in per] + _fill(1)


def test_d_dense_budget(oracle):
    n, sigs = _d_signatures()
    ix = _Index(oracle, n)
    ix.add_bulk(sigs)
    assert ix.eng.stats()["dense_words"] == 4096
    q = np.arange(1, n + 1, dtype=np.int32)
    ix.guard(q, _drop(ix.sigs, range(n - 103, n + 1)))              # as many words as miss the budget
    ix.check(q)
    p = ix.eng.profile_score_work()
    assert p["unique_words"] == n and p["dense_words"] == 4096
    assert p["directory_lookups"] == 2 * (n - 4096) and p["directory_hits"] == 2 * (n - 4096)
    assert p["sparse_postings"] == 2 * 32 * (n - 4096) and p["dense_row_bytes"] == 2 * 4096 * R
    rng = np.random.default_rng(11)
    for k in range(4):                                              # frames that mix budgeted and past-budget words
        qk = np.sort(rng.choice(n, 400 + 700 * k, replace=False) + 1).astype(np.int32)
        ix.guard(qk, _drop(ix.sigs, qk[::9]))
        ix.check(qk)
        p = ix.eng.profile_score_work()
        past = p["unique_words"] - p["dense_words"]
        assert p["directory_lookups"] == 2 * past and p["sparse_postings"] == 64 * past
    ix.close()


# ------------------------------------------------------------------------------------------------ E. query sizes x score_block
def test_e_query_sizes(oracle):
    """unique words around the first pass (512 / 1024 per workgroup) and the TF_MAX_WORDS maximum, dense words around one trip
    (64 / 128): every workgroup size gives the same bits"""
    dense, sparse = np.arange(1, 201), np.arange(201, 8601)
    sigs = []
    for key in (0, 17):
        post = [(int(w), s, 1 + ((int(w) + i) % 5 == 0)) for w in dense for i, s in enumerate(spread_slots(40, int(w) + key))]
        post += [(int(w), s, 1 + ((int(w) + i) % 7 == 0)) for w in sparse for i, s in enumerate(spread_slots(3, int(w) + key))]
        sigs += signatures_from_postings(post)
    rng = np.random.default_rng(5)
    sigs += [np.sort(rng.integers(1, 8601, 150)).astype(np.int32) for _ in range(12)]
    ix = _Index(oracle, 8600)
    ix.add_bulk(sigs)
    assert ix.eng.stats()["dense_words"] == 200
    for U in (511, 512, 513, 1023, 1024, 1025, 8192):
        for Ud in (63, 64, 65, 127, 128, 129):
            q = np.concatenate([rng.choice(dense, Ud, replace=False), rng.choice(sparse, U - Ud, replace=False)]).astype(np.int32)
            rng.shuffle(q)
            if U <= 1025:
                assert min_word_visibility(ix.sigs, q) > GUARD          # losing ANY one word of the frame shows
            else:
                ix.guard(q, _drop(ix.sigs, q[512:]))
            ix.check(q)
            p = ix.eng.profile_score_work()
            assert p["unique_words"] == U and p["dense_words"] == Ud
    ix.close()


# --------------------------------------------------------------------------------------------------- F. history independence
def _f_signatures():
    rng = np.random.default_rng(2)
    b0 = [np.sort(rng.integers(1, 301, 8)).astype(np.int32) for _ in range(R)]          # no word reaches 32 postings
    def dense_part(words, s, key):
        return [int(w) for w in words for _ in range(1 + (int(w) * s + key) % 3) if (int(w) + s) % 4 == 0]
    b1 = []
    for s in range(R):
        w = dense_part(range(1, 21), s, 1) + list(rng.integers(301, 601, 6))
        if s % 37 == 0:
            w += [3] * 300                                            # excess in the dense rows' bucket
        b1.append(np.sort(np.array(w, np.int32)))
    b2 = []
    for s in range(R):
        w = dense_part(range(21, 61), s, 2) + list(rng.integers(601, 700, 3)) + [700 + s % 8] * (1 + s % 2)
        b2.append(np.sort(np.array(w, np.int32)))
    opn = [np.sort(rng.integers(1, 709, 20)).astype(np.int32) for _ in range(40)]
    twin = np.array([1] * 2 + [2] + [3] * 300 + [5] + [7] * 3 + [21, 22, 301, 302, 650, 701, -1], np.int32)
    for part, k in ((b0, 10), (b1, 100), (opn, 20)):                 # only sparse postings / dense rows (+ excess) / the open bucket
        part[k] = np.random.default_rng(k).permutation(twin).astype(np.int32)
    sigs = b0 + b1 + b2 + opn
    return sigs, (10, R + 100, 3 * R + 20)


def test_f_history_independence(oracle):
    sigs, twins = _f_signatures()
    assert np.bincount(np.concatenate([np.unique(s[s > 0]) for s in sigs[:R]])).max() < 32      # bucket 0: no dense word of its own
    ix = [_Index(oracle, 710) for _ in range(3)]
    for s in sigs:
        ix[0].add(s)
    ix[1].add_bulk(sigs)
    ix[2].add_bulk(sigs[:300])
    ix[2].add_bulk(sigs[300:])
    for e in ix:
        assert e.eng.stats()["buckets_sealed"] == 3
    rng = np.random.default_rng(4)
    queries = [np.concatenate([sigs[t], [3, 21, 22]]).astype(np.int32) for t in twins[:1]]
    queries += [np.sort(rng.choice(709, n, replace=False) + 1).astype(np.int32) for n in (30, 200, 600)]
    queries += [np.arange(1, 710, dtype=np.int32)]
    ix[0].guard(queries[0], _clamp255(ix[0].sigs))
    ix[0].guard(queries[-1], _drop(ix[0].sigs, range(1, 61), rows=range(R, 3 * R)))
    ids = ix[0].live_ids()
    slot = {s: k for k, s in enumerate(ids)}
    tw = [slot[int(ix[0].ids[t])] for t in twins]
    for q in queries:
        _, got = ix[0].check(q)
        for e in ix[1:]:
            np.testing.assert_array_equal(_like3(e.eng, q, ids, e.N()), got)
        assert got[tw[0]] == got[tw[1]] == got[tw[2]] and (got[tw[0]] > 0 or q is not queries[0])
    for e in ix:
        e.close()


# ------------------------------------------------------------------------------------------- G. retirement and recycled keys
def test_g_retirement_and_recycled_keys(oracle):
    """retire signatures with saturated cells and excess postings and a whole sealed bucket; the words left without references are
    removed and new words take their keys, which the old buckets still list for retired signatures: nothing of that scores"""
    X, E = 1, 400
    R1, R2 = np.arange(301, 341), np.arange(341, 361)               # referenced only by signatures that retire
    rng = np.random.default_rng(8)
    def sig(s, b):
        w = list(rng.integers(2, 300, 10)) + [E]
        if b == 0 and s % 4 == 0:
            w += [X] * (300 if s < 12 else 1 + s % 3)
        if b == 0 and s < 10:
            w += [int(r) for r in R1[(s * 4) % 40:(s * 4) % 40 + 4]] + ([int(R1[s])] * 300 if s < 3 else [])
        if b == 1 and s % 2 == 0:
            w += [int(r) for r in R2]                                 # dense in bucket 1 only
        return np.sort(np.array(w, np.int32))
    sigs = [sig(s, b) for b in range(3) for s in range(R)] + [sig(s, 3) for s in range(20)]
    ix = _Index(oracle, 400, vocab=True)
    ix.add_bulk(sigs)
    assert ix.eng.stats()["buckets_sealed"] == 3
    gone = list(range(12)) + list(range(R, 2 * R))                  # saturated cells + excess; bucket 1 entirely (dead)
    for k in gone:
        ix.retire(k)
    assert all(ix.eng.word_nrefs(int(w)) == 0 for w in np.concatenate([R1, R2]))
    dropped = np.concatenate([R1, R2]).astype(np.int32)
    ix.eng.vocab_remove(dropped)
    ix.m.vwd.remove_words(dropped)
    ix.eng.vocab_rebuild()
    ix.eng.synchronize()
    new = np.arange(401, 461, dtype=np.int32)
    ix.eng.vocab_append(synth.vocab_surf(60, seed=9), new)          # they take the freed keys
    ix.add_words(new)
    for s in range(30):
        ix.add(np.sort(np.concatenate([rng.choice(new, 6, replace=False), rng.integers(2, 300, 4), [E]])).astype(np.int32))
    q = np.concatenate([new, [X], np.arange(2, 40)]).astype(np.int32)
    ix.guard(q, _drop(ix.sigs, new))
    ix.check(q)
    ix.eng.likelihood(new, ix.live_ids(), ix.N())
    p = ix.eng.profile_score_work()
    assert p["directory_lookups"] > 0 and p["directory_hits"] > 0   # recycled keys inside the old buckets' directories, postings there
    _, got = ix.check(new)
    assert got.max() > 0
    retired = np.array([ix.ids[k] for k in gone], np.int32)
    assert (ix.eng.likelihood(q, retired, ix.N()) == 0).all()
    # idf at N == nw: word E is in every live signature -- idf 0, the same bits with or without it
    assert ix.eng.word_nrefs(E) == ix.N()
    np.testing.assert_array_equal(_like3(ix.eng, np.append(q, E), ix.live_ids(), ix.N()), _like3(ix.eng, q, ix.live_ids(), ix.N()))
    ix.check(np.append(q, E))
    ix.close()


# ------------------------------------------------------------------------------------------------------------------- H. limits
def test_h_limits(oracle):
    """TF_MAX_WORDS (8192) words per signature through lcd_sig_add and lcd_sig_add_bulk and per query; 8193 is LCD_ERR_UNSUPPORTED
    for all three (include/lcd.h), and the handle stays usable"""
    from rtabmap_amd.capi import LcdError
    rng = np.random.default_rng(6)
    n = 9000
    small = [np.sort(rng.integers(1, n + 1, 40)).astype(np.int32) for _ in range(300)]
    small[5] = np.sort(rng.integers(1, n + 1, 8192)).astype(np.int32)                       # bulk, sealed bucket
    ix = _Index(oracle, n)
    ix.add_bulk(small)
    ix.add(np.sort(rng.choice(n, 8192, replace=False) + 1).astype(np.int32))                  # one call, open bucket
    ix.add(np.sort(rng.integers(1, 50, 8192)).astype(np.int32))
    assert ix.eng.stats()["buckets_sealed"] == 1
    q = (rng.choice(n, 8192, replace=False) + 1).astype(np.int32)
    ix.guard(q, _drop(ix.sigs, q[4096:]))
    _, got = ix.check(q)
    big = np.arange(1, 8194, dtype=np.int32)
    with pytest.raises(LcdError) as e1:
        ix.eng.sig_add(10 ** 6, big)
    with pytest.raises(LcdError) as e2:
        ix.eng.sig_add_bulk(np.array([10 ** 6, 10 ** 6 + 1], np.int32), np.array([0, 5, 5 + 8193], np.int64),
                            np.concatenate([big[:5], big]))
    with pytest.raises(LcdError) as e3:
        ix.eng.likelihood(big, ix.live_ids(), ix.N())
    assert e1.value.status == e2.value.status == e3.value.status == LCD_ERR_UNSUPPORTED
    assert ix.eng.sig_count()[0] == len(ix.ids)
    np.testing.assert_array_equal(_like3(ix.eng, q, ix.live_ids(), ix.N()), got)
    ix.add(np.sort(rng.integers(1, n + 1, 100)).astype(np.int32))
    ix.check(q)
    ix.close()
