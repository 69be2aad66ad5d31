"""GPU parity of the pair similarity (lcd_similarity / lcd_similarity_dev, rtabmap_amd/csrc/similarity_body.cuh): Signature::compareTo's
words branch of a query against every signature of the inverted index, for Memory::computeLikelihood with Kp/TfIdfLikelihoodUsed=false.

pairs = sum over words of min(cq, cs) is an integer and the similarity one IEEE float division, so EVERY comparison here is
assert_array_equal on the floats and on the integers behind them (out_pairs, out_valid) against tests/similarity_model.py: there is no
tolerance anywhere.  The index shapes are the planted ones of tests/test_gpu_index_limits.py (directory fields, saturated dense cells,
dense ids that do not fit a bucket), because the routes a sealed bucket takes are the same and the term is different."""
import numpy as np
import pytest
import torch  # noqa: F401  (before liblcd_hip.so is loaded: one HIP runtime per process, rtabmap_amd/capi.py)

import similarity_model as M
from rtabmap_amd import synth
from test_gpu_index_limits import _a_signatures, _b_signatures, _bucket, _fill

pytestmark = pytest.mark.gpu
R = 256                       # slots per bucket (TF_R)
LCD_ERR_INVALID, LCD_ERR_UNSUPPORTED = 1, 5


class _Sim:
    """signatures 1, 2, ... in a HIP engine and as plain word lists (None once retired)"""

    def __init__(self, vocab_words=0, **kw):
        import rtabmap_amd
        self.eng = rtabmap_amd.Engine("f32", 64, **kw)
        if vocab_words:   # vocabulary rows: a removed row's postings key is recycled
            self.eng.vocab_append(synth.vocab_surf(vocab_words, seed=7), np.arange(1, vocab_words + 1, dtype=np.int32))
        self.sigs = []

    def add(self, words):
        words = np.asarray(words, np.int32)
        self.eng.sig_add(len(self.sigs) + 1, words)
        self.sigs.append(words)

    def add_bulk(self, lists):
        first = len(self.sigs) + 1
        off = np.zeros(len(lists) + 1, np.int64)
        off[1:] = np.cumsum([len(w) for w in lists])
        self.eng.sig_add_bulk(np.arange(first, first + len(lists), dtype=np.int32), off, np.concatenate([np.asarray(w, np.int32) for w in lists]))
        self.sigs += [np.asarray(w, np.int32) for w in lists]

    def retire(self, k):
        self.eng.sig_remove(k + 1)
        self.sigs[k] = None

    def all_ids(self):
        return np.arange(1, len(self.sigs) + 1, dtype=np.int32)

    def check(self, q, ids=None):
        """lcd_similarity == the model, floats and integers, bit for bit; ids default to every signature ever added (retired ones: 0)"""
        q = np.asarray(q, np.int32)
        ids = self.all_ids() if ids is None else np.asarray(ids, np.int32)
        exp = M.similarity_closed_form(q, [self.sigs[i - 1] if 0 < i <= len(self.sigs) else None for i in ids.tolist()])
        got = self.eng.similarity(q, ids, with_counts=True)
        np.testing.assert_array_equal(got[1], exp[1])                 # pairs
        np.testing.assert_array_equal(got[2], exp[2])                 # valid words of the signature
        np.testing.assert_array_equal(got[0], exp[0])                 # the float
        np.testing.assert_array_equal(self.eng.similarity(q, ids), exp[0])      # (without the integer outputs)
        return got

    def close(self):
        self.eng.close()


# ------------------------------------------------------------------------------------------------------------ 1. open bucket only
def test_open_bucket_only():
    rng = np.random.default_rng(1)
    ix = _Sim()
    for s in range(40):
        w = rng.integers(1, 60, int(rng.integers(5, 90)))            # repeated words
        w[rng.random(w.size) < 0.15] = rng.integers(-3, 1, 1)[0]     # features without a word (ids <= 0)
        ix.add(np.full(9, -1 - s % 2) if s == 7 else w)              # signature 8: only invalid ids (vs == 0)
    assert ix.eng.stats()["buckets_sealed"] == 0
    unseen = np.array([5000, 5000, 5001, 77777], np.int32)           # ids the engine never saw: valid words of the query
    own = ix.sigs[3]
    queries = [np.zeros(0, np.int32), np.array([-1, 0, -5], np.int32), np.concatenate([own, unseen]), own, np.repeat(np.arange(1, 60), 4),
               rng.integers(-2, 80, 300), unseen]
    for q in queries:
        got = ix.check(q)
        for k in (0, 3, 7, 39):                                      # and the literal multimap walk, signature by signature
            sim, pairs, valid = M.compare_to_literal(np.asarray(q, np.int32), ix.sigs[k])
            assert (got[0][k].tobytes(), got[1][k], got[2][k]) == (np.float32(sim).tobytes(), pairs, valid)
    # vq counts the unseen ids: the signature's own words plus four unseen ones pair completely and still score below 1
    vs = int((own > 0).sum())
    got = ix.check(np.concatenate([own, unseen]))
    assert got[1][3] == vs and got[0][3] == np.float32(vs) / np.float32(vs + 4) and got[2][7] == 0 and got[0][7] == 0
    assert (ix.check(np.zeros(0, np.int32))[0] == 0).all()
    ix.close()


# ------------------------------------------------------------------------------------------------------------ 2. directory routes
@pytest.mark.parametrize("path", ["bulk", "one_by_one"])
def test_directory_routes(path):
    """the planted 5-bit fields and saturated records of the word-major directory; counts there are 1-3, so querying each word once
    binds the cap and querying it three times does not"""
    c, sigs = _a_signatures()
    ix = _Sim()
    if path == "bulk":
        ix.add_bulk(sigs)
    else:
        for s in sigs:
            ix.add(s)
    st = ix.eng.stats()
    assert st["dense_words"] == 0 and st["buckets_sealed"] == 2
    q1 = np.arange(1, c.size + 1, dtype=np.int32)
    g1 = ix.check(q1)
    g3 = ix.check(np.repeat(q1, 3))
    assert (g3[1] >= g1[1]).all() and (g3[1][R:2 * R] > g1[1][R:2 * R]).any()      # the cap bound at one occurrence
    for b in range(5):
        ix.check(np.repeat(np.arange(32 * b + 1, 32 * b + 33, dtype=np.int32), 2))
    ix.check(np.array([160, 1, 1, 97, -1, 0, 5, 5, 5, 5], np.int32))
    ix.close()


# ------------------------------------------------------------------------------------------------------ 3. saturated dense cells
@pytest.mark.parametrize("path", ["bulk", "one_by_one"])
def test_saturated_dense_cells(path):
    """counts 254 .. 8192 of a dense word (row cell 255 + the excess as a sparse posting) against query multiplicities on both sides of
    the 255 split; bucket 0 has dense rows and no excess flag"""
    X, Y, V = 1, 2, 50
    sigs = _b_signatures()
    ix = _Sim()
    if path == "bulk":
        ix.add_bulk(sigs)
    else:
        for s in sigs:
            ix.add(s)
    assert ix.eng.stats()["dense_words"] == 4
    for m in (1, 254, 255, 256, 257, 300, 511, 1000, 8192):
        got = ix.check(np.full(m, X, np.int32))
        cx = np.array([int((s == X).sum()) for s in ix.sigs])
        np.testing.assert_array_equal(got[1], np.minimum(cx, m))
        if m <= 1000:
            ix.check(np.concatenate([np.full(m, X), np.full(m, Y), np.full(min(m, 40), V), np.arange(101, 181)]).astype(np.int32))
    ix.check(np.array([V] * 3 + [Y] * 256 + [3, 3], np.int32))
    ix.close()


# --------------------------------------------------------------------------------------- 4. a dense id outside a bucket's rows
def test_dense_word_that_does_not_fit_a_buckets_rows():
    """one signature at a time (the shape of test_c_headroom_incremental, smaller): bucket 0 makes 10 words dense; bucket 1 is sealed with
    128 rows more than the 10 known and creates 200 dense ids, 72 of which do not fit: sparse postings there, capped at cq"""
    A, B = np.arange(1, 11), np.arange(101, 301)
    sigs = _bucket(A, 40, 0) + _bucket(B, 40, 0) + _bucket(B, 40, 5)
    rng = np.random.default_rng(3)
    sigs += [np.sort(rng.integers(1, 301, 60)).astype(np.int32) for _ in range(10)]
    ix = _Sim()
    for s in sigs:
        ix.add(s if len(s) else np.array([-1], np.int32))
    st = ix.eng.stats()
    assert st["dense_words"] == 210 and st["buckets_sealed"] == 3      # 210 dense ids > the 10 + 128 rows bucket 1 was given
    q = np.concatenate([A, B]).astype(np.int32)
    for m in (1, 2, 3):
        ix.check(np.repeat(q, m))
    ix.check(np.repeat(B[100:], 2))
    ix.close()


# ---------------------------------------------------------------------------------------------------------------- 5. query sizes
def test_query_sizes():
    from rtabmap_amd.capi import LcdError
    from helpers import signatures_from_postings, spread_slots
    dense, sparse = np.arange(1, 151), np.arange(151, 1501)
    sigs = []
    for key in (0, 17):
        post = [(int(w), s, 1 + ((int(w) + i) % 5 == 0)) for w in dense for i, s in enumerate(spread_slots(40, int(w) + key))]
        post += [(int(w), s, 1 + ((int(w) + i) % 7 == 0)) for w in sparse for i, s in enumerate(spread_slots(3, int(w) + key))]
        sigs += [s if len(s) else np.array([-1], np.int32) for s in signatures_from_postings(post)]
    rng = np.random.default_rng(5)
    sigs += [np.sort(rng.integers(1, 1501, 150)).astype(np.int32) for _ in range(12)]
    ix = _Sim()
    ix.add_bulk(sigs)
    assert ix.eng.stats()["dense_words"] == 150
    for U, Ud in ((511, 127), (512, 128), (513, 129), (700, 140), (1025, 150)):     # > 512 unique, > 128 dense words
        q = np.concatenate([rng.choice(dense, Ud, replace=False), rng.choice(sparse, U - Ud, replace=False)]).astype(np.int32)
        ix.check(rng.permutation(np.concatenate([q, q[::3]])))
    ix.check(rng.integers(1, 1501, 8192))                              # exactly 8192 entries, with repeats
    got = ix.check(np.arange(1, 8193, dtype=np.int32))                 # 8192 distinct ids, 1500 of them known to the index
    assert got[1].max() > 0
    with pytest.raises(LcdError) as e:
        ix.eng.similarity(np.arange(1, 8194, dtype=np.int32), ix.all_ids())
    assert e.value.status == LCD_ERR_UNSUPPORTED
    ix.check(np.arange(1, 400, dtype=np.int32))                        # the handle stays usable
    ix.close()


# ---------------------------------------------------------------------------------------------------------------------- 6. idf = 0
def test_word_held_by_every_signature_pairs():
    rng = np.random.default_rng(6)
    E = 9
    ix = _Sim()
    ix.add_bulk([np.concatenate([[E] * (1 + s % 3), rng.integers(20, 200, 12)]).astype(np.int32) for s in range(300)])
    N = 300.0
    assert ix.eng.word_nrefs(E) == N
    q = np.array([E, E], np.int32)
    got = ix.check(q)
    np.testing.assert_array_equal(got[1], np.minimum(2, 1 + np.arange(300) % 3))
    assert (got[0] > 0).all()
    assert (ix.eng.likelihood(q, ix.all_ids(), N) == 0).all()          # TF-IDF gives the same word weight log10(N / nw) = 0
    ix.close()


# ------------------------------------------------------------------------------------------- 7. retirement and recycled keys
def test_retirement_and_recycled_keys():
    X, E = 1, 400
    R1 = np.arange(301, 341)                                           # referenced only by signatures that retire
    rng = np.random.default_rng(8)

    def sig(s, b):
        w = list(rng.integers(2, 300, 10)) + [E]
        if b == 0 and s % 4 == 0:
            w += [X] * (300 if s < 12 else 1 + s % 3)
        if b == 0 and s < 10:
            w += [int(r) for r in R1[(s * 4) % 40:(s * 4) % 40 + 4]] + ([int(R1[s])] * 300 if s < 3 else [])
        return np.sort(np.array(w, np.int32))
    ix = _Sim(vocab_words=400)
    ix.add_bulk([sig(s, b) for b in range(3) for s in range(R)] + [sig(s, 3) for s in range(20)])
    assert ix.eng.stats()["buckets_sealed"] == 3
    q0 = np.concatenate([[X] * 400, R1, R1[:3].repeat(300), np.arange(2, 60), [E]]).astype(np.int32)
    ix.check(q0)
    gone = list(range(12)) + list(range(R, 2 * R)) + [3 * R + 4, 3 * R + 9]      # sealed bucket 0; bucket 1 entirely (dead); the open one
    for k in gone:
        ix.retire(k)
    ix.check(q0)
    assert all(ix.eng.word_nrefs(int(w)) == 0 for w in R1)
    ix.eng.vocab_remove(R1.astype(np.int32))
    ix.eng.vocab_rebuild()
    ix.eng.synchronize()
    new = np.arange(401, 441, dtype=np.int32)
    ix.eng.vocab_append(synth.vocab_surf(40, seed=9), new)             # they take the freed keys, which bucket 0 still lists
    for s in range(30):
        ix.add(np.sort(np.concatenate([rng.choice(new, 6, replace=False), rng.integers(2, 300, 4), [E]])).astype(np.int32))
    ix.eng.vocab_append(synth.vocab_surf(1, seed=10), R1[:1].astype(np.int32))   # a removed word created again
    ix.add(np.array([R1[0]] * 3 + [5], np.int32))
    q = np.concatenate([new, new[:5], [X] * 3, np.arange(2, 40), R1]).astype(np.int32)
    got = ix.check(q, np.concatenate([ix.all_ids(), [10 ** 6, -1, 0]]))          # unknown ids, the virtual place
    assert (got[0][gone] == 0).all() and (got[0][-3:] == 0).all() and (got[2][-3:] == 0).all() and got[1][-4] == 2
    ix.close()


# ------------------------------------------------------------------------------------------------------------ 8. no interference
def test_likelihood_is_the_same_before_and_after():
    rng = np.random.default_rng(12)
    words = synth.zipf_words(600, 80, 2000, seed=13)
    ix = _Sim()
    ix.add_bulk(list(words))
    q = words[77]
    before = ix.eng.likelihood(q, ix.all_ids(), 600.0)
    ix.check(rng.integers(1, 2001, 500))
    ix.check(q)
    np.testing.assert_array_equal(ix.eng.likelihood(q, ix.all_ids(), 600.0), before)
    assert before.max() > 0
    ix.close()


def test_pipelined_frames_are_undisturbed():
    """a similarity call between the frames of a pipelined handle (it completes what the handle owes, then runs its own launches): the
    frames' word ids and likelihoods equal an undisturbed twin's"""
    import rtabmap_amd
    n_words, q, n_sig, T = 6000, 200, 600, 8
    vocab = synth.vocab_surf(n_words, seed=41)
    words = synth.zipf_words(n_sig, q, n_words, seed=42)
    ids = np.arange(1, n_words + 1, dtype=np.int32)
    frames = [torch.from_numpy(synth.frame_from_signature(vocab, words[(37 * t) % n_sig], seed=50 + t)).cuda() for t in range(T)]
    out, sims = {}, []
    for disturbed in (0, 1):
        eng = rtabmap_amd.Engine("f32", 64, sig_capacity=n_sig + T, pipeline=True)
        eng.vocab_append(vocab, ids)
        eng.sig_add_bulk(np.arange(1, n_sig + 1, dtype=np.int32), np.arange(0, (n_sig + 1) * q, q, dtype=np.int64), words.reshape(-1))
        cap = n_sig + T
        d_w = torch.zeros((T, q), dtype=torch.int32, device="cuda")
        d_l = torch.zeros((T, cap), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for t in range(T):
            eng.frame_dev(frames[t].data_ptr(), q, n_sig + 1 + t, float(n_sig + 1 + t), d_w[t].data_ptr(), d_l[t].data_ptr(), cap,
                          first_new_word_id=n_words + 1 + t * q)
            if disturbed and t in (2, 3, 6):
                sims.append(eng.similarity(words[5], np.arange(1, n_sig + 1, dtype=np.int32), with_counts=True))
        eng.synchronize()
        out[disturbed] = (d_w.cpu().numpy(), d_l.cpu().numpy())
        eng.close()
    np.testing.assert_array_equal(out[1][0], out[0][0])
    np.testing.assert_array_equal(out[1][1], out[0][1])
    assert out[0][1].max() > 0
    exp = M.similarity_closed_form(words[5], list(words))              # (and the calls themselves saw the bulk-loaded signatures right)
    for s in sims:
        for k in range(3):
            np.testing.assert_array_equal(s[k], exp[k])


# -------------------------------------------------------------------------------------------------------- 9. lazy valid-word counts
def test_valid_word_counts_follow_newly_sealed_buckets():
    words = list(synth.zipf_words(600, 70, 1500, seed=21))
    words[300] = np.concatenate([words[300][:40], np.full(30, -1)]).astype(np.int32)
    q = np.concatenate([words[10], words[400][:30]]).astype(np.int32)
    ix = _Sim()
    ix.add_bulk(words[:300])                                           # bucket 0 sealed
    first = ix.check(q)
    ix.add_bulk(words[300:])                                           # bucket 1 sealed behind the first call
    ix.retire(20)
    again = ix.check(q)
    np.testing.assert_array_equal(again[0][:300][np.arange(300) != 20], first[0][np.arange(300) != 20])
    fresh = _Sim()
    fresh.add_bulk(words)
    fresh.retire(20)
    once = fresh.check(q)
    for k in range(3):
        np.testing.assert_array_equal(again[k], once[k])
    assert ix.eng.stats()["buckets_sealed"] == 2
    ix.close()
    fresh.close()


# ----------------------------------------------------------------------------------------------------------- 10. registration paths
def test_registration_paths_build_the_same_index():
    """lcd_sig_add, lcd_sig_add_bulk and frames through lcd_frame_dev (first_new_word_id > 0: the ids of the words a frame creates are
    known here) register the same signatures: the same bits"""
    import rtabmap_amd
    n_words, q, n_sig = 3000, 60, 270
    vocab = synth.vocab_surf(n_words, seed=31)
    base = synth.zipf_words(n_sig, q, n_words, seed=32)
    eng = rtabmap_amd.Engine("f32", 64, sig_capacity=n_sig + 8)
    eng.vocab_append(vocab, np.arange(1, n_words + 1, dtype=np.int32))
    d_w = torch.zeros(q, dtype=torch.int32, device="cuda")
    d_l = torch.zeros(n_sig + 8, dtype=torch.float32, device="cuda")
    sigs = []
    for s in range(n_sig):
        d = torch.from_numpy(synth.frame_from_signature(vocab, base[s], seed=100 + s)).cuda()
        first_new = n_words + 1 + s * q
        eng.frame_dev(d.data_ptr(), q, s + 1, float(s + 1), d_w.data_ptr(), d_l.data_ptr(), n_sig + 8, first_new_word_id=first_new)
        eng.synchronize()
        w = d_w.cpu().numpy()
        sigs.append(np.where(w < 0, first_new - 1 - w, w).astype(np.int32))       # code -(k + 1): the frame's k-th new word
    assert eng.stats()["buckets_sealed"] == 1 and any((s > n_words).any() for s in sigs)
    one, bulk = _Sim(), _Sim()
    for s in sigs:
        one.add(s)
    bulk.add_bulk(sigs)
    rng = np.random.default_rng(33)
    all_ids = np.arange(1, n_sig + 1, dtype=np.int32)
    for qq in (sigs[5], sigs[260], np.concatenate([sigs[100], sigs[200], sigs[200]]), rng.integers(1, n_words + 1, 400).astype(np.int32),
               np.concatenate(sigs)[::3][:8192]):
        a = one.check(qq)
        b = bulk.check(qq)
        c = eng.similarity(qq, all_ids, with_counts=True)
        for k in range(3):
            np.testing.assert_array_equal(b[k], a[k])
            np.testing.assert_array_equal(c[k], a[k])
    eng.close()
    one.close()
    bulk.close()


# ------------------------------------------------------------------------------------------------------------ 11. device entry
def test_similarity_dev_equals_the_host_entry():
    from rtabmap_amd.capi import LcdError
    words = list(synth.zipf_words(600, 70, 1500, seed=21))
    ix = _Sim()
    ix.add_bulk(words)
    for k in (3, 299, 580):
        ix.retire(k)
    n = 600                                                            # signatures were added in slot order: slot = id - 1
    d_out = torch.full((n + 5,), -1.0, dtype=torch.float32, device="cuda")
    for q in (words[10], np.concatenate([words[400], words[400], [-1, 99999]]).astype(np.int32), np.zeros(0, np.int32)):
        d_q = torch.from_numpy(np.ascontiguousarray(q, np.int32)).cuda()
        d_out.fill_(-1.0)
        ix.eng.similarity_dev(d_q, d_out)
        ix.eng.synchronize()
        got = d_out.cpu().numpy()
        np.testing.assert_array_equal(got[:n], ix.check(q)[0])         # every slot written, retired ones 0
        assert (got[n:] == -1).all()
    with pytest.raises(LcdError) as e:
        ix.eng.similarity_dev(d_q, d_out[:n - 1])
    assert e.value.status == LCD_ERR_INVALID
    ix.check(words[10])
    ix.close()


# --------------------------------------------------------------------------------------------------------------- 12. host mirror
def test_host_mirror_similarity_branch():
    """MemoryHip with Kp/TfIdfLikelihoodUsed=false: computeLikelihood over a stream of 600 signatures (and of frames through update(),
    whose device call brings a TF-IDF likelihood back that must not be used) equals the model, the virtual place -1 maps to 0;
    compareTo on consecutive signatures equals the literal restatement; with the parameter true nothing changes"""
    from rtabmap_amd.vwdictionary import MemoryHip
    n_words = 800
    vocab = synth.vocab_surf(n_words, seed=51)
    words = synth.zipf_words(600, 50, n_words, seed=52).astype(np.int32)
    words[::7, :5] = -1                                                # features without a word
    h = MemoryHip(nndr=0.8)
    for i, r in enumerate(vocab):
        h.vwd.add_word(i + 1, r)
    h.vwd.update()
    sigs = {}
    rng = np.random.default_rng(53)

    def check(q, n_now):
        ids = np.concatenate([[-1], np.arange(1, n_now + 1)]).astype(np.int32)
        oi, got = h.compute_likelihood(np.asarray(q, np.int32), ids)
        exp = M.similarity_closed_form(q, [None] + [sigs[i] for i in range(1, n_now + 1)])[0]
        np.testing.assert_array_equal(oi, ids)
        np.testing.assert_array_equal(got, exp)
        assert got[0] == 0

    tfidf_q = words[3]
    for s in range(600):
        assert h.add_signature(words[s], s + 1) == s + 1
        sigs[s + 1] = words[s]
        if s + 1 == 100:
            ids100 = np.arange(1, 101, dtype=np.int32)
            tfidf_before = h.compute_likelihood(tfidf_q, ids100)[1]
            assert tfidf_before.max() > 0
            h.set_tfidf_likelihood_used(False)
            check(words[3], 100)
            h.set_tfidf_likelihood_used(True)                          # with the parameter true nothing changes
            np.testing.assert_array_equal(h.compute_likelihood(tfidf_q, ids100)[1], tfidf_before)
            h.set_tfidf_likelihood_used(False)
        if s + 1 in (300, 600):
            check(words[s], s + 1)
            check(np.concatenate([words[5], words[5], rng.integers(-1, 2000, 40)]), s + 1)
    for a in range(560, 600):                                          # Memory::rehearsal compares the new signature with the one before it
        sim = M.compare_to_literal(sigs[a + 1], sigs[a])[0]
        assert np.float32(h.compare_to(a + 1, a)).tobytes() == np.float32(sim).tobytes()
    assert h.compare_to(5, 5) == 1.0 and h.compare_to(5, 10 ** 6) == 0.0 and h.compare_to(5, -1) == 0.0
    # frames through update(): one device call registers the signature and brings its TF-IDF likelihood back
    n = 600
    for t in range(4):
        desc = synth.frame_from_signature(vocab, np.abs(words[40 + t]) % n_words + 1, seed=60 + t)
        sid, wid = h.update(desc)
        n += 1
        assert sid == n
        sigs[n] = np.array(wid, np.int32)
        ids = np.concatenate([[-1], np.arange(1, n + 1)]).astype(np.int32)
        oi, got = h.compute_likelihood_of(sid, ids)
        exp = M.similarity_closed_form(sigs[n], [None] + [sigs[i] for i in range(1, n + 1)])[0]
        np.testing.assert_array_equal(got, exp)
        assert got[-1] == 1.0
    h.close()


# ------------------------------------------------------------------------------------------------------------------------ 13. fuzz
def test_fuzz_zipf_word_lists():
    """700 signatures (two sealed buckets and an open one) of random length over a Zipf vocabulary, 20 queries"""
    rng = np.random.default_rng(71)
    pool = synth.zipf_words(700, 120, 3000, seed=72)
    sigs = []
    for s in range(700):
        w = pool[s][: int(rng.integers(20, 121))].copy()
        w[rng.random(w.size) < 0.05] = -1
        if s % 50 == 0:
            w = np.concatenate([w, np.full(int(rng.integers(200, 400)), w[0] if w[0] > 0 else 1)])
        sigs.append(w.astype(np.int32))
    ix = _Sim()
    ix.add_bulk(sigs[:400])
    for s in sigs[400:420]:
        ix.add(s)
    ix.add_bulk(sigs[420:])
    assert ix.eng.stats()["buckets_sealed"] == 2
    for k in (17, 300, 650):
        ix.retire(k)
    for t in range(20):
        parts = [sigs[int(rng.integers(0, 700))] for _ in range(int(rng.integers(1, 4)))] + [rng.integers(-1, 3500, int(rng.integers(0, 200)))]
        if t % 4 == 0:
            parts.append(np.full(int(rng.integers(250, 600)), sigs[(t // 4) * 50][0]))
        ix.check(rng.permutation(np.concatenate(parts))[:8192])
    ix.close()
