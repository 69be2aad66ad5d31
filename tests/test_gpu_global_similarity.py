"""GPU tests of the global-descriptor branch of Signature::compareTo (lcd_compare_to / lcd_compare_to_dev, lcd_sig_set_globals*,
rtabmap_amd/csrc/global_similarity.hip) against tests/global_similarity_model.py.

The float summation order of cv::Mat::dot is not part of the reference tree, so the engine defines its own (include/lcd.h): what is
tested is (a) exact results wherever every product and partial sum is exact in fp32 -- assert_array_equal, (b) that the order is a
function of the channel's dim alone -- bit equality across slots, index sizes, entry points and operand order, (c) random unit vectors
within the bound the model computes from the data (never a hand-picked tolerance), and (d) that wherever no channel matches the value is
lcd_similarity's, bit for bit.  At most 600 slots, under 40 MB per test."""
import numpy as np
import pytest
import torch  # noqa: F401  (before liblcd_hip.so is loaded: one HIP runtime per process, rtabmap_amd/capi.py)

import global_similarity_model as G
from rtabmap_amd import synth

pytestmark = pytest.mark.gpu
LCD_ERR_INVALID, LCD_ERR_STATE, LCD_ERR_UNSUPPORTED = 1, 4, 5
DIMS = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 4096, 16384]


def _unit(rng, dim, signed=True):
    v = rng.standard_normal(dim) if signed else rng.random(dim)
    return (v / np.linalg.norm(v)).astype(np.float32)


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


class _Index:
    """signatures 1, 2, ... (slot = id - 1) in a HIP engine, and what the model needs of them: words, global descriptors, retired or not"""

    def __init__(self, **kw):
        import rtabmap_amd
        self.eng = rtabmap_amd.Engine("f32", 64, **kw)
        self.words, self.globs, self.gone = [], [], []

    def add(self, words, globs=None, how="host"):
        words = np.asarray(words, np.int32)
        sid = len(self.words) + 1
        self.eng.sig_add(sid, words)
        self.words.append(words)
        self.globs.append([])
        self.gone.append(False)
        if globs is not None:
            self.set(sid, globs, how)
        return sid

    def set(self, sid, globs, how="host"):
        if how == "host":
            self.eng.sig_set_globals(sid, globs)
        else:
            def dev(row):
                return None if row is None else torch.from_numpy(np.asarray(row, np.float32)).cuda()
            self.eng.sig_set_globals_dev(sid, [(g[0], dev(g[1])) if isinstance(g, tuple) else dev(g) for g in globs])
            self.eng.synchronize()
        self.globs[sid - 1] = list(globs)

    def ids(self):
        return np.arange(1, len(self.words) + 1, dtype=np.int32)

    def model(self, q_words, q_globs, ids=None):
        ids = self.ids() if ids is None else np.asarray(ids, np.int32)
        sim, cnt, bound = np.zeros(ids.size), np.zeros(ids.size, np.int32), np.zeros(ids.size)
        for k, i in enumerate(ids.tolist()):
            if 0 < i <= len(self.words) and not self.gone[i - 1]:
                sim[k], cnt[k], bound[k] = G.compare_to_full(q_words, q_globs, self.words[i - 1], self.globs[i - 1])
        return sim, cnt, bound

    def check(self, q_words, q_globs, ids=None):
        """lcd_compare_to against the model: totalDescs equal, |got - sim64| <= bound, and lcd_similarity's bits wherever totalDescs == 0.
        Returns (got, counts, largest err / bound)"""
        ids = self.ids() if ids is None else np.asarray(ids, np.int32)
        q_words = np.asarray(q_words, np.int32)
        got, cnt = self.eng.compare_to(q_words, q_globs, ids, with_counts=True)
        sim, ecnt, bound = self.model(q_words, q_globs, ids)
        np.testing.assert_array_equal(cnt, ecnt)
        err = np.abs(got.astype(np.float64) - sim)
        assert (err <= bound).all(), (err.max(), bound[np.argmax(err - bound)])
        words_only = self.eng.similarity(q_words, ids)
        np.testing.assert_array_equal(_bits(got[cnt == 0]), _bits(words_only[cnt == 0]))
        np.testing.assert_array_equal(_bits(self.eng.compare_to(q_words, q_globs, ids)), _bits(got))       # (without the counts)
        m = cnt > 0
        return got, cnt, float((err[m] / bound[m]).max()) if m.any() else 0.0

    def close(self):
        self.eng.close()


def _one_hot(dim, k, v=1.0):
    e = np.zeros(dim, np.float32)
    e[k] = v
    return e


# --------------------------------------------------------------------------------------------------------------- 1. exact indexing
@pytest.mark.parametrize("dim", DIMS)
def test_exact_indexing(dim):
    """the stored row is r_i = (i + 1) * 2^-15 and the query one-hot: every product and partial sum is exact, so the result is
    ((k + 1) * 2^-15 + 1) / 2 in ANY summation order -- a dropped tail, a wrong stride or leaking padding shows as a wrong integer"""
    ix = _Index()
    ramp = ((np.arange(dim) + 1) * 2.0 ** -15).astype(np.float32)
    last = dim - 1
    ix.add([1, 2], [ramp])
    ix.add([1, 3], [_one_hot(dim, last)])
    ix.add([4], [_one_hot(dim, last, -1.0)])
    ks = range(dim) if dim <= 257 else sorted({0, 1, 3, 4, 63, 64, dim // 2, dim - 2, dim - 1})
    for k in ks:
        got, cnt = ix.eng.compare_to(np.array([1], np.int32), [_one_hot(dim, k)], ix.ids(), with_counts=True)
        d = 1.0 if k == last else 0.0
        exp = np.array([((k + 1) * 2.0 ** -15 + 1.0) / 2.0, (d + 1.0) / 2.0, (-d + 1.0) / 2.0], np.float32)
        np.testing.assert_array_equal(got, exp)
        np.testing.assert_array_equal(cnt, [1, 1, 1])
    got = ix.eng.compare_to(np.zeros(0, np.int32), [_one_hot(dim, last)], ix.ids())      # a against a: 1.0, a against -a: 0.0
    assert got[1] == 1.0 and got[2] == 0.0
    ix.close()


# -------------------------------------------------------------------------------------------- 2. the order is a function of dim alone
@pytest.mark.parametrize("dim", [257, 4096])
def test_order_is_a_function_of_dim_alone(dim):
    rng = np.random.default_rng(20 + dim)
    a, b = _unit(rng, dim), _unit(rng, dim)
    same = (0, 1, 255, 256, 257, 599)                                  # across the 256-slot bucket boundary
    results = {}
    for n in (600, 7):
        import rtabmap_amd
        eng = rtabmap_amd.Engine("f32", 64)
        ids = np.arange(1, n + 1, dtype=np.int32)
        eng.sig_add_bulk(ids, np.arange(n + 1, dtype=np.int64) * 2, (np.arange(2 * n) % 40 + 1).astype(np.int32))
        rows = np.stack([_unit(rng, dim) for _ in range(n)])
        at = [s for s in same if s < n] if n == 600 else [3]
        rows[at] = b
        eng.sig_set_global_bulk(0, ids, rows)
        got = eng.compare_to(np.array([1], np.int32), [a], ids)
        assert len(set(_bits(got[at]).tolist())) == 1
        results[n] = got[at[0]]
        # a against stored b == b against stored a
        eng.sig_set_globals(int(ids[2]), [a])
        assert _bits(eng.compare_to(np.array([1], np.int32), [b], ids[2:3]))[0] == _bits(got[at[0]])
        sim, _, bound = G.compare_to_full([], [a], [], [b])
        assert abs(float(got[at[0]]) - sim) <= bound
        eng.close()
    assert _bits(results[600]) == _bits(results[7])


# ------------------------------------------------------------------------------------------------------------ 3. entry points agree
def test_entry_points_agree():
    rng = np.random.default_rng(3)
    dim, n = 257, 20
    rows = np.stack([_unit(rng, dim) for _ in range(n)])
    ix = _Index()
    for how in ("host", "dev"):
        for k in range(n):
            ix.add([1 + k, 2 + k, 50], [rows[k]], how)
    for k in range(n):
        ix.add([1 + k, 2 + k, 50])
    ix.eng.sig_set_global_bulk(0, np.arange(2 * n + 1, 3 * n + 1, dtype=np.int32), rows)
    for k in range(n):
        ix.globs[2 * n + k] = [rows[k]]
    ix.add([50, 51])                                                   # one without a row: the words branch
    ix.eng.sig_remove(5)
    ix.gone[4] = True
    q_words, q = np.array([50, 3, 4], np.int32), _unit(rng, dim)
    got, cnt, _ = ix.check(q_words, [q])
    np.testing.assert_array_equal(_bits(got[n:2 * n]), _bits(got[2 * n:3 * n]))
    keep = np.arange(n) != 4
    np.testing.assert_array_equal(_bits(got[:n][keep]), _bits(got[n:2 * n][keep]))
    assert got[4] == 0 and cnt[4] == 0 and cnt[-1] == 0 and got[-1] > 0
    # the device entry: dense over the slots (slot = id - 1), every slot written
    d_out = torch.full((3 * n + 6,), -1.0, dtype=torch.float32, device="cuda")
    ix.eng.compare_to_dev(torch.from_numpy(q_words).cuda(), [torch.from_numpy(q).cuda()], d_out)
    ix.eng.synchronize()
    dense = d_out.cpu().numpy()
    np.testing.assert_array_equal(_bits(dense[:3 * n + 1]), _bits(got))
    assert (dense[3 * n + 1:] == -1).all()
    ix.close()


# ------------------------------------------------------------------------------------------------------------ 4. random unit vectors
@pytest.mark.parametrize("signed", [True, False])
@pytest.mark.parametrize("dim", [64, 257, 4096])
def test_random_unit_vectors_within_the_bound(dim, signed):
    rng = np.random.default_rng(40 + dim + int(signed))
    n = 300
    ix = _Index()
    ids = np.arange(1, n + 1, dtype=np.int32)
    ix.eng.sig_add_bulk(ids, np.arange(n + 1, dtype=np.int64) * 3, (np.arange(3 * n) % 70 + 1).astype(np.int32))
    rows = np.stack([_unit(rng, dim, signed) for _ in range(n)])
    ix.eng.sig_set_global_bulk(0, ids, rows)
    for s in range(n):
        ix.words.append((np.arange(3 * s, 3 * s + 3) % 70 + 1).astype(np.int32))
        ix.globs.append([rows[s]])
        ix.gone.append(False)
    worst = 0.0
    for q in (_unit(rng, dim, signed), rows[17], -rows[100] if signed else rows[100]):
        got, cnt, ratio = ix.check([1, 2], [q])
        assert (cnt == 1).all()
        worst = max(worst, ratio)
    print("dim %d %s: largest err / bound = %.4f" % (dim, "signed" if signed else "non-negative", worst))
    assert worst < 1.0
    ix.close()


# ---------------------------------------------------------------------------------------------------------------------- 5. fallback
def test_fallback_to_the_words_branch():
    rng = np.random.default_rng(5)
    dim = 65
    base = synth.zipf_words(300, 30, 400, seed=51)
    ix = _Index()
    for s in range(300):
        w = base[s]
        if s % 6 == 0:
            ix.add(w, [_unit(rng, dim)])                               # a row
        elif s % 6 == 1:
            ix.add(w)                                                  # never had one
        elif s % 6 == 2:
            ix.add(w, [(0, _unit(rng, dim))])                          # type 0: stored as absent
        elif s % 6 == 3:
            sid = ix.add(w, [_unit(rng, dim)])                         # cleared again
            ix.eng.sig_clear_globals(sid)
            ix.globs[sid - 1] = []
        elif s % 6 == 4:
            ix.add(w, [(0, None), _unit(rng, 8)])                      # a row on a channel the query lacks
        else:
            ix.add(w, [_unit(rng, dim), _unit(rng, 8)])
    bad = ix.add(np.array([-1, -2, 0], np.int32), [_unit(rng, dim)])   # invalid word ids only, with a row: isBadSignature does not matter there
    again = ix.add(base[7], [_unit(rng, dim)])                         # a row replaced by "none": set_globals replaces every channel
    ix.set(again, [])
    for sid in (1, 2, 7, 260, 300):                                    # retired: with a row, without, sealed bucket, open bucket
        ix.eng.sig_remove(sid)
        ix.gone[sid - 1] = True
    assert ix.eng.stats()["buckets_sealed"] == 1
    q_words, q = np.concatenate([base[12], base[13][:10]]).astype(np.int32), _unit(rng, dim)
    ids = np.concatenate([ix.ids(), [10 ** 6, 0, -1]]).astype(np.int32)
    got, cnt, _ = ix.check(q_words, [q], ids)
    assert cnt[bad - 1] == 1 and got[bad - 1] != 0 and cnt[again - 1] == 0
    assert (got[[0, 1, 6, 259, 299]] == 0).all() and (got[-3:] == 0).all() and (cnt[-3:] == 0).all()
    assert set(np.unique(cnt).tolist()) == {0, 1}
    got2, cnt2, _ = ix.check(q_words, [q, _unit(rng, 8)], ids)         # the query with both channels
    assert set(np.unique(cnt2).tolist()) == {0, 1, 2}
    # no query descriptors at all, type 0, or a channel the handle has never stored a row on: lcd_similarity everywhere
    sim = ix.eng.similarity(q_words, ids)
    for qg in ([], [(0, q)], [(0, None)], [(0, None), (0, None), _unit(rng, 33)]):
        g, c = ix.eng.compare_to(q_words, qg, ids, with_counts=True)
        np.testing.assert_array_equal(_bits(g), _bits(sim))
        assert (c == 0).all()
    assert sim.max() > 0
    ix.close()


# ------------------------------------------------------------------------------------------------- 6. two channels of different dims
def test_two_channels_of_different_dims():
    rng = np.random.default_rng(6)
    d0, d1 = 64, 257
    ix = _Index()
    for s in range(280):
        w = [1 + s % 30, 2 + s % 7, 40]
        k = s % 4
        g = [[_unit(rng, d0), _unit(rng, d1)], [_unit(rng, d0)], [(0, None), _unit(rng, d1)], None][k]
        ix.add(w, g)
    q0, q1 = _unit(rng, d0), _unit(rng, d1)
    got, cnt, ratio = ix.check([40, 1], [q0, q1])
    np.testing.assert_array_equal(cnt, np.array([2, 1, 1, 0] * 70))
    assert ratio < 1.0
    ix.check([40, 1], [q0])
    ix.check([40, 1], [(0, None), q1])
    ix.close()
    # exact dyadic rows (every entry +-2^-1 .. 2^-4: all products and partial sums are multiples of 2^-8 below 2^7, exact in fp32 in any
    # order; not unit vectors, which the engine answers as computed): the mean over the matching count, bit for bit
    def dyadic(dim, key):
        i = np.arange(dim)
        return (np.where((i * 7 + key) % 3 == 0, -1.0, 1.0) * 2.0 ** -(1 + (i * 3 + key) % 4)).astype(np.float32)
    ix = _Index()
    for s in range(40):
        g0, g1 = dyadic(d0, s), dyadic(d1, 5 * s + 1)
        ix.add([1, 2], [[g0, g1], [g0], [(0, None), g1], []][s % 4])
    for key in (0, 3, 8, 63):
        qg = [dyadic(d0, key + 2), dyadic(d1, key)]
        got, cnt = ix.eng.compare_to(np.array([1], np.int32), qg, ix.ids(), with_counts=True)
        sim, ecnt, _ = ix.model([1], qg)
        np.testing.assert_array_equal(cnt, ecnt)
        m = cnt > 0
        assert m.sum() == 30 and np.unique(sim[m]).size > 5
        assert (sim[m].astype(np.float32).astype(np.float64) == sim[m]).all()   # every value a dyadic fraction: the cast is exact
        np.testing.assert_array_equal(got[m], sim[m].astype(np.float32))
    ix.close()


# ------------------------------------------------------------------------------------------------------------------------ 7. growth
def test_rows_survive_growth():
    rng = np.random.default_rng(7)
    dim = 63
    ix = _Index(sig_capacity=4)
    q = _unit(rng, dim)
    first = None
    for s in range(300):
        ix.add([1 + s % 9, 20 + s % 5], [_unit(rng, dim)])             # the row right behind lcd_sig_add
        if s == 3:
            first = ix.eng.compare_to(np.array([1], np.int32), [q], ix.ids())
    assert ix.eng.stats()["buckets_sealed"] == 1
    got, cnt, ratio = ix.check([1], [q])                               # the sealed bucket's signatures and the open bucket's
    assert (cnt == 1).all() and ratio < 1.0
    np.testing.assert_array_equal(_bits(got[:4]), _bits(first))
    ix.close()


# ------------------------------------------------------------------------------------------------------------------------ 8. errors
def test_errors_leave_the_handle_usable():
    from rtabmap_amd.capi import LcdError
    rng = np.random.default_rng(8)
    dim = 5
    ix = _Index()
    for s in range(6):
        ix.add([1 + s, 9], [_unit(rng, dim)])
    ix.eng.sig_remove(6)
    ix.gone[5] = True
    q = _unit(rng, dim)
    before, _, _ = ix.check([9], [q])
    row = _unit(rng, dim)

    def refused(status, fn):
        with pytest.raises(LcdError) as e:
            fn()
        assert e.value.status == status and len(str(e.value).split(": ", 1)[1]) > 0        # last_error is not empty
        np.testing.assert_array_equal(_bits(ix.check([9], [q])[0]), _bits(before))         # nothing was stored, the handle answers

    five = [row] * 5
    for fn in (ix.eng.sig_set_globals, lambda i, g: ix.eng.sig_set_globals_dev(i, [torch.from_numpy(np.asarray(x, np.float32)).cuda() for x in g])):
        refused(LCD_ERR_STATE, lambda: fn(77, [row]))                                      # unknown signature
        refused(LCD_ERR_STATE, lambda: fn(6, [row]))                                       # retired signature
        refused(LCD_ERR_UNSUPPORTED, lambda: fn(1, five))                                  # n > 4
        refused(LCD_ERR_UNSUPPORTED, lambda: fn(1, [np.zeros(16385, np.float32)]))         # dim > 16384
        refused(LCD_ERR_INVALID, lambda: fn(1, [_unit(rng, dim + 1)]))                     # not the channel's dim
        refused(LCD_ERR_INVALID, lambda: fn(1, [np.zeros(0, np.float32)]))                 # type 1 with dim 0 / no data
    refused(LCD_ERR_INVALID, lambda: ix.eng.sig_set_globals(1, [(1, None)]))
    refused(LCD_ERR_INVALID, lambda: ix.eng.sig_set_globals(2, [row, np.zeros(0, np.float32)]))   # (the valid first entry is not stored either)
    refused(LCD_ERR_STATE, lambda: ix.eng.sig_clear_globals(77))
    ids3 = np.array([1, 2, 3], np.int32)
    refused(LCD_ERR_STATE, lambda: ix.eng.sig_set_global_bulk(0, np.array([1, 77], np.int32), np.stack([row, row])))
    refused(LCD_ERR_UNSUPPORTED, lambda: ix.eng.sig_set_global_bulk(4, ids3, np.stack([row] * 3)))
    refused(LCD_ERR_UNSUPPORTED, lambda: ix.eng.sig_set_global_bulk(1, ids3, np.zeros((3, 16385), np.float32)))
    refused(LCD_ERR_INVALID, lambda: ix.eng.sig_set_global_bulk(0, ids3, np.zeros((3, dim + 2), np.float32)))
    refused(LCD_ERR_INVALID, lambda: ix.eng.sig_set_global_bulk(0, np.array([1, 1], np.int32), np.stack([row, row])))
    # the query obeys the same rules
    refused(LCD_ERR_UNSUPPORTED, lambda: ix.eng.compare_to([9], [q] * 5, ix.ids()))
    refused(LCD_ERR_UNSUPPORTED, lambda: ix.eng.compare_to([9], [np.zeros(16385, np.float32)], ix.ids()))
    refused(LCD_ERR_INVALID, lambda: ix.eng.compare_to([9], [_unit(rng, dim + 1)], ix.ids()))
    refused(LCD_ERR_INVALID, lambda: ix.eng.compare_to([9], [(1, None)], ix.ids()))
    refused(LCD_ERR_UNSUPPORTED, lambda: ix.eng.compare_to(np.arange(1, 8194, dtype=np.int32), [q], ix.ids()))
    d_q, d_w = torch.from_numpy(q).cuda(), torch.from_numpy(np.array([9], np.int32)).cuda()
    d_out = torch.zeros(8, dtype=torch.float32, device="cuda")
    refused(LCD_ERR_INVALID, lambda: ix.eng.compare_to_dev(d_w, [d_q], d_out[:5]))         # smaller than the slots in use
    refused(LCD_ERR_INVALID, lambda: ix.eng.compare_to_dev(d_w, [torch.zeros(dim + 3, dtype=torch.float32, device="cuda")], d_out))
    assert ix.eng.compare_to([9], [q], np.zeros(0, np.int32)).size == 0                    # n_ids == 0: LCD_OK
    # a query channel on which the handle never stored a row matches nothing, whatever its length
    g, c = ix.eng.compare_to([9], [q, _unit(rng, 99)], ix.ids(), with_counts=True)
    np.testing.assert_array_equal(_bits(g), _bits(before))
    # and a valid call after all of it stores and answers
    ix.set(1, [row])
    got, cnt, _ = ix.check([9], [row])
    assert cnt[0] == 1 and abs(got[0] - 1.0) < 1e-6
    ix.close()


def test_a_handle_without_rows_allocates_nothing():
    ix = _Index()
    for s in range(5):
        ix.add([1 + s, 9])
    b0 = ix.eng.stats()["bytes_device"]
    ix.eng.sig_clear_globals(2)
    ix.set(3, [(0, None)])
    sim = ix.eng.similarity([9], ix.ids())
    b1 = ix.eng.stats()["bytes_device"]
    np.testing.assert_array_equal(_bits(ix.eng.compare_to([9], [np.ones(4, np.float32)], ix.ids())), _bits(sim))
    assert ix.eng.stats()["bytes_device"] == b1                        # no row was ever stored: nothing was allocated for the comparison either
    ix.set(3, [np.ones(4, np.float32) / 2])
    assert ix.eng.stats()["bytes_device"] > b1 >= b0                   # the rows count in lcd_stats.bytes_device
    assert ix.check([9], [np.ones(4, np.float32) / 2])[1].tolist() == [0, 0, 1, 0, 0]
    ix.close()


# -------------------------------------------------------------------------------------------------------------- 9. pipelined handle
def test_pipelined_handle():
    """four frames in flight on a pipelined handle; a row attached to the newest frame's signature (the call completes what the handle
    owes, so the signature has its slot) answers, and the frames' word ids are those of a plain handle"""
    import rtabmap_amd
    n_words, q, n_sig, T, dim = 1024, 100, 40, 4, 257
    vocab = synth.vocab_surf(n_words, seed=91)
    words = synth.zipf_words(n_sig, q, n_words, seed=92)
    frames = [torch.from_numpy(synth.frame_from_signature(vocab, words[(7 * t) % n_sig], seed=93 + t)).cuda() for t in range(T)]
    rng = np.random.default_rng(9)
    rows = np.stack([_unit(rng, dim) for _ in range(n_sig)])
    new_row, qrow = _unit(rng, dim), _unit(rng, dim)
    out = {}
    for pipelined in (False, True):
        eng = rtabmap_amd.Engine("f32", 64, sig_capacity=n_sig + T, pipeline=pipelined)
        eng.vocab_append(vocab, np.arange(1, n_words + 1, dtype=np.int32))
        ids = np.arange(1, n_sig + 1, dtype=np.int32)
        eng.sig_add_bulk(ids, np.arange(0, (n_sig + 1) * q, q, dtype=np.int64), words.reshape(-1))
        eng.sig_set_global_bulk(0, ids, rows)
        cap = n_sig + T
        d_w = torch.zeros((T, q), dtype=torch.int32, device="cuda")
        d_l = torch.zeros((T, cap), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for t in range(T):
            eng.frame_dev(frames[t].data_ptr(), q, n_sig + 1 + t, float(n_sig + 1 + t), d_w[t].data_ptr(), d_l[t].data_ptr(), cap,
                          first_new_word_id=n_words + 1 + t * q)
        newest = n_sig + T
        eng.sig_set_globals(newest, [new_row])
        all_ids = np.arange(1, newest + 1, dtype=np.int32)
        got, cnt = eng.compare_to(words[3], [qrow], all_ids, with_counts=True)
        eng.synchronize()
        out[pipelined] = (d_w.cpu().numpy(), got, cnt)
        eng.close()
    np.testing.assert_array_equal(out[True][0], out[False][0])         # the word ids of the frames
    np.testing.assert_array_equal(_bits(out[True][1]), _bits(out[False][1]))
    got, cnt = out[True][1], out[True][2]
    np.testing.assert_array_equal(cnt, [1] * n_sig + [0] * (T - 1) + [1])
    for k, r in ((0, rows[0]), (n_sig - 1, rows[-1]), (n_sig + T - 1, new_row)):
        sim, _, bound = G.compare_to_full([], [qrow], [], [r])
        assert abs(float(got[k]) - sim) <= bound


# ----------------------------------------------------------------------------------------------------------------------- 10. mirror
def test_host_mirror():
    """MemoryHip with Kp/TfIdfLikelihoodUsed=false: computeLikelihood(signature, ids) returns the floats of Engine.compare_to on a twin
    index, compareTo is symmetric, a forgotten signature loses its descriptors"""
    import rtabmap_amd
    from rtabmap_amd.vwdictionary import MemoryHip
    n_words, n, dim = 300, 60, 65
    vocab = synth.vocab_surf(n_words, seed=101)
    words = synth.zipf_words(n, 25, n_words, seed=102).astype(np.int32)
    rng = np.random.default_rng(10)
    h = MemoryHip(nndr=0.8)
    for i, r in enumerate(vocab):
        h.vwd.add_word(i + 1, r)
    h.vwd.update()
    h.set_tfidf_likelihood_used(False)
    twin = _Index()
    globs = {}
    for s in range(n):
        assert h.add_signature(words[s], s + 1) == s + 1
        g = [[_unit(rng, dim)], [], [(0, _unit(rng, dim))], [_unit(rng, dim), _unit(rng, 8)]][s % 4]
        globs[s + 1] = g
        if g:
            assert h.set_global_descriptors(s + 1, g)
        twin.add(words[s], g if g else None)
    assert h.num_global_descriptors(4) == 2 and h.num_global_descriptors(2) == 0
    assert not h.set_global_descriptors(10 ** 6, [_unit(rng, dim)]) and not h.set_global_descriptors(1, [_unit(rng, dim)] * 5)
    ids = np.concatenate([[-1], np.arange(1, n + 1)]).astype(np.int32)
    for sid in (1, 2, 3, 4, 57):
        oi, got = h.compute_likelihood_of(sid, ids)
        exp, cnt = twin.eng.compare_to(words[sid - 1], globs[sid], ids, with_counts=True)
        np.testing.assert_array_equal(oi, ids)
        np.testing.assert_array_equal(_bits(got), _bits(exp))
        assert got[0] == 0 and (cnt.max() > 0) == (sid in (1, 4, 57))
    twin.check(words[0], globs[1])                                     # (and the twin is right)
    for a, b in ((1, 5), (4, 8), (1, 4), (2, 5), (3, 7), (4, 4)):
        ab, ba = h.compare_to(a, b), h.compare_to(b, a)
        assert _bits(ab) == _bits(ba)
        assert _bits(ab) == _bits(twin.eng.compare_to(words[a - 1], globs[a], np.array([b], np.int32))[0])
    # a signature whose descriptors are replaced or cleared
    new = [_unit(rng, dim)]
    assert h.set_global_descriptors(5, new) and h.set_global_descriptors(9, [])
    twin.set(5, new)
    twin.set(9, [])
    oi, got = h.compute_likelihood_of(1, ids)
    np.testing.assert_array_equal(_bits(got), _bits(twin.eng.compare_to(words[0], globs[1], ids)))
    # forget(): the node leaves, with its descriptors
    h.forget(13)
    assert h.num_global_descriptors(13) == 0
    twin.eng.sig_remove(13)
    oi, got = h.compute_likelihood_of(1, ids)
    np.testing.assert_array_equal(_bits(got), _bits(twin.eng.compare_to(words[0], globs[1], ids)))
    assert got[13] == 0
    h.close()
    twin.close()
