"""The decision stage (rtabmap_amd/csrc/bayes.hip) at the sizes where its launch plan and its neighbour lists change shape: one workgroup and
two, 256 partials and 257 (the fold's PER branch), 1024 workgroups and the grid-stride loop's second and third trip; neighbour lists of 47,
48, 49, 64, 65, 96, 97 and 165 entries (one round trip of the list walk, two, four; the table's width K 64 -> 128 -> 256); the tables'
growth from 4096 to 8192 slots under a live filter; the "all other places" fill past one wave of workgroups.

The likelihood statistics are compared with tests/decision_model.py (exact sums, float32 statement by statement, the device's error bounds as
functions of the input), the posteriors with the oracle's BayesFilter through tests/bayes_checks.py, under the project's tolerances.  Every case
prints its figures (lines starting with "decision-stage") before it asserts; profiles/decision_stage.txt is such a run."""
import time

import numpy as np
import pytest
import torch

from bayes_checks import ATOL, ETOL, _check, _engine_with_signatures, _pick, _result
from bayes_model import DEFAULT_LC, DeviceModel, Graph, csr_lists, params, prediction_lc_as_parsed, random_adjusted, random_graph
from decision_inputs import (CAP_INITIAL, DEPTH, K_INITIAL, boundary_graph, exact_vector, hub_graph, list_lengths, named_slots,
                             near_cancel_vector, sparse_vector, stat_vector, statistics)
from rtabmap_amd import synth

pytestmark = pytest.mark.gpu
PAD, CANARY = 64, -7.25
N_WORDS, Q = 600, 8


def _note(*a):
    print("decision-stage", *a)


@pytest.fixture(scope="module")
def plain_engine():
    import rtabmap_amd
    eng = rtabmap_amd.Engine("f32", 64)
    yield eng
    eng.close()


def _adjust_dev(eng, L, ratio):
    """lcd_adjust_likelihood_dev in place on [virtual place, slots...] between two canaries"""
    n = L.shape[0] + 1
    host = np.full(PAD + n + PAD, CANARY, np.float32)
    host[PAD] = 0.0
    host[PAD + 1:PAD + n] = L
    d = torch.from_numpy(host).cuda()
    eng.adjust_likelihood_dev(d.data_ptr() + 4 * PAD, n, ratio)
    eng.synchronize()
    got = d.cpu().numpy()
    assert (got[:PAD] == CANARY).all() and (got[PAD + n:] == CANARY).all(), "written outside the vector"
    return got[PAD:PAD + n]


def _compare_vector(got, a, ctx):
    """got against a model adjustment: decided entries within the model's tolerance, unselected ones exactly 1, slots that do not take part 0.
    Returns the virtual place's error relative to its bound."""
    err = np.abs(got.astype(np.float64) - a.vector.astype(np.float64))
    ok = a.decided
    worst = float((err[ok] - a.tol[ok]).max())
    rel0 = float(err[0] / a.tol[0]) if a.tol[0] > 0 else float(err[0] != 0)
    _note(ctx, "L[0] got %r expected %r err/bound %.3g; entries: selected %d undecided %d worst excess %.3g" %
          (float(got[0]), float(a.vector[0]), rel0, int(a.selected.sum()), int((~ok).sum()), worst))
    assert (err[ok] <= a.tol[ok]).all(), (ctx, int(np.argmax(np.where(ok, err - a.tol, -np.inf))), worst)
    exact = ok[1:] & ~a.selected
    assert np.array_equal(got[1:][exact], a.vector[1:][exact]), ctx               # 1.0, or 0.0 for a slot that does not take part
    return rel0


# ------------------------------------------------------------------------------------------------------------------ (a) plain statistics
@pytest.mark.parametrize("n_slots", [1, 255, 256, 257, 65536, 65537, 262144, 262145, 600000])
def test_plain_statistics(plain_engine, n_slots):
    """lcd_adjust_likelihood_dev over n_slots likelihood slots (a vector of n_slots + 1): the maximum at each named position, exact small
    integers (bit for bit), sparse vectors, near-cancelling values; both ratios.  The host entry at 257, 65 537 and 262 145.
    The exact vector with its top entries raised by one ulp sits (1 / (4 c + 2)) ulp from the threshold: the model's bounds leave those
    entries undecided, but its mean and the float of its variance are decided, so with sqrtf correctly rounded (HIP's default) the
    device makes the model's float32 operations and the vector is compared bit for bit."""
    eng = plain_engine
    worst = 0.0
    for name, at in named_slots(n_slots).items():
        L = stat_vector(n_slots, at)
        st = statistics(L)
        for ratio in (0.0, 0.5):
            a = st.adjust(ratio)
            assert a.decided.all()
            got = _adjust_dev(eng, L, ratio)
            worst = max(worst, _compare_vector(got, a, (n_slots, "max at " + name, ratio)))
            if name == "last" and n_slots in (257, 65537, 262145):
                np.testing.assert_array_equal(eng.adjust_likelihood(np.concatenate([[0.0], L]).astype(np.float32), ratio), got)
    L, c = exact_vector(n_slots)
    for ratio in (0.0, 0.5):
        got = _adjust_dev(eng, L, ratio)
        _note((n_slots, "exact", ratio), "L[0] = %r, entries other than 1.0: %d" % (float(got[0]), int((got[1:] != 1).sum())))
        assert (got[1:] == 1.0).all()                                           # the top values EQUAL the threshold
        assert got[0] == ((3.0 if ratio == 0 else 2.0) if c else 2.0)            # m / d + 1 = 8 / 4 + 1; d / (m + d - m) + 1
        np.testing.assert_array_equal(got, statistics(L).adjust(ratio).vector)
    R, c = exact_vector(n_slots, raised=True)
    for ratio in (0.0, 0.5):
        a = statistics(R).adjust(ratio)
        got = _adjust_dev(eng, R, ratio)
        _compare_vector(got, a, (n_slots, "exact, top raised one ulp", ratio))
        top = got[1:][R > 8]
        _note((n_slots, "raised", ratio), "the %d raised entries: device %r, the model's float32 evaluation %r" %
              (c, sorted(set(top.tolist())), sorted(set(a.vector[1:][R > 8].tolist()))))
        assert np.unique(top).shape[0] <= 1                                     # equal values, one statistic: one result
        st = statistics(R)
        assert st.mean_tol == 0 and st.var_float_decided                        # (the generator's properties)
        np.testing.assert_array_equal(got, a.vector)                            # the raised entries are selected, the rest are not: the model's values
    for kind in ("one", "two", "none", "last_partial"):
        L = sparse_vector(n_slots, kind)
        for ratio in (0.0, 0.5):
            a = statistics(L).adjust(ratio)
            assert a.decided.all()
            got = _adjust_dev(eng, L, ratio)
            _compare_vector(got, a, (n_slots, kind, ratio))
            if kind != "last_partial":                                          # nothing to round: one value, two equal ones, none
                np.testing.assert_array_equal(got, a.vector)
    L = near_cancel_vector(n_slots)
    for ratio in (0.0, 0.5):
        worst = max(worst, _compare_vector(_adjust_dev(eng, L, ratio), statistics(L).adjust(ratio), (n_slots, "near cancel", ratio)))
    _note("size %d: largest L[0] error / bound %.3g" % (n_slots, worst))


# --------------------------------------------------------------------------------- (b) slot_sig, the exclusion and the hypothesis
RETIRED_SLOTS = [255, 256, 257, 511, 512, 513, 767, 768, 1023, 1024, 1025, 4095, 4096, 8191, 8192, 12287, 12288, 16127, 16128, 16129]


def _hypothesis(d_hyp):
    from rtabmap_amd.capi import LcdHypothesis
    return LcdHypothesis.from_buffer_copy(d_hyp.cpu().numpy().tobytes())


def _check_hypothesis(h, L, considered, ratio, ctx, adj=None):
    """The hypothesis (and the adjusted vector) against the model on the likelihood the engine wrote.  Returns (model adjustment, errors
    of mean, stddev and L[0] relative to their bounds)."""
    st = statistics(L, considered)
    if np.float32(h.mean) != st.mean:                                           # the neighbouring float: the variance is taken around it
        assert abs(float(h.mean) - float(st.mean)) <= st.mean_tol, (ctx, h.mean, st.mean, st.mean_tol)
        st = statistics(L, considered, mean=h.mean)
    a = st.adjust(ratio)
    rel = (float(np.float32(h.mean) != st.own_mean), abs(float(h.stddev) - float(st.stddev)) / st.std_tol if st.std_tol else float(h.stddev != st.stddev),
           abs(float(h.virtual_place) - float(a.virtual_place)) / a.virtual_place_tol if a.virtual_place_tol else float(h.virtual_place != a.virtual_place))
    _note(ctx, "n_positive %d/%d slot %d/%d mean %r/%r stddev %r/%r (err/bound %.3g) L[0] %r/%r (err/bound %.3g) adjusted %r/%r" %
          (h.n_positive, a.n_positive, h.slot, a.slot, h.mean, float(st.own_mean), h.stddev, float(st.stddev), rel[1], h.virtual_place,
           float(a.virtual_place), rel[2], h.adjusted, float(a.adjusted)))
    assert h.n_positive == a.n_positive and h.slot == a.slot, ctx
    assert h.sig_id == (a.slot + 1 if a.slot >= 0 else 0), ctx                    # signature id s sits in slot s - 1 here
    assert np.float32(h.likelihood).tobytes() == (L[a.slot] if a.slot >= 0 else np.float32(0)).tobytes(), ctx
    assert abs(float(h.stddev) - float(st.stddev)) <= st.std_tol, ctx
    assert not a.decided[0] or abs(float(h.virtual_place) - float(a.virtual_place)) <= a.virtual_place_tol, ctx
    assert not a.adjusted_decided or abs(float(h.adjusted) - float(a.adjusted)) <= a.adjusted_tol, ctx
    if adj is not None:
        _compare_vector(adj, a, ctx)
        assert not adj[1:][~considered].any(), ctx
        assert np.float32(h.virtual_place) == adj[0] and (a.slot < 0 or np.float32(h.adjusted) == adj[1 + a.slot]), ctx
    return a, rel


@pytest.mark.parametrize("n_sig", [16385, 65537, 262145])
def test_hypothesis_and_adjusted_vector_over_slot_sig(n_sig):
    """lcd_frame_dev with d_hypothesis (decide_fold1_kernel: 1024 fold threads; at 16 385 signatures its second wave holds a partial) and with
    d_adjusted too (the fold in pass 2's prologue: 256 threads, PER = 4 from 65 537 on), twenty signatures retired across workgroup
    boundaries, the newest 0, 1 and 300 slots excluded, both ratios.  The input of the model is the likelihood the engine wrote: this tests
    the decision stage, not TF-IDF.  A frame is retired after its call, so the next call scores the same signatures with the same counts:
    the two paths then see the same likelihood (asserted) and must return the same hypothesis bit for bit.
    Ties: the frame's words are registered in six slots -- another wavefront of the same workgroup, the same wavefront, another workgroup,
    the middle of the table, among the newest 300 -- and the hypothesis is the HIGHEST considered one of them (include/lcd.h, lcd_hypothesis)."""
    import rtabmap_amd
    vocab = synth.vocab_surf(N_WORDS, seed=3)
    words = synth.zipf_words(n_sig, Q, N_WORDS, seed=4)
    src = 1000
    ties = [src - 100, src, src + 3, src + 261, n_sig // 2, n_sig - 101]        # slots 900 and 1000: two waves of one workgroup; 1000 and 1003: one wave
    words[ties] = words[src]
    eng = rtabmap_amd.Engine("f32", 64, sig_capacity=n_sig + 64)
    eng.vocab_append(vocab, np.arange(1, N_WORDS + 1, dtype=np.int32))
    eng.sig_add_bulk(np.arange(1, n_sig + 1, dtype=np.int32), np.arange(0, (n_sig + 1) * Q, Q, dtype=np.int64), words.reshape(-1))
    gone = list(RETIRED_SLOTS)
    for s in gone:
        eng.sig_remove(s + 1)
    cap = n_sig + 64
    d_desc = torch.from_numpy(synth.frame_from_signature(vocab, words[src], seed=70, resample=0.0)).cuda()
    d_words = torch.zeros(Q, dtype=torch.int32, device="cuda")
    d_like = torch.zeros(cap, dtype=torch.float32, device="cuda")
    d_adj = torch.zeros(cap + 1, dtype=torch.float32, device="cuda")
    d_hyp = torch.zeros(8, dtype=torch.int32, device="cuda")
    sid = n_sig
    worst = [0.0, 0.0, 0.0]

    def frame(exclude, ratio, with_adjusted):
        nonlocal sid
        sid += 1
        d_hyp.zero_()
        d_adj.fill_(CANARY)
        eng.frame_dev(d_desc.data_ptr(), Q, sid, float(n_sig), d_words.data_ptr(), d_like.data_ptr(), cap, d_hypothesis_ptr=d_hyp.data_ptr(),
                      d_adjusted_ptr=d_adj.data_ptr() if with_adjusted else None, exclude_recent=exclude, virtual_place_ratio=ratio)
        eng.synchronize()
        _, n_slots = eng.slots_dev()
        assert n_slots == sid
        L = d_like[:n_slots].cpu().numpy()
        considered = np.ones(n_slots, bool)
        considered[max(n_slots - exclude, 0):] = False
        considered[gone] = False
        adj = None
        if with_adjusted:
            full = d_adj.cpu().numpy()
            assert (full[n_slots + 1:] == CANARY).all()
            adj = full[: n_slots + 1]
        h = _hypothesis(d_hyp)
        a, rel = _check_hypothesis(h, L, considered, ratio, (n_sig, "exclude", exclude, "ratio", ratio, "d_adjusted", with_adjusted), adj)
        for k in range(3):
            worst[k] = max(worst[k], rel[k])
        eng.sig_remove(sid)                                                     # the next frame scores what this one scored
        gone.append(sid - 1)
        return h, L, considered

    for exclude in (0, 1, 300):
        for ratio in (0.0, 0.5):
            h1, L1, c1 = frame(exclude, ratio, False)
            h2, L2, c2 = frame(exclude + 1 if exclude else 0, ratio, True)
            if exclude:
                assert np.array_equal(np.flatnonzero(c1), np.flatnonzero(c2)) and np.array_equal(L1[c1], L2[c2])     # the same input to both folds
                assert bytes(h1) == bytes(h2), "decide_fold1_kernel and pass 2's prologue fold differ"
                top = L1[c1].max()
                tied = np.flatnonzero(c1 & (L1 == top))
                _note((n_sig, exclude), "best likelihood %r in slots %s" % (float(top), tied.tolist()))
                assert tied.shape[0] >= 2 and set(tied.tolist()) <= set(ties), "the planted tie is not the best likelihood"
                assert h1.slot == tied[-1] == [s for s in ties if c1[s]][-1]                    # of equal likelihoods the higher slot
    _note("size %d: largest error / bound of mean (1 = the neighbouring float) %.3g, stddev %.3g, L[0] %.3g" % (n_sig, *worst))
    eng.close()


# ----------------------------------------------------------------------------------------- (c) Bayes with a raw likelihood
@pytest.mark.parametrize("n_sig", [31, 32, 33, 8192, 8193, 32768, 32769])
def test_bayes_from_a_raw_likelihood(oracle, n_sig):
    """lcd_frame_dev with d_posterior / d_bayes (and d_adjusted), three frames: the second and third read the stored unnormalised posterior
    and its sum.  At 32 slots per workgroup the slot counts n_sig + 1 .. n_sig + 3 cross one workgroup (32, 33), 256 partials (8192, 8193:
    the fold's PER branch with Part1's Bayes sums) and the second grid-stride trip (32 768, 32 769: the list rows prefetched for c + stride).
    Reference: oracle.adjust_likelihood on the engine's own likelihood, then OracleBayesFilter.compute_posterior(dense=False), compared by
    bayes_checks._check.
    The reference adds the n likelihoods into a float one by one: its statistics differ from the device's by up to n * 2^-24.  Where that
    exceeds the posterior's tolerance (ETOL = 2e-5: from 336 signatures on) the oracle filter is fed the DEVICE's adjusted vector.  Measured
    with the reference's own vector: every selected entry of the posterior off by 2.6e-5 (8 192 signatures), 3.1e-5 (8 193), 6.8e-5 (32 768)
    relative, within n * 2^-24 = 4.9e-4 .. 2.0e-3 and all of it in the reference's float sums -- the device's vector equals
    tests/decision_model.py's exact-sum evaluation to the last bit there.  At EVERY size the device's adjusted vector is checked against that
    model within the model's bounds, and against oracle.adjust_likelihood within n * 2^-24 propagated by the model."""
    words = synth.zipf_words(n_sig, Q, N_WORDS, seed=4)                          # what _engine_with_signatures registers
    vocab = synth.vocab_surf(N_WORDS, seed=3)
    eng = _engine_with_signatures(n_sig)
    total = n_sig + 3
    g, info = boundary_graph(total)
    stm = 1                                          # only the frame itself is left out: the slots of the last workgroup and of the second trip take part
    eng.bayes_configure(DEFAULT_LC, 0.9)
    ob = oracle.OracleBayesFilter(DEFAULT_LC, 0.9)
    ids0 = np.arange(1, n_sig + 1, dtype=np.int32)
    off, nbr, mg = csr_lists(g, ids0, DEPTH, keep=lambda k: k <= n_sig)
    eng.bayes_set_neighbors(ids0, off, nbr, mg)
    off, nbr, mg = csr_lists(g, np.arange(1, total + 1), DEPTH)
    for i in range(total):
        ob.set_neighbors(i + 1, nbr[off[i]:off[i + 1]], mg[off[i]:off[i + 1]])
    retired = [s for s in info["retire"] if s < n_sig - stm - 40] if n_sig >= 1100 else []
    for s in retired:
        eng.sig_remove(s)
    cap = total + 8
    d_words = torch.zeros(Q, dtype=torch.int32, device="cuda")
    d_like = torch.zeros(cap, dtype=torch.float32, device="cuda")
    d_adj = torch.zeros(cap + 1, dtype=torch.float32, device="cuda")
    d_post = torch.zeros(cap + 1, dtype=torch.float32, device="cuda")
    d_res = torch.zeros(8, dtype=torch.int32, device="cuda")
    for t in range(3):
        sid = n_sig + 1 + t
        src = [n_sig // 3, n_sig - 3, n_sig // 2][t]
        d_desc = torch.from_numpy(synth.frame_from_signature(vocab, words[src - 1], seed=100 + t, resample=0.0)).cuda()
        eng.frame_dev(d_desc.data_ptr(), Q, sid, float(sid), d_words.data_ptr(), d_like.data_ptr(), cap, exclude_recent=stm,
                      d_adjusted_ptr=d_adj.data_ptr(), d_posterior_ptr=d_post.data_ptr(), d_bayes_ptr=d_res.data_ptr())
        off, nbr, mg = csr_lists(g, [sid], DEPTH, keep=lambda k: k <= sid)
        eng.bayes_set_neighbors([sid], off, nbr, mg)
        eng.synchronize()
        _, n_slots = eng.slots_dev()
        assert n_slots == sid
        L = d_like[:n_slots].cpu().numpy()
        wm = [s for s in range(1, sid - stm + 1) if s not in retired]
        ids = [-1] + wm
        considered = np.zeros(n_slots, bool)
        considered[np.asarray(wm) - 1] = True
        adj_d = d_adj[: n_slots + 1].cpu().numpy()
        st = statistics(L, considered)
        a = st.adjust(0.0)
        _compare_vector(adj_d, a, (n_sig, "frame", t, "adjusted vector"))
        vec_o = oracle.adjust_likelihood(np.concatenate([[0.0], L[considered]]).astype(np.float32), 0.0)
        vec_d = np.concatenate([[adj_d[0]], adj_d[np.asarray(wm)]])
        rel = len(ids) * 2.0 ** -24                                               # the reference's float sums
        loose = st.adjust(0.0, mean_tol=rel * float(st.mean), std_tol=(rel + 3 * 2.0 ** -24) * float(st.stddev))
        ok = np.concatenate([[loose.decided[0]], loose.decided[1:][considered]])
        err = np.abs(vec_o.astype(np.float64) - vec_d.astype(np.float64))
        tol = np.concatenate([[loose.tol[0]], loose.tol[1:][considered]])
        _note((n_sig, "frame", t), "oracle.adjust_likelihood against the device: largest relative difference %.3g, n * 2^-24 = %.3g, undecided %d" %
              (float((err / np.abs(vec_d)).max()), rel, int((~ok).sum())))
        assert (err[ok] <= tol[ok]).all(), (n_sig, t)
        vec = vec_d if rel > ETOL else vec_o
        ob.set_stm(list(range(sid - stm + 1, sid + 1)))
        post_o = ob.compute_posterior(ids, vec, dense=False)
        res = _result(d_res)
        _note((n_sig, "frame", t), "slots %d considered %d selected %d; hypothesis %d value %r" % (n_slots, len(wm), int(a.selected.sum()), res.sig_id, res.value))
        assert a.selected.sum() >= 1                                             # the likelihood is not flat
        _check(ids, post_o, _pick(d_post, ids), res, (n_sig, "frame", t))
        got = d_post[: n_slots + 1].cpu().numpy()
        assert not got[1:][~considered].any(), "a signature outside the likelihood has a posterior"
    eng.close()


# ------------------------------------------------------------------------------------------------------------------------ (d) lists
def _adjusted_for(n_sig, considered, rng):
    ids = [-1] + considered
    like = random_adjusted(len(ids), rng)
    adj = np.zeros(n_sig + 1, np.float32)
    adj[0] = like[0]
    adj[np.asarray(considered)] = like[1:]
    return ids, like, adj


class _Filter:
    """An engine and the oracle's filter side by side: the same lists, the same updates"""

    def __init__(self, oracle, n_sig, lc=DEFAULT_LC, vp=0.9, eng=None):
        self.n = n_sig
        self.eng = eng if eng is not None else _engine_with_signatures(n_sig)
        self.eng.bayes_configure(lc, vp)
        self.ob = oracle.OracleBayesFilter(lc, vp)
        self.d_adj = torch.zeros(n_sig + 1, dtype=torch.float32, device="cuda")
        self.d_post = torch.zeros(n_sig + 1, dtype=torch.float32, device="cuda")
        self.d_res = torch.zeros(8, dtype=torch.int32, device="cuda")
        self.retired = set()

    def oracle_lists(self, g, depth, n=None):
        n = self.n if n is None else n
        off, nbr, mg = csr_lists(g, np.arange(1, n + 1), depth)
        for i in range(n):
            self.ob.set_neighbors(i + 1, nbr[off[i]:off[i + 1]], mg[off[i]:off[i + 1]])
        return off, nbr, mg

    def retire(self, ids):
        for s in ids:
            if s not in self.retired:
                self.eng.sig_remove(int(s))
                self.retired.add(int(s))

    def update(self, upto, stm, rng, ctx, dense=False, model=None):
        """one update over the signatures 1 .. upto - stm that are not retired (the engine holds `upto` signatures).  model: a
        bayes_model.DeviceModel that takes the oracle's place in _check; the oracle is then compared within ETOL + m * 2^-24"""
        considered = [s for s in range(1, upto - stm + 1) if s not in self.retired]
        ids, like, adj = _adjusted_for(self.n, considered, rng)
        self.d_adj.copy_(torch.from_numpy(adj))
        self.eng.bayes_update_dev(self.d_adj.data_ptr(), stm, self.d_post.data_ptr(), self.d_res.data_ptr())
        self.eng.synchronize()
        self.ob.set_stm(list(range(upto - stm + 1, upto + 1)))
        t0 = time.perf_counter()
        post_o = self.ob.compute_posterior(ids, like, dense=dense)
        t_oracle = time.perf_counter() - t0
        res = _result(self.d_res)
        post_d = _pick(self.d_post, ids)
        _note(ctx, "considered %d hypothesis %d value %r; the %s oracle took %.3f s" % (len(considered), res.sig_id, res.value, "dense" if dense else "sparse", t_oracle))
        if model is None:
            _check(ids, post_o, post_d, res, ctx)
        else:
            inset = np.zeros(self.n, bool)
            inset[np.asarray(considered) - 1] = True
            pm = model.update(adj, inset)
            _check(ids, np.concatenate([[pm[0]], pm[np.asarray(considered)]]), post_d, res, ctx)
            r = float(np.median(post_d.astype(np.float64) / post_o.astype(np.float64)))
            worst = float(np.max(np.abs(post_d - post_o.astype(np.float64) * r) / (post_o.astype(np.float64) * r)))
            _note(ctx, "dense oracle: largest relative difference %.3g, m * 2^-24 = %.3g" % (worst, len(ids) * 2.0 ** -24))
            np.testing.assert_allclose(post_d, post_o.astype(np.float64) * r, rtol=ETOL + len(ids) * 2.0 ** -24, atol=ATOL, err_msg=str(ctx))
        got = self.d_post.cpu().numpy()
        mask = np.ones(self.n + 1, bool)
        mask[0] = False
        mask[np.asarray(considered)] = False
        assert not got[mask].any(), "a signature outside the likelihood has a posterior"
        return considered, got


def test_lists_at_the_round_trip_boundaries(oracle):
    """boundary_graph, 2 100 signatures: lists of 47, 48, 49 (one round trip of 48 entries, and one entry into the second), 64, 65 (the
    table's first width), 96, 97 entries; a wavefront tile with lists on both sides of 48; a long list reaching into the short-term memory
    and over retired signatures.  Five updates, the short-term memory sliding, retirements in between, against the sparse oracle."""
    n_sig = 2100
    g, info = boundary_graph(n_sig)
    f = _Filter(oracle, n_sig)
    off, nbr, mg = f.oracle_lists(g, DEPTH)
    assert {47, 48, 49, 64, 65, 96, 97} <= set(list_lengths(off).tolist())
    f.eng.bayes_set_neighbors(np.arange(1, n_sig + 1, dtype=np.int32), off, nbr, mg)
    rng = np.random.default_rng(5)
    for t, stm in enumerate([900, info["stm"], info["stm"], 12, 0]):
        if t == 2:
            f.retire(info["retire"])
        if t == 3:
            f.retire(rng.choice(np.arange(1, n_sig - 100), size=50, replace=False).tolist())
        f.update(n_sig, stm, rng, ("boundary graph, update", t))
    f.eng.close()


def test_lists_past_128_entries_entered_one_signature_at_a_time(oracle):
    """hub_graph, 700 signatures: five lists of 165 entries.  A list arrives when its signature enters and names the signatures that exist
    by then; the engine appends it to the older signatures' lists -- at positions past 64 and past 128 -- and widens the table twice (K 64
    -> 128 -> 256, a pitched copy of every tile).  The device memory in use grows at exactly those two calls, by the table's size; the
    posterior equals the oracle's before and after each.  Then a signature beside the hub is listed again: its entry in every neighbour's
    list is REPLACED, found by a search that runs past lane 63."""
    n_sig = 700
    g, hub, places = hub_graph(n_sig)
    f = _Filter(oracle, n_sig)
    off, nbr, mg = f.oracle_lists(g, DEPTH)
    length = np.zeros(n_sig + 1, np.int64)
    widen = {}
    for s in range(1, n_sig + 1):
        mine = nbr[off[s - 1]:off[s]]
        mine = mine[mine <= s]
        before = length.max()
        length[mine] += 1
        length[s] = mine.shape[0]
        for k in (K_INITIAL, 2 * K_INITIAL):
            if before <= k < length.max():
                widen[s] = k
    assert sorted(widen.values()) == [K_INITIAL, 2 * K_INITIAL]
    stops = sorted(set([1, 40] + [s + d for s in widen for d in (-1, 0)] + [n_sig]))
    rng = np.random.default_rng(6)
    grew = {}
    for s in range(1, n_sig + 1):
        o1, n1, m1 = csr_lists(g, [s], DEPTH, keep=lambda k: k <= s)
        before = f.eng.stats()["bytes_device"]
        f.eng.bayes_set_neighbors([s], o1, n1, m1)
        after = f.eng.stats()["bytes_device"]
        if s > 1 and after != before:
            grew[s] = after - before
        if s in stops:
            f.update(n_sig, n_sig - s, rng, ("hub graph, entered", s, "widened" if s in widen else ""))
    _note("hub graph: device memory grew at", grew, "expected at", widen)
    assert grew == {s: k * CAP_INITIAL * 4 for s, k in widen.items()}             # the new table less the old one: K * cap * 4 bytes more
    beside = hub - 1
    o1, n1, m1 = csr_lists(g, [beside], DEPTH)
    before = f.eng.stats()["bytes_device"]
    f.eng.bayes_set_neighbors([beside], o1, n1, m1)
    assert f.eng.stats()["bytes_device"] == before and list_lengths(o1)[0] > 2 * K_INITIAL
    f.update(n_sig, 0, rng, ("hub graph, signature %d listed again" % beside, "hub's list has %d entries" % length[hub]))
    f.eng.close()


def test_table_widens_while_its_last_tile_is_in_use(oracle):
    """4 096 signatures fill the table's first capacity to its last tile (slots 4 088 .. 4 095).  Chain lists first (K = 64) and an update,
    then the hub's loop links: the signatures around the five places are listed again with up to 165 entries, the table is widened with every
    tile in use -- the pitched copy must carry the last one too -- and the posterior still equals the oracle's."""
    n_sig = CAP_INITIAL
    g, hub, places = hub_graph(n_sig)
    chain = Graph(n_sig)
    f = _Filter(oracle, n_sig)
    off, nbr, mg = f.oracle_lists(chain, DEPTH)
    assert list_lengths(off).max() <= K_INITIAL
    ids = np.arange(1, n_sig + 1, dtype=np.int32)
    f.eng.bayes_set_neighbors(ids, off, nbr, mg)
    rng = np.random.default_rng(9)
    f.update(n_sig, 0, rng, ("last tile, chain lists",))
    before = f.eng.stats()["bytes_device"]
    off2, nbr2, mg2 = f.oracle_lists(g, DEPTH)
    changed = ids[list_lengths(off2) != list_lengths(off)]
    assert 0 < changed.shape[0] < 400 and list_lengths(off2).max() > 2 * K_INITIAL
    f.eng.bayes_set_neighbors(changed, *csr_lists(g, changed, DEPTH))
    assert f.eng.stats()["bytes_device"] == before + 3 * K_INITIAL * CAP_INITIAL * 4      # K 64 -> 256 in one step
    considered, got = f.update(n_sig, 0, rng, ("last tile, after the table widened",))
    assert (got[n_sig - 7:] > 0).all()
    f.update(n_sig, 0, rng, ("last tile, second update",))
    f.eng.close()


# ------------------------------------------------------------------------------------------------------- (e) growth under a live filter
def test_tables_grow_under_a_live_filter(oracle):
    """4 000 signatures and two updates (cnt, post, was_in and the neighbour table hold 4 096 slots), then 200 more signatures with their
    lists -- links across slot 4 096 among them -- which grows every table to 8 192 slots while a posterior is alive, two more updates, and
    lcd_bayes_posterior over ids on both sides of 4 096.  The oracle never noticed the growth."""
    import rtabmap_amd
    n0, n1 = 4000, 4200
    assert n0 < CAP_INITIAL < n1
    words = synth.zipf_words(n1, Q, N_WORDS, seed=4)
    eng = rtabmap_amd.Engine("f32", 64, sig_capacity=n1 + 64)
    eng.vocab_append(synth.vocab_surf(N_WORDS, seed=3), np.arange(1, N_WORDS + 1, dtype=np.int32))
    eng.sig_add_bulk(np.arange(1, n0 + 1, dtype=np.int32), np.arange(0, (n0 + 1) * Q, Q, dtype=np.int64), words[:n0].reshape(-1))
    g, info = boundary_graph(n1, extra_loops=[(4120, 4080), (4150, 3000), (4097, 500)])
    f = _Filter(oracle, n1, eng=eng)
    f.oracle_lists(g, DEPTH)
    ids0 = np.arange(1, n0 + 1, dtype=np.int32)
    eng.bayes_set_neighbors(ids0, *csr_lists(g, ids0, DEPTH, keep=lambda k: k <= n0))
    rng = np.random.default_rng(8)
    f.update(n0, 30, rng, ("growth, update", 0))
    f.retire([s for s in info["retire"] if s < n0 - 100])
    f.update(n0, 10, rng, ("growth, update", 1))
    ids1 = np.arange(n0 + 1, n1 + 1, dtype=np.int32)
    eng.sig_add_bulk(ids1, np.arange(0, (n1 - n0 + 1) * Q, Q, dtype=np.int64), words[n0:].reshape(-1))
    eng.bayes_set_neighbors(ids1, *csr_lists(g, ids1, DEPTH, keep=lambda k: k <= n1))
    f.update(n1, 30, rng, ("growth, update", 2))
    considered, got = f.update(n1, 0, rng, ("growth, update", 3))
    some = [-1, 1, 500, 3000, 4080, 4095, 4096, 4097, 4098, 4120, 4150, n1, info["retire"][0]]
    np.testing.assert_array_equal(eng.bayes_posterior(some), [got[0]] + [got[s] for s in some[1:-1]] + [0.0])
    assert got[4096] > 0 and got[4097] > 0
    eng.close()


# -------------------------------------------------------------------------------------- (f) the fill past one wave of workgroups
@pytest.mark.parametrize("lc,vp", [([0.1, 0.3, 0.2, 0.1], 0.9), ([0.2, 0.5, 0.2, 0.05, 0.05], 0.0)])
def test_fill_of_all_other_places_past_one_wave_of_workgroups(oracle, lc, vp):
    """A pattern that sums to less than 1 (every other place gets a share: decide_count_kernel ahead of pass 1, `cols < 0`) and the
    prior-0 pattern of test_other_prediction_patterns, at 2 100 signatures: 66 workgroups of 32 slots, 9 blocks of 256 for the count.
    Three updates against the DENSE oracle (2 101^2 floats, 18 MB; about 0.1 s per update on the host).
    Where a column is filled, the reference adds the fill value into the column's float sum once per empty element (normalize :455-465), m
    additions; the device adds one rounded product (bayes.hip, decide_pass1_kernel).  Measured at m = 1 401 with the first pattern: the
    virtual place and four places beside the ends of the chain differ from the dense oracle by 3.9e-5 relative once the constants are
    divided out, above ETOL = 2e-5 and inside m * 2^-24 = 8.4e-5; bayes_model.DeviceModel, the device's algorithm in NumPy, differs from the
    oracle by the same 3.92888533e-05 in the same five entries.  So the kernel is held to that model under the project's tolerances
    (bayes_checks._check; the model itself is held to the oracle in tests/test_oracle_bayes.py), and to the dense oracle within
    ETOL + m * 2^-24, the reference's own accumulation."""
    n_sig = 2100
    lcp = prediction_lc_as_parsed(lc)
    depth = min(lcp.shape[0] - 1, 5)
    rng = np.random.default_rng(11)
    g = random_graph(n_sig, 30, rng)
    f = _Filter(oracle, n_sig, lcp, vp)
    off, nbr, mg = f.oracle_lists(g, depth)
    f.eng.bayes_set_neighbors(np.arange(1, n_sig + 1, dtype=np.int32), off, nbr, mg)
    model = DeviceModel(n_sig, lcp, vp) if params(lcp, vp)["all_other"] > 0 else None      # without a fill the oracle stays the only reference
    for i in range(n_sig if model else 0):
        for k, m in zip(nbr[off[i]:off[i + 1]].tolist(), mg[off[i]:off[i + 1]].tolist()):
            model.link(i, k - 1, m)
    for t, stm in enumerate([700, 30, 0]):
        if t == 2:
            f.retire([31, 32, 33, 255, 256, 257, 1056, 1057, 2047, 2048])
        f.update(n_sig, stm, rng, (lc, "update", t), dense=True, model=model)
    f.eng.close()
