"""CPU proofs about the designed frames of tests/resolve_inputs.py: the integer bounds that make every distance the same bits on every path,
the filter certificate of every descriptor that is meant to be certified (so the exact redo stays inside its cap for the inputs alone), the
named property of each generator -- shown with tests/resolve_model.py -- and the census of routes per producer.  No GPU."""
import collections

import numpy as np
import pytest

import resolve_inputs as I
import resolve_model as M
from test_bf16_split_bound import bf16_rne
from test_certificate_model import filter_and_rerank
from test_resolve_model import INPUTS, evaluated

U, U16 = 2.0 ** -24, 2.0 ** -11
LIST_ROUTES = M.ROUTES
BITROW_ROUTES = M.ROUTES[5:]


def lists_exist(name):
    """the matrix-core filter's re-rank is the producer from 256 vocabulary rows on"""
    return evaluated(name)[0][0].shape[0] >= 256


# ---- eps of the three filters as rerank_body.cuh charges them (the terms are the ones test_bf16_split_bound.py, test_fp16_split_bound.py and
# ---- test_f32_filter_eps_bound.py check)
def eps_bf16(dim, qn, vn):
    return (3.1 * 2.0 ** -16 + ((3.0 * dim + 4.0) * 8.0 + 1.5 * dim + 12.0) * U) * 1.25 * (qn + vn)


def eps_f16(dim, qn, vn):
    return ((2 * U16 + U16 * U16) + ((dim + 4.0) * 8.0 + 1.5 * dim + 12.0) * U) * 1.25 * (qn + vn) + 2.0 * dim * 2.0 ** -25 * (2.0 + qn + vn)


def eps_f32(dim, qn, vn):
    return (3.5 * dim + 16.0) * U * 1.25 * (qn + vn)


def eps_worst(qn, vn):
    return max(f(dim, qn, vn) for f in (eps_bf16, eps_f16, eps_f32) for dim in (64, 128))


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_coordinates_are_small_integers_and_distances_exact(name):
    (vocab, ids, frame, _), (idx_id, idx_d, sd), _, _, _ = evaluated(name)
    for a in (vocab, frame):
        assert a.dtype == np.float32 and (a == np.rint(a)).all() and np.abs(a).max(initial=0) <= I.MAX_ABS
        assert (bf16_rne(a) == a).all() and (a.astype(np.float16).astype(np.float32) == a).all(), "exact as bf16 and as fp16 operands"
    # a partial sum of a squared distance, of a norm or of a product sum is an integer of at most 128 * (2 * MAX_ABS)^2
    assert 128 * (2 * I.MAX_ABS) ** 2 < 2 ** 24
    assert (sd == np.rint(sd)).all() and sd.max(initial=0) < 2 ** 24 and (idx_d == np.rint(idx_d)).all()
    # ... so float32 arithmetic in another order gives the same bits
    if vocab.shape[0]:
        d32 = ((frame[:, None, :] - vocab[None, :8, :]) ** 2).sum(axis=2, dtype=np.float32)
        assert (d32 == M.distances(frame, vocab[:8])).all()


_CERT = {}


def certified(vocab_key, vocab, row):
    """the certificate model of test_certificate_model.py on one descriptor, the filter's errors chosen against it: +eps on the two true neighbours,
    -eps on every other row; for two row-block sizes"""
    key = (vocab_key, row.tobytes())
    if key not in _CERT:
        d = M.distances(row[None, :], vocab)[0].astype(np.float64)
        eps = eps_worst(float((row.astype(np.float64) ** 2).sum()), float((vocab.astype(np.float64) ** 2).sum(axis=1).max()))
        order = np.lexsort((np.arange(len(d)), d))
        noise = np.full(len(d), -eps)
        noise[order[:2]] = eps
        ok = True
        for rpb in (32, 192):
            good, b, s = filter_and_rerank(d, d + noise, eps, rpb)
            ok = ok and good and b == order[0] and s == order[1]
        few = int((d <= d[order[1]] * (1 + 2.0 ** -15) + 4 * eps).sum()) <= 128            # RR_MAX_CAND
        _CERT[key] = ok and few
    return _CERT[key]


@pytest.mark.parametrize("name", sorted(n for n in INPUTS if lists_exist(n)))
def test_every_descriptor_is_certified_except_the_cluster_on_identical_rows(name):
    vocab, _, frame, _ = evaluated(name)[0]
    got = np.array([certified(name == "redo", vocab, r) for r in frame])
    if name == "redo":
        assert (~got).sum() == 7 and not got[4:11].any(), "the seven on the identical rows, and only they, go to the exact redo"
        assert (~got).sum() > frame.shape[0] // 4, "this input leaves the cap on purpose"
    else:
        assert got.all(), "rejected by the certificate: %r" % (np.flatnonzero(~got).tolist(),)


def _ids(name):
    return evaluated(name)[2][0]


def _census(name):
    return evaluated(name)[3][2] if lists_exist(name) else evaluated(name)[4][2]


def test_filler_descriptors_have_no_candidates_and_alternate():
    v, ids = I.vocabulary()
    frame = I._f32(I.fill(1040))
    a = M.model_inputs(v, ids, frame)
    got, n_new, c = M.jacobi(*a, 0.8)
    assert (c["cn"] == 0).all() and c["sweeps"] == 1
    assert all((w < 0) == (i % 2 == 1) for i, w in enumerate(got)), "matched, new, matched, new, ..."
    assert n_new == 520


@pytest.mark.parametrize("name,k,first", [("chain40", 40, 0), ("chain20_in_513", 20, 493), ("chain20_in_1025", 20, 1005)])
def test_chain_alternates_and_needs_a_sweep_per_descriptor(name, k, first):
    got, c = _ids(name), _census(name)
    new = [w < 0 and (i == 0 or w != got[first + i - 1]) for i, w in enumerate(got[first:first + k])]
    assert new == [i % 2 == 0 for i in range(k)], "new, matched, new, matched, ..."
    assert all(got[first + i] == got[first + i - 1] for i in range(1, k, 2)), "each matched one takes the word in front of it"
    assert c["sweeps"] >= k // 2 and c["last_change"][first:first + k].max() >= 3
    print(name, "sweeps", c["sweeps"], "last change", c["last_change"][first:first + k].tolist())


@pytest.mark.parametrize("m", range(2, 8))
def test_cluster_reaches_every_list_length_and_the_first_bit_row(m):
    got, c = _ids("cluster%d" % m), _census("cluster%d" % m)
    assert got == [-1] * m
    assert c["cn"].tolist() == list(range(m))
    assert c["route"] == (["none", "list_1", "list_2", "list_3", "list_4", "bitrow_reg_hit", "bitrow_reg_hit"])[:m]


def test_popular_copies_are_each_others_candidates_and_none_is_new():
    for name, first, route in (("popular40", 0, "bitrow_reg_skip"), ("popular40_in_600", 560, "bitrow_mem_skip")):
        got, c = _ids(name), _census(name)
        assert got[first:first + 40] == [12 + 3 * 1 + 1] * 40, "all forty are their word"
        assert c["cn"][first:first + 40].tolist() == list(range(40))
        assert c["route"][first + 5:first + 40] == [route] * 35
        assert c["sweeps"] == 1


def test_later_only_descriptor_comes_out_as_it_does_alone():
    (vocab, ids, frame, nndr), (idx_id, idx_d, sd), seq, _, _ = evaluated("later_only")
    thr = M.thresholds(idx_id, idx_d)
    assert (sd[1:, 0] < thr[0]).all() and _census("later_only")["cn"][0] == 0, "bits only above the descriptor"
    alone = M.sequential(*M.model_inputs(vocab, ids, frame[:1]), nndr)
    assert seq[0][0] == alone[0][0] > 0 and seq[0][1:] == [-1, -1]


def test_ties():
    (_, _, _, nndr), (_, _, sd), seq, _, _ = evaluated("ties_lower_j")
    assert nndr == 1.0 and sd[0, 2] == sd[1, 2] == sd[0, 3] == sd[1, 3] == 8
    assert seq[0] == [-1, -2, -1, -1, -1], "the lower j wins"
    (vocab, ids, frame, nndr), (idx_id, idx_d, sd), seq, jac, _ = evaluated("ties_indexed_first")
    assert idx_d[1].tolist() == [49.0, 65.0] and sd[0, 1] == 49 and jac[2]["win"][1] == idx_id[1, 0] > 0, "the indexed word stays c0"
    assert seq[0] == [-1, -2] and M.sequential(*M.model_inputs(vocab, ids, frame[1:]), nndr)[0][0] == idx_id[1, 0], "rejected by the equal pair; matched when alone"
    (vocab, ids, frame, nndr), (idx_id, idx_d, sd), seq, jac, _ = evaluated("ties_second_excluded")
    assert idx_d[1, 1] == sd[0, 1] == 65 and jac[2]["cn"][1] == 0, "no bit at the second indexed distance"
    assert seq[0] == [-1, idx_id[1, 0]] and M.sequential(*M.model_inputs(vocab, ids, frame[1:]), nndr)[0][0] == idx_id[1, 0]


def test_nndr_edge():
    _, (idx_id, idx_d, sd), seq, jac, _ = evaluated("nndr_half")
    assert idx_d[0].tolist() == [2.0, 4.0] and idx_d[1].tolist() == [3.0, 4.0]
    assert idx_d[3].tolist() == [2.0, 13.0] and sd[2, 3] == 4 and idx_d[5].tolist() == [3.0, 13.0] and sd[4, 5] == 4
    assert seq[0] == [1, -1, -2, 5, -3, -4], "2 : 4 accepted at equality, 3 : 4 rejected, with c1 indexed and with c1 a new word of the frame"
    assert jac[2]["cn"].tolist() == [0, 0, 0, 1, 0, 1]


@pytest.mark.parametrize("frame", sorted(I.EMPTY_FRAMES))
def test_empty_dictionary_sets_every_bit(frame):
    for n in (0, 1):
        _, (idx_id, idx_d, _), seq, _, jac = evaluated("empty%d_%s" % (n, frame))
        assert (idx_id == 0).all() and (idx_d < 0).all()
        assert jac[2]["cn"].tolist() == list(range(len(seq[0]))), "cn = i"
        assert seq[0][:2] == [-1, -2], "fewer than two candidates"
    assert evaluated("empty0_" + frame)[2] == evaluated("empty1_" + frame)[2]


@pytest.mark.parametrize("b", I.SEAMS)
def test_seams_have_the_dependency_on_either_side(b):
    got, c = _ids("seam%d_cluster" % b), _census("seam%d_cluster" % b)
    members = [b - 1, b, b + 1] + list(range(b + 8, b + 11))
    assert got[b - 1] < 0 and all(got[i] == got[b - 1] for i in members), "the word created below the seam is matched above it"
    assert c["cn"][members].tolist() == list(range(6))
    got, c = _ids("seam%d_chain" % b), _census("seam%d_chain" % b)
    assert [got[i] for i in range(b - 3, b + 3)] == [got[b - 3], got[b - 3], got[b - 1], got[b - 1], got[b + 1], got[b + 1]]
    assert len({got[b - 3], got[b - 1], got[b + 1]}) == 3 and got[b - 1] < 0 and c["last_change"][b + 2] == 5
    got, c = _ids("seam%d_ties" % b), _census("seam%d_ties" % b)
    assert got[b - 1] < 0 and got[b] < 0 and got[b] != got[b - 1] and c["cn"][b] == 1
    for p in ("cluster", "chain", "ties"):
        assert (np.delete(_census("seam%d_%s" % (b, p))["cn"], range(b - 3, b + 11)) == 0).all()


@pytest.mark.parametrize("q", I.SIZES)
def test_sizes_cover_straight_bit_row_width_and_body(q):
    got, c = _ids("size%d" % q), _census("size%d" % q)
    assert len(got) == q
    assert c["straight"] == (8 <= q <= 512) and c["bw"] == (q + 63) // 64 * 2 and c["body"] == ("fast" if q <= 1024 else "plain")
    if q >= 64:
        assert got[3:13] == [got[3]] * 10 and got[3] < 0 and c["cn"][3:13].tolist() == list(range(10))
        assert c["last_change"][q - 1] == 7 and c["sweeps"] == 8
        rest = np.r_[0:3, 13:q - 8]
        assert (c["cn"][rest] == 0).all()
        new = np.array(got)[rest] < 0
        assert abs(int(new.sum()) - int((~new).sum())) <= 1, "half of the filler matches, half is new"
        ranks = sorted(-w - 1 for w in got if w < 0)
        assert q < 512 or ranks[-1] >= 64, "new-word ranks cross mask words"


def test_census_of_routes_per_producer():
    with_lists, without = collections.Counter(), collections.Counter()
    straight, body = collections.Counter(), collections.Counter()
    for name in sorted(INPUTS):
        _, _, _, jl, jn = evaluated(name)
        if lists_exist(name):
            with_lists.update(jl[2]["route"])
            straight[jl[2]["straight"]] += 1
            body[jl[2]["body"]] += 1
        without.update(jn[2]["route"])                                # (the same frames against the vocabulary cut below 256 rows take these routes too)
        body[jn[2]["body"]] += 0
    print("descriptors per route, list producer:", dict(with_lists))
    print("descriptors per route, list-less producers:", dict(without))
    print("frames straight / not:", straight[True], straight[False], " fast / plain body:", body["fast"], body["plain"])
    for r in LIST_ROUTES:
        assert with_lists[r] >= 5, r
    for r in BITROW_ROUTES:
        assert without[r] >= 20, r
    assert straight[True] > 0 and straight[False] > 0 and body["fast"] > 0 and body["plain"] > 0
