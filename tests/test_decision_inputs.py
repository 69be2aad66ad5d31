"""The properties tests/decision_inputs.py promises, proved without a GPU, and every new graph through the device algorithm's model
(bayes_model.DeviceModel) against the oracle's filter."""
import numpy as np
import pytest

import oracle as O
from bayes_model import DEFAULT_LC, DeviceModel, csr_lists, random_adjusted
from decision_inputs import (BOUNDARY_LENGTHS, CHAIN_LIST, DC_MAX_GRID, DEPTH, FOLD_PROLOGUE, K_INITIAL, MAX_SEEDS, ROUND_TRIP, SLOTS_BAYES, SLOTS_PLAIN,
                             boundary_graph, exact_vector, hub_graph, launch_plan, list_lengths, named_slots, near_cancel_vector, sparse_vector, stat_vector,
                             statistics)
from decision_model import f32

SIZES = [1, 255, 256, 257, 65536, 65537, 262144, 262145, 600000]


def test_the_sizes_cross_every_boundary_of_the_launch_plan():
    p = {n: launch_plan(n) for n in SIZES}
    assert [p[n]["grid"] for n in (1, 255, 256, 257)] == [1, 1, 1, 2]
    assert p[65536]["grid"] == FOLD_PROLOGUE and p[65536]["per"] == 0 and p[65537]["grid"] == FOLD_PROLOGUE + 1 and p[65537]["per"] == 4
    assert p[262144]["grid"] == DC_MAX_GRID and p[262144]["trips"] == 1 and p[262145]["trips"] == 2 and p[600000]["trips"] == 3
    assert 600000 % p[600000]["stride"] != 0                                # uneven trips
    b = {n: launch_plan(n, bayes=True) for n in (31, 32, 33, 8192, 8193, 32768, 32769)}
    assert [b[n]["grid"] for n in (32, 33, 8192, 8193, 32768, 32769)] == [1, 2, 256, 257, 1024, 1024]
    assert b[8193]["per"] == 4 and b[32768]["trips"] == 1 and b[32769]["trips"] == 2
    assert MAX_SEEDS == 8 and ROUND_TRIP == 48 and SLOTS_BAYES == 32 and SLOTS_PLAIN == 256 and K_INITIAL == 64
    assert named_slots(600000) == {"first": 0, "last": 599999, "last_workgroup": 599808, "second_trip": 524287}


@pytest.mark.parametrize("n", SIZES)
def test_stat_vector(n):
    for name, at in named_slots(n).items():
        L, k = stat_vector(n, at, with_seed=True)
        assert k < MAX_SEEDS
        st = statistics(L)
        assert int(np.argmax(L)) == at and st.best_slot == at and (L == L[at]).sum() == 1
        for ratio in (0.0, 0.5):
            assert st.adjust(ratio).decided.all()                              # the property: no entry undecided
        if n >= 255:
            assert 0.6 < (L > 0).mean() < 0.8 and 0.3 < float(st.stddev) / float(st.mean) < 3


@pytest.mark.parametrize("n", SIZES)
def test_exact_vector(n):
    L, c = exact_vector(n)
    assert ((L == 4).sum(), (L == 12).sum(), (L == 8).sum(), (L > 0).sum()) == (c, c, 1, 2 * c + 1)
    if n >= 3:
        assert c >= 1
        steps = np.unique(np.flatnonzero(L) // SLOTS_PLAIN)
        assert steps.shape[0] == -(-n // SLOTS_PLAIN)                          # a positive entry in every workgroup step
        st = statistics(L)
        assert st.exact_sums and st.var == 16.0 and st.mean == 8 and st.stddev == 4 and st.mean_tol == st.var_tol == st.std_tol == 0
        for ratio, vp in ((0.0, 3.0), (0.5, 2.0)):
            a = st.adjust(ratio)
            assert a.decided.all() and a.vector[0] == vp and (a.vector[1:] == 1).all()
    R, c2 = exact_vector(n, raised=True)
    assert c2 == c and (R != L).sum() == c and (R[R != L] == np.nextafter(f32(12), f32(13))).all()
    if n >= 3:
        st = statistics(R)
        assert st.mean == 8 and st.mean_tol == 0                               # c / (2 c + 1) of an ulp: rounds back to m, whatever the sum's error
        a = st.adjust(0.0)
        assert a.decided[1:][R <= 8].all() and not a.selected[R <= 8].any()    # only the raised entries are open
        assert st.var_float_decided and st.stddev == np.nextafter(f32(4), f32(5)) and a.selected[R > 8].all()      # the model's float32 evaluation selects them


@pytest.mark.parametrize("n", SIZES)
def test_sparse_and_near_cancel_vectors(n):
    assert (sparse_vector(n, "one") > 0).sum() == 1 and (sparse_vector(n, "none") > 0).sum() == 0
    two = sparse_vector(n, "two")
    assert (two > 0).sum() == min(2, n) and np.unique(two[two > 0]).shape[0] == 1
    assert statistics(two).stddev == 0
    last = sparse_vector(n, "last_partial")
    p = launch_plan(n)
    at = np.flatnonzero(last)
    assert at.shape[0] >= 1 and ((at // p["spb"]) % p["grid"] == p["grid"] - 1).all()
    for kind in ("one", "two", "none", "last_partial"):
        st = statistics(sparse_vector(n, kind))
        assert all(st.adjust(r).decided.all() for r in (0.0, 0.5)), kind
    nc = near_cancel_vector(n)
    st = statistics(nc)
    if st.n_positive >= 2:
        assert 0 < st.std_tol < 1e-3 * float(st.stddev) and abs(float(st.stddev) - 1e-4) < 2e-6


def test_boundary_graph_lists():
    n = 2100
    g, info = boundary_graph(n)
    ids = np.arange(1, n + 1)
    off, nbr, mg = csr_lists(g, ids, DEPTH)
    ln = list_lengths(off)
    considered = np.ones(n, bool)
    considered[n - info["stm"]:] = False
    considered[np.asarray(info["retire"]) - 1] = False
    for length in BOUNDARY_LENGTHS:
        a = info["anchors"][length]
        assert ln[a - 1] == length and considered[a - 1], length
    assert set(BOUNDARY_LENGTHS) <= set(ln[considered].tolist())
    assert ROUND_TRIP - 1 in BOUNDARY_LENGTHS and ROUND_TRIP in BOUNDARY_LENGTHS and ROUND_TRIP + 1 in BOUNDARY_LENGTHS
    assert K_INITIAL in BOUNDARY_LENGTHS and K_INITIAL + 1 in BOUNDARY_LENGTHS and 2 * ROUND_TRIP in BOUNDARY_LENGTHS and 2 * ROUND_TRIP + 1 in BOUNDARY_LENGTHS
    assert ln.max() < 2 * K_INITIAL                                           # K grows once here; hub_graph is the one that passes 128
    tiles = ln[: (n // 8) * 8].reshape(-1, 8)
    assert ((tiles.max(axis=1) > ROUND_TRIP) & (tiles.min(axis=1) < ROUND_TRIP)).any()      # one wavefront tile, both kinds of list
    a = info["anchors"]["stm"]
    mine = nbr[off[a - 1]:off[a]]
    assert ln[a - 1] > ROUND_TRIP and considered[a - 1] and (mine > n - info["stm"]).any() and np.isin(mine, info["retire"]).any()
    assert all(np.isin(nbr[off[x - 1]:off[x]], info["retire"]).any() for x in (info["anchors"][96], info["anchors"][97]))
    # the small sizes of the Bayes cases still give a graph
    for small in (31, 32, 33, 300):
        gs, _ = boundary_graph(small)
        assert gs.n == small


def test_hub_graph_lists():
    n = 700
    g, hub, places = hub_graph(n)
    off, nbr, mg = csr_lists(g, np.arange(1, n + 1), DEPTH)
    ln = list_lengths(off)
    assert min(abs(a - b) for a in places + [hub] for b in places + [hub] if a != b) > 40
    assert [ln[s - 1] for s in [hub] + places] == [5 * CHAIN_LIST] * 5 and 5 * CHAIN_LIST > 2 * K_INITIAL
    # entered one signature at a time, a list names the signatures that exist by then: the lengths pass 64 and 128 at known steps, and
    # entries are appended at positions >= 64 of the older lists
    length = np.zeros(n + 1, np.int64)
    crossed = []
    for s in range(1, n + 1):
        mine = nbr[off[s - 1]:off[s]]
        mine = mine[mine <= s]
        before = length.max()
        length[mine] += 1
        length[s] = mine.shape[0]
        for k in (K_INITIAL, 2 * K_INITIAL):
            if before <= k < length.max():
                crossed.append((k, s))
    assert [k for k, _ in crossed] == [K_INITIAL, 2 * K_INITIAL] and crossed[0][1] < crossed[1][1]
    assert np.array_equal(length[1:], ln)


def _model_against_oracle(g, n, stm_sizes, retire=()):
    ob, dv = O.OracleBayesFilter(DEFAULT_LC, 0.9), DeviceModel(n, DEFAULT_LC, 0.9)
    for s in range(1, n + 1):
        d = g.neighbors(s, DEPTH)
        ob.set_neighbors(s, sorted(d), [d[k] for k in sorted(d)])
        for k, m in d.items():
            dv.link(s - 1, k - 1, m)
    rng = np.random.default_rng(3)
    gone = set()
    for t, exclude in enumerate(stm_sizes):
        if t == 2:
            gone = set(retire)
        considered = [s for s in range(1, n - exclude + 1) if s not in gone]
        ids = [-1] + considered
        like = random_adjusted(len(ids), rng)
        adj = np.zeros(n + 1, np.float32)
        adj[0] = like[0]
        adj[np.asarray(considered)] = like[1:]
        inset = np.zeros(n, bool)
        inset[np.asarray(considered) - 1] = True
        ob.set_stm(list(range(n - exclude + 1, n + 1)))
        po = ob.compute_posterior(ids, like, dense=False)
        pd = dv.update(adj, inset)
        np.testing.assert_allclose(np.concatenate([[pd[0]], pd[np.asarray(considered)]]), po, rtol=2e-5, atol=1e-12)


def test_boundary_graph_through_the_device_model():
    g, info = boundary_graph(1100)
    assert set(BOUNDARY_LENGTHS) <= set(info["anchors"])
    _model_against_oracle(g, 1100, [400, info["stm"], info["stm"], 0], info["retire"])


def test_hub_graph_through_the_device_model():
    g, hub, places = hub_graph(700)
    _model_against_oracle(g, 700, [300, 30, 30, 0], [hub - 2, places[1] + 1])
