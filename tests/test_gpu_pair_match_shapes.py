"""GPU tests of lcd_match_pairs / lcd_match_pairs_dev (rtabmap_amd/csrc/pair_match.hip) at the row sizes, frame sizes, ratios and batch
shapes tests/test_gpu_pair_match.py does not reach.  The expected value is always the model (pair_match_model over the oracle), every
comparison is exact (ids, indices, distance bits), every case goes through the host entry and the device entry (a padded handle: the
device entry refuses, which is asserted).  The inputs and the property each one is there for are tests/pair_match_inputs.py's;
tests/test_pair_match_inputs.py checks those properties without a GPU, the tests here assert them again on the expected output."""
import ctypes as C

import numpy as np
import pytest
import torch

import pair_match_inputs as I
import pair_match_model as M
import test_gpu_pair_match as B

pytestmark = pytest.mark.gpu

LCD_ERR_UNSUPPORTED = 5


def _expect(oracle, pairs, mode, compared=True, nndr=0.8, ids=None):
    """the model's answer for a batch, concatenated as the engine returns it"""
    if mode == "dictionary":
        e = [M.dictionary_pair(oracle, f, t, nndr, compared, from_word_ids=None if ids is None else ids[k]) for k, (f, t) in enumerate(pairs)]
    else:
        e = [M.cross_check(I.dist(oracle, t, f)) for f, t in pairs]
    return _cat(e)


def _cat(e):
    return np.concatenate([x[0] for x in e]), np.concatenate([x[1] for x in e])


def _same(got, exp, mode, what):
    np.testing.assert_array_equal(got[0], exp[0], err_msg=what)
    if mode == "cross_check":
        np.testing.assert_array_equal(B._bits(got[1]), B._bits(exp[1]), err_msg=what + " (distance bits)")
    else:
        np.testing.assert_array_equal(got[1], exp[1], err_msg=what)


def _both_entries(eng, pairs, mode, exp, ids=None, dev=True, what="", **kw):
    """one batch through lcd_match_pairs and through lcd_match_pairs_dev, each compared with the model"""
    f, t, fo, to = B._concat(pairs)
    got = eng.match_pairs(f, t, fo, to, mode, from_word_ids=None if ids is None else np.concatenate(ids), **kw)
    _same(got, exp, mode, "%s %s host entry" % (what, mode))
    if dev:
        _same(B._dev(eng, pairs, mode, ids=ids, **kw)[:2], exp, mode, "%s %s device entry" % (what, mode))


def _all_modes(oracle, eng, pairs, dev=True, what=""):
    for compared in (True, False):
        _both_entries(eng, pairs, "dictionary", _expect(oracle, pairs, "dictionary", compared), dev=dev, what=what, new_words_compared=compared)
    _both_entries(eng, pairs, "cross_check", _expect(oracle, pairs, "cross_check"), dev=dev, what=what)


# ------------------------------------------------------------------------------------------------ 1. every distance kernel
# which pair_dist_kernel<DTYPE, K> launch_pair_dist picks for the handle (K in dwords; K == 0: l2_ref_dyn / hamming_dyn over kdyn dwords)
KERNELS = [
    ("f32", 3, "<0,0>, kdyn 3: l2_ref_dyn's scalar tail alone, rows 12 bytes apart"),
    ("f32", 32, "<0,0>, kdyn 32: eight trips of four, no tail"),
    ("f32", 61, "<0,0>, kdyn 61: fifteen trips of four and one tail element"),
    ("f32", 64, "<0,64>"),
    ("f32", 128, "<0,128>"),
    ("f32", 256, "<0,0>, kdyn 256"),
    ("u8", 8, "<1,0>, kdyn 2"),
    ("u8", 16, "<1,0>, kdyn 4"),
    ("u8", 24, "<1,0>, kdyn 6"),
    ("u8", 32, "<1,8>"),
    ("u8", 33, "<1,0>, kdyn 9: rows stored padded to 36 bytes, host entry only"),
    ("u8", 64, "<1,16>"),
    ("u8", 128, "<1,0>, kdyn 32"),
]


@pytest.mark.parametrize("dtype,dim", [k[:2] for k in KERNELS])
def test_every_distance_kernel(oracle, dtype, dim):
    """(33, 65) and (65, 31) cross TILE_A = 32 and TILE_B = 64 with either frame in either role, (1, 3) has no index, the duplicate pair
    ties at distance 0; a distance that misses one dword or one tail element changes the cross-check's distance bits at once"""
    import rtabmap_amd
    from rtabmap_amd import capi
    pairs = I.kernel_case_pairs(dtype, dim)
    padded = dtype == "u8" and dim % 4 != 0
    e = M.dictionary_pair(oracle, *pairs[0], 0.8, True)
    cls = I.to_classes(*e)
    assert (cls == I.TOOK_FROM_WORD).any() and (cls == I.CREATED).any()
    assert M.tie_resolved_by_index(I.dist(oracle, pairs[3][1], pairs[3][0]))
    eng = rtabmap_amd.Engine(dtype, dim)
    _all_modes(oracle, eng, pairs, dev=not padded)
    if padded:
        with pytest.raises(capi.LcdError) as err:
            B._dev(eng, pairs, "cross_check")
        assert err.value.status == LCD_ERR_UNSUPPORTED
        _both_entries(eng, pairs, "cross_check", _expect(oracle, pairs, "cross_check"), dev=False)      # the handle stays usable
    eng.close()


@pytest.mark.parametrize("dim", [61, 128])
def test_integer_valued_float_rows(oracle, dim):
    """raw histogram descriptors: every distance a small integer, best and second-best tie at distances that are not 0, nndr * d exact or
    rounded once -- <0,0> with its tail (61) and <0,128> on rows that are not unit-norm"""
    import rtabmap_amd
    pairs = [I.integer_pair(dim, nf, nt, 50 + dim) for nf, nt in ((33, 65), (65, 31))]
    for f, t in pairs:
        s = np.sort(I.dist(oracle, t, f), axis=1)
        assert ((s[:, 0] == s[:, 1]) & (s[:, 0] > 0)).any() and (s[:, 0] == 0).any()
    eng = rtabmap_amd.Engine("f32", dim)
    _all_modes(oracle, eng, pairs)
    eng.close()


# ------------------------------------------------------------------------------------------------ 2. sides past one workgroup's width
@pytest.mark.parametrize("nf,nt", I.LARGE_SIZES)
@pytest.mark.parametrize("dtype,dim", [("f32", 64), ("u8", 32)])
def test_sides_longer_than_the_workgroup(oracle, dtype, dim, nf, nt):
    """every loop of dictionary_pair and cross_check_pair strided by RBLOCK, RBLOCK / 64 or the bit-row word makes a second (third) trip,
    and what the later trips decide depends on rows of the earlier ones and the other way round (asserted on the model)"""
    import rtabmap_amd
    f, t, together = I.large_pair(oracle, dtype, dim, nf, nt)
    assert I.spans_boundaries(*together)
    eng = rtabmap_amd.Engine(dtype, dim)
    _both_entries(eng, [(f, t)], "dictionary", together, new_words_compared=True)
    apart = M.dictionary_pair(oracle, f, t, 0.8, False)
    assert apart[0].tolist() == list(range(1, nf + 1))
    _both_entries(eng, [(f, t)], "dictionary", apart, new_words_compared=False)
    cf, ct, D, cross = I.tie_pair(oracle, dtype, dim, nf, nt)
    assert M.tie_resolved_by_index(D) and I.cross_spans_boundaries(cross[0], nf)
    _both_entries(eng, [(f, t), (cf, ct)], "cross_check", _cat([M.cross_check(I.dist(oracle, t, f)), cross]))
    eng.close()


@pytest.mark.parametrize("dtype,dim", [("f32", 64), ("u8", 32)])
def test_given_ids_on_a_long_from_frame(oracle, dtype, dim):
    """from_word_ids at 2049 rows: the rank loop and the atomicMax take three trips; exact twins on both sides of row 1024 meet a to-row
    at distance 0 and the lower ID wins, in front of the boundary or behind it"""
    import rtabmap_amd
    f, t, ids, triples, exp = I.given_ids_pair(oracle, dtype, dim)
    assert {bool(ids[b] < ids[a]) for a, b, _ in triples} == {True, False}
    assert all(a < 1024 <= b and exp[1][i] == min(ids[a], ids[b]) for a, b, i in triples)
    assert np.array_equal(exp[0], ids) and exp[1].max() > ids.max()
    eng = rtabmap_amd.Engine(dtype, dim)
    _both_entries(eng, [(f, t)], "dictionary", exp, ids=[ids])
    eng.close()


# ------------------------------------------------------------------------------------------------ 3. the limit itself
@pytest.mark.parametrize("nf,nt", I.LIMIT_SIZES)
def test_8192_rows_on_one_side(oracle, nf, nt):
    """MAX_SIDE rows: resolve_body's two masks and prefix sums fill pair_match_kernel's LDS array to its last word.  8192 from-rows compared
    (8192 to-rows) compared together need a 256 MiB from x from (to x to) block beside the to x from block: more than the default budget,
    "a single pair always fits" """
    import rtabmap_amd
    f, t, together = I.large_pair(oracle, "f32", 64, nf, nt)
    assert I.spans_boundaries(*together)
    ld = lambda n: (n + 63) // 64 * 64
    floats = nt * ld(nf) + nf * ld(nf) + nt * ld(nt)
    assert floats * 4 > 256 << 20                                              # (8192 to-rows: the to x to block)
    eng = rtabmap_amd.Engine("f32", 64)
    bytes0 = eng.stats()["bytes_device"]
    _both_entries(eng, [(f, t)], "dictionary", M.dictionary_pair(oracle, f, t, 0.8, False), new_words_compared=False)
    _both_entries(eng, [(f, t)], "cross_check", M.cross_check(I.dist(oracle, t, f)))
    assert eng.stats()["bytes_device"] - bytes0 < floats * 4                   # (neither needs a same-frame block)
    _both_entries(eng, [(f, t)], "dictionary", together, new_words_compared=True)
    assert eng.stats()["bytes_device"] - bytes0 >= floats * 4
    eng.close()


# ------------------------------------------------------------------------------------------------ 4. the ratio
@pytest.mark.parametrize("nf,nt", I.RATIO_SIZES)
@pytest.mark.parametrize("dtype,dim", [("f32", 64), ("u8", 32)])
def test_ratios_other_than_the_default(oracle, dtype, dim, nf, nt):
    """c0.d > nndr * c1.d at 0.0 (only distance 0 passes), 0.6 and 1.0 (only "fewer than two candidates" rejects): four different results
    on one input, all of them the model's"""
    import rtabmap_amd
    f, t, exp = I.ratio_pair(oracle, dtype, dim, nf, nt)
    assert I.ratios_tell_apart(f, t, exp)
    assert set(exp[(1.0, True)][0].tolist()) == {1, 2} and np.unique(exp[(0.0, True)][0]).size < nf
    eng = rtabmap_amd.Engine(dtype, dim)
    for nndr in (0.0, 0.6, 1.0):
        for compared in (True, False):
            _both_entries(eng, [(f, t)], "dictionary", exp[(nndr, compared)], what="nndr %g" % nndr, new_words_compared=compared, nndr=nndr)
    eng.close()


# ------------------------------------------------------------------------------------------------ 5. the have_index boundary
@pytest.mark.parametrize("dtype,dim", [("f32", 64), ("u8", 32)])
def test_from_frames_that_collapse_into_two_or_three_words(oracle, dtype, dim):
    """many from-rows, k distinct: compared together the to-frame searches exactly two words (k = 1, 2: the smallest vocabulary with an
    index) or three; in one batch with pairs that have no index at all (one from-row, no from-row) between them"""
    import rtabmap_amd
    rng = np.random.default_rng(dim)
    one = I.fresh(rng, dtype, dim, 1)
    c = {(k, nf): I.collapsing_pair(dtype, dim, k, nf, 40) for k in (1, 2, 3) for nf in (5, 1100)}
    pairs = [c[(1, 5)], c[(2, 1100)], (one, np.ascontiguousarray(np.repeat(one, 3, axis=0))), c[(3, 5)], c[(1, 1100)],
             I.interleaved_pair(dtype, dim, 0, 5, 1), c[(2, 5)], c[(3, 1100)]]
    for compared in (True, False):
        e = [M.dictionary_pair(oracle, f, t, 0.8, compared) for f, t in pairs]
        if compared:
            assert [np.unique(x[0]).size for x in e] == [2, 2, 1, 3, 2, 0, 2, 3]
            assert e[0][0].tolist() == [1, 2, 1, 1, 1] and e[4][0][:4].tolist() == [1, 2, 1, 1] and e[2][1].tolist() == [2, 3, 2]
        else:
            assert [np.unique(x[0]).size for x in e] == [5, 1100, 1, 5, 1100, 0, 5, 1100]
        eng = rtabmap_amd.Engine(dtype, dim)
        _both_entries(eng, pairs, "dictionary", _cat(e), new_words_compared=compared)
        eng.close()


# ------------------------------------------------------------------------------------------------ 6. many pairs
@pytest.mark.parametrize("dtype,dim", [("f32", 64), ("u8", 32)])
def test_700_small_pairs_in_one_call(oracle, dtype, dim):
    """2100 distance blocks behind one binary search (the existing tests stop at about 45), empty sides among them; once in one group,
    once under a budget of 256 KiB, which cuts the batch into groups of several pairs each (a 40 + 40 pair needs 30 KiB)"""
    import rtabmap_amd
    pairs = I.many_small_pairs(dtype, dim, 700, 11 + dim)
    sizes = [(f.shape[0], t.shape[0]) for f, t in pairs]
    assert (0, 0) in sizes and any(a == 0 and b > 0 for a, b in sizes) and any(a > 0 and b == 0 for a, b in sizes)
    exp = {m: _expect(oracle, pairs, *m) for m in (("dictionary", True), ("dictionary", False), ("cross_check",))}
    eng = rtabmap_amd.Engine(dtype, dim)
    for budget in (0, 256 << 10):
        eng.set_option("pair_match_budget", budget)
        _both_entries(eng, pairs, "dictionary", exp[("dictionary", True)], what="budget %d" % budget, new_words_compared=True)
        _both_entries(eng, pairs, "dictionary", exp[("dictionary", False)], what="budget %d" % budget, new_words_compared=False)
        _both_entries(eng, pairs, "cross_check", exp[("cross_check",)], what="budget %d" % budget)
    eng.close()


# ------------------------------------------------------------------------------------------------ 7. the group boundary
def test_budget_that_fits_exactly_and_one_float_less(oracle):
    """The fifteen pairs of test_groups_and_scratch_growth_do_not_change_results.  The host loop closes a group when
    floats + need > budget: with the budget at exactly the distance floats of the first eight pairs they share a group, four bytes less
    and the eighth starts the next one.  Both calls go through the device entry back to back, without a synchronisation between them (the
    second uses the other job-table slot while the first may still run), then through the host entry.  The grouping cannot be observed
    from outside: what this pins is that the results are the model's on either side of the comparison."""
    import rtabmap_amd
    pairs = [B._pair("f32", 64, nf, nt, 300 + k) for k, (nf, nt) in enumerate(B.SEVEN)]
    big = pairs + [B._pair("f32", 64, 200, 260, 399)] + pairs[::-1]
    ld_of = lambda n: (n + 63) // 64 * 64                                     # pair_match.hip's, restated
    floats = lambda nf, nt: nt * ld_of(nf) + nf * ld_of(nf) + nt * ld_of(nt)  # to x from, from x from, to x to (compared together)
    first8 = sum(floats(f.shape[0], t.shape[0]) for f, t in big[:8])
    assert first8 == 9 * 64 + (40 * 64 + 33 * 64 * 2) + (130 * 192 + 70 * 192 + 70 * 128) + 12 * 64 + 3 * 64 + (65 * 128 + 64 * 128 + 64 * 64) \
        + (7 * 64 + 200 * 64 + 200 * 256) + (200 * 256 + 260 * 256 + 260 * 320)
    exp = _expect(oracle, big, "dictionary", True)
    f, t, fo, to = B._concat(big)
    d_f, d_t = torch.from_numpy(f).cuda(), torch.from_numpy(t).cuda()
    o = [torch.full((n,), -7, dtype=torch.int32, device="cuda") for n in (f.shape[0], t.shape[0], f.shape[0], t.shape[0])]
    eng = rtabmap_amd.Engine("f32", 64)
    torch.cuda.synchronize()
    eng.set_option("pair_match_budget", 4 * first8)
    eng.match_pairs_dev(d_f, d_t, fo, to, o[0], o[1], "dictionary")
    eng.set_option("pair_match_budget", 4 * first8 - 4)
    eng.match_pairs_dev(d_f, d_t, fo, to, o[2], o[3], "dictionary")
    eng.synchronize()
    for k in range(4):
        np.testing.assert_array_equal(o[k].cpu().numpy(), exp[k % 2], err_msg="device call %d" % (k // 2))
    for budget in (4 * first8, 4 * first8 - 4):
        eng.set_option("pair_match_budget", budget)
        _same(eng.match_pairs(f, t, fo, to, "dictionary"), exp, "dictionary", "host entry, budget %d" % budget)
    eng.close()


# ------------------------------------------------------------------------------------------------ 8. the largest accepted batch
def test_65535_pairs_of_one_row_each(oracle):
    """n_pairs at its limit (65536 is refused).  One from-row is one word, which is no index: the to-row is a new word, id 2, whatever it
    holds; the cross-check matches from-row 0 at the pair's distance.  Rows with integer entries, the to-row one entry off by p % 7: the
    distance is (p % 7)^2 exactly.  Five of the pairs also against the model."""
    import rtabmap_amd
    n = 65535
    rng = np.random.default_rng(8)
    f = rng.integers(0, 9, (n, 64)).astype(np.float32)
    t = f.copy()
    t[np.arange(n), np.arange(n) % 64] += (np.arange(n) % 7).astype(np.float32)
    off = np.arange(n + 1, dtype=np.int64)
    want_d = ((np.arange(n) % 7) ** 2).astype(np.float32)
    for p in (0, 1, 6, 40000, n - 1):
        for compared in (True, False):
            e = M.dictionary_pair(oracle, f[p:p + 1], t[p:p + 1], 0.8, compared)
            assert e[0].tolist() == [1] and e[1].tolist() == [2]
        m, d = M.cross_check(I.dist(oracle, t[p:p + 1], f[p:p + 1]))
        assert m.tolist() == [0] and d.tolist() == [want_d[p]]
    eng = rtabmap_amd.Engine("f32", 64)
    for compared in (True, False):
        gf, gt = eng.match_pairs(f, t, off, off, "dictionary", new_words_compared=compared)
        np.testing.assert_array_equal(gf, np.full(n, 1, np.int32))
        np.testing.assert_array_equal(gt, np.full(n, 2, np.int32))
    gm, gd = eng.match_pairs(f, t, off, off, "cross_check")
    np.testing.assert_array_equal(gm, np.zeros(n, np.int32))
    np.testing.assert_array_equal(B._bits(gd), B._bits(want_d))
    eng.close()


# ------------------------------------------------------------------------------------------------ 9. no distance output
@pytest.mark.parametrize("dtype,dim", [("f32", 64), ("u8", 32)])
def test_cross_check_without_a_distance_output(oracle, dtype, dim):
    """out_to_dist == NULL (include/lcd.h allows it) on both entries: the matches are the model's and nothing else is written -- not the
    words behind the matches, and not the place where the distances would go when both outputs are slices of one buffer"""
    import rtabmap_amd
    from rtabmap_amd import capi
    pairs = [I.interleaved_pair(dtype, dim, nf, nt, 60 + k) for k, (nf, nt) in enumerate(B.SEVEN)] + [I.kernel_case_pairs(dtype, dim)[3]]
    exp_m, exp_d = _expect(oracle, pairs, "cross_check")
    assert (exp_m >= 0).any() and (exp_m < 0).any()
    f, t, fo, to = B._concat(pairs)
    nt = t.shape[0]
    eng = rtabmap_amd.Engine(dtype, dim)
    # device entry: [matches | where the distances would go | guard]
    d_f, d_t = torch.from_numpy(f).cuda(), torch.from_numpy(t).cuda()
    buf = torch.full((2 * nt + 64,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    eng.match_pairs_dev(d_f, d_t, fo, to, buf[:nt], None, "cross_check")
    eng.synchronize()
    got = buf.cpu().numpy()
    np.testing.assert_array_equal(got[:nt], exp_m)
    assert (got[nt:] == -7).all()
    # ... and with the distances asked for, into the second slice
    eng.match_pairs_dev(d_f, d_t, fo, to, buf[:nt], buf[nt:2 * nt].view(torch.float32), "cross_check")
    eng.synchronize()
    got = buf.cpu().numpy()
    np.testing.assert_array_equal(got[:nt], exp_m)
    np.testing.assert_array_equal(got[nt:2 * nt].view(np.uint32), B._bits(exp_d))
    assert (got[2 * nt:] == -7).all()
    # host entry, a raw argument struct with out_to_dist = NULL
    host = np.full(2 * nt + 64, -7, np.int32)
    a = capi.LcdMatchArgs(C.sizeof(capi.LcdMatchArgs), capi.LCD_MATCH_CROSS_CHECK, len(pairs), 0, 0.8, 0)
    a.from_rows, a.to_rows, a.from_offsets, a.to_offsets = f.ctypes.data, t.ctypes.data, fo.ctypes.data, to.ctypes.data
    a.out_to_match, a.out_to_dist = host.ctypes.data, None
    assert eng.L.lcd_match_pairs(eng.h, C.byref(a)) == 0
    np.testing.assert_array_equal(host[:nt], exp_m)
    assert (host[nt:] == -7).all()
    eng.close()
