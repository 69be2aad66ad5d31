"""GPU tests of lcd_register_icp and lcd_register_icp_dev (rtabmap_amd/csrc/register_icp.hip) against tests/register_icp_model.py.  Every
comparison is exact: status, stop, iterations, counts, out_match over the whole region, and every float and double bit for bit, through both
entries and every search form (LCD_ICP_SEARCH_AUTO, LCD_ICP_SEARCH_BRUTE, LCD_ICP_SEARCH_GRID)."""
import numpy as np
import pytest
import torch

import register_icp_inputs as I
import register_icp_model as M

pytestmark = pytest.mark.gpu

LCD_ERR_INVALID, LCD_ERR_UNSUPPORTED = 1, 5
PER_PAIR = ("transform", "icp_transform", "correction", "status", "stop", "iterations", "n_correspondences", "ratio", "variance")
SEARCHES = (M.SEARCH_AUTO, M.SEARCH_BRUTE, M.SEARCH_GRID)
_model_cache = {}


def model_of(pair, **kw):
    key = (id(pair), tuple(sorted(kw.items())))
    if key not in _model_cache:
        _model_cache[key] = (pair, M.register(*I.scans(pair), **kw))       # the pair is kept so that its id stays its own
    return _model_cache[key][1]


def expected(pairs, device_entry=False, **kw):
    """the model's results laid out as the call lays its outputs out"""
    rs = [model_of(p, device_entry=device_entry, **kw) for p in pairs]
    out = {k: np.stack([np.asarray(r[k]) for r in rs]) for k in PER_PAIR}
    out["match"] = np.concatenate([r["match"] for r in rs] + [np.zeros(0, np.int32)])
    return out


def assert_same(got, want, what=""):
    for k in ("status", "stop", "iterations", "n_correspondences", "match"):
        np.testing.assert_array_equal(got[k], want[k], err_msg="%s %s" % (what, k))
    for k in ("transform", "icp_transform", "correction", "ratio"):
        np.testing.assert_array_equal(I.bits(got[k]), I.bits(want[k]), err_msg="%s %s" % (what, k))
    np.testing.assert_array_equal(np.ascontiguousarray(got["variance"]).view(np.uint64), np.ascontiguousarray(want["variance"], np.float64).view(np.uint64),
                                  err_msg=what + " variance")


def stage_dev(pairs):
    """the batch on the device, outputs canary-filled, uploaded and synchronised"""
    fx, fo, tx, to, gs = I.concatenate(pairs)
    n, nf = len(pairs), fx.shape[0]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device="cuda")
    st = dict(fx=dev(fx), fo=fo, tx=dev(tx), to=to, gs=gs, transform=full((n, 12), float("nan"), torch.float32),
              icp_transform=full((n, 12), float("nan"), torch.float32), correction=full((n, 12), float("nan"), torch.float32),
              status=full((n,), -7, torch.int32), stop=full((n,), -7, torch.int32), iterations=full((n,), -7, torch.int32),
              n_correspondences=full((n,), -7, torch.int32), ratio=full((n,), float("nan"), torch.float32), variance=full((n,), float("nan"), torch.float64),
              match=full((max(nf, 1),), -7, torch.int32))
    torch.cuda.synchronize()
    return st


def launch_dev(eng, st, **kw):
    eng.register_icp_dev(st["fx"], st["fo"], st["tx"], st["to"], st["gs"], st["transform"], st["icp_transform"], st["correction"], st["status"], st["stop"],
                         st["iterations"], st["n_correspondences"], st["ratio"], st["variance"], st["match"], **kw)
    return st


def to_host(eng, st):
    eng.synchronize()
    out = {k: st[k].cpu().numpy() for k in PER_PAIR + ("match",)}
    out["match"] = out["match"][:int(st["fo"][-1])]
    return out


def run_dev(eng, pairs, **kw):
    return to_host(eng, launch_dev(eng, stage_dev(pairs), **kw))


def run_host(eng, pairs, **kw):
    fx, fo, tx, to, gs = I.concatenate(pairs)
    return eng.register_icp(fx, fo, tx, to, gs, **kw)


def check_both(eng, pairs, what="", **kw):
    want = expected(pairs, **kw)
    for search in SEARCHES:
        assert_same(run_dev(eng, pairs, search=search, **kw), want, "%s dev, search %d" % (what, search))
        assert_same(run_host(eng, pairs, search=search, **kw), want, "%s host, search %d" % (what, search))
    return want


def _refused(status, call, *args, **kw):
    from rtabmap_amd import capi
    with pytest.raises(capi.LcdError) as err:
        call(*args, **kw)
    assert err.value.status == status, err.value


@pytest.fixture(scope="module")
def eng():
    import rtabmap_amd
    e = rtabmap_amd.Engine("f32", 64)
    yield e
    assert e.vocab_count() == (0, 0) and e.sig_count() == (0, 0)
    e.close()


@pytest.mark.parametrize("flat", [True, False])
def test_both_entries_equal_the_model_at_every_size(eng, flat):
    """sides of 0, 1, 2, 3, 255, 256, 257, 511, 512 and 513 rows in ONE batch, the empty and the tiny pairs between full ones"""
    want = check_both(eng, I.size_batch(flat), force_3dof=flat, **I.KW)
    assert {M.OK, M.EMPTY, M.NOT_CONVERGED} <= set(want["status"].tolist())


def test_8192_rows_on_both_sides(eng):
    pair = I.pair(8192, 8192, False, 41, noise=0.003)
    kw = dict(I.KW, max_iterations=2)
    want = expected([pair], **kw)
    assert want["stop"][0] == M.STOP_ITERATIONS and want["n_correspondences"][0] > 2000
    for search in SEARCHES:
        assert_same(run_dev(eng, [pair], search=search, **kw), want, "8192 dev, search %d" % search)
    assert_same(run_host(eng, [pair], **kw), want, "8192 host")
    small = I.size_batch(False)[8:11]                                      # beside small pairs, which the same launch's carve serves
    batch = [small[0], pair, small[1], small[2]]
    assert_same(run_dev(eng, batch, **kw), expected(batch, **kw), "8192 beside small pairs")


def test_non_finite_rows_on_the_device_entry(eng):
    """rows 255, 256 and 511 of both sides carry a NaN or an infinity: on the device entry they take part in nothing, the host entry refuses"""
    pairs = [I.with_non_finite(I.pair(600, 600, False, 7, noise=0.004)), I.pair(40, 50, True, 8), I.with_non_finite(I.pair(513, 512, True, 9, noise=0.004)),
             I.raw(np.full((4, 3), np.nan), np.ones((5, 3)))]
    for flat in (False, True):
        want = expected(pairs, device_entry=True, force_3dof=flat, **I.KW)
        for search in SEARCHES:
            assert_same(run_dev(eng, pairs, search=search, force_3dof=flat, **I.KW), want, "non-finite dev")
    assert want["status"][3] == M.EMPTY and (want["match"][[255, 256, 511]] == -1).all()
    _refused(LCD_ERR_INVALID, run_host, eng, pairs, **I.KW)


@pytest.mark.parametrize("name", sorted(I.hand_cases()))
def test_the_hand_made_cases_through_the_device(eng, name):
    p, kw = I.hand_cases()[name]
    check_both(eng, [p], name, force_3dof=p["flat"], **kw)


def test_epsilon_decided_by_one_float(eng):
    eps, below, _ = I.epsilon_pair(M)
    p, kw = I.hand_cases()["stop_mse"]
    a = check_both(eng, [p], force_3dof=True, **dict(kw, epsilon=eps))
    b = check_both(eng, [p], force_3dof=True, **dict(kw, epsilon=below))
    assert (a["stop"][0], a["iterations"][0]) != (b["stop"][0], b["iterations"][0])


def lattice_pairs():
    """targets on a lattice of the correspondence distance's spacing, negative coordinates and -0.0 among them, against rows on its faces,
    edges and centres: equal distances to several targets wherever a row looks, the lower row wins; flat, and with one point off the plane"""
    d = 0.25
    g = np.arange(-3, 4) * d
    flat = np.array([[x, y, 0.0] for x in g for y in g])
    flat[flat == 0] = -0.0
    rng = np.random.default_rng(3)
    rows = np.concatenate([flat[rng.permutation(len(flat))[:30]] + [d / 2, 0, 0], flat[:20] + [d / 2, d / 2, 0], flat[5:25] + [0, d / 2, 0], flat[::3]])
    off = np.concatenate([flat, [[0.0, 0.0, d]]])
    cube = np.array([[x, y, z] for x in g[2:5] for y in g[2:5] for z in g[2:5]])
    return [I.raw(rows, flat, flat=True), I.raw(rows, off), I.raw(cube + [d / 2, d / 2, d / 2], cube), I.raw(flat, rows, flat=True)]


def test_equal_distances_on_a_lattice(eng):
    pairs = lattice_pairs()
    for flat in (True, False):
        want = check_both(eng, pairs, "lattice", force_3dof=flat, max_iterations=3, max_correspondence_distance=0.25, correspondence_ratio=0.0)
        assert (want["n_correspondences"] > 0).all()


def test_the_grid_form_at_its_edges(eng):
    """ONE batch: every target in one cell, targets on cell faces and corners, a nearest target in a diagonal neighbour cell, equal distances
    across two cells (the lower row wins), a flat scan (nine cells), one with a point off the plane, a target row beyond the key's cell
    range (the pair is searched in the brute form inside the GRID call), a from-row beyond it (that row walks the target) and rows at the
    very edge of the range"""
    pairs = list(I.grid_edge_pairs().values())
    for flat in (False, True):
        want = check_both(eng, pairs, "grid edges", force_3dof=flat, **I.GRID_KW)
        assert (want["n_correspondences"] >= 3).all()
    kw = dict(I.GRID_KW, max_iterations=1, max_correspondence_distance=0.125)
    check_both(eng, [I.grid_edge_pairs()["equal_across_cells"]], "ties across cells", **kw)


def test_auto_on_either_side_of_its_threshold(eng):
    pairs = [I.pair(n, n, True, 900 + n, noise=0.004) for n in (1023, 1024, 1025)] + [I.pair(1500, 700, False, 77, noise=0.004), I.pair(700, 1500, False, 78, noise=0.004)]
    check_both(eng, pairs[:3], "auto 2-D", force_3dof=True, **dict(I.KW, max_iterations=3))
    check_both(eng, pairs[3:], "auto 3-D, the second grid on the other side of the threshold", **dict(I.KW, max_iterations=3))


def test_refusals_write_nothing(eng):
    pairs = I.size_batch(True)[8:10]
    fx, fo, tx, to, gs = I.concatenate(pairs)
    bad = [dict(max_iterations=0), dict(max_laser_scans=-1), dict(search=3), dict(max_correspondence_distance=0.0), dict(max_correspondence_distance=float("nan")),
           dict(max_correspondence_distance=1e200), dict(epsilon=-1.0), dict(correspondence_ratio=1.5)]
    for kw in bad:
        st = stage_dev(pairs)
        _refused(LCD_ERR_INVALID, launch_dev, eng, st, **dict(I.KW, **kw))
        _refused(LCD_ERR_INVALID, run_host, eng, pairs, **dict(I.KW, **kw))
        got = to_host(eng, st)
        assert (got["status"] == -7).all() and (got["match"] == -7).all() and np.isnan(got["transform"]).all()
    _refused(LCD_ERR_INVALID, eng.register_icp, fx, fo, tx, to, gs, struct_size=8, **I.KW)
    _refused(LCD_ERR_INVALID, eng.register_icp, fx, fo, tx, to, None, **I.KW)
    _refused(LCD_ERR_INVALID, eng.register_icp, fx, fo, tx, to, np.full_like(gs, np.inf), **I.KW)
    _refused(LCD_ERR_INVALID, eng.register_icp, fx, fo[::-1].copy(), tx, to, gs, **I.KW)
    big = I.raw(np.zeros((8193, 3)), np.zeros((3, 3)))
    _refused(LCD_ERR_UNSUPPORTED, run_host, eng, [big], **I.KW)
    out = eng.register_icp(np.zeros((0, 3), np.float32), [0], np.zeros((0, 3), np.float32), [0], np.zeros((0, 12), np.float32), **I.KW)
    assert out["status"].shape == (0,)
    assert_same(run_host(eng, pairs, **I.KW), expected(pairs, **I.KW), "after the refusals")


def test_unsynchronised_back_to_back_calls_share_the_scratch(eng):
    """three device calls enqueued without a synchronisation in between, the largest second: its scratch and job table grow while the first
    launch is still in flight, and each call reads its own"""
    batch = I.size_batch(False)
    groups = [batch[:4], batch[8:], batch[4:8]]
    sts = [launch_dev(eng, stage_dev(g), **I.KW) for g in groups]
    for g, st in zip(groups, sts):
        assert_same(to_host(eng, st), expected(g, **I.KW))


def test_the_mirror_class_through_the_engine():
    """RegistrationIcpHip::computeTransformation over a dictionary's engine: the rule's transform behind the host-side gates"""
    from rtabmap_amd import vwdictionary as V
    p = I.pair(300, 280, False, 31, guess_off=True)
    want = M.register(*I.scans(p), **I.KW)
    from rtabmap_amd import synth
    d = V.VWDictionaryHip(nndr=0.8, new_words_compared_together=True)
    d.add_new_words(synth.vocab_surf(50, seed=8), 1)
    d.update()
    before = (d.index_ids(), d.visual_words, d.indexed_words, d.not_indexed_words, d.total_active_references)
    t, info = d.register_icp(*I.scans(p), max_translation=0.0, max_rotation=0.0, **I.KW)
    np.testing.assert_array_equal(I.bits(t), I.bits(want["transform"]))
    assert info["icp_correspondences"] == want["n_correspondences"] and I.bits(info["icp_inliers_ratio"]) == I.bits(want["ratio"])
    v = want["variance"] / 10.0
    np.testing.assert_array_equal(info["covariance"], np.diag([v, v, v, v / 10.0, v / 10.0, v / 10.0]))
    t, info = d.register_icp(*I.scans(p), max_translation=1e-6, max_rotation=0.0, **I.KW)
    assert t is None and info["icp_translation"] > 1e-6
    assert (d.index_ids(), d.visual_words, d.indexed_words, d.not_indexed_words, d.total_active_references) == before
    d.close()


def test_pipelined_frame_stream_is_untouched_by_the_registration():
    """A pipelined SURF handle runs an appending frame stream; lcd_register_icp_dev calls between the frames change no frame output, bit for
    bit, against a run without them, and their own results are the model's"""
    import rtabmap_amd
    from rtabmap_amd import capi, synth
    n_words, q, n_sig, T = 2000, 96, 30, 8
    rng = np.random.default_rng(11)
    vocab = synth.vocab_surf(n_words, seed=12)
    words = synth.zipf_words(n_sig, q, n_words, seed=13)
    ids = np.arange(1, n_words + 1, dtype=np.int32)
    frames = []
    for t in range(T):
        d = vocab[rng.integers(0, n_words, q)] + rng.standard_normal((q, 64)).astype(np.float32) * np.float32(0.02)
        fresh = rng.random(q) < 0.3
        d[fresh] = synth.vocab_surf(q, seed=100 + t)[fresh]
        frames.append(torch.from_numpy(np.ascontiguousarray(d, np.float32)).cuda())
    pairs = I.size_batch(True)[6:12]
    kw = dict(I.KW, force_3dof=True)
    want = expected(pairs, **kw)
    cap = n_sig + T + 4
    out = {}
    for with_icp in (False, True):
        eng = rtabmap_amd.Engine("f32", 64, sig_capacity=cap, pipeline=True)
        eng.vocab_append(vocab, ids)
        eng.sig_add_bulk(np.arange(1, n_sig + 1, dtype=np.int32), np.arange(0, (n_sig + 1) * q, q, dtype=np.int64), words.reshape(-1))
        eng.set_option("next_word_id", n_words + 1)
        d_w = torch.zeros((T, q), dtype=torch.int32, device="cuda")
        d_l = torch.zeros((T, cap), dtype=torch.float32, device="cuda")
        d_first = torch.zeros(T, dtype=torch.int32, device="cuda")
        sts = [stage_dev(pairs) for _ in range(T)]
        for t in range(T):
            eng.frame_dev(frames[t].data_ptr(), q, n_sig + 1 + t, float(n_sig + 1 + t), d_w[t].data_ptr(), d_l[t].data_ptr(), cap,
                          first_new_word_id=capi.LCD_NEW_WORD_IDS_AUTO, append_new_words=True, d_first_new_word_id_ptr=d_first[t:].data_ptr())
            if with_icp:                                                # between the frames, nothing drained
                launch_dev(eng, sts[t], **kw)
        eng.synchronize()
        out[with_icp] = (d_w.cpu().numpy(), d_l.cpu().numpy(), d_first.cpu().numpy(), eng.vocab_count(), eng.sig_count())
        if with_icp:
            for st in sts:
                assert_same(to_host(eng, st), want, "between frames")
        eng.close()
    for a, b in zip(out[False][:3], out[True][:3]):
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))
    assert out[False][3:] == out[True][3:]
    assert out[True][3][0] > n_words
