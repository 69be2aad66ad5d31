"""GPU test of the scratch the stateless calls share (rtabmap_amd/csrc/stateless_scratch.h): lcd_match_pairs, lcd_match_guided,
lcd_select_features and lcd_expand_word_ids take the two pinned job-table slots in turn and stage their host entries' data in the same
four buffers.  Calls of DIFFERENT families follow each other here, each with a table of another size and content, and every result is
compared exactly with the family's model (tests/*_model.py)."""
import numpy as np
import pytest
import torch

import feature_select_inputs as FI
import feature_select_model as FM
import guided_match_inputs as GI
import guided_match_model as GM
import pair_match_inputs as PI
import pair_match_model as PM

pytestmark = pytest.mark.gpu


def _pairs_concat(pairs):
    fo = np.cumsum([0] + [f.shape[0] for f, _ in pairs]).astype(np.int64)
    to = np.cumsum([0] + [t.shape[0] for _, t in pairs]).astype(np.int64)
    return np.concatenate([f for f, _ in pairs]), np.concatenate([t for _, t in pairs]), fo, to


def _dictionary(oracle, pairs):
    e = [PM.dictionary_pair(oracle, f, t, 0.8, True) for f, t in pairs]
    return np.concatenate([x[0] for x in e]), np.concatenate([x[1] for x in e])


def _expansion(rng, sizes):
    """-> (offsets, count, index, word_ids, first ids) of a batch of expansion frames"""
    ex = [FI.expansion_frame(rng, n) for n in sizes]
    off = np.cumsum([0] + list(sizes)).astype(np.int64)
    count = np.array([e["count"] for e in ex], np.int32)
    index = np.full(int(off[-1]), -9, np.int32)
    word_ids = np.full(int(off[-1]), 77, np.int32)                        # behind a frame's count: never read
    for f, e in enumerate(ex):
        index[off[f]:off[f] + e["count"]] = e["index"]
        word_ids[off[f]:off[f] + e["count"]] = e["word_ids"]
    return off, count, index, word_ids, np.array([9000 + 100 * f for f in range(len(ex))], np.int32)


def _inputs(oracle, dtype, dim):
    """per family a larger and a smaller batch with the model's answer; the pairs also one by one"""
    rng = np.random.default_rng(600 + dim)
    pair_a, pair_b = PI.interleaved_pair(dtype, dim, 65, 40, 610 + dim), PI.interleaved_pair(dtype, dim, 33, 31, 620 + dim)
    guided = {"large": [GI.general_pair(dtype, dim, 33, 31, 65, 630 + dim), GI.general_pair(dtype, dim, 20, 18, 30, 640 + dim)],
              "small": [GI.general_pair(dtype, dim, 12, 10, 17, 650 + dim)]}
    frames = {"large": [FI.tied_frame(rng, n) for n in (40, 55, 70)], "small": [FI.tied_frame(rng, 60)]}
    x = dict(pairs={"one": [pair_a], "large": [pair_a, pair_b], "small": [pair_b]}, guided=guided, frames=frames, max_features=50,
             rows={k: FI.rows_of(rng, dtype, dim, sum(len(f["response"]) for f in v)) for k, v in frames.items()},
             expand={"large": _expansion(rng, (50, 64)), "small": _expansion(rng, (30,))})
    x["pairs_exp"] = {k: _dictionary(oracle, v) for k, v in x["pairs"].items()}
    x["cross_exp"] = PM.cross_check(PI.dist(oracle, pair_b[1], pair_b[0]))
    x["guided_exp"] = {k: GI.expected_batch(oracle, v, GI.RADIUS, 0.8, GM.RATIO, GM.P2F) for k, v in guided.items()}
    x["expand_exp"] = {k: FM.expand_batch(*v) for k, v in x["expand"].items()}
    assert (FM.select_batch(frames["large"], 50)[0] == [40, 50, 50]).all()   # max_features cuts two of the three frames
    return x


def _host_entries(eng, x):
    """the four host entries with the larger inputs, then all four again with the smaller ones: every staging buffer is then used at a
    smaller size, with another call's bytes behind"""
    for size in ("large", "small"):
        f, t, fo, to = _pairs_concat(x["pairs"][size])
        gf, gt = eng.match_pairs(f, t, fo, to, "dictionary")
        np.testing.assert_array_equal(gf, x["pairs_exp"][size][0], err_msg=size + " pairs, from")
        np.testing.assert_array_equal(gt, x["pairs_exp"][size][1], err_msg=size + " pairs, to")
        GI.assert_same(GI.run_host(eng, x["guided"][size]), x["guided_exp"][size], size + " guided")
        FI.assert_same(FI.run_host(eng, x["frames"][size], x["max_features"], rows=x["rows"][size]), x["frames"][size], x["max_features"],
                       rows=x["rows"][size], what=size + " select")
        np.testing.assert_array_equal(eng.expand_word_ids(*x["expand"][size]), x["expand_exp"][size], err_msg=size + " expand")
    f, t = x["pairs"]["small"][0]
    gm, gd = eng.match_pair(f, t, "cross_check")                          # the other mode, over what the dictionary calls left behind
    np.testing.assert_array_equal(gm, x["cross_exp"][0])
    np.testing.assert_array_equal(np.ascontiguousarray(gd, np.float32).view(np.uint32), x["cross_exp"][1].view(np.uint32))


def test_calls_of_every_family_back_to_back(oracle):
    """match_pairs_dev, match_guided_dev, select_features_dev, expand_word_ids_dev and a match_pairs_dev that makes two groups (two table
    uploads) are enqueued with no synchronisation between them: six job tables through the two slots, each slot's next user a call of
    another family.  Then the host entries in turn, larger inputs first."""
    import rtabmap_amd
    x = _inputs(oracle, "f32", 64)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    canary = lambda n, dt=torch.int32: torch.full((n,), -7, dtype=dt, device="cuda")
    eng = rtabmap_amd.Engine("f32", 64)
    eng.set_option("pair_match_budget", 4)                                # one distance: every pair is a group of its own
    p1 = _pairs_concat(x["pairs"]["one"])
    p5 = _pairs_concat(x["pairs"]["large"])
    d1, d5 = [dev(a) for a in p1[:2]], [dev(a) for a in p5[:2]]
    o1, o5 = [canary(a.shape[0]) for a in p1[:2]], [canary(a.shape[0]) for a in p5[:2]]
    g = GI.concat(x["guided"]["large"])
    dg = [dev(a) for a in g[:5]]
    og = [canary(g[2].shape[0]), canary(g[2].shape[0]), torch.full((g[2].shape[0], 2), -7.0, dtype=torch.float32, device="cuda"), canary(g[1].shape[0])]
    st = FI.stage_dev(x["frames"]["large"], rows=x["rows"]["large"])
    e_off, e_count, e_index, e_words, e_first = x["expand"]["large"]
    de = [dev(a) for a in (e_count, e_index, e_words, e_first)]
    oe = canary(int(e_off[-1]))
    torch.cuda.synchronize()

    eng.match_pairs_dev(d1[0], d1[1], p1[2], p1[3], o1[0], o1[1], "dictionary")
    eng.match_guided_dev(*dg, *g[5:], *og)
    FI.launch_dev(eng, st, x["max_features"])
    eng.expand_word_ids_dev(e_off, de[0], de[1], de[2], oe, de[3])
    eng.match_pairs_dev(d5[0], d5[1], p5[2], p5[3], o5[0], o5[1], "dictionary")
    eng.synchronize()

    for got, exp, what in ((o1, x["pairs_exp"]["one"], "first call"), (o5, x["pairs_exp"]["large"], "two groups")):
        np.testing.assert_array_equal(got[0].cpu().numpy(), exp[0], err_msg=what + ", from")
        np.testing.assert_array_equal(got[1].cpu().numpy(), exp[1], err_msg=what + ", to")
    GI.assert_same(dict(count=og[0].cpu().numpy(), match=og[1].cpu().numpy(), dist=og[2].cpu().numpy(), owner=og[3].cpu().numpy()), x["guided_exp"]["large"])
    FI.assert_same(FI.to_host(eng, st), x["frames"]["large"], x["max_features"], rows=x["rows"]["large"], device=True)
    np.testing.assert_array_equal(oe.cpu().numpy(), x["expand_exp"]["large"])
    _host_entries(eng, x)
    assert eng.vocab_count() == (0, 0) and eng.sig_count() == (0, 0)
    eng.close()


def test_host_entries_in_turn_on_a_padded_handle(oracle):
    """u8 x 61: rows are stored 64 bytes apart, so every host entry pads them on the way in and lcd_select_features un-pads them on the
    way out"""
    import rtabmap_amd
    x = _inputs(oracle, "u8", 61)
    eng = rtabmap_amd.Engine("u8", 61)
    _host_entries(eng, x)
    eng.close()
