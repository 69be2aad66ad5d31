"""What the GPU tests of the Bayes filter share: the engine they fill, the readers of the device's outputs and the comparison with the
oracle's posterior.  Moved here unchanged from tests/test_gpu_bayes.py; the tolerances are the project's (argued there and in _check).

Tolerance: every posterior entry within 2e-5 relative (+1e-12 absolute) of the oracle's after the normalisation constants are
divided out, and the constants within m * 2^-24 of each other -- the reference adds the m unnormalised entries into a float one by
one before dividing (BayesFilter.cpp:205-230) and multiplies through cv::gemm; the device sums in double in a fixed order.  The
selected hypothesis must be the oracle's unless the oracle's best two posteriors are closer than that tolerance."""
import numpy as np

from rtabmap_amd import synth

RTOL, ETOL, ATOL = 1e-4, 2e-5, 1e-12


def _engine_with_signatures(n_sig, q=8, pipeline=False):
    import rtabmap_amd
    n_words = 600
    eng = rtabmap_amd.Engine("f32", 64, sig_capacity=n_sig + 64, pipeline=pipeline)
    eng.vocab_append(synth.vocab_surf(n_words, seed=3), np.arange(1, n_words + 1, dtype=np.int32))
    words = synth.zipf_words(n_sig, q, n_words, seed=4)
    eng.sig_add_bulk(np.arange(1, n_sig + 1, dtype=np.int32), np.arange(0, (n_sig + 1) * q, q, dtype=np.int64), words.reshape(-1))
    return eng


def _pick(d_post, ids):
    """posterior entries of `ids` (-1 first) from a device vector laid out [virtual place, slot 0, slot 1, ...]; slot = id - 1"""
    got = d_post.cpu().numpy()
    return np.concatenate([[got[0]], got[np.asarray(ids[1:], np.int64)]]) if len(ids) > 1 else got[:1]


def _result(d_res):
    from rtabmap_amd.capi import LcdBayesResult
    return LcdBayesResult.from_buffer_copy(d_res.cpu().numpy().tobytes())


def _check(ids, post_o, post_d, res, ctx):
    """Entry by entry within ETOL once the two normalisation constants are divided out; the constants themselves within the error
    the reference's own accumulation carries: it adds the m unnormalised entries into a float one by one (BayesFilter.cpp:205-218),
    up to m * 2^-24 relative, while the device sums in double (measured: 6e-4 at m = 50 000, all of it in the reference's sum)."""
    m = len(ids)
    pos = post_o > 0
    r = float(np.median(post_d[pos].astype(np.float64) / post_o[pos].astype(np.float64))) if pos.any() else 1.0
    assert abs(r - 1.0) <= max(m * 2.0 ** -24, 2e-6), (ctx, r)
    np.testing.assert_allclose(post_d, post_o.astype(np.float64) * r, rtol=ETOL, atol=ATOL, err_msg=str(ctx))
    gtol = max(m * 2.0 ** -24, RTOL)
    hid, hval = __import__("oracle").OracleBayesFilter.hypothesis(ids, post_o)
    assert res.n_considered == m - 1
    np.testing.assert_allclose(res.value, hval, rtol=gtol, atol=gtol)
    np.testing.assert_allclose(res.virtual_place, post_o[0], rtol=gtol, atol=ATOL)
    if hid == 0:
        assert res.sig_id == 0 and res.slot == -1
        return
    po = np.asarray(post_o[1:], np.float64)
    top = np.sort(po)[::-1]
    if len(top) > 1 and top[0] - top[1] <= 4 * ETOL * top[0]:
        assert res.sig_id in [ids[1 + k] for k in np.flatnonzero(po >= top[0] * (1 - 8 * ETOL))]
    else:
        assert res.sig_id == hid, ctx
        assert res.slot == hid - 1
