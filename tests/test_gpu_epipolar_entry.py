"""The epipolar check through the host mirrors: VWDictionaryHip.verify_epipolar -> EpipolarGeometryHip::check and findFFromWords against the model, and
RtabmapHip::process(descriptors, keypoints) under VhEp/Enabled on a short stream."""
import numpy as np
import pytest

import epipolar_inputs as I
import epipolar_model as M

pytestmark = pytest.mark.gpu


def test_check_and_find_f_from_words_equal_the_model():
    from rtabmap_amd import synth
    from rtabmap_amd.vwdictionary import VWDictionaryHip
    d = VWDictionaryHip(nndr=0.8, new_words_compared_together=True)
    d.add_new_words(synth.vocab_surf(50, seed=8), 1)                       # the engine exists once the dictionary holds words
    d.update()
    try:
        for pair, kw in ((I.scene(1, 120), {}), (I.with_m(7), {}), (I.all_equal(), {}), (I.scene(3, 100), dict(match_count_min=90)), (I.id_cases(), {})):
            want = M.verify(*I.frames(pair), iterations=1000, **kw)
            got = d.verify_epipolar((pair["from_ids"], pair["from_points"]), (pair["to_ids"], pair["to_points"]), **kw)
            assert got is not None
            accepted, f, pairs, status, engine_status = got
            assert accepted == (want["status"] == M.OK) and engine_status == want["status"]
            assert pairs == want["matches"].tolist()
            assert np.array_equal(M.bits(f), M.bits(want["fundamental"]))
            assert [i for i, s in zip(pairs, status) if s] == want["inliers"].tolist()
            assert d.check_epipolar((pair["from_ids"], pair["from_points"]), (pair["to_ids"], pair["to_points"]), **kw) == accepted
        assert d.verify_epipolar((pair["from_ids"], pair["from_points"]), (pair["to_ids"], pair["to_points"]), ransac_param1=0.0) is None   # refused
    finally:
        d.close()


PLACES, GOOD, BAD, STM, ROWS, THR = 16, range(2, 8), range(8, 14), 3, 100, 0.11
ROUTE = list(range(PLACES)) + list(GOOD) + list(BAD)


def stream():
    """Sixteen places seen once, then places 2 .. 7 and 8 .. 13 again, each revisit with its place's descriptors under a little noise, so that
    row i of a revisit gets the word row i of the first visit created.  Keypoints: the first visit sees a scene's from-keypoints; a revisit of
    2 .. 7 sees the same scene's to-keypoints (a camera motion, no outliers); a revisit of 8 .. 13 sees unrelated keypoints."""
    from rtabmap_amd import synth
    rng = np.random.default_rng(11)
    places = [synth.vocab_surf(ROWS, seed=5000 + p) for p in range(PLACES)]
    scenes = [I.scene(40 + p, ROWS, outliers=0.0, extra=0, shuffle=False) for p in range(PLACES)]
    frames = []
    for t, p in enumerate(ROUTE):
        d = places[p] + rng.standard_normal(places[p].shape).astype(np.float32) * np.float32(0.02)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        kp = scenes[p]["from_points"] if t < PLACES else scenes[p]["to_points"] if p in GOOD else rng.uniform(0, 480, (ROWS, 2)).astype(np.float32)
        frames.append((p, np.ascontiguousarray(d), kp))
    return frames


def run_stream(frames, epipolar, forget_first=False):
    from rtabmap_amd.vwdictionary import RtabmapHip
    r = RtabmapHip(loop_thr=THR, stm_size=STM, epipolar=epipolar)
    try:
        out, place_of = [], {}
        for t, (p, desc, kp) in enumerate(frames):
            o = r.process(desc, kp)
            place_of[o["id"]] = p
            o["loop_place"] = place_of.get(o["loop"][0])
            o["kept"] = r.epipolar_kept()
            out.append(o)
            if forget_first and t == PLACES - 1:
                r.memory.forget(out[0]["id"])
        for t, o in enumerate(out):
            print("frame %2d place %2d id %2d highest %s loop %s kept %d" % (t, frames[t][0], o["id"], o["highest"], o["loop"], o["kept"]))
        return out
    finally:
        r.close()


def test_process_with_keypoints_accepts_the_true_revisits_and_rejects_the_others():
    """The same stream three times.  Flag off: revisits of both kinds close loops on their own place (and, the filter being what it is, a few
    hypotheses on a neighbouring place close too).  VhEp/Enabled with VhEp/MatchCountMin = 20: every loop that closes is on the frame's own
    place; true revisits close; no unrelated revisit closes, although its hypothesis is the right place and above the threshold.
    VhEp/MatchCountMin = 1000, more than the pairs there are: every hypothesis is rejected, the true revisits' too.  A run whose caller
    forgets a location keeps no words for it."""
    frames = stream()
    good_t = [t for t, (p, _, _) in enumerate(frames) if t >= PLACES and p in GOOD]
    bad_t = [t for t, (p, _, _) in enumerate(frames) if t >= PLACES and p in BAD]
    off = run_stream(frames, dict(enabled=False))
    on = run_stream(frames, dict(enabled=True, match_count_min=20, ransac_param1=3.0))
    few = run_stream(frames, dict(enabled=True, match_count_min=1000, ransac_param1=3.0))
    assert all(o["ok"] for o in off + on + few)
    assert [o["id"] for o in off] == [o["id"] for o in on] == [o["id"] for o in few] == list(range(1, len(frames) + 1))
    assert all(o["kept"] == 0 for o in off) and [o["kept"] for o in on] == list(range(1, len(frames) + 1))
    own = lambda run, t: run[t]["loop"][0] > 0 and run[t]["loop_place"] == frames[t][0]
    assert any(own(off, t) for t in good_t) and any(own(off, t) for t in bad_t)       # with the flag off both kinds of revisit are accepted
    assert all(o["loop"][0] == 0 or own(on, t) for t, o in enumerate(on))             # with it on, only a loop the geometry supports closes
    assert any(own(on, t) for t in good_t)                                            # the true revisits pass the check
    assert not any(on[t]["loop"][0] > 0 for t in bad_t)                               # unrelated keypoints: rejected by epipolar geometry ...
    assert any(on[t]["highest"][1] >= THR and on[t]["highest"][0] == off[t]["loop"][0] and own(off, t) for t in bad_t)   # ... not by the threshold
    assert not any(o["loop"][0] > 0 for o in few)                                     # fewer pairs than VhEp/MatchCountMin: every hypothesis rejected
    assert any(few[t]["highest"][1] >= THR and few[t]["highest"][0] == on[t]["loop"][0] for t in good_t if own(on, t))
    forgot = run_stream(frames, dict(enabled=True, match_count_min=20, ransac_param1=3.0), forget_first=True)
    assert forgot[PLACES - 1]["kept"] == PLACES and forgot[PLACES]["kept"] == PLACES
