"""The two running maxima of the matrix-core 2-NN, which their writers read before they raise (an atomic only for a value above what the
maximum was seen to be), and the tail of launch B's re-rank, which hands the candidate threshold over before the results are stored and stores
them from the two lanes that hold them.

* knn_max_err_ratio (lcd_get_stats): the largest |filter score - exact distance| / eps any re-ranked candidate has shown.  A stream whose
  frames show a larger ratio each, sent back to back and one at a time: non-decreasing values, equal final bits.  The frames are built so
  that every error term scales alike: vocabulary block j holds rows of norm g_j, frame t's descriptors are noisy copies of block t's rows,
  so |q| |v| = g_t^2 while eps is made with the vocabulary's largest |row|^2 = 1: the ratio grows like g_t^2 / (g_t^2 + 1), by a factor of
  1.4 to 1.7 per frame.  (A pipelined handle keeps the maximum per ring set of four frames: the newest frame's set is what it reports, and a
  stream that rises with every frame shows that frame's own maximum.)
* the running maximum of |row|^2 (the filters' error bound): a frame appends words of |row|^2 = 9 to a vocabulary of unit rows, the next
  frames ask for neighbours next to them.
* results, candidate bit rows and lists: frames with clusters of near-duplicate fresh descriptors (more than the list's four entries below a
  descriptor), at q = 1, 2, 63, 64, 65, 129, against the plain handle through lcd_debug_last_frame_knn and the frames' word ids."""
import ctypes as C

import numpy as np
import pytest
import torch

from rtabmap_amd import capi, synth

pytestmark = pytest.mark.gpu
MODES = ["f16", "bf16"]
N_WORDS = 600
G2 = [0.02, 0.034, 0.058, 0.1, 0.17, 0.29, 0.5, 1.0]                   # |row|^2 of the eight vocabulary blocks (75 rows each)

_CACHE = {}


def _base(dim=64):
    """unit rows, computed once per row length and never written to"""
    if dim not in _CACHE:
        if dim == 64:
            v = synth.vocab_surf(N_WORDS, seed=1000 + N_WORDS)
        else:
            v = np.random.default_rng(7 + dim).standard_normal((N_WORDS, dim)).astype(np.float32)
            v = np.ascontiguousarray(v / np.linalg.norm(v, axis=1, keepdims=True), dtype=np.float32)
        v.setflags(write=False)
        _CACHE[dim] = v
    return _CACHE[dim]


def _graded(dim):
    """the vocabulary in eight blocks of rising norm, and one frame of q descriptors per block: noisy copies of its rows"""
    key = ("graded", dim)
    if key not in _CACHE:
        base = _base(dim)
        per = N_WORDS // len(G2)
        g = np.repeat(np.sqrt(np.array(G2, np.float32)), per)[:, None]
        vocab = np.ascontiguousarray(base * g, dtype=np.float32)
        rng = np.random.default_rng(31 + dim)
        frames = {}
        for q in (65, 129):
            fr = []
            for t in range(len(G2)):
                rows = t * per + rng.integers(0, per, q)
                f = vocab[rows] * (1.0 + 0.01 * rng.standard_normal((q, dim))).astype(np.float32)
                fr.append(np.ascontiguousarray(f, dtype=np.float32))
            frames[q] = fr
        vocab.setflags(write=False)
        _CACHE[key] = (vocab, frames)
    return _CACHE[key]


def _bits(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


def _frame_knn(eng, q):
    """lcd_debug_last_frame_knn: (rows, words, distances) [q x 2] of the latest frame's 2-NN stage as it stands, its descriptor count, its rejected queries"""
    lib = capi.load()
    row, word, dist = np.zeros((q, 2), np.int32), np.zeros((q, 2), np.int32), np.zeros((q, 2), np.float32)
    nq, rej = C.c_int(0), C.c_int(0)
    rc = lib.lcd_debug_last_frame_knn(eng.h, row.ctypes.data_as(C.c_void_p), word.ctypes.data_as(C.c_void_p), dist.ctypes.data_as(C.c_void_p), q, C.byref(nq), C.byref(rej))
    assert rc == 0
    return (row[: nq.value], word[: nq.value], dist[: nq.value]), nq.value, rej.value


# ---------------------------------------------------------------------------------------------- 1. the error ratio's running maximum
def _ratio_stream(knn_mode, vocab, frames, one_at_a_time):
    """the frames through a pipelined handle (no word is appended: every frame meets the same vocabulary); knn_max_err_ratio behind every frame
    (one at a time) or behind the last one only"""
    import rtabmap_amd
    T, q = len(frames), frames[0].shape[0]
    eng = rtabmap_amd.Engine("f32", 64, sig_capacity=T + 8, pipeline=True, knn_mode=knn_mode)
    eng.vocab_append(vocab, np.arange(1, vocab.shape[0] + 1, dtype=np.int32))
    d_desc = [torch.from_numpy(f).cuda() for f in frames]
    d_w = torch.zeros((T, q), dtype=torch.int32, device="cuda")
    d_l = torch.zeros((T, T + 8), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    seen = []
    for t in range(T):
        eng.frame_dev(d_desc[t].data_ptr(), q, t + 1, float(t + 1), d_w[t].data_ptr(), d_l[t].data_ptr(), T + 8, first_new_word_id=vocab.shape[0] + 1 + t * q)
        if one_at_a_time:
            seen.append(eng.stats()["knn_max_err_ratio"])
    if not one_at_a_time:
        seen.append(eng.stats()["knn_max_err_ratio"])
    words = d_w.cpu().numpy()
    eng.close()
    return seen, words


@pytest.mark.parametrize("knn_mode", MODES)
@pytest.mark.parametrize("q", [65, 129])
def test_error_ratio_maximum_of_a_stream_back_to_back_and_frame_by_frame(knn_mode, q):
    vocab, frames = _graded(64)
    together, w0 = _ratio_stream(knn_mode, vocab, frames[q], False)
    single, w1 = _ratio_stream(knn_mode, vocab, frames[q], True)
    print("knn_max_err_ratio frame by frame:", ["%.5f" % v for v in single], "back to back:", "%.5f" % together[0])
    np.testing.assert_array_equal(w0, w1)
    rises = sum(1 for a, b in zip(single[1:-1], single[2:]) if b > a)
    assert single[0] > 0.0 and rises >= 2, "the stream must raise the maximum at least twice after the first frame: %r" % (single,)
    assert all(b >= a for a, b in zip(single, single[1:])), "a running maximum went down: %r" % (single,)
    assert single[-1] < 0.5, "half of eps used up: the frames would go to the exact redo"
    assert _bits(together[0]) == _bits(single[-1])


@pytest.mark.parametrize("knn_mode", MODES)
def test_error_ratio_maximum_of_a_handle_of_128_float_rows(knn_mode):
    """wide_filter_body.cuh: the stand-alone search of a 128-float handle keeps ONE maximum"""
    import rtabmap_amd
    vocab, frames = _graded(128)
    out = {}
    for one_at_a_time in (False, True):
        eng = rtabmap_amd.Engine("f32", 128, knn_mode=knn_mode)
        eng.vocab_append(vocab, np.arange(1, vocab.shape[0] + 1, dtype=np.int32))
        seen, ids = [], []
        for f in frames[65]:
            ids.append(eng.knn2(f)[0])
            if one_at_a_time:
                seen.append(eng.stats()["knn_max_err_ratio"])
        if not one_at_a_time:
            seen.append(eng.stats()["knn_max_err_ratio"])
        eng.close()
        out[one_at_a_time] = (seen, ids)
    single, together = out[True][0], out[False][0]
    print("knn_max_err_ratio search by search:", ["%.5f" % v for v in single], "at the end:", "%.5f" % together[0])
    for a, b in zip(out[True][1], out[False][1]):
        np.testing.assert_array_equal(a, b)
    rises = sum(1 for a, b in zip(single[1:-1], single[2:]) if b > a)
    assert single[0] > 0.0 and rises >= 2, "the searches must raise the maximum at least twice after the first: %r" % (single,)
    assert all(b >= a for a, b in zip(single, single[1:])), "a running maximum went down: %r" % (single,)
    assert _bits(together[0]) == _bits(single[-1])


# ---------------------------------------------------------------------------------------------- the streams that append words
def _run(pipeline, knn_mode, base, frames):
    """the stream on one handle (words appended on the device and numbered there): word ids, first new id and rows per frame, every frame's 2-NN stage
    (pipelined: as launch B left it, with its rejected count; plain: final), the last frame's final 2-NN, the certificate's count of the last frame"""
    import rtabmap_amd
    n_words, T = base.shape[0], len(frames)
    qmax = max(f.shape[0] for f in frames)
    eng = rtabmap_amd.Engine("f32", 64, sig_capacity=T + 8, pipeline=pipeline, knn_mode=knn_mode)
    eng.vocab_append(base, np.arange(1, n_words + 1, dtype=np.int32))
    eng.set_option("next_word_id", n_words + 1)
    d_desc = [torch.from_numpy(f).cuda() for f in frames]
    d_w = torch.zeros((T, qmax), dtype=torch.int32, device="cuda")
    d_l = torch.zeros((T, T + 8), dtype=torch.float32, device="cuda")
    d_first = torch.zeros(T, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    stage, rejected = {}, {}
    for t, f in enumerate(frames):
        eng.frame_dev(d_desc[t].data_ptr(), f.shape[0], t + 1, float(t + 1), d_w[t].data_ptr(), d_l[t].data_ptr(), T + 8,
                      first_new_word_id=capi.LCD_NEW_WORD_IDS_AUTO, append_new_words=True, d_first_new_word_id_ptr=d_first[t:].data_ptr())
        of = t - 1 if pipeline else t                                  # (the frame whose 2-NN stage has run when the call returns)
        if of >= 0:
            stage[of], nq, rejected[of] = _frame_knn(eng, qmax)
            assert nq == frames[of].shape[0]
    eng.synchronize()
    final, nq, _ = _frame_knn(eng, qmax)
    assert nq == frames[-1].shape[0]
    st = eng.stats()
    rows, live = eng.vocab_count()
    words, first = d_w.cpu().numpy(), d_first.cpu().numpy()
    created = [len(set(w for w in words[t, : frames[t].shape[0]].tolist() if w < 0)) for t in range(T)]
    assert rows == live == n_words + sum(created)
    eng.close()
    return dict(words=words, first=first, created=created, rows=rows, stage=stage, rejected=rejected, final=final,
                fallback=st["knn_last_fallback_queries"])


def _same_knn(a, b, what):
    np.testing.assert_array_equal(a[0], b[0], err_msg=what + ": rows")
    np.testing.assert_array_equal(a[1], b[1], err_msg=what + ": words")
    np.testing.assert_array_equal(a[2].view(np.uint32), b[2].view(np.uint32), err_msg=what + ": distances")


def _both(knn_mode, base, frames):
    plain = _run(False, knn_mode, base, frames)
    piped = _run(True, knn_mode, base, frames)
    np.testing.assert_array_equal(piped["words"], plain["words"])
    np.testing.assert_array_equal(piped["first"], plain["first"])
    assert piped["rows"] == plain["rows"]
    for t in sorted(piped["stage"]):                                   # the re-rank's own output, frame by frame
        if piped["rejected"][t] == 0:
            _same_knn(piped["stage"][t], plain["stage"][t], "frame %d behind launch B" % t)
    _same_knn(piped["final"], plain["final"], "last frame, complete")
    return plain, piped


def _unit(x):
    return np.ascontiguousarray(x / np.linalg.norm(x, axis=1, keepdims=True), dtype=np.float32)


# ---------------------------------------------------------------------------------------------- 2. the running maximum of |row|^2
@pytest.mark.parametrize("knn_mode", MODES)
def test_a_query_next_to_an_appended_word_of_the_largest_norm(knn_mode):
    base = _base()
    rng = np.random.default_rng(51)
    q = 65
    big = 3.0 * synth.vocab_surf(12, seed=777)                         # |row|^2 = 9 against the vocabulary's 1: far from every row, words of their own
    frames = []
    for t in range(5):
        f = base[rng.integers(0, N_WORDS, q)] + rng.standard_normal((q, 64)).astype(np.float32) * np.float32(0.002)
        f = _unit(f)
        if t == 0:
            f[5:17] = big                                              # the frame that appends them
        else:
            f[20:32] = big * (1.0 + 0.001 * rng.standard_normal((12, 64))).astype(np.float32)   # queries next to them
        frames.append(np.ascontiguousarray(f, dtype=np.float32))
    plain, piped = _both(knn_mode, base, frames)
    assert plain["created"][0] == 12 and sum(plain["created"][1:]) == 0, plain["created"]
    ids = plain["words"][0, 5:17]
    assert (ids < 0).all()
    for t in range(1, 5):                                              # every later frame finds the twelve appended words
        assert sorted(plain["words"][t, 20:32].tolist()) == list(range(N_WORDS + 1, N_WORDS + 13)), plain["words"][t, 20:32]
    assert all(r == 0 for r in piped["rejected"].values()), piped["rejected"]
    assert plain["fallback"] == 0 and piped["fallback"] == 0


# ---------------------------------------------------------------------------------------------- 3. results, bit rows and lists
def _cluster_frames(base, q, n_frames, seed):
    """fresh descriptors in clusters of seven near-duplicates (each becomes ONE word through the candidate bits and lists: six set bits below the
    cluster's last descriptor, more than the list holds), the rest noisy copies of vocabulary rows and of earlier frames' descriptors"""
    rng = np.random.default_rng(seed)
    frames = []
    for t in range(n_frames):
        src = base if not frames or t % 2 == 0 else frames[-1]
        f = src[rng.integers(0, src.shape[0], q)] + rng.standard_normal((q, 64)).astype(np.float32) * np.float32(0.002)
        n_cl = q // 16
        centres = synth.vocab_surf(max(n_cl, 1), seed=int(rng.integers(1 << 30)))
        for c in range(n_cl):
            at = rng.permutation(q)[:7] if c == 0 else np.arange(16 * c, 16 * c + 7)
            f[at] = centres[c] + rng.standard_normal((7, 64)).astype(np.float32) * np.float32(0.001)
        frames.append(_unit(f))
    return frames


def _most_bits_below(base, f):
    """the largest number of earlier descriptors of the frame that lie closer to a descriptor than its second nearest vocabulary row"""
    d_v = ((f[:, None, :].astype(np.float64) - base[None, :, :]) ** 2).sum(-1)
    second = np.sort(d_v, axis=1)[:, 1]
    d_f = ((f[:, None, :].astype(np.float64) - f[None, :, :]) ** 2).sum(-1)
    below = np.tril(d_f < second[:, None] * 0.999, -1)
    return int(below.sum(1).max())


@pytest.mark.parametrize("knn_mode", MODES)
@pytest.mark.parametrize("q", [1, 2, 63, 64, 65, 129])
def test_results_bit_rows_and_lists_against_the_plain_handle(knn_mode, q):
    base = _base()
    frames = _cluster_frames(base, q, 5, seed=300 + q)
    if q >= 63:
        assert _most_bits_below(base, frames[0]) > 4, "a descriptor with more candidates below it than the list holds"
    plain, piped = _both(knn_mode, base, frames)
    if q >= 63:
        assert min(plain["created"]) >= q // 16 - 1, plain["created"]    # (the first cluster's places are drawn: the others may take some of them)
        # a cluster is ONE word: its seven descriptors carry the same code
        w = plain["words"][0, 16:23]
        assert len(set(w.tolist())) == 1 and w[0] < 0, w
