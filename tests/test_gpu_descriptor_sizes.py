"""GPU parity of the word-assignment path at every descriptor shape the engine picks different device code for (tests/helpers.py:
DESCRIPTOR_SHAPES) -- lcd_quantize, lcd_find_nn, lcd_frame_dev with update()'s append on the device, the enqueued clean, one rank of the
sharded frame and the host mirror, against the oracle's restated addNewWords / findNN / Memory::update.  Word ids are compared as
integers, vocabulary rows read back byte for byte, likelihoods within the project's 1e-4 / 1e-7.

The other GPU files follow this path at 64 floats (SURF) and 32 bytes (ORB) only; what the shapes here add:
  * the row writers for rows that are not 64 floats (append_new_rows in frame_tail_body.cuh behind lcd_frame_dev, shard_append_body in
    tfidf.hip behind lcd_shard_frame_dev): fewer dwords than the 16 lanes of a row (4, 6), exactly 16, and 32 / 64 / 128 dwords (2 / 4 / 8 trips).
    (The third copy, in append_rows_body, serves deferred appends, which only handles of 64-float rows have: no shape reaches it.)
  * knn2_merge_selfdist_hamming_kernel past the 512 descriptors whose distances it keeps in registers;
  * the candidate bit rows of selfdist_l2_kernel<128>, selfdist_l2_dyn_kernel and selfdist_hamming_dyn_kernel at ragged frame sizes;
  * launch_shard_merge followed by a distance launch that cannot carry the merge, and the merge in the head of selfdist_l2_kernel<128>;
  * the exact scans knn2_l2_kernel<128>, knn2_l2_dyn_kernel, knn2_hamming_kernel<4|16>, knn2_hamming_dyn_kernel under a frame: rows appended
    on the device, a row count the host only knows an upper bound of;
  * a handle created with pipeline = 1 that the matrix-core filter does not serve (it takes the plain path).
Every premise (words are created, a planted duplicate resolves to the word its same-frame original created) is asserted from the oracle's
answer before an engine exists."""
import numpy as np
import pytest
import torch

from helpers import DESCRIPTOR_SHAPES, noisy, queries_of, rows_of, shape_id
from test_gpu_append_dev import _oracle_stream, _stream
from test_gpu_frame_stream import ATOL, RTOL
from test_gpu_stream import _incremental_stream

pytestmark = pytest.mark.gpu

F128, F256, F6, U16, U64, U24, U61 = [s[:2] for s in DESCRIPTOR_SHAPES]
U32 = ("u8", 32)
UNPADDED = [F128, F256, F6, U16, U64, U24]


def _engine(shape, **kw):
    import rtabmap_amd
    return rtabmap_amd.Engine(shape[0], shape[1], **kw)


def _dictionary(oracle, vocab, ids, together=True):
    m = oracle.OracleVWDictionary(strategy=oracle.kNNBruteForce, nndr=0.8, new_words_compared_together=together)
    for i, r in zip(ids, vocab):
        m.add_word(int(i), r)
    m.update()
    return m


def _frame_dev_words(eng, desc, together=True):
    """lcd_frame_dev on a frame that is neither registered nor appended: the decision loop's codes, as lcd_quantize returns them"""
    q = desc.shape[0]
    d = torch.from_numpy(desc).cuda()
    d_words = torch.zeros(q, dtype=torch.int32, device="cuda")
    eng.frame_dev(d.data_ptr(), q, 0, 10.0, d_words.data_ptr(), 0, 0, incremental=True, new_words_compared=together, nndr=0.8)
    eng.synchronize()
    return d_words.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- a. quantise stream
def _quantize_stream_oracle(oracle, shape, together, n_frames=10, q=150, base_n=400):
    """tests/test_gpu_quantize.py's stream for any shape, the oracle's half: per frame (ids of the indexed rows, their descriptors, last word id,
    the frame, addNewWords' answer)."""
    base = rows_of(shape, base_n, seed=78)
    frames = [queries_of(shape, base, q, seed=200 + t, frac_known=0.8, sigma=0.03, flip=0.05) for t in range(n_frames)]
    m = oracle.OracleMemory(strategy=oracle.kNNBruteForce, nndr=0.8, new_words_compared_together=together)
    words, steps = {}, []
    for t, desc in enumerate(frames):
        unused = m.vwd.get_unused_word_ids()                    # what Memory::update does before addNewWords: cleanUnusedWords + update()
        if unused:
            m.vwd.remove_words(unused)
            for w in unused:
                words.pop(w)
        m.vwd.update()
        index_ids = np.array(m.vwd.index_ids(), np.int32)
        rows = np.stack([words[i] for i in index_ids]) if len(index_ids) else None
        last_id = m.vwd.last_word_id
        exp = m.vwd.add_new_words(desc, t + 1)
        steps.append((index_ids, rows, last_id, desc, exp))
        for i, w in enumerate(exp):
            if w > last_id and w not in words:
                words[w] = desc[i].copy()
        if t >= 3:                                              # forget an old frame: words become unused
            for w in m.vwd.word_ids():
                m.vwd.remove_all_word_ref(w, t - 2)
    return steps


def _joined_a_same_frame_word(exp, last_id):
    """descriptors that carry a word an EARLIER descriptor of the same frame created"""
    seen, n = set(), 0
    for w in exp:
        if w > last_id:
            n += w in seen
            seen.add(w)
    return n


@pytest.mark.parametrize("together", [True, False])
@pytest.mark.parametrize("shape", [s[:2] for s in DESCRIPTOR_SHAPES], ids=shape_id)
def test_quantize_stream_at_every_shape(oracle, shape, together):
    """Frame by frame: the engine's vocabulary is loaded with exactly the oracle's indexed rows (same order), then lcd_quantize must reproduce
    addNewWords() -- including the same-frame new-word dependency chain, which new_words_compared = 0 switches off in the reference too."""
    steps = _quantize_stream_oracle(oracle, shape, together)
    assert sum(len({w for w in exp if w > last}) for _, _, last, _, exp in steps) > 0
    assert steps[-1][0].shape[0] >= 2                           # (the later frames are searched against an index)
    joined = max(_joined_a_same_frame_word(exp, last) for _, _, last, _, exp in steps)
    assert (joined > 0) == together
    eng = _engine(shape)
    for t, (index_ids, rows, last_id, desc, exp) in enumerate(steps):
        eng.vocab_clear()
        if rows is not None:
            eng.vocab_append(rows, index_ids)
        got, n_new = eng.quantize(desc, incremental=True, new_words_compared=together, nndr=0.8)
        assert np.where(got < 0, last_id - got, got).tolist() == exp, "frame %d" % t      # -(k+1) -> last_id + k + 1
        assert n_new == len({e for e in exp if e > last_id})
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- b. device frames with the append
@pytest.mark.parametrize("auto_ids", [False, True], ids=["ids-given", "ids-auto"])
@pytest.mark.parametrize("shape", UNPADDED, ids=shape_id)
def test_append_on_the_device_at_every_row_size(oracle, shape, auto_ids):
    """lcd_frame_dev with append_new_words, frames enqueued back to back: the decision loop's workgroup writes the rows (append_new_rows,
    16 lanes per row, a dword each per trip) -- the rows read back are update()'s, in id order, byte for byte, findable at distance 0, and
    the next frames' exact scans find them (the host plans them for an upper bound of the row count)."""
    assert _stream(oracle, False, n_words=800, q=96, n_frames=8, seed=211, shape=shape, auto_ids=auto_ids, min_words_in_a_frame=8) > 0


@pytest.mark.parametrize("shape", [F128, U64], ids=shape_id)
def test_append_on_the_device_with_the_clean_enqueued(oracle, shape):
    """cleanUnusedWords enqueued behind every frame of a stream in which no word is ever unused: it removes nothing"""
    assert _stream(oracle, False, n_words=800, q=96, n_frames=8, seed=223, shape=shape, clean_every_frame=True, min_words_in_a_frame=8) > 0


def test_a_pipelined_handle_of_128_floats_takes_the_plain_path(oracle):
    """lcd_config.pipeline on a handle the matrix-core filter does not serve: every frame goes the plain way, same results"""
    assert _stream(oracle, True, n_words=800, q=96, n_frames=8, seed=211, shape=F128, min_words_in_a_frame=8) > 0


def _shard_append_stream(oracle, shape, n_words=600, q=96, n_frames=5, seed=307):
    """One rank of the sharded frame with "shard_append": the words a frame creates become rows of the rank's shard inside
    lcd_shard_frame_dev (shard_append_body: its own copy of the row writer).  Word ids, likelihood and the rows read back are
    Memory::update's."""
    base, ids, words, frames, first_new, expected, likes = _oracle_stream(oracle, n_words, q, n_frames, seed, shape=shape)
    n_bulk = words.shape[0]
    created = [len({w for w in exp if w >= first}) for exp, first in zip(expected, first_new)]
    assert min(created[:-1]) >= 8                               # every frame appends; the later ones are searched over appended rows
    assert any(first_new[0] <= w < first_new[t] for t in range(1, n_frames) for w in expected[t])     # ... and match them
    cap = n_bulk + n_frames + 8
    eng = _engine(shape, sig_capacity=cap)
    eng.set_option("shard_append", 1)
    eng.vocab_append(base, ids)
    eng.sig_add_bulk(np.arange(1, n_bulk + 1, dtype=np.int32), np.arange(0, (n_bulk + 1) * q, q, dtype=np.int64), words.reshape(-1))
    d_cand = torch.zeros(q * 2 * 16, dtype=torch.uint8, device="cuda")
    d_words = torch.zeros(q, dtype=torch.int32, device="cuda")
    d_lfix = torch.zeros(cap, dtype=torch.int64, device="cuda")
    d_like = torch.zeros(cap, dtype=torch.float32, device="cuda")
    by_id, total = {}, n_words
    for t in range(n_frames):
        d = torch.from_numpy(frames[t]).cuda()
        sid = n_bulk + 1 + t
        eng.shard_knn2_dev(d.data_ptr(), q, d_cand.data_ptr())
        eng.shard_frame_dev(d.data_ptr(), q, sid, float(sid), 0, 1, d_cand.data_ptr(), total, d_words.data_ptr(), d_lfix.data_ptr(), cap,
                            incremental=True, new_words_compared=True, nndr=0.8, first_new_word_id=first_new[t])
        eng.finalize_dev(d_lfix.data_ptr(), sid, d_like.data_ptr())
        eng.synchronize()
        got = d_words.cpu().numpy()
        assert np.where(got < 0, first_new[t] - got - 1, got).tolist() == expected[t], "frame %d" % t
        np.testing.assert_allclose(d_like[:sid].cpu().numpy(), likes[t], rtol=RTOL, atol=ATOL, err_msg="frame %d" % t)
        for i, w in enumerate(got.tolist()):
            if w < 0:
                by_id.setdefault(first_new[t] - w - 1, frames[t][i])
        total = n_words + len(by_id)
    rows, live = eng.vocab_count()
    assert rows == live == total
    vr, vi = eng.vocab_read(n_words, total - n_words)
    assert vi.tolist() == sorted(by_id)
    np.testing.assert_array_equal(vr, np.stack([by_id[i] for i in vi.tolist()]))
    kid, kd = eng.knn2(vr[::7])
    assert kid[:, 0].tolist() == vi[::7].tolist() and not kd[:, 0].any()
    eng.close()


@pytest.mark.parametrize("shape", UNPADDED, ids=shape_id)
def test_shard_append_at_every_row_size(oracle, shape):
    _shard_append_stream(oracle, shape)


# ---------------------------------------------------------------------------------------------------------------- c. Hamming frames beyond 512 descriptors
def _planted_hamming_frame(shape, vocab, q, seed):
    """q descriptors (60 % noisy copies of vocabulary rows, the others unseen) with planted pairs (i, j), j < i: descriptor j is unseen, descriptor i
    is j with 0..2 bits flipped.  20 pairs behind descriptor 511 where the frame has room for them, pairs that straddle 511 / 512, pairs in the
    register blocks' last column block (448..511), and one whose i lies in the frame's last 64-column block."""
    rng = np.random.default_rng(seed)
    desc = queries_of(shape, vocab, q, seed=seed + 1, frac_known=0.6, flip=0.05)
    free = list(range(512, q))
    rng.shuffle(free)
    pairs = []
    while len(free) >= 2 and len(pairs) < 20:                   # 512 <= j < i
        a, b = free.pop(), free.pop()
        pairs.append((max(a, b), min(a, b)))
    used = {x for p in pairs for x in p}
    for j, i in ((511, 512), (509, 515), (500, 640), (3, q - 1), (450, 470), (448, 511), (64 * ((q - 1) // 64), q - 1)):
        if j < i < q and i not in used and j not in used:
            pairs.append((i, j))
            used.update((i, j))
    for k, (i, j) in enumerate(pairs):
        desc[j] = rng.integers(0, 256, shape[1], dtype=np.uint8)
        desc[i] = desc[j]
        for b in rng.choice(shape[1] * 8, k % 3, replace=False):
            desc[i, b >> 3] ^= np.uint8(1 << (b & 7))
    return desc, pairs


@pytest.mark.parametrize("q", [512, 513, 577, 1100])
@pytest.mark.parametrize("shape", [U32, U64], ids=shape_id)
def test_hamming_frames_beyond_512_descriptors(oracle, shape, q):
    """knn2_merge_selfdist_hamming_kernel keeps a query's distances to the frame's first 512 descriptors in registers and computes the others in
    its second loop; a descriptor behind the 512th can only join the word a same-frame descriptor behind the 512th created through those
    distances and the ballots that make its bit row."""
    n = 1500
    vocab = rows_of(shape, n, seed=401)
    ids = np.arange(1, n + 1, dtype=np.int32)
    desc, pairs = _planted_hamming_frame(shape, vocab, q, seed=410 + q)
    exp = _dictionary(oracle, vocab, ids).add_new_words(desc, 1)
    assert len([1 for i, j in pairs if j >= 512]) >= (20 if q >= 552 else 0) and (q < 513 or any(j < 512 <= i for i, j in pairs))
    assert q % 64 == 0 or any(i // 64 == (q - 1) // 64 for i, j in pairs)
    for i, j in pairs:                                          # the premise: j created a word, i carries it
        assert exp[j] > n and exp.index(exp[j]) == j and exp[i] == exp[j], (i, j)
    eng = _engine(shape, sig_capacity=8)
    eng.vocab_append(vocab, ids)
    got, n_new = eng.quantize(desc, incremental=True, new_words_compared=True, nndr=0.8)
    assert np.where(got < 0, n - got, got).tolist() == exp
    assert n_new == len({e for e in exp if e > n})
    assert _frame_dev_words(eng, desc).tolist() == got.tolist()
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- d. bit rows at ragged frame sizes
def _ragged_frame(shape, vocab, q, seed):
    """q descriptors, half of them unseen, with same-frame near-duplicates (i of j, j < i, j unseen): both in the frame's last partial group of 8
    rows, both in its last partial block of 64 columns, and one for every position j % 8 of a row in its group (a bit each of a bit row's byte)."""
    rng = np.random.default_rng(seed)
    desc = queries_of(shape, vocab, q, seed=seed + 1, frac_known=0.5) if vocab.shape[0] else rows_of(shape, q, seed + 1)
    pairs, used = [], set()

    def plant(j, i):                                            # a pair whose places are free and in the frame; otherwise nothing
        if 0 <= j < i < q and i not in used and j not in used:
            pairs.append((i, j))
            used.update((i, j))
    # the frame's last row q - 1 with the first row of its group of 8 (q = 7: (0, 6), q = 150: (144, 149)); where q - 1 opens its group (q = 33, 65)
    # with a row of the group before, so that the last row group and the last column block always take part
    plant(8 * ((q - 1) // 8), q - 1)
    plant(q - 9, q - 1)
    plant(64 * ((q - 1) // 64), q - 2)                          # both in the last block of 64 columns (q = 150: (128, 148); q = 33: (0, 31))
    for k in range(8):                                          # every position j % 8 of a row in its group: the first free such j with the last free i
        plant(next((j for j in range(k, q, 8) if j not in used), -1), next((i for i in range(q - 1, -1, -1) if i not in used), -1))
    for k in range(8):                                          # frames of 33 descriptors and more: pairs nine rows apart near the end (adjacent row groups)
        plant(q - 20 + k, q - 11 + k)
    fresh = rows_of(shape, len(pairs) + 1, seed + 2)
    for k, (i, j) in enumerate(pairs):
        desc[j] = fresh[k]
        desc[i:i + 1] = noisy(desc[j:j + 1], rng, sigma=0.004, flip=0.006) if k % 2 else desc[j:j + 1]
    return desc, pairs


@pytest.mark.parametrize("n_index", [0, 1, 300])
@pytest.mark.parametrize("shape", [F128, F256, U24], ids=shape_id)
def test_bit_rows_at_ragged_frame_sizes(oracle, shape, n_index):
    """The candidate bit rows of selfdist_l2_kernel<128> and selfdist_l2_dyn_kernel, and of the merged Hamming kernel at six dwords per row
    (lcd_quantize and lcd_frame_dev), decide which same-frame word a descriptor joins.  Frames of 1, 7, 33, 65 and 150 descriptors over
    an empty index, one word (no indexed search either, VWDictionary.cpp:1015: every threshold is +inf) and 300 words."""
    vocab = rows_of(shape, n_index, seed=501) if n_index else np.zeros((0, shape[1]), np.float32 if shape[0] == "f32" else np.uint8)
    ids = np.arange(1, n_index + 1, dtype=np.int32)
    cases = []
    for q in (1, 7, 33, 65, 150):
        desc, pairs = _ragged_frame(shape, vocab, q, seed=710 + q)
        exp = _dictionary(oracle, vocab, ids).add_new_words(desc, 1)
        for i, j in pairs:
            assert exp[j] > n_index and exp.index(exp[j]) == j and exp[i] == exp[j], (q, i, j)
        assert q < 2 or any(i == q - 1 for i, j in pairs)       # the frame's last row group and column block take part
        assert q < 33 or {j % 8 for i, j in pairs} == set(range(8))
        cases.append((q, desc, exp))
    eng = _engine(shape, sig_capacity=8)
    if n_index:
        eng.vocab_append(vocab, ids)
    for q, desc, exp in cases:
        got, n_new = eng.quantize(desc, incremental=True, new_words_compared=True, nndr=0.8)
        assert np.where(got < 0, n_index - got, got).tolist() == exp, "q = %d" % q
        assert n_new == len({e for e in exp if e > n_index})
        assert _frame_dev_words(eng, desc).tolist() == got.tolist(), "q = %d" % q
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- e. lcd_find_nn with not-yet-indexed words
@pytest.mark.parametrize("n_extra", [1, 40])
@pytest.mark.parametrize("shape", [F128, U61], ids=shape_id)
def test_find_nn_with_words_that_are_not_indexed_yet(oracle, shape, n_extra):
    v = rows_of(shape, 1200, seed=601)
    q = queries_of(shape, v, 120, seed=602, frac_known=0.8, sigma=0.02, flip=0.03)
    extra = rows_of(shape, n_extra, seed=603)
    q[:n_extra] = extra                                         # some queries ARE not-yet-indexed words
    q[n_extra:2 * n_extra] = noisy(extra, np.random.default_rng(604), sigma=0.01, flip=0.01)      # ... or lie next to one
    ids = np.arange(1, 1201, dtype=np.int32)
    extra_ids = np.arange(5001, 5001 + n_extra, dtype=np.int32)
    m = _dictionary(oracle, v, ids)
    for i, r in zip(extra_ids, extra):
        m.add_word(int(i), r)                                   # stays in _notIndexedWords
    exp = m.find_nn(q)
    assert exp[:n_extra] == extra_ids.tolist() and set(exp[n_extra:2 * n_extra]) & set(extra_ids.tolist())
    eng = _engine(shape)
    eng.vocab_append(v, ids)
    assert eng.find_nn(q, extra, extra_ids, incremental=True, nndr=0.8).tolist() == exp
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- f. one rank of the sharded frame
@pytest.mark.parametrize("compared", [True, False], ids=["compared", "not-compared"])
@pytest.mark.parametrize("shape", [F128, F256, U32], ids=shape_id)
def test_one_rank_of_the_sharded_frame(oracle, shape, compared):
    """One rank, its own records as the gathered ones.  128 floats: the merge rides in the head of selfdist_l2_kernel<128>; 256 floats and 32
    bytes: launch_shard_merge, then the dynamic distance kernels make the bit rows from the merged neighbours; frames that do not compare their
    new words: launch_shard_merge alone.  Three frames that are not registered: the word assignment is lcd_quantize's on an unsharded handle
    with the same rows -- and the oracle's; a descriptor that equals three identical vocabulary rows tells the merge's first slot from its
    second (the lowest row wins the tie).  Then one frame that is registered: its references go through the postings keys the merge hands
    on, so its likelihood must be Memory::computeLikelihood's."""
    from rtabmap_amd import synth
    n, q = 1500, 160
    v = rows_of(shape, n, seed=701)
    v[[900, 1200]] = v[77]                                       # three identical rows
    ids = np.arange(1, n + 1, dtype=np.int32)
    rng = np.random.default_rng(702)
    frames = []
    for t in range(3):
        x = queries_of(shape, v, q, seed=710 + t, frac_known=0.6)
        x[5] = v[77]
        x[60] = rows_of(shape, 1, seed=720 + t)
        x[120:124] = x[60]                                      # same-frame duplicates of an unseen descriptor: the bit rows decide
        x[150:153] = noisy(x[31:34], rng, sigma=0.004, flip=0.006)
        frames.append((x, _dictionary(oracle, v, ids, together=compared).add_new_words(x, 1)))
    assert all(len({w for w in exp if w > n}) >= 8 for _, exp in frames)
    assert all(exp[5] == 78 for _, exp in frames)
    assert all(exp[60] > n and (len({exp[k] for k in (60, 120, 121, 122, 123)}) == 1) == compared for _, exp in frames)
    # the registered frame: a memory whose signatures reference every word (cleanUnusedWords drops none), Memory::update on frame 0's descriptors
    n_bulk = (n + q - 1) // q + 2
    words = synth.zipf_words(n_bulk, q, n, seed=703)
    words.reshape(-1)[-n:] = ids
    m = oracle.OracleMemory(strategy=oracle.kNNBruteForce, nndr=0.8, new_words_compared_together=compared)
    for i, r in zip(ids, v):
        m.vwd.add_word(int(i), r)
    m.vwd.update()
    for s in range(n_bulk):
        m.add_signature(words[s])
    sid, exp_reg = m.update(frames[0][0])
    assert sid == n_bulk + 1 and exp_reg == frames[0][1] and sum(w <= n for w in exp_reg) >= 40
    like_reg = m.compute_likelihood(np.array(exp_reg, np.int32), np.array(m.signature_ids(), np.int32))[1]
    assert (like_reg[:-1] > 0).sum() >= n_bulk // 2
    cap = n_bulk + 8
    plain, shard = _engine(shape, sig_capacity=cap), _engine(shape, sig_capacity=cap)
    for e in (plain, shard):
        e.vocab_append(v, ids)
    shard.sig_add_bulk(np.arange(1, n_bulk + 1, dtype=np.int32), np.arange(0, (n_bulk + 1) * q, q, dtype=np.int64), words.reshape(-1))
    d_cand = torch.zeros(q * 2 * 16, dtype=torch.uint8, device="cuda")
    d_words = torch.zeros(q, dtype=torch.int32, device="cuda")
    for t, (x, exp) in enumerate(frames):
        ref, _ = plain.quantize(x, incremental=True, new_words_compared=compared, nndr=0.8)
        assert np.where(ref < 0, n - ref, ref).tolist() == exp, "frame %d" % t
        d = torch.from_numpy(x).cuda()
        shard.shard_knn2_dev(d.data_ptr(), q, d_cand.data_ptr())
        shard.shard_frame_dev(d.data_ptr(), q, 0, 10.0, 0, 1, d_cand.data_ptr(), n, d_words.data_ptr(), 0, 0,
                              incremental=True, new_words_compared=compared, nndr=0.8)
        torch.cuda.synchronize()
        assert d_words.cpu().numpy().tolist() == ref.tolist(), "frame %d" % t
    d = torch.from_numpy(frames[0][0]).cuda()
    d_lfix = torch.zeros(cap, dtype=torch.int64, device="cuda")
    d_like = torch.zeros(cap, dtype=torch.float32, device="cuda")
    shard.shard_knn2_dev(d.data_ptr(), q, d_cand.data_ptr())
    shard.shard_frame_dev(d.data_ptr(), q, sid, float(sid), 0, 1, d_cand.data_ptr(), n, d_words.data_ptr(), d_lfix.data_ptr(), cap,
                          incremental=True, new_words_compared=compared, nndr=0.8, first_new_word_id=n + 1)
    shard.finalize_dev(d_lfix.data_ptr(), sid, d_like.data_ptr())
    shard.synchronize()
    got = d_words.cpu().numpy()
    assert np.where(got < 0, n - got, got).tolist() == exp_reg
    np.testing.assert_allclose(d_like[:sid].cpu().numpy(), like_reg, rtol=RTOL, atol=ATOL)
    plain.close()
    shard.close()


# ---------------------------------------------------------------------------------------------------------------- g. exact scan at edge sizes
@pytest.mark.parametrize("shape,sizes", [(F128, [(1, 1), (3, 63), (33, 65), (257, 513), (1025, 63), (6145, 65)]),
                                         (F6, [(2, 1), (31, 65), (255, 63), (257, 513), (1025, 65), (6145, 513)])], ids=["f32x128", "f32x6"])
def test_exact_float_scan_at_edge_sizes(oracle, shape, sizes):
    """knn2_l2_kernel<128> and knn2_l2_dyn_kernel (6 floats: rows that are not 16-byte aligned, l2_ref_dyn's scalar tail) around the tile,
    workgroup and query-block boundaries, with duplicate rows (ties go to the lower row) and tombstones: ids and distances bit for bit."""
    rng = np.random.default_rng(801)
    for n, q in sizes:
        v = rows_of(shape, n, seed=810 + n)
        qs = queries_of(shape, v, q, seed=820 + q, frac_known=0.6)
        if n > 8:                                               # duplicates
            v[rng.integers(0, n, 4)] = v[rng.integers(0, n)]
            qs[rng.integers(0, q)] = v[rng.integers(0, n)]
        ids = rng.permutation(np.arange(1, n + 1)).astype(np.int32)
        eng = _engine(shape)
        eng.vocab_append(v, ids)
        removed = None
        if n > 2:                                               # tombstones
            dead = rng.choice(n, size=max(1, n // 5), replace=False)
            eng.vocab_remove(ids[dead])
            removed = np.zeros(n, np.uint8)
            removed[dead] = 1
        got_ids, got_d = eng.knn2(qs)
        idx, d = oracle.knn2_linear(v, qs, removed=removed)
        exp_ids = np.where(idx >= 0, ids[np.maximum(idx, 0)], 0).astype(np.int32)
        np.testing.assert_array_equal(got_ids, exp_ids, err_msg="n=%d q=%d" % (n, q))
        np.testing.assert_array_equal(got_d, d, err_msg="n=%d q=%d" % (n, q))
        eng.close()


# ---------------------------------------------------------------------------------------------------------------- h. host mirror
@pytest.mark.parametrize("shape", [F128, U61], ids=shape_id)
def test_host_mirror_stream(oracle, shape):
    """MemoryHip over ten frames: 128 floats take lcd_frame_host with the device append; 61 bytes are stored padded, lcd_frame_host answers
    LCD_ERR_UNSUPPORTED and VWDictionaryHip falls back to the call-by-call path -- the same word ids, bookkeeping and likelihood either way."""
    base = rows_of(shape, 500, seed=78)
    frames = [queries_of(shape, base, 160, seed=200 + t, frac_known=0.8, sigma=0.03, flip=0.05) for t in range(10)]
    _incremental_stream(oracle, frames, together=True, device_frames=True, fast_path=shape != U61)
