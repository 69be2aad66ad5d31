"""Shared test helpers (numpy restatements of the reference's MATLAB model used to pin the oracle)."""
import numpy as np


def update_common_signature(mem, dic):
    """archive/2010-LoopClosure/Bayes/updateCommonSignature.m + updateDictionary.m on zero-padded int matrices.

    mem: [n_sig, 1+W] rows (id, words.., 0 pad);  dic: [n_words, 1+R] rows (word id, referencing signature ids.., 0 pad).
    Returns (new virtual-place row, updated dictionary).
    """
    mem = mem.copy()
    dic = dic.copy()
    cs_id = int(mem[0, 0])
    cs = [cs_id]
    # clear references to the virtual place
    for w in mem[0, 1:]:
        idx = np.nonzero(dic[:, 0] == w)[0]
        if w != 0 and idx.size:
            row = dic[idx[0]]
            row[1:][row[1:] == cs_id] = 0
    nb_common = 0
    mem_size = mem.shape[0] - 1
    if mem_size > 0:
        total_active = int(np.count_nonzero(dic[:, 1:]))
        nb_common = total_active // mem_size
    if nb_common > 0:
        counts = np.count_nonzero(dic[:, 1:], axis=1)
        order = np.lexsort((dic[:, 0], counts))          # sortrows([count id])
        lst = np.stack([counts[order], dic[order, 0]], axis=1)
        added = 0
        for i in range(lst.shape[0] - 1, -1, -1):
            if i != lst.shape[0] - 1 and len(cs) > 1:
                ratio = int(lst[i + 1, 0] // lst[i, 0]) if lst[i, 0] else 0
                ln = len(cs)
                stop = False
                for _ in range(2, ratio + 1):
                    for k in range(1, ln):
                        cs.append(cs[k])
                        added += 1
                        if added >= nb_common:
                            break
                    if added >= nb_common:
                        stop = True
                        break
                del stop
            if added < nb_common:
                cs.append(int(lst[i, 1]))
                added += 1
            if added >= nb_common:
                break
        row = np.zeros(mem.shape[1], mem.dtype)
        row[:len(cs)] = cs
        # updateDictionary: first zero slot (or a new column) of each word's row gets the signature id
        for w in cs[1:]:
            if w == 0:
                continue
            idx = np.nonzero(dic[:, 0] == w)[0]
            if not idx.size:
                new = np.zeros((1, dic.shape[1]), dic.dtype)
                new[0, 0] = w
                new[0, 1] = cs_id
                dic = np.vstack([dic, new])
            else:
                r = idx[0]
                zeros = np.nonzero(dic[r] == 0)[0]
                if zeros.size == 0:
                    dic = np.hstack([dic, np.zeros((dic.shape[0], 1), dic.dtype)])
                    dic[r, -1] = cs_id
                else:
                    dic[r, zeros[0]] = cs_id
        return row, dic
    row = np.zeros(mem.shape[1], mem.dtype)
    row[0] = cs_id
    return row, dic


def matlab_compute_likelihood(sign, mem, dic):
    """archive/2010-LoopClosure/Bayes/computeLikelihood.m in float64 (MATLAB doubles)."""
    L = np.zeros(mem.shape[0])
    N = mem.shape[0]
    for w in np.unique(sign[1:]):
        if w == 0:
            continue
        r = np.nonzero(dic[:, 0] == w)[0][0]
        refs = np.unique(dic[r, 1:])
        refs = refs[refs != 0]
        nw = len(refs)
        lg = np.log10(N / nw)
        if lg != 0:
            for s in refs:
                pos = np.nonzero(mem[:, 0] == s)[0][0]
                row = mem[pos]
                nwi = np.count_nonzero(row[1:] == w)
                ni = np.count_nonzero(row[1:] > 0)
                if ni:
                    L[pos] += (nwi * lg) / ni
    return L


# ---- planted signatures for the inverted index's encoding limits (tests/test_gpu_index_limits.py)

def spread_slots(n_post, key, n_slots=256):
    """n_post distinct slot numbers in [0, n_slots) picked by `key` (an odd stride over the bucket: distinct while n_post <= n_slots)."""
    start = (int(key) * 53) % n_slots
    step = 2 * (int(key) % 61) + 1
    return (start + step * np.arange(n_post)) % n_slots


def signatures_from_postings(postings, n_slots=256):
    """postings: iterable of (word id, slot, count).  Returns n_slots int32 word lists (a word repeated `count` times), ascending word ids."""
    per = [[] for _ in range(n_slots)]
    for w, s, c in postings:
        per[int(s)].extend([int(w)] * int(c))
    return [np.array(sorted(p), np.int32) for p in per]


def tfidf_f64(sigs, query, live=None):
    """Memory::computeLikelihood's TF-IDF sum in float64 over plain word lists (ids <= 0 count in ni only, ni = len).
    Returns (L[len(sigs)], (sig index, word id, term) of every posting of a query word).  The host-side yardstick the
    sensitivity guards edit; the parity checks themselves use the C++ oracle."""
    n = len(sigs)
    live = np.ones(n, bool) if live is None else np.asarray(live, bool)
    q = np.unique(np.asarray(query, np.int64))
    q = q[q > 0]
    ni = np.array([len(s) for s in sigs], np.float64)
    L = np.zeros(n)
    if n == 0 or q.size == 0:
        return L, (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0))
    rows = np.repeat(np.arange(n, dtype=np.int64), [len(s) for s in sigs])
    words = np.concatenate([np.asarray(s, np.int64) for s in sigs]) if n else np.zeros(0, np.int64)
    m = np.isin(words, q) & live[rows]
    uk, cnt = np.unique(rows[m] * (1 << 32) + words[m], return_counts=True)
    s, w = uk >> 32, uk & 0xFFFFFFFF
    _, inv, nw = np.unique(w, return_inverse=True, return_counts=True)
    term = cnt * np.log10(float(live.sum()) / nw[inv]) / ni[s]
    np.add.at(L, s, term)
    return L, (s, w, term)


def max_rel_change(base, edited):
    """Largest relative move of a score between two float64 score vectors (scores that are 0 in both do not count)."""
    base, edited = np.asarray(base, np.float64), np.asarray(edited, np.float64)
    d = np.abs(edited - base)
    ref = np.maximum(np.abs(base), np.abs(edited))
    ok = ref > 0
    return float((d[ok] / ref[ok]).max()) if ok.any() else 0.0


def min_word_visibility(sigs, query, live=None):
    """min over the query's words (those with a nonzero term) of max over signatures of term(w, s) / L(s): dropping the postings of
    ANY one of these words moves at least one score by this much, relative."""
    L, (s, w, term) = tfidf_f64(sigs, query, live)
    keep = term != 0
    s, w, term = s[keep], w[keep], term[keep]
    rel = term / L[s]
    uw, inv = np.unique(w, return_inverse=True)
    best = np.zeros(uw.size)
    np.maximum.at(best, inv, rel)
    return float(best.min()) if best.size else 0.0


# ---- descriptor shapes the engine picks different device code for (tests/test_gpu_descriptor_sizes.py)

# (dtype, dim, the detector it stands for).  What each one selects: f32 x 128 the fixed-DIM float kernels and a row writer that makes 8 trips;
# f32 x 256 the dynamic float kernels, 16 trips; f32 x 6 rows that are not 16-byte aligned, l2_ref_dyn's scalar tail, 6 dwords per row (10 of a
# row's 16 lanes idle); u8 x 16 knn2_hamming_kernel<4>, 4 dwords; u8 x 64 knn2_hamming_kernel<16>, exactly one trip; u8 x 24 w32 == 6: the
# dynamic Hamming scan; u8 x 61 rows padded to 64 bytes on the device
DESCRIPTOR_SHAPES = [
    ("f32", 128, "SIFT, extended SURF / KAZE"),
    ("f32", 256, "SuperPoint"),
    ("f32", 6, "no detector"),
    ("u8", 16, "BRIEF-16"),
    ("u8", 64, "BRISK, FREAK"),
    ("u8", 24, "no detector"),
    ("u8", 61, "AKAZE MLDB"),
]


def shape_id(shape):
    return "%sx%d" % (shape[0], shape[1])


def unit_rows(n, dim, seed):
    """n unit-norm Gaussian float32 rows of ANY dimension (synth.vocab_surf shapes its rows in groups of four floats)."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, dim)).astype(np.float32)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return np.ascontiguousarray(v, dtype=np.float32)


def rows_of(shape, n, seed):
    """n fresh descriptors of a shape: unit-norm floats or uniform random bytes."""
    if shape[0] == "f32":
        return unit_rows(n, shape[1], seed)
    return np.random.default_rng(seed).integers(0, 256, (n, shape[1]), dtype=np.uint8)


def noisy(rows, rng, sigma=0.02, flip=0.02):
    """Copies of `rows` a detector would produce at the same place again: Gaussian noise of `sigma` per component and renormalised (float), or
    each bit flipped with probability `flip` (binary)."""
    out = rows.copy()
    if rows.dtype == np.uint8:
        out ^= np.packbits(rng.random((rows.shape[0], rows.shape[1] * 8)) < flip, axis=1)
        return np.ascontiguousarray(out)
    out += rng.standard_normal(out.shape).astype(np.float32) * np.float32(sigma)
    out /= np.linalg.norm(out, axis=1, keepdims=True)
    return np.ascontiguousarray(out, dtype=np.float32)


def queries_of(shape, vocab, q, seed, frac_known=0.8, sigma=0.03, flip=0.05):
    """q descriptors: `frac_known` of them noisy copies of vocabulary rows (NNDR accepts), the others fresh (would-be new words) -- what
    synth.queries_surf / queries_orb give at 64 floats / any byte count, for every shape."""
    rng = np.random.default_rng(seed)
    out = rows_of(shape, q, seed + 7919)
    known = rng.random(q) < frac_known
    src = rng.integers(0, vocab.shape[0], q)
    out[known] = noisy(vocab[src[known]], rng, sigma, flip)
    return np.ascontiguousarray(out)
