"""Plain Python / numpy model of Signature::compareTo's words branch (reference corelib/src/Signature.cpp:250-288) and of
Memory::computeLikelihood with Kp/TfIdfLikelihoodUsed=false (Memory.cpp:2179-2214): what lcd_similarity must reproduce bit for bit.

(i)  find_pairs_literal / compare_to_literal: the multimap walk of EpipolarGeometry::findPairs (EpipolarGeometry.h:123-151) and
     compareTo's words branch restated line by line; a std::multimap<int, int> is a list of (key, value) sorted by key, equal keys in
     insertion order.
(ii) pairs_closed_form / similarity_closed_form: sum over words w > 0 of min(cq(w), cs(w)), for large cases.
The float is np.float32(pairs) / np.float32(total) in both.

One departure is part of the contract (include/lcd.h): ids <= 0 are "no word".  The reference's findPairs would admit a key 0
("*i >= 0"); RTAB-Map never issues word id 0, and Signature counts ids <= 0 as invalid (Signature.cpp:341-344), so the literal walk
here skips ids <= 0."""
import numpy as np


# ---- (i) the literal restatement
def _multimap(word_ids):
    """Signature::_words as the sorted (key, value) list a std::multimap iterates: value = the feature's index"""
    return sorted(((int(w), k) for k, w in enumerate(word_ids)), key=lambda kv: kv[0])      # (stable: equal keys keep insertion order)


def _find(mm, key):
    """std::multimap::find: the position of the first element with that key, len(mm) (== end()) when there is none"""
    for i, kv in enumerate(mm):
        if kv[0] == key:
            return i
    return len(mm)


def find_pairs_literal(words_a, words_b):
    """EpipolarGeometry::findPairs(wordsA, wordsB, pairs): the list of (id, (valueA, valueB))"""
    ids = []
    for k, _ in words_a:                                   # uUniqueKeys(wordsA)
        if not ids or ids[-1] != k:
            ids.append(k)
    pairs = []
    for i in ids:
        if i > 0:                                          # ignoreNegativeIds (and id 0: see the module docstring)
            ia, ib = _find(words_a, i), _find(words_b, i)
            while ia != len(words_a) and ib != len(words_b) and words_a[ia][0] == words_b[ib][0] and words_a[ia][0] == i:
                pairs.append((i, (words_a[ia][1], words_b[ib][1])))
                ia += 1
                ib += 1
    return pairs


def _invalid_words_count(word_ids):
    return sum(1 for w in word_ids if int(w) <= 0)         # Signature::setWords counts ids <= 0 (Signature.cpp:341-344)


def compare_to_literal(this_ids, s_ids):
    """this->compareTo(s), words branch (Signature.cpp:273-286), for two signatures given by their word ids in feature order.
    Returns (similarity as np.float32, pairs, words.size() - invalidWordsCount of s)."""
    similarity = np.float32(0.0)
    this_words, words = _multimap(this_ids), _multimap(s_ids)
    this_valid = len(this_words) - _invalid_words_count(this_ids)
    s_valid = len(words) - _invalid_words_count(s_ids)
    n_pairs = 0
    if not (s_valid <= 0) and not (this_valid <= 0):       # !s.isBadSignature() && !this->isBadSignature()
        total_words = this_valid if this_valid > s_valid else s_valid
        assert total_words > 0
        pairs = find_pairs_literal(words, this_words)      # findPairs(words, _words, pairs)
        n_pairs = len(pairs)
        similarity = np.float32(n_pairs) / np.float32(total_words)
    return similarity, n_pairs, s_valid


# ---- (ii) the closed form
def _counts(word_ids):
    w = np.asarray(word_ids, np.int64).reshape(-1)
    u, c = np.unique(w[w > 0], return_counts=True)
    return u, c


def pairs_closed_form(q_ids, s_ids):
    uq, cq = _counts(q_ids)
    us, cs = _counts(s_ids)
    _, iq, i_s = np.intersect1d(uq, us, assume_unique=True, return_indices=True)
    return int(np.minimum(cq[iq], cs[i_s]).sum())


def similarity_closed_form(q_ids, sigs):
    """the query against a list of signatures: (sim float32[n], pairs int32[n], valid int32[n]); sigs[k] is None for an unknown / retired
    signature or an id <= 0 (everything 0)"""
    n = len(sigs)
    sim, pairs, valid = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    vq = int((np.asarray(q_ids, np.int64).reshape(-1) > 0).sum())
    uq, cq = _counts(q_ids)
    for k, s in enumerate(sigs):
        if s is None:
            continue
        us, cs = _counts(s)
        vs = int(cs.sum())
        valid[k] = vs
        if vq == 0 or vs == 0:
            continue
        _, iq, i_s = np.intersect1d(uq, us, assume_unique=True, return_indices=True)
        p = int(np.minimum(cq[iq], cs[i_s]).sum())
        pairs[k] = p
        sim[k] = np.float32(p) / np.float32(max(vq, vs))
    return sim, pairs, valid
