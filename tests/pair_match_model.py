"""NumPy / oracle models of the two matchers of lcd_match_pairs (include/lcd.h), test infrastructure only.

cross_check():      the engine's cross-check rule over a distance matrix D[to-row][from-row] (oracle.dist_matrix(to, from) has the engine's bits).
mutual_nn():        symmetric mutual nearest neighbours -- NOT the rule; here so that a test can show where the two differ.
dictionary_pair():  the temporary two-frame dictionary as the three-call sequence over oracle.OracleVWDictionary.
"""
import numpy as np


def cross_check(D):
    """nn(i) = argmin_j D[i][j] (lowest j on ties); back(j) = the i with the smallest D[i][j] among the to-rows with nn(i) == j (lowest i on
    ties); match[i] = nn(i) if back(nn(i)) == i else -1; dist[i] = D[i][nn(i)] kept or not, -1 when there is no from-row."""
    D = np.asarray(D, np.float32)
    nt, nf = D.shape
    match = np.full(nt, -1, np.int32)
    dist = np.full(nt, -1.0, np.float32)
    if nt == 0 or nf == 0:
        return match, dist
    nn = D.argmin(axis=1)                                   # first minimum: the lowest j
    dist = D[np.arange(nt), nn].astype(np.float32)
    for j in np.unique(nn):
        chose = np.flatnonzero(nn == j)                     # ascending i
        match[chose[np.argmin(D[chose, j])]] = j            # first minimum: the lowest i
    return match, dist


def mutual_nn(D):
    """match[i] = nn(i) if the nearest to-row of from-row nn(i) (over ALL to-rows, lowest i on ties) is i, else -1"""
    D = np.asarray(D, np.float32)
    nt, nf = D.shape
    match = np.full(nt, -1, np.int32)
    if nt == 0 or nf == 0:
        return match
    nn = D.argmin(axis=1)
    back = D.argmin(axis=0)
    keep = back[nn] == np.arange(nt)
    match[keep] = nn[keep]
    return match


def tie_resolved_by_index(D):
    """True when some to-row has two from-rows at its minimum distance, or some chosen from-row has two choosers at the same distance"""
    D = np.asarray(D, np.float32)
    nt, nf = D.shape
    if nt == 0 or nf == 0:
        return False
    nn = D.argmin(axis=1)
    d = D[np.arange(nt), nn]
    if ((D == d[:, None]).sum(axis=1) > 1).any():
        return True
    for j in np.unique(nn):
        c = d[nn == j]
        if (c == c.min()).sum() > 1:
            return True
    return False


def dictionary_pair(oracle, frm, to, nndr=0.8, new_words_compared=True, from_word_ids=None):
    """RegistrationVis.cpp:1482-1503 over the restated VWDictionary: addNewWords(from, 1) [or addWord(id, row) per row] -> update() ->
    addNewWords(to, 2).  Returns (from ids, to ids) as int32 arrays."""
    o = oracle.OracleVWDictionary(strategy=oracle.kNNBruteForce, nndr=nndr, new_words_compared_together=new_words_compared)
    try:
        if from_word_ids is None:
            f = o.add_new_words(frm, 1) if len(frm) else []
        else:
            for i, r in zip(from_word_ids, frm):
                o.add_word(int(i), r)
            f = [int(i) for i in from_word_ids]
        o.update()
        t = o.add_new_words(to, 2) if len(to) else []
        assert len(f) == len(frm) and len(t) == len(to), o.last_error()
        return np.asarray(f, np.int32), np.asarray(t, np.int32)
    finally:
        o.close()
