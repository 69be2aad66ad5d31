"""Plain numpy model of the whole of Signature::compareTo (reference corelib/src/Signature.cpp:250-288): the global-descriptor branch
(:257-272) in front of the words branch (tests/similarity_model.py), i.e. what lcd_compare_to answers.

A signature's global descriptors are a list, one entry per channel (the index in SensorData::globalDescriptors()): None (no entry / an
empty one), or (type, row) with row a float vector; a bare array means (1, row).  The reference asserts that both lists have the same
length; the engine instead counts a channel one side lacks as "not type 1" (include/lcd.h), and so does this model.

The dot products are computed in float64, so the model is the exact value up to 2^-53 and the engine's fp32 result is compared within a
BOUND computed from the data, never a tolerance picked by hand:

    per matching channel   |fl(a . b) - a . b| <= gamma_D * sum|a_i b_i|  with gamma_D <= D * 2^-24 for ANY summation order of D fp32 products
                           (fused or not); the "+ 1" and the "/ 2" add one rounding of a value <= ~1 each -> + 2 * 2^-24, and "/ 2" halves the rest:
                           (D / 2 * sum|a_i b_i| + 2) * 2^-24
    the mean               totalDescs - 1 additions and one division of values <= ~1: (totalDescs + 1) * 2^-24

    bound = sum over matching channels of (dim / 2 * sum|a_i b_i| + 2) * 2^-24 / totalDescs + (totalDescs + 1) * 2^-24
"""
import numpy as np

import similarity_model as S

U = 2.0 ** -24                 # unit roundoff of fp32


def _entry(d):
    """-> (type, float64 row) or None"""
    if d is None:
        return None
    typ, row = d if isinstance(d, tuple) else (1, d)
    if row is None:
        return (int(typ), None)
    return (int(typ), np.asarray(row, np.float32).astype(np.float64).reshape(-1))


def _is_type1(g, i):
    if i >= len(g):
        return False
    e = _entry(g[i])
    return e is not None and e[0] == 1 and e[1] is not None and e[1].size > 0


def compare_to_full(q_words, q_globals, s_words, s_globals):
    """this->compareTo(s) with this = (q_words, q_globals), s = (s_words, s_globals) -> (similarity float64, totalDescs, bound)"""
    q_globals, s_globals = list(q_globals or []), list(s_globals or [])
    similarity = 0.0
    total_descs = 0
    err = 0.0
    for i in range(max(len(q_globals), len(s_globals))):
        if _is_type1(q_globals, i) and _is_type1(s_globals, i):
            a, b = _entry(q_globals[i])[1], _entry(s_globals[i])[1]
            assert a.size == b.size, "cv::Mat::dot asserts equal sizes"
            dot_prod = (float(np.dot(a, b)) + 1.0) / 2.0
            similarity += dot_prod
            total_descs += 1
            err += (a.size / 2.0 * float(np.abs(a * b).sum()) + 2.0) * U
    if total_descs:
        similarity /= total_descs
        return similarity, total_descs, err / total_descs + (total_descs + 1) * U
    sim, _, _ = S.compare_to_literal(np.asarray(q_words, np.int32), np.asarray(s_words, np.int32))
    return float(np.float32(sim)), 0, 0.0


# ---- two fp32 summation orders, emulated in numpy (what a device may do): each must stay under the bound
def dot_sequential_f32(a, b):
    acc = np.float32(0.0)
    for x, y in zip(np.asarray(a, np.float32), np.asarray(b, np.float32)):
        acc = np.float32(acc + np.float32(x * y))
    return acc


def dot_lanes_f32(a, b, lanes=64, vec=4):
    """lane l adds the elements of the vectors l, l + lanes, ... in ascending index (products rounded to fp32: no fused multiply-add in
    numpy, which only moves the result inside the same bound), then a xor butterfly over the lanes"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    n = -(-a.size // (lanes * vec)) * lanes * vec
    pa, pb = np.zeros(n, np.float32), np.zeros(n, np.float32)
    pa[:a.size], pb[:b.size] = a, b
    prod = (pa * pb).reshape(-1, lanes, vec)                   # [step, lane, component]
    acc = np.zeros(lanes, np.float32)
    for step in range(prod.shape[0]):
        for c in range(vec):
            acc = (acc + prod[step, :, c]).astype(np.float32)
    off = lanes // 2
    while off >= 1:
        acc = (acc + acc[np.arange(lanes) ^ off]).astype(np.float32)
        off //= 2
    return acc[0]


def term_f32(dot32):
    return np.float32(np.float32(np.float32(dot32) + np.float32(1.0)) / np.float32(2.0))
