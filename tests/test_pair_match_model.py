"""CPU-only: the models of the two matchers of lcd_match_pairs (tests/pair_match_model.py) on hand-made inputs, and the boundary: the header
declares both entry points, the Python struct has the C layout, the ABI version stays 7 and the cross-compiled library exports them."""
import ctypes
import os
import re

import numpy as np

import pair_match_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cross_check_rule_on_hand_made_matrices():
    # every to-row has its own from-row
    m, d = M.cross_check([[1, 5, 9], [7, 2, 8], [6, 4, 3]])
    assert m.tolist() == [0, 1, 2] and d.tolist() == [1, 2, 3]
    # two to-rows choose from-row 0: the closer one keeps it, the other is rejected but still reports its distance
    m, d = M.cross_check([[2, 9], [1, 9], [8, 3]])
    assert m.tolist() == [-1, 0, 1] and d.tolist() == [2, 1, 3]
    # no from-rows / no to-rows
    m, d = M.cross_check(np.zeros((3, 0), np.float32))
    assert m.tolist() == [-1, -1, -1] and d.tolist() == [-1, -1, -1]
    m, d = M.cross_check(np.zeros((0, 4), np.float32))
    assert m.size == 0 and d.size == 0


def test_cross_check_ties_go_to_the_lower_index_in_both_directions():
    D = np.array([[4, 4, 9],       # to-row 0: from-rows 0 and 1 tie -> nn = 0
                  [4, 6, 9],       # to-row 1: nn = 0 at the same distance as to-row 0 -> back(0) = 0, row 1 rejected
                  [9, 5, 5],       # to-row 2: from-rows 1 and 2 tie -> nn = 1
                  [9, 5, 7]],      # to-row 3: nn = 1, ties with to-row 2 -> rejected
                 np.float32)
    m, d = M.cross_check(D)
    assert m.tolist() == [0, -1, 1, -1] and d.tolist() == [4, 4, 5, 5]
    assert M.tie_resolved_by_index(D)
    assert not M.tie_resolved_by_index([[1, 5], [7, 2]])


def test_cross_check_is_not_symmetric_mutual_nn():
    """from-row 0 is chosen by to-row 0 only, but its own nearest to-row is row 1 (which prefers from-row 1): the rule keeps the match --
    a from-row is kept by the closest of the to-rows that CHOSE it -- mutual nearest neighbours would drop it"""
    D = np.array([[3, 9], [1, 0.5]], np.float32)
    assert M.cross_check(D)[0].tolist() == [0, 1]
    assert M.mutual_nn(D).tolist() == [-1, 1]
    # where every from-row's nearest to-row also chose it the two agree
    D = np.array([[1, 5, 9], [7, 2, 8], [6, 4, 3]], np.float32)
    assert M.cross_check(D)[0].tolist() == M.mutual_nn(D).tolist()


def test_cross_check_over_the_oracle_distances(oracle):
    rng = np.random.default_rng(5)
    base = rng.integers(0, 256, (6, 32), dtype=np.uint8)
    frm, to = base[[0, 1, 1, 2, 3]], base[[1, 0, 0, 4, 3, 3]]
    D = oracle.dist_matrix(to, frm)
    assert D.shape == (6, 5) and D[0, 1] == 0 and D[0, 2] == 0
    m, d = M.cross_check(D)
    # to 0 -> from 1 (not 2: lower index); to 1 and 2 both at distance 0 from from 0 -> row 1 keeps it; to 4 and 5 likewise on from 4
    assert m.tolist()[:3] == [1, 0, -1] and m.tolist()[4:] == [4, -1]
    assert d[[0, 1, 2, 4, 5]].tolist() == [0, 0, 0, 0, 0]


def test_dictionary_model_is_the_three_call_sequence(oracle):
    rng = np.random.default_rng(9)
    a = rng.standard_normal((12, 64)).astype(np.float32)
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    b = np.ascontiguousarray(np.concatenate([a[[3, 7, 7]], -a[:2]]))
    f, t = M.dictionary_pair(oracle, a, b, new_words_compared=False)
    assert f.tolist() == list(range(1, 13))                       # every from-row is a word
    assert t[:3].tolist() == [4, 8, 8] and t[3:].tolist() == [13, 14]
    # one from-word: no indexed search, the to-rows are new words (compared together: the copies of a row still meet each other's word)
    f, t = M.dictionary_pair(oracle, a[:1], np.repeat(a[:1], 3, axis=0), new_words_compared=False)
    assert f.tolist() == [1] and t.tolist() == [2, 3, 4]
    # given ids: echoed, rows in ascending id, the to-frame numbers from max + 1
    ids = [50, 7, 1000, 3]
    f, t = M.dictionary_pair(oracle, a[:4], np.ascontiguousarray(np.concatenate([a[[2, 0]], -a[:1]])), from_word_ids=ids)
    assert f.tolist() == ids and t.tolist() == [1000, 50, 1001]
    # empty sides
    f, t = M.dictionary_pair(oracle, a[:0], a[:2])
    assert f.size == 0 and t.tolist() == [1, 2]
    f, t = M.dictionary_pair(oracle, a[:2], a[:0])
    assert f.tolist() == [1, 2] and t.size == 0


def test_header_declares_both_entry_points_and_says_what_the_rule_is_not():
    header = open(os.path.join(ROOT, "include", "lcd.h")).read()
    assert re.search(r"\bint\s+lcd_match_pairs\s*\(\s*lcd_engine\s*\*\s*h\s*,\s*const\s+lcd_match_args\s*\*", header)
    assert re.search(r"\bint\s+lcd_match_pairs_dev\s*\(\s*lcd_engine\s*\*\s*h\s*,\s*const\s+lcd_match_args\s*\*", header)
    assert "enum lcd_match_mode { LCD_MATCH_DICTIONARY = 0, LCD_MATCH_CROSS_CHECK = 1 }" in header
    assert "NOT the symmetric" in header and "mutual nearest neighbour" in header
    assert "#define LCD_ABI_VERSION 7" in header


def test_match_args_layout_is_the_c_layout():
    from rtabmap_amd import capi
    assert ctypes.sizeof(capi.LcdMatchArgs) == 96
    src = open(os.path.join(ROOT, "rtabmap_amd", "csrc", "pair_match.hip")).read()
    assert re.search(r"static_assert\(sizeof\(lcd_match_args\) == 96\b", src)
    offs = {n: getattr(capi.LcdMatchArgs, n).offset for n, _ in capi.LcdMatchArgs._fields_}
    assert offs["from_rows"] == 24 and offs["from_offsets"] == 40 and offs["from_word_ids"] == 56 and offs["out_to_dist"] == 88
    assert (capi.LCD_MATCH_DICTIONARY, capi.LCD_MATCH_CROSS_CHECK) == (0, 1)


def test_library_exports_the_pair_matcher():
    """fails on a library without the feature"""
    import rtabmap_amd
    L = rtabmap_amd.load()
    lib = ctypes.CDLL(rtabmap_amd.library_path())
    for s in ("lcd_match_pairs", "lcd_match_pairs_dev"):
        assert hasattr(lib, s), s
    assert L.lcd_abi_version() == 7
    # a null handle is refused, not dereferenced
    assert lib.lcd_match_pairs(None, None) == 1 and lib.lcd_match_pairs_dev(None, None) == 1


def test_cross_check_id_bookkeeping_of_the_host_mirror():
    """RegistrationVis.cpp:1391-1477 in VWDictionaryHip::crossCheckWordIds (plain host code, no engine): from ids i + 1 or the original ids,
    a matched to-row takes its from-row's id, an unmatched one fromWordIds.back() + i + 1"""
    from rtabmap_amd import build as b
    host = ctypes.CDLL(b.build_host())
    assert hasattr(host, "hvwd_match_frames")
    fn = host.hvwd_cross_check_word_ids
    fn.restype = None
    vp = ctypes.c_void_p
    fn.argtypes = [ctypes.c_int, vp, vp, ctypes.c_int, vp, vp]

    def run(n_from, orig, match):
        match = np.asarray(match, np.int32)
        of, ot = np.zeros(max(n_from, 1), np.int32), np.zeros(max(match.size, 1), np.int32)
        o = None if orig is None else np.asarray(orig, np.int32)
        fn(n_from, None if o is None else o.ctypes.data, match.ctypes.data, match.size, of.ctypes.data, ot.ctypes.data)
        return of[:n_from].tolist(), ot[: match.size].tolist()

    assert run(4, None, [2, -1, 0, -1, 3]) == ([1, 2, 3, 4], [3, 4 + 1 + 1, 1, 4 + 3 + 1, 4])
    assert run(3, [50, 7, 9], [1, -1, -1]) == ([50, 7, 9], [7, 9 + 1 + 1, 9 + 2 + 1])          # back() is the LAST id, not the largest
    assert run(0, None, [-1, -1]) == ([], [1, 2])
    assert run(2, None, []) == ([1, 2], [])
