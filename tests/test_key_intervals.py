"""The interval set of recycled postings keys (host code of liblcd_hip.so, no GPU): freeing a batch of verdicts run by run
(KeyIntervals::free_verdicts, what the engine does since round 4) leaves exactly the intervals that freeing key by key leaves."""
import ctypes as C

import numpy as np

import rtabmap_amd


def _intervals(lib, keys, ok, by_runs, take=0):
    keys = np.ascontiguousarray(keys, np.int32)
    ok = np.ascontiguousarray(ok, np.uint8)
    out = np.zeros(2 * (len(keys) + 4), np.int32)
    cnt = C.c_longlong(0)
    lib.lcd_debug_key_intervals.restype = C.c_int
    n = lib.lcd_debug_key_intervals(keys.ctypes.data_as(C.c_void_p), ok.ctypes.data_as(C.c_void_p), len(keys), int(by_runs), int(take),
                                    out.ctypes.data_as(C.c_void_p), len(keys) + 4, C.byref(cnt))
    assert n >= 0
    return out[: 2 * n].reshape(-1, 2).tolist(), cnt.value


def test_runs_and_single_keys_leave_the_same_intervals():
    lib = rtabmap_amd.load()
    rng = np.random.default_rng(5)
    for trial in range(40):
        # what a batch looks like: the keys frames reserved (runs of up to 500 consecutive keys, in any order of the runs), most of them
        # unused (verdict "free"), some used or still referenced in the middle of a run
        starts = rng.permutation(np.arange(0, 64 * 600, 600))[: rng.integers(1, 40)]
        keys = np.concatenate([np.arange(s, s + rng.integers(1, 500)) for s in starts])
        ok = (rng.random(len(keys)) < (0.95 if trial % 2 else 0.6)).astype(np.uint8)
        a, ca = _intervals(lib, keys, ok, by_runs=False)
        b, cb = _intervals(lib, keys, ok, by_runs=True)
        assert a == b and ca == cb == int(ok.sum())
        free = np.unique(keys[ok == 1])                       # ... and they are the maximal runs of the SET of freed keys
        cuts = np.flatnonzero(np.diff(free) != 1)
        first = np.concatenate([[0], cuts + 1])
        last = np.concatenate([cuts, [free.size - 1]])
        assert b == [[int(free[i]), int(free[j] - free[i] + 1)] for i, j in zip(first, last)] if free.size else b == []
        # the set is a partition into maximal intervals: sorted, disjoint, not adjacent
        for (s0, l0), (s1, _) in zip(b, b[1:]):
            assert s0 + l0 < s1
        # and taking keys back (the highest first) agrees as well
        take = int(rng.integers(0, max(1, int(ok.sum()))))
        assert _intervals(lib, keys, ok, False, take) == _intervals(lib, keys, ok, True, take)


def test_a_key_freed_twice_is_ignored_either_way():
    lib = rtabmap_amd.load()
    keys = np.array([10, 11, 12, 11, 12, 13, 40, 41, 13], np.int32)
    ok = np.ones(len(keys), np.uint8)
    a, _ = _intervals(lib, keys, ok, by_runs=False)
    b, _ = _intervals(lib, keys, ok, by_runs=True)
    assert a == b == [[10, 4], [40, 2]]


def _take_runs(lib, keys, ok, want, max_runs):
    keys = np.ascontiguousarray(keys, np.int32)
    ok = np.ascontiguousarray(ok, np.uint8)
    runs = np.zeros(2 * max(max_runs, 1), np.int32)
    left = np.zeros(2 * (len(keys) + 4), np.int32)
    n_left, cnt = C.c_int(0), C.c_longlong(0)
    lib.lcd_debug_key_take_runs.restype = C.c_int
    r = lib.lcd_debug_key_take_runs(keys.ctypes.data_as(C.c_void_p), ok.ctypes.data_as(C.c_void_p), len(keys), int(want), int(max_runs),
                                    runs.ctypes.data_as(C.c_void_p), left.ctypes.data_as(C.c_void_p), len(keys) + 4, C.byref(n_left), C.byref(cnt))
    assert 0 <= r <= max_runs and n_left.value >= 0
    return runs[: 2 * r].reshape(-1, 2).tolist(), left[: 2 * n_left.value].reshape(-1, 2).tolist(), cnt.value


def _check_take_runs(lib, keys, ok, want, max_runs):
    runs, left, cnt = _take_runs(lib, keys, ok, want, max_runs)
    free = np.unique(np.asarray(keys)[np.asarray(ok) == 1])
    got = sum(l for _, l in runs)
    assert all(l > 0 for _, l in runs) and got <= want
    # the keys handed out are exactly the `got` highest free keys: every run ascending, the runs descending
    handed = np.concatenate([np.arange(s, s + l) for s, l in runs]) if runs else np.zeros(0, np.int64)
    assert sorted(handed.tolist()) == free[free.size - got:].tolist()
    for (s0, _), (s1, l1) in zip(runs, runs[1:]):
        assert s1 + l1 <= s0
    # what is left is what `got` single takes leave
    assert (left, cnt) == _intervals(lib, keys, ok, False, got) and cnt == free.size - got
    # fewer than wanted only because the set ran out or the cap on the number of runs was reached
    if got < want:
        assert cnt == 0 or len(runs) == max_runs
    return runs, left


def test_take_runs_hands_out_the_highest_keys_as_single_takes_would():
    lib = rtabmap_amd.load()
    keys = np.array([3, 4, 5, 20, 21, 22, 23, 9], np.int32)          # intervals [3, 3], [9, 1], [20, 4]
    ok = np.ones(len(keys), np.uint8)
    assert _check_take_runs(lib, keys, ok, 0, 15) == ([], [[3, 3], [9, 1], [20, 4]])
    assert _check_take_runs(lib, keys, ok, 3, 15) == ([[21, 3]], [[3, 3], [9, 1], [20, 1]])              # splits the top interval
    assert _check_take_runs(lib, keys, ok, 4, 15) == ([[20, 4]], [[3, 3], [9, 1]])                       # erases it
    assert _check_take_runs(lib, keys, ok, 6, 15) == ([[20, 4], [9, 1], [5, 1]], [[3, 2]])
    assert _check_take_runs(lib, keys, ok, 100, 15) == ([[20, 4], [9, 1], [3, 3]], [])                   # more than the whole set
    assert _check_take_runs(lib, keys, ok, 6, 2) == ([[20, 4], [9, 1]], [[3, 3]])                        # the cap on the runs binds
    assert _check_take_runs(lib, keys, ok, 6, 0) == ([], [[3, 3], [9, 1], [20, 4]])
    assert _check_take_runs(lib, keys[:0], ok[:0], 5, 15) == ([], [])                                    # an empty set
    singles = np.arange(0, 40, 2, dtype=np.int32)                                                        # 20 intervals of one key each
    runs, left = _check_take_runs(lib, singles, np.ones(20, np.uint8), 20, 15)
    assert runs == [[k, 1] for k in range(38, 8, -2)] and left == [[k, 1] for k in range(0, 10, 2)]
    rng = np.random.default_rng(11)
    for trial in range(48):
        starts = rng.permutation(np.arange(0, 24 * 40, 40))[: rng.integers(1, 24)]
        keys = np.concatenate([np.arange(s, s + rng.integers(1, 30)) for s in starts])
        ok = (rng.random(len(keys)) < (0.9 if trial % 2 else 0.5)).astype(np.uint8)
        want = int(rng.integers(0, int(ok.sum()) + 8))
        _check_take_runs(lib, keys, ok, want, int(rng.integers(1, 16)) if trial % 3 else 15)
