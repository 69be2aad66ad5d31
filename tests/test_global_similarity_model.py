"""CPU-only: the model of the whole of Signature::compareTo (tests/global_similarity_model.py) is consistent with itself and with the
words-branch model, the error bound it computes holds for two fp32 summation orders emulated in numpy, and the cross-compiled libraries
export the feature's entry points."""
import ctypes
import os
import re

import numpy as np

import global_similarity_model as G
import similarity_model as S


def _unit(rng, dim, signed=True):
    v = rng.standard_normal(dim) if signed else rng.random(dim)
    return (v / np.linalg.norm(v)).astype(np.float32)


def test_model_is_symmetric():
    rng = np.random.default_rng(1)
    for _ in range(60):
        dims = [int(rng.choice([1, 3, 64, 257])) for _ in range(int(rng.integers(0, 4)))]

        def globs():
            out = []
            for d in dims:
                k = int(rng.integers(0, 4))
                out.append([None, (0, _unit(rng, d)), _unit(rng, d), (1, _unit(rng, d, False))][k])
            return out[: int(rng.integers(0, len(dims) + 1))] if rng.random() < 0.3 else out
        qa, qb = globs(), globs()
        wa, wb = rng.integers(-1, 12, int(rng.integers(0, 30))), rng.integers(-1, 12, int(rng.integers(0, 30)))
        ab, ba = G.compare_to_full(wa, qa, wb, qb), G.compare_to_full(wb, qb, wa, qa)
        assert ab == ba


def test_without_a_matching_channel_the_words_branch_answers_bit_for_bit():
    rng = np.random.default_rng(2)
    a64, b64, a8 = _unit(rng, 64), _unit(rng, 64), _unit(rng, 8)
    cases = [([], []), ([a64], []), ([], [b64]), ([(0, a64)], [b64]), ([a64], [(0, b64)]), ([a64, None], [None, a8]), ([None], [None]),
             ([(1, None)], [b64]), ([(2, a64)], [(2, b64)])]
    for qg, sg in cases:
        for _ in range(10):
            wa, wb = rng.integers(-1, 9, int(rng.integers(0, 25))).astype(np.int32), rng.integers(-1, 9, int(rng.integers(0, 25))).astype(np.int32)
            sim, n, bound = G.compare_to_full(wa, qg, wb, sg)
            assert n == 0 and bound == 0.0
            assert np.float32(sim).tobytes() == np.float32(S.compare_to_literal(wa, wb)[0]).tobytes()
    # and with one, the words do not matter
    sim, n, _ = G.compare_to_full([1, 2], [a64], [1, 2], [a64])
    sim2, n2, _ = G.compare_to_full([], [a64], [7], [a64])
    assert (n, n2) == (1, 1) and sim == sim2 and abs(sim - 1.0) < 1e-6
    # two channels: the mean, in the reference's statement order
    sim, n, _ = G.compare_to_full([], [a64, a8], [], [b64, a8])
    d0 = (float(np.dot(a64.astype(np.float64), b64.astype(np.float64))) + 1.0) / 2.0
    d1 = (float(np.dot(a8.astype(np.float64), a8.astype(np.float64))) + 1.0) / 2.0
    assert n == 2 and sim == (0.0 + d0 + d1) / 2


def test_two_fp32_orders_stay_under_the_bound():
    """a sequential fp32 sum and the 64-lane strided sum with a butterfly reduction, unit vectors signed and non-negative"""
    rng = np.random.default_rng(3)
    worst = 0.0
    for dim in (1, 5, 64, 257, 1023, 4096, 16384):
        for signed in (True, False):
            a, b = _unit(rng, dim, signed), _unit(rng, dim, signed)
            sim, n, bound = G.compare_to_full([], [a], [], [b])
            assert n == 1 and bound > 0
            orders = [G.dot_lanes_f32(a, b)] + ([G.dot_sequential_f32(a, b)] if dim <= 4096 else [])
            for d32 in orders:
                err = abs(float(G.term_f32(d32)) - sim)
                assert err <= bound, (dim, signed, err, bound)
                worst = max(worst, err / bound)
    print("largest err / bound over the emulated orders: %.3f" % worst)
    assert worst < 1.0


def test_libraries_export_the_global_descriptor_entry_points():
    import rtabmap_amd
    from rtabmap_amd import build as b
    rtabmap_amd.load()
    lib = ctypes.CDLL(rtabmap_amd.library_path())
    for s in ("lcd_sig_set_globals", "lcd_sig_set_globals_dev", "lcd_sig_set_global_bulk", "lcd_sig_clear_globals", "lcd_compare_to",
              "lcd_compare_to_dev"):
        assert hasattr(lib, s), s
    host = ctypes.CDLL(b.build_host())
    for s in ("hmem_set_global_descriptors", "hmem_num_global_descriptors"):
        assert hasattr(host, s), s


def test_loader_constants_equal_the_headers():
    from rtabmap_amd import capi
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lcd.h")).read()
    for name in ("LCD_GLOBAL_MAX_CHANNELS", "LCD_GLOBAL_MAX_DIM"):
        m = re.search(r"#define\s+%s\s+(\d+)" % name, hdr)
        assert m and int(m.group(1)) == getattr(capi, name), name
    assert ctypes.sizeof(capi.LcdGlobalDesc) == 16            # int32 type, int32 dim, const float* data
