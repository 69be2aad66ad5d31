"""CPU-only: the matrix-core 2-NN of 128- and 256-float rows (LCD_KNN_BF16X3 / LCD_KNN_F16 written on an LCD_F32 handle of SIFT / SuperPoint
descriptors; rtabmap_amd/csrc/wide_filter_body.cuh).  The boundary did not move (no new enum value, ABI 7), the kernels are in the library that
build() links for gfx950, the launch plan (host code, lcd_debug_wide_mfma_plan) covers every row and every padded query exactly once with strips
the in-loop key can index, and the filter's arithmetic -- operands rounded to bf16 hi + lo or to half, fp32 accumulation on top of the in-kernel
norms -- stays inside eps_bf16 / eps_f16 of rerank_body.cuh at both row lengths, emulated here in numpy on adversarial inputs."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIP_TILES = 8                                          # MF_STRIP_TILES: the in-loop key has 7 index bits, 4 of them the accumulator register


def _header_enum(name):
    header = open(os.path.join(ROOT, "include", "lcd.h")).read()
    m = re.search(r"\b%s\s*=?\s*(\d+)" % name, header)
    assert m, "%s is not declared in include/lcd.h" % name
    return int(m.group(1))


def test_boundary_did_not_move():
    from rtabmap_amd import capi
    for name, value in (("LCD_KNN_DEFAULT", 0), ("LCD_KNN_EXACT_VALU", 1), ("LCD_KNN_F32_MFMA", 2), ("LCD_KNN_BF16X3", 3), ("LCD_KNN_F16", 4),
                        ("LCD_KNN_HAMMING_MFMA", 5)):
        assert _header_enum(name) == value == getattr(capi, name)
    assert _header_enum("LCD_ABI_VERSION") == 7
    assert capi.KNN_MODES["bf16"] == 3 and capi.KNN_MODES["f16"] == 4 and capi.KNN_MODES["default"] == 0
    header = open(os.path.join(ROOT, "include", "lcd.h")).read()
    assert "profiles/wide_mfma_scan.txt" in header      # the enum's comment says where the measurement is


def test_library_builds_with_the_kernels():
    import rtabmap_amd
    from rtabmap_amd import build as b
    # the kernels are a section of the matrix-core translation unit, included the way bf16_filter_body.cuh is
    assert "knn_mfma_kernels.hip" in b.SOURCES
    assert os.path.exists(os.path.join(b.CSRC, "wide_filter_body.cuh"))
    assert '#include "wide_filter_body.cuh"' in open(os.path.join(b.CSRC, "knn_mfma_kernels.hip")).read()
    L = rtabmap_amd.load()
    assert L.lcd_abi_version() == 7
    blob = open(rtabmap_amd.library_path(), "rb").read()
    # the name lcd_profile_read reports, and the three kernels (their mangled names carry the plain ones)
    assert b"knn_wide_filter_kernel (fp16 operands)" in blob
    for name in (b"knn_wide_filter_kernel", b"knn_wide_rerank_kernel", b"knn_wide_rowpar_kernel"):
        assert name in blob


# ---------------------------------------------------------------------------------------------------------------- the launch plan
def _plan_lib():
    import ctypes as C
    import rtabmap_amd
    rtabmap_amd.load()
    lib = C.CDLL(rtabmap_amd.library_path())
    lib.lcd_debug_wide_mfma_plan.restype = C.c_int
    lib.lcd_debug_wide_mfma_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    return lib


def test_plan_covers_every_row_and_query_once():
    """q in {1 .. 4096}, both row lengths, 1 .. 304 compute units, 256 rows to 2^31 - 1.  Share b of the rows is tiles [b * tps, (b + 1) * tps) of 32
    rows: the shares partition the tiles, so every row lies in exactly one; a share is at most 32 tiles and is walked in strips of at most
    MF_STRIP_TILES; workgroup x takes shares x, x + grid.x, ...: every share has a workgroup; the query blocks cover the padded queries; the
    records are sized for the shares (two 8-byte keys and a 4-byte bound per share and padded query), and a search whose records would pass
    2^31 - 1 bytes has no plan."""
    import ctypes as C
    lib = _plan_lib()
    out = (C.c_int * 9)()
    sizes = sorted(set(list(range(256, 4000, 97)) + list(range(4000, 130000, 1777)) + list(range(130000, 1300000, 41011)) +
                       [3000, 49000, 125000, 1000000, 30000000, 2 ** 31 - 33, 2 ** 31 - 32, 2 ** 31 - 1]))
    refused = 0
    for q in (1, 33, 64, 500, 512, 513, 1000, 4096):
        for dim in (128, 256):
            group_q = 8 * (256 // dim) * 32             # eight waves of 256 / dim groups of 32 queries
            qpad = (q + 63) // 64 * 64
            for units in (-1, 1, 7, 24, 256, 304):
                cus = 256 if units == -1 else units     # (no engine was created in this process: the built-in count)
                target = max(1, cus // -(-qpad // group_q))     # workgroups along the rows: one per compute unit and query block
                for n in sizes:
                    n_tiles = (n + 31) // 32
                    rc = lib.lcd_debug_wide_mfma_plan(q, n, dim, units, out)
                    if rc != 0:                         # refused: only where even the fewest shares (32 tiles each) make records beyond 2^31 - 1 bytes
                        assert rc == -1 and -(-n_tiles // 32) * qpad * 20 > 2 ** 31 - 1, (q, n, dim, units)
                        refused += 1
                        continue
                    tps, shares, qblocks, gq, qpad_, part4, strip, strips, wgs = list(out)
                    msg = str((q, n, dim, units, list(out)))
                    assert 1 <= tps <= 32 and shares * tps >= n_tiles > (shares - 1) * tps, msg     # the shares partition the tiles
                    assert strip == STRIP_TILES and strips == -(-tps // strip) <= 4, msg              # no strip beyond the key's index bits
                    assert gq == group_q and qpad_ == qpad, msg
                    assert qblocks * gq >= qpad > (qblocks - 1) * gq, msg                           # every padded query has a block
                    assert part4 * 4 == shares * qpad * (2 * 8 + 4) <= 2 ** 31 - 1, msg
                    assert wgs == min(shares, target) >= 1, msg                                      # one workgroup per compute unit at the most
                    if units == -1:
                        ref = list(out)
                        assert lib.lcd_debug_wide_mfma_plan(q, n, dim, 256, out) == 0 and list(out) == ref, msg
    assert refused > 0
    # the measured sizes (profiles/wide_mfma_scan.txt): 500 queries, the device's 256 units
    assert lib.lcd_debug_wide_mfma_plan(500, 49000, 128, -1, out) == 0 and [out[i] for i in (0, 1, 2, 3, 8)] == [6, 256, 1, 512, 256]
    assert lib.lcd_debug_wide_mfma_plan(500, 1000000, 128, -1, out) == 0 and [out[i] for i in (0, 1, 2, 3, 8)] == [31, 1009, 1, 512, 256]
    assert lib.lcd_debug_wide_mfma_plan(500, 1000000, 256, -1, out) == 0 and [out[i] for i in (0, 1, 2, 3, 8)] == [31, 1009, 2, 256, 128]
    # other row lengths and nonsense are refused
    for bad in ((10, 3000, 64, -1), (10, 3000, 127, -1), (10, 3000, 512, -1), (10, 3000, 0, -1), (0, 3000, 128, -1), (-5, 3000, 128, -1),
                (10, 0, 128, -1), (10, -1, 256, -1), (2 ** 31 - 1, 3000, 128, -1)):
        assert lib.lcd_debug_wide_mfma_plan(*bad, out) == -1, bad
    assert lib.lcd_debug_wide_mfma_plan(10, 3000, 128, -1, None) == -1


# ---------------------------------------------------------------------------------------------------------------- the filter's arithmetic
U = np.float32(5.9604645e-8)


def eps_bf16(dim, qn, vn):
    """rerank_body.cuh, restated in fp32"""
    f = np.float32
    return (f(3.1) * f(1.5258789e-5) + ((f(3.0) * f(dim) + f(4.0)) * f(8.0) + f(1.5) * f(dim) + f(12.0)) * U) * f(1.25) * (qn + vn)


def eps_f16(dim, qn, vn):
    f = np.float32
    u16 = f(4.8828125e-4)
    return ((f(2.0) * u16 + u16 * u16) + ((f(dim) + f(4.0)) * f(8.0) + f(1.5) * f(dim) + f(12.0)) * U) * f(1.25) * (qn + vn) + \
        f(2.0) * f(dim) * f(2.9802322e-8) * (f(2.0) + qn + vn)


def bf16_rne(x):
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def split_operands(x, f16):
    """op_split2<M>: hi = the float rounded to bf16 / half (nearest even), lo = the remainder rounded likewise (bf16x3 only multiplies it)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if f16:
        with np.errstate(over="ignore"):
            return x.astype(np.float16).astype(np.float32), None
    hi = bf16_rne(x)
    return hi, bf16_rne((x - hi).astype(np.float32))


def fma_norm(x):
    """the in-kernel |x|^2: an fp32 FMA chain over the components (x * x is exact in float64; one rounding per step)"""
    acc = np.zeros(x.shape[0], np.float32)
    for k in range(x.shape[1]):
        acc = (x[:, k].astype(np.float64) ** 2 + acc.astype(np.float64)).astype(np.float32)
    return acc


def filter_scores(q, v, f16):
    """knn_wide_filter_kernel, emulated: the accumulator starts from the exact fp32 augmentation step |v|^2 + |q|^2 and takes, K step by K step,
    the products of the rounded operands (-2 q on the query side) -- exact in fp32, each addition rounded to fp32"""
    dim = q.shape[1]
    qh, ql = split_operands(np.float32(-2.0) * q, f16)
    vh, vl = split_operands(v, f16)
    qn, vn = fma_norm(q), fma_norm(v)
    acc = (vn[None, :].astype(np.float64) + qn[:, None].astype(np.float64)).astype(np.float32)
    order = np.concatenate([np.arange(dim // 2).reshape(-1, 8), np.arange(dim // 2, dim).reshape(-1, 8)], axis=1)   # a step: 8 of each half
    for step in order:
        terms = [(vh, qh)] if f16 else [(vh, qh), (vh, ql), (vl, qh)]
        for a, b in terms:
            for k in step:
                acc = (acc + (b[:, k][:, None] * a[:, k][None, :]).astype(np.float32)).astype(np.float32)
    return acc, qn, vn


def reference_distances(q, v):
    """rtflann::L2 (dist.h:150-177) in fp32: per four components ((d0 d0 + d1 d1) + d2 d2) + d3 d3, every operation rounded, terms added left to right"""
    res = np.zeros((q.shape[0], v.shape[0]), np.float32)
    for g in range(0, q.shape[1], 4):
        d = (v[None, :, g:g + 4] - q[:, None, g:g + 4]).astype(np.float32)
        p = (d * d).astype(np.float32)
        t = (p[..., 0] + p[..., 1]).astype(np.float32)
        t = (t + p[..., 2]).astype(np.float32)
        t = (t + p[..., 3]).astype(np.float32)
        res = (res + t).astype(np.float32)
    return res


def worst_ratio(q, v, f16):
    dim = q.shape[1]
    score, qn, vn = filter_scores(q, v, f16)
    ref = reference_distances(q, v)
    eps = (eps_f16 if f16 else eps_bf16)(dim, qn[:, None], vn[None, :])   # (the kernel takes the vocabulary's largest |v|^2: never smaller)
    return float((np.abs(score.astype(np.float64) - ref.astype(np.float64)) / eps.astype(np.float64)).max())


def _cases(rng, dim, f16):
    nq, nv = 12, 48
    a = rng.standard_normal((nv, dim)).astype(np.float32)
    unit = a / np.linalg.norm(a, axis=1, keepdims=True)
    yield "unit rows, noisy copies", (unit[:nq] + np.float32(0.05) * rng.standard_normal((nq, dim)).astype(np.float32)), unit
    # wide dynamic range inside one row: e^-6 .. e^6 (fp16: everything stays inside half's range, some components below its normal range)
    w = (rng.standard_normal((nv, dim)) * np.exp(rng.uniform(-6, 6, (nv, dim)))).astype(np.float32)
    yield "wide range", w[rng.permutation(nv)[:nq]], w
    yield "wide range, near-identical pairs", (w[:nq] * (1 + 1e-3 * rng.standard_normal((nq, dim)))).astype(np.float32), w
    # SIFT-like: integer components 0 .. 255, |v|^2 ~ 10^5 .. 10^6
    s = rng.integers(0, 256, (nv, dim)).astype(np.float32)
    yield "integer rows", np.clip(s[:nq] + rng.integers(-6, 7, (nq, dim)), 0, 255).astype(np.float32), s
    # adversarial: every component just below a rounding boundary of the operand format (largest remainder), signs aligned so that the errors add
    frac = 2.0 ** -11 if f16 else 2.0 ** -8
    adv = ((1.0 + frac * (1 - 2.0 ** -9)) * 2.0 ** rng.integers(-3, 3, (nv, dim))).astype(np.float32)
    yield "rounding boundaries, aligned", adv[::-1][:nq].copy(), adv
    yield "rounding boundaries, identical rows", adv[:nq].copy(), adv
    if f16:                                              # components below half's normal range (2^-14): the absolute-error term of eps_f16
        tiny = (rng.standard_normal((nv, dim)) * 2.0 ** rng.uniform(-24, -12, (nv, dim))).astype(np.float32)
        yield "below half's normal range", tiny[:nq].copy(), tiny
        yield "unit rows against tiny rows", unit[:nq].copy(), tiny


@pytest.mark.parametrize("dim", [128, 256])
@pytest.mark.parametrize("f16", [False, True], ids=["bf16x3", "fp16"])
def test_filter_error_stays_inside_eps(dim, f16):
    rng = np.random.default_rng(1000 * dim + int(f16))
    worst = {}
    for name, q, v in _cases(rng, dim, f16):
        worst[name] = worst_ratio(q, v, f16)
    print(dim, "fp16" if f16 else "bf16x3", worst)
    # (most of eps at these row lengths is the worst-case charge of 2u per fp32 addition of the 3 dim + 2 products: round-to-nearest sums of
    # mixed signs use a small part of it; the printed figures say how much)
    assert 0.0 < max(worst.values()) < 1.0, worst


def test_emulation_helpers():
    x = np.array([1.0, 1.00390625, -2.5, 3.0e38], np.float32)
    hi, lo = split_operands(x, False)
    assert hi[0] == 1.0 and hi[2] == -2.5 and np.all(np.abs(x[:3].astype(np.float64) - hi[:3] - lo[:3]) <= 2.0 ** -16 * np.abs(x[:3]))
    h16, none = split_operands(np.array([1.0, 1.0 + 2.0 ** -12, 70000.0], np.float32), True)
    assert none is None and h16[0] == 1.0 and h16[1] == 1.0 and np.isinf(h16[2])      # beyond half's range: the re-rank rejects such queries
    q = np.array([[3.0, 4.0, 0.0, 0.0] * 32], np.float32)
    v = np.array([[0.0, 0.0, 0.0, 0.0] * 32, [3.0, 4.0, 0.0, 0.0] * 32], np.float32)
    assert reference_distances(q, v).tolist() == [[800.0, 0.0]]
    s, qn, vn = filter_scores(q, v, False)
    assert s.tolist() == [[800.0, 0.0]] and qn.tolist() == [800.0] and vn.tolist() == [0.0, 800.0]
