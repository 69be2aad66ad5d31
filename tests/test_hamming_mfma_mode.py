"""CPU-only: LCD_KNN_HAMMING_MFMA (the Hamming 2-NN of u8 handles on the i8 matrix cores) is part of the boundary -- the value in
include/lcd.h, the same value in the ctypes glue, and the kernel's translation unit in the library that build() links for gfx950."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_enum(name):
    header = open(os.path.join(ROOT, "include", "lcd.h")).read()
    m = re.search(r"\b%s\s*=?\s*(\d+)" % name, header)
    assert m, "%s is not declared in include/lcd.h" % name
    return int(m.group(1))


def test_mode_value_in_header_and_glue():
    from rtabmap_amd import capi
    assert _header_enum("LCD_KNN_HAMMING_MFMA") == 5
    assert capi.LCD_KNN_HAMMING_MFMA == 5
    assert capi.KNN_MODES["hamming_mfma"] == 5
    # the modes that existed keep their values, and the ABI version does not move for an added enum value
    for name, value in (("LCD_KNN_DEFAULT", 0), ("LCD_KNN_EXACT_VALU", 1), ("LCD_KNN_F32_MFMA", 2), ("LCD_KNN_BF16X3", 3), ("LCD_KNN_F16", 4)):
        assert _header_enum(name) == value == getattr(capi, name)
    assert _header_enum("LCD_ABI_VERSION") == 7


def test_library_builds_with_the_kernel():
    import rtabmap_amd
    from rtabmap_amd import build as b
    assert "knn_hamming_mfma.hip" in b.SOURCES
    assert os.path.exists(os.path.join(b.CSRC, "knn_hamming_mfma.hip"))
    L = rtabmap_amd.load()
    assert L.lcd_abi_version() == 7
    # the name lcd_profile_read reports for the kernel is a string of the linked library
    assert b"knn2_hamming_mfma_kernel" in open(rtabmap_amd.library_path(), "rb").read()


def _plan_lib():
    import ctypes as C
    import rtabmap_amd
    rtabmap_amd.load()
    lib = C.CDLL(rtabmap_amd.library_path())
    lib.lcd_debug_hamming_mfma_plan.restype = C.c_int
    lib.lcd_debug_hamming_mfma_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    return lib


def _restated_plan(q, n, dim_bytes, cus):
    """knn_hamming_mfma_plan, restated: two workgroups per compute unit and query group, strips of whole chunks, never KM = 127 * 127 rows or more"""
    w32 = (dim_bytes + 3) // 4
    fixed = w32 in (2, 4, 8, 16)
    qpad = (q + 63) // 64 * 64
    group_q = (256 if w32 == 16 else 512) if fixed else 64
    groups = -(-qpad // group_q)
    unit = 64 if fixed else 128
    chunk = (32 if w32 == 16 else 64) if fixed else 128
    target = max(1, -(-2 * cus // groups))
    rpb = min(max(-(-(-(-n // target)) // unit) * unit, unit), 16128)
    n_blocks = -(-n // rpb)
    return rpb, n_blocks, groups, chunk, qpad, group_q


def test_plan_covers_every_size_and_keeps_the_row_offset_below_km():
    """The launch plan of the matrix-core Hamming 2-NN (knn_hamming_mfma_plan, host code: no device needed) over frames of 1 .. 4096 descriptors, every
    kind of row length, 1 .. 304 compute units and vocabularies from 256 rows to 2^31 - 1: every row belongs to exactly one workgroup's strip, a strip
    is whole chunks and never reaches KM = 127 * 127 rows (the row offset shares the 32-bit key with the distance; decode_key divides by KM), every
    padded query has a group, the partial keys are sized for the grid; the plan is the measured one at the measured size."""
    import ctypes as C
    lib = _plan_lib()
    out = (C.c_int * 6)()
    sizes = sorted(set(list(range(256, 4000, 97)) + list(range(4000, 130000, 1777)) + list(range(130000, 1300000, 41011)) +
                       [3000, 33000, 70001, 200000, 1000000, 8257536, 8257537, 2147483647]))
    for q in (1, 33, 64, 500, 512, 513, 1000, 1024, 4096):
        for dim in (8, 16, 32, 64, 24, 36, 128, 4096):
            for units in (-1, 1, 7, 24, 256, 304):
                for n in sizes:
                    # (no engine was created in this process: the built-in count, 256 units)
                    rpb_x, nb_x, groups_x, chunk_x, qpad_x, group_q = _restated_plan(q, n, dim, 256 if units == -1 else units)
                    rc = lib.lcd_debug_hamming_mfma_plan(q, n, dim, units, out)
                    if nb_x * 2 * qpad_x * 8 > 2 ** 31 - 1:
                        assert rc == -1, (q, n, dim, units)
                        continue
                    assert rc == 0, (q, n, dim, units)
                    rpb, nb, groups, chunk, qpad, part16 = list(out)
                    msg = str((q, n, dim, units, list(out)))
                    assert chunk == chunk_x and rpb % chunk == 0 and rpb % (64 if dim in (8, 16, 32, 64) else 128) == 0, msg
                    assert 64 <= rpb <= 16128 < 127 * 127, msg
                    assert nb * rpb >= n > (nb - 1) * rpb, msg
                    assert qpad == (q + 63) // 64 * 64 and groups * group_q >= qpad > (groups - 1) * group_q, msg
                    assert part16 * 16 == nb * 2 * qpad * 8, msg
                    assert (rpb, nb, groups, qpad) == (rpb_x, nb_x, groups_x, qpad_x), msg
                    if units == -1:
                        assert lib.lcd_debug_hamming_mfma_plan(q, n, dim, 256, out) == 0 and list(out) == [rpb, nb, groups, chunk, qpad, part16], msg
    # 0 has no meaning here ("never persistent" is the float filter's): today's plan, as -1
    assert lib.lcd_debug_hamming_mfma_plan(500, 200000, 32, 0, out) == 0 and list(out)[:2] == [448, 447]
    # the measured size (profiles/hamming_mfma_scan.txt): 447 workgroups of 7 chunks
    assert lib.lcd_debug_hamming_mfma_plan(500, 200000, 32, -1, out) == 0 and list(out) == [448, 447, 1, 64, 512, 447 * 2 * 512 * 8 // 16]
    # where the clamp starts to bind on 256 units: 512 strips of 16 128 rows, then a 513th
    assert lib.lcd_debug_hamming_mfma_plan(500, 8257536, 32, 256, out) == 0 and list(out)[:2] == [16128, 512]
    assert lib.lcd_debug_hamming_mfma_plan(500, 8257537, 32, 256, out) == 0 and list(out)[:2] == [16128, 513]
    # rows the handle pads (61 -> 64 bytes) plan as the padded length; nonsense is refused
    assert lib.lcd_debug_hamming_mfma_plan(300, 3000, 61, 8, out) == 0 and list(out)[:4] == [384, 8, 2, 32]
    for bad in ((0, 3000, 32, -1), (10, 0, 32, -1), (10, 3000, 0, -1), (10, 3000, 4097, -1)):
        assert lib.lcd_debug_hamming_mfma_plan(*bad, out) == -1
