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
