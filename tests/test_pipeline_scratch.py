"""The private segment (scratch memory) and the register count of the two fused launches of a pipelined frame, read from the kernel
descriptors of the library build() produced -- the 64-byte records the .amdhsa_private_segment_fixed_size and .amdhsa_next_free_vgpr
directives of a listing end up in, i.e. what the dispatch really sets up.  No GPU: the descriptors are found in the gfx950 code objects
of the library's fat binary.

Launch B's re-rank role is a chain of dependent memory round trips, and on gfx950 a spill store or reload counts in the same in-order
counter as the chain's loads and stores: frame_b_kernel<false> (every launch B of a memory below 1024 sealed buckets) keeps its live
set inside the 80 registers that six waves per SIMD allow, with no scratch at all.  frame_b_kernel<true> (its scoring role spills when
the row writers ride along) must not get worse than the 76 bytes it had, and launch A, which never touched its 36 bytes, reserves none.
Only that field and the register count are looked at."""
import struct

import pytest

from rtabmap_amd import build as lcd_build

BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _code_objects(blob):
    """every gfx950 code object of a library's fat binaries"""
    at = blob.find(BUNDLE_MAGIC)
    while at >= 0:
        (n,) = struct.unpack_from("<Q", blob, at + len(BUNDLE_MAGIC))
        p = at + len(BUNDLE_MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", blob, p)
            triple = blob[p + 24: p + 24 + tlen].decode()
            p += 24 + tlen
            if "gfx950" in triple and size:
                yield blob[at + off: at + off + size]
        at = blob.find(BUNDLE_MAGIC, at + 1)


def _kernel_descriptors(elf):
    """{symbol name without .kd: (private_segment_fixed_size, vgprs allocated, private segment enabled)} of one code object (ELF64, little endian)"""
    assert elf[:6] == b"\x7fELF\x02\x01"
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]   # name, type, flags, addr, offset, size, link, info, align, entsize
    out = {}
    for name, typ, flags, addr, offset, size, link, info, align, entsize in secs:
        if typ not in (2, 11):                                         # SHT_SYMTAB, SHT_DYNSYM
            continue
        str_off = secs[link][4]
        for i in range(size // 24):
            st_name, st_info, st_other, st_shndx, st_value, st_size = struct.unpack_from("<IBBHQQ", elf, offset + 24 * i)
            sym = elf[str_off + st_name: elf.index(b"\0", str_off + st_name)].decode()
            if not sym.endswith(".kd") or st_shndx == 0 or st_shndx >= shnum:
                continue
            s = secs[st_shndx]
            kd = elf[s[4] + st_value - s[3]: s[4] + st_value - s[3] + 64]
            private, = struct.unpack_from("<I", kd, 4)
            rsrc1, rsrc2 = struct.unpack_from("<II", kd, 48)
            out[sym[:-3]] = (private, ((rsrc1 & 63) + 1) * 8, bool(rsrc2 & 1))   # gfx90a and later allocate registers in blocks of eight
    return out


@pytest.fixture(scope="module")
def descriptors():
    with open(lcd_build.build(), "rb") as f:
        blob = f.read()
    kds = {}
    for elf in _code_objects(blob):
        kds.update(_kernel_descriptors(elf))
    assert kds, "no gfx950 kernel descriptor found in the library"
    return kds


def _one(kds, *parts):
    hits = [(k, v) for k, v in kds.items() if all(p in k for p in parts)]
    assert len(hits) == 1, (parts, [k for k, _ in hits])
    return hits[0][1]


def test_launch_b_without_appenders_has_no_private_segment(descriptors):
    private, vgprs, enabled = _one(descriptors, "frame_b_kernelILb0E")
    print("frame_b_kernel<false>: private segment %d bytes per lane, %d registers" % (private, vgprs))
    assert private == 0 and not enabled
    assert vgprs <= 80, "six waves per SIMD (512 registers) -- all of the headline's 687 workgroups resident at once -- need 80 registers or fewer"


def test_launch_b_with_appenders_spills_no_more_than_it_did(descriptors):
    private, vgprs, _ = _one(descriptors, "frame_b_kernelILb1E")
    print("frame_b_kernel<true>: private segment %d bytes per lane, %d registers" % (private, vgprs))
    assert private <= 76
    assert vgprs <= 80


@pytest.mark.parametrize("m", [0, 1])
def test_launch_a_has_no_private_segment(descriptors, m):
    """Launch A touches no scratch and must not have the dispatch set a private segment up.  (It used to reserve 36 bytes: a spill slot the register
    allocator assigned to an 8-register kernel-argument tuple of the decision loop and never used, plus the emergency slot a frame with a stack object
    gets -- frame_resolve_part now takes those arguments as scalars of their own; profiles/launch_b_scratch.txt, 5.)"""
    private, vgprs, enabled = _one(descriptors, "frame_a_kernelILi%dE" % m)
    print("frame_a_kernel<%d>: private segment %d bytes per lane, %d registers" % (m, private, vgprs))
    assert private == 0 and not enabled
