"""ctypes mirror of include/plr_image_io.h: the reference's DDS reader / writer (Common/ImageIO.cpp loadDDSFile / writeDDSFile)."""
import ctypes as C

import numpy as np

from .backend import ImageDescription, ImageFormat, ImageType, MipCount, PlrError, _ImageDesc, _load

IMAGE_IO_SYMBOLS = ["plr_write_dds_file", "plr_load_dds_file", "plr_encode_dds", "plr_decode_dds", "plr_decode_bc_to_rgba8", "plr_encode_rgba8_to_bc"]


def _check(lib, rc):
    if rc != 0:
        raise PlrError("plr error %d: %s" % (rc, lib.plr_last_error().decode()))


def _cdesc(d: ImageDescription):
    return _ImageDesc(d.width, d.height, d.depth, int(d.type), int(d.format), int(d.usageFlags), int(d.mipCount), d.manualMipCount, int(d.autoCreateMips))


def _pydesc(c):
    return ImageDescription(width=c.width, height=c.height, depth=c.depth, type=ImageType(c.type), format=ImageFormat(c.format), usageFlags=c.usage_flags,
                            mipCount=MipCount(c.mip_count), manualMipCount=c.manual_mip_count, autoCreateMips=bool(c.auto_create_mips))


def encode_dds(desc: ImageDescription, data) -> bytes:
    lib = _load()
    payload = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    cd = _cdesc(desc)
    n = C.c_size_t()
    _check(lib, lib.plr_encode_dds(C.byref(cd), payload.ctypes.data_as(C.c_void_p), C.c_size_t(payload.size), None, C.c_size_t(0), C.byref(n)))
    out = np.empty(n.value, np.uint8)
    _check(lib, lib.plr_encode_dds(C.byref(cd), payload.ctypes.data_as(C.c_void_p), C.c_size_t(payload.size), out.ctypes.data_as(C.c_void_p), C.c_size_t(out.size), C.byref(n)))
    return out.tobytes()


def decode_dds(file_bytes: bytes):
    """-> (ImageDescription, payload bytes)"""
    lib = _load()
    buf = np.frombuffer(file_bytes, np.uint8)
    cd = _ImageDesc()
    off, size = C.c_size_t(), C.c_size_t()
    _check(lib, lib.plr_decode_dds(buf.ctypes.data_as(C.c_void_p), C.c_size_t(buf.size), C.byref(cd), C.byref(off), C.byref(size)))
    return _pydesc(cd), file_bytes[off.value:off.value + size.value]


def write_dds_file(path, desc: ImageDescription, data):
    lib = _load()
    payload = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    cd = _cdesc(desc)
    _check(lib, lib.plr_write_dds_file(str(path).encode(), C.byref(cd), payload.ctypes.data_as(C.c_void_p), C.c_size_t(payload.size)))


def load_dds_file(path):
    """-> (ImageDescription, uint8 array)"""
    lib = _load()
    cd = _ImageDesc()
    size = C.c_size_t()
    _check(lib, lib.plr_load_dds_file(str(path).encode(), C.byref(cd), None, C.c_size_t(0), C.byref(size)))
    out = np.empty(size.value, np.uint8)
    _check(lib, lib.plr_load_dds_file(str(path).encode(), C.byref(cd), out.ctypes.data_as(C.c_void_p), C.c_size_t(out.size), C.byref(size)))
    return _pydesc(cd), out


def bc_level_bytes(fmt: ImageFormat, width, height):
    """the bytes of one width x height level of BC1 (8-byte blocks), BC3 or BC5 (16-byte blocks)"""
    return ((int(width) + 3) // 4) * ((int(height) + 3) // 4) * (8 if fmt == ImageFormat.BC1 else 16)


def decode_bc_to_rgba8(fmt: ImageFormat, width, height, blocks):
    """one BC1 / BC3 / BC5 level -> height x width uint32 RGBA8 words, R in the low byte: the decode the depth prepass applies to a compressed scene texture"""
    lib = _load()
    src = np.frombuffer(blocks, np.uint8) if isinstance(blocks, (bytes, bytearray)) else np.ascontiguousarray(blocks).view(np.uint8).reshape(-1)
    out = np.empty((max(int(height), 0), max(int(width), 0)), np.uint32)
    lib.plr_decode_bc_to_rgba8.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]
    _check(lib, lib.plr_decode_bc_to_rgba8(int(fmt), int(width), int(height), src.ctypes.data if src.size else None, src.size, out.ctypes.data if out.size else None))
    return out


def encode_rgba8_to_bc(fmt: ImageFormat, width, height, words):
    """one level of height x width uint32 RGBA8 words, R in the low byte -> the uint8 bytes of its BC1 / BC3 / BC5 blocks, by the encode contract the GPU's
    "textureBlockEncode.comp" applies (include/plr_image_io.h plr_encode_rgba8_to_bc); needs no GPU"""
    lib = _load()
    src = np.ascontiguousarray(words, np.uint32).reshape(-1)
    if src.size != max(int(width), 0) * max(int(height), 0):
        raise ValueError("%d words for a %d x %d level" % (src.size, width, height))
    out = np.empty(bc_level_bytes(fmt, max(int(width), 0), max(int(height), 0)), np.uint8)
    lib.plr_encode_rgba8_to_bc.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64]
    _check(lib, lib.plr_encode_rgba8_to_bc(int(fmt), int(width), int(height), src.ctypes.data if src.size else None, out.ctypes.data if out.size else None, out.size))
    return out
