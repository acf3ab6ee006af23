"""sn_tiles_unpack: the argument checks run before any launch and need no device; sn_last_error names the argument."""
import ctypes

from scene_net_amd import _hip

F32, F64, U8, OCC8, BF16, I32 = _hip.SN_F32, _hip.SN_F64, _hip.SN_U8, _hip.SN_OCC8, _hip.SN_BF16, _hip.SN_I32
INVALID, UNSUPPORTED = -1, -2


def _call(lib, rows, dtype, cols, total, offsets, B, pts, labels, bad):
    rc = lib.sn_tiles_unpack(rows, dtype, cols, total, offsets, B, pts, labels, bad, None)
    return rc, lib.sn_last_error()


def test_tiles_unpack_is_declared_and_bound():
    assert "sn_tiles_unpack" in _hip.SYMBOLS and callable(_hip.tiles_unpack)
    assert hasattr(_hip.load(), "sn_tiles_unpack")


def test_tiles_unpack_argument_checks_need_no_gpu():
    lib = _hip.load()
    buf = ctypes.create_string_buffer(256)
    base = (ctypes.addressof(buf) + 15) & ~15
    p = ctypes.c_void_p(base)
    rc, msg = _call(lib, None, F64, 4, 10, p, 1, p, p, p)
    assert rc == INVALID and b"rows" in msg
    rc, msg = _call(lib, p, F64, 4, 10, p, 1, None, p, p)
    assert rc == INVALID and b"pts" in msg
    for total in (0, -5):
        rc, msg = _call(lib, p, F64, 4, total, p, 1, p, p, p)
        assert rc == INVALID and b"total" in msg
    for B in (0, -1):
        rc, msg = _call(lib, p, F64, 4, 10, p, B, p, p, p)
        assert rc == INVALID and b"B " in msg
    for cols in (2, 9, 0, -4):
        rc, msg = _call(lib, p, F64, cols, 10, p, 1, p, None, p)
        assert rc == INVALID and b"cols" in msg
    rc, msg = _call(lib, p, F64, 3, 10, p, 1, p, p, p)            # labels with cols == 3
    assert rc == INVALID and b"labels" in msg
    rc, msg = _call(lib, p, F32, 4, 10, None, 1, p, p, p)         # bad without offsets
    assert rc == INVALID and b"offsets" in msg
    for dtype in (U8, OCC8, BF16, I32):
        rc, msg = _call(lib, p, dtype, 4, 10, p, 1, p, p, p)
        assert rc == UNSUPPORTED and b"row_dtype" in msg
    for dtype in (-1, 6, 99):
        rc, msg = _call(lib, p, dtype, 4, 10, p, 1, p, p, p)
        assert rc == INVALID and b"row_dtype" in msg
    # element alignment of rows (f64: 8 bytes, f32: 4)
    rc, msg = _call(lib, ctypes.c_void_p(base + 4), F64, 4, 10, p, 1, p, p, p)
    assert rc == INVALID and b"rows" in msg
    rc, msg = _call(lib, ctypes.c_void_p(base + 2), F32, 4, 10, p, 1, p, p, p)
    assert rc == INVALID and b"rows" in msg
