"""Argument validation of ``coocc_copy_many`` and of ``coocc_fuser_search``'s optional side stream happens before any launch:
no GPU needed."""
import ctypes

from co_occ_amd import _lib


def test_copy_many_refuses_a_bad_table_before_launching():
    lib = _lib.load()
    tab = (_lib.CopyItem * 17)()
    for it in tab:
        it.dst, it.src, it.bytes = 4096, 8192, 36
    for n in (0, -1, 17):
        assert lib.coocc_copy_many(tab, n, None) == -1 and b"copy_many" in lib.coocc_last_error()
    assert lib.coocc_copy_many(None, 1, None) == -1
    tab[2].dst = None
    assert lib.coocc_copy_many(tab, 3, None) == -1 and b"item 2" in lib.coocc_last_error()
    assert ctypes.sizeof(_lib.CopyItem) == 24 and _lib.COPY_MANY_MAX == 16


def test_fuser_search_needs_a_side_stream_only_where_the_fps_is_not_paired():
    lib = _lib.load()
    d = _lib.SearchDesc()
    for name in ("cat4", "pts", "offsets", "lin", "counts", "near_img", "near_pts", "rows", "rows_p", "ws", "counts_host"):
        setattr(d, name, 4096)              # non-null dummies: validation never dereferences them
    d.C, d.K, d.fps_num, d.max_cluster, d.noff, d.ws_bytes = 128, 2, 2048, 200, 1, 0
    one, two = ctypes.c_void_p(16), ctypes.c_void_p(32)
    d.X, d.Y, d.Z = 200, 200, 16            # too many buckets for the paired FPS: the unpaired fork / join needs the second stream
    assert lib.coocc_fps_voxels_pair_ok(200 * 200 * 16, 200, 200, 16) == 0
    assert lib.coocc_fuser_search(ctypes.byref(d), one, None) == -1 and b"second stream" in lib.coocc_last_error()
    assert lib.coocc_fuser_search(ctypes.byref(d), one, one) == -1 and b"second stream" in lib.coocc_last_error()
    assert lib.coocc_fuser_search(ctypes.byref(d), one, two) == -1 and b"workspace" in lib.coocc_last_error()
    d.X, d.Y, d.Z = 100, 100, 8             # paired: no second stream needed, the next check (workspace size) is reached
    assert lib.coocc_fps_voxels_pair_ok(100 * 100 * 8, 100, 100, 8) == 1
    assert lib.coocc_fuser_search(ctypes.byref(d), one, None) == -1 and b"workspace" in lib.coocc_last_error()
    assert lib.coocc_fuser_search(ctypes.byref(d), one, one) == -1 and b"second stream" in lib.coocc_last_error()
