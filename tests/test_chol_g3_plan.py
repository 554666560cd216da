"""Host-only check of the item tables of one ``qt_cholesky_inverse_upper`` chain (``qt_chol_g3_plan_check``, no GPU):
the separate tables of ``QT_CHOL_MERGE=0`` / ``order`` and the merged ones of ``QT_CHOL_MERGE=1`` (one table per block
row over both of its long products).  The C side verifies coverage, contiguity, piece length, slab ids and the item
cap; here the counts of the two are compared: merging may never need more slabs, more launches or more table bytes, and
the workspace's slab count (taken from the separate tables) is the same for both."""
import ctypes

import pytest

KS = [640, 1536, 4096, 8192, 14336, 28672]


def _counts(lib, K, merged, min_chunks):
    out = (ctypes.c_longlong * 5)()
    rc = lib.qt_chol_g3_plan_check(K, merged, min_chunks, ctypes.cast(out, ctypes.c_void_p))
    assert rc == 0, (K, merged, min_chunks, rc)
    return dict(zip(("launches", "items", "slabs", "ws_slabs", "table_bytes"), (int(v) for v in out)))


@pytest.mark.parametrize("min_chunks", [0, 1], ids=["default-threshold", "every-product"])
@pytest.mark.parametrize("K", KS)
def test_merged_tables_are_valid_and_need_no_more_slabs(K, min_chunks, monkeypatch):
    from quantool_amd.hip import _lib

    monkeypatch.delenv("QT_G3_TARGET_ITEMS", raising=False)
    lib = _lib.load()
    sep = _counts(lib, K, 0, min_chunks)
    mrg = _counts(lib, K, 1, min_chunks)
    print(f"\n[chol g3 plan] K={K} min_chunks={min_chunks or 64}: separate {sep} | merged {mrg}")
    assert mrg["slabs"] <= sep["slabs"]
    assert mrg["launches"] <= sep["launches"]
    assert mrg["table_bytes"] <= sep["table_bytes"]
    assert mrg["ws_slabs"] == sep["ws_slabs"]
    cap = 96 if K < 8192 else 256
    assert mrg["ws_slabs"] <= cap
    # a row is merged where the cap leaves each of its K / 256 x (1 or 2) tiles two pieces: 512-row blocks up to K = 16384
    if K > 16384:
        assert mrg == sep
    elif min_chunks == 1 or K >= 4096:
        assert mrg["launches"] < sep["launches"] and mrg["slabs"] < sep["slabs"]


def test_bad_arguments():
    from quantool_amd.hip import _lib

    assert _lib.load().qt_chol_g3_plan_check(0, 0, 0, None) != 0
    assert _lib.load().qt_chol_g3_plan_check(4096, 1, 0, None) == 0
