"""The workspace contract (tests/test_gpu_workspace_contract.py) for ``qt_xtx_accumulate_batched``: called with exactly
the bytes ``qt_xtx_batched_plan`` asks for (``*workspace_bytes``) between two guards of one byte pattern, the pointer 0
or 16 bytes off a 256-byte boundary, it writes nothing outside them; ``need - 1`` and a NULL workspace are refused with
``QT_ERR_WORKSPACE`` and nothing is written; the outputs are bit-equal to the call through ``ops``.  One case per branch
of the batched plan (tests/xtx_batched_cases.py), plus a batch of one (the delegate's workspace)."""
import ctypes

import pytest
import torch

from quantool_amd.hip import _lib
from quantool_amd.hip._lib import QT_BF16, QT_ERR_INVALID, QT_ERR_WORKSPACE, QT_F16, QT_OK
from tests.xtx_batched_cases import CASES, check_branch

pytestmark = pytest.mark.gpu

PATTERN = 0xA5
ALL = dict(CASES, batch_of_one=([0, 2117, 0], 520, "one problem with tokens: qt_xtx_accumulate's slabs, tail and table"))


def _call(lib, Xs, Gs, K, code, ws, nbytes, pitches=None):
    m = len(Xs)
    counts = (ctypes.c_int64 * m)(*[x.shape[0] for x in Xs])
    ldx = (ctypes.c_int64 * m)(*(pitches or [K] * m))
    xp = (ctypes.c_void_p * m)(*[x.data_ptr() for x in Xs])
    gp = (ctypes.c_void_p * m)(*[g.data_ptr() for g in Gs])
    return lib.qt_xtx_accumulate_batched(xp, code, counts, ldx, K, gp, m, ws, nbytes,
                                         torch.cuda.current_stream().cuda_stream)


def _need(lib, tokens, K):
    counts = (ctypes.c_int64 * len(tokens))(*tokens)
    need = ctypes.c_size_t(0)
    assert lib.qt_xtx_batched_plan(counts, len(tokens), K, None, 0, None, None, ctypes.byref(need)) == QT_OK
    return int(need.value)


def _bad(region):
    bad = (region != PATTERN).nonzero()
    return None if bad.numel() == 0 else (int(bad[0]), int(bad[-1]), int(bad.numel()))


@pytest.mark.parametrize("offset", [0, 16])
@pytest.mark.parametrize("name", list(ALL))
def test_writes_stay_inside_the_bytes_asked_for(ops, dev, name, offset):
    tokens, K, branch = ALL[name]
    if name in CASES:
        check_branch(name, *ops.xtx_batched_plan(tokens, K))
    dtype, code = (torch.bfloat16, QT_BF16) if offset == 0 else (torch.float16, QT_F16)
    lib = _lib.load()
    g = torch.Generator().manual_seed(len(tokens) + K)
    host = [(torch.randn(n, K, generator=g) * 0.5).to(dtype) for n in tokens]

    def make():
        return [h.to(dev) for h in host], [torch.full((K, K), 0.25, dtype=torch.float32, device=dev) for _ in tokens]

    Xs, Gs = make()
    need = _need(lib, tokens, K)
    assert need > 0
    guard = (max(1 << 20, need) + 255) // 256 * 256
    start = guard + offset
    buf = torch.full((start + need + guard,), PATTERN, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 256 == 0
    ws = buf.data_ptr() + start
    before = [G.clone() for G in Gs]
    torch.cuda.synchronize()

    assert _call(lib, Xs, Gs, K, code, ws, need - 1) == QT_ERR_WORKSPACE
    assert _call(lib, Xs, Gs, K, code, None, need) == QT_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert _bad(buf) is None, f"{name}: a refused call wrote to the workspace buffer"
    assert all(torch.equal(a, b) for a, b in zip(Gs, before)), f"{name}: a refused call wrote to a G"

    rc = _call(lib, Xs, Gs, K, code, ws, need)
    assert rc == QT_OK, f"{name}: status {rc}: {lib.qt_last_error()}"
    torch.cuda.synchronize()
    lo, hi = _bad(buf[:start]), _bad(buf[start + need:])
    assert hi is None, f"{name} [{branch}]: wrote past the {need} bytes it asked for: {hi}"
    assert lo is None, f"{name} [{branch}]: wrote in front of the workspace: {lo}"

    X2, G2 = make()
    ops.xtx_accumulate_batched(X2, G2)
    torch.cuda.synchronize()
    for p, (a, b) in enumerate(zip(Gs, G2)):
        assert torch.equal(a, b), f"{name}: problem {p} differs from the call through ops"


def test_ragged_and_strided_is_refused(dev):
    """A token count that is no multiple of 64 with ldx != K: QT_ERR_INVALID with a message, nothing written; the same
    pitch with a whole number of token tiles is taken."""
    lib = _lib.load()
    K, pad = 264, 8
    wide = torch.ones((200, K + pad), dtype=torch.bfloat16, device=dev)
    Gs = [torch.zeros((K, K), dtype=torch.float32, device=dev) for _ in range(2)]
    need = _need(lib, [200, 128], K)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    Xs = [wide[:, :K], wide[:128, :K]]
    assert _call(lib, Xs, Gs, K, QT_BF16, ws.data_ptr(), need, pitches=[K + pad, K + pad]) == QT_ERR_INVALID
    assert b"ragged" in lib.qt_last_error()
    torch.cuda.synchronize()
    assert not Gs[0].any() and not Gs[1].any()
    Xs = [wide[:192, :K], wide[:128, :K]]
    need = _need(lib, [192, 128], K)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    assert _call(lib, Xs, Gs, K, QT_BF16, ws.data_ptr(), need, pitches=[K + pad, K + pad]) == QT_OK
    torch.cuda.synchronize()
    assert float(Gs[0][0, 0]) == 192.0 and float(Gs[1][K - 1, 0]) == 128.0
