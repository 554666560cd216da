"""The workspace contract of ``qt_lm_head_nll``, by the guard-pattern method of ``test_gpu_workspace_contract.py``,
restated here: the library is called directly on a workspace the test owns -- ``guard + need + guard`` bytes of one byte
pattern, the middle ``need = qt_lm_head_nll_workspace_size(M, V)`` bytes handed over, once on a 256-byte boundary and
once 16 bytes behind one.  After the call both guards still hold the pattern byte for byte, and every output is
bit-identical to the same call through ``ops``; ``workspace_bytes = need - 1`` and a NULL workspace are refused with
``QT_ERR_WORKSPACE`` and leave the outputs and the whole buffer untouched."""
import pytest
import torch

from quantool_amd.hip import _lib
from quantool_amd.hip._lib import QT_BF16, QT_ERR_WORKSPACE, QT_F16, QT_OK

pytestmark = pytest.mark.gpu

PATTERN = 0xA5
OUTS = ("nll", "lse", "tgt", "argmax")
CASES = [  # (M, V, K, dtype, branch)
    (257, 513, 128, torch.bfloat16, "two row tiles, three vocabulary tiles, the last one column wide"),
    (100, 256, 256, torch.float16, "one vocabulary tile: one record per row"),
]


def _first_bad(region):
    bad = (region != PATTERN).nonzero()
    return None if bad.numel() == 0 else (int(bad[0]), int(bad[-1]), int(bad.numel()))


def _make(M, V, K, dtype, dev):
    g = torch.Generator().manual_seed(M + V + K)
    t = dict(H=torch.randn(M, K, generator=g).to(dtype).to(dev),
             W=(torch.randn(V, K, generator=g) * 0.25).to(dtype).to(dev),
             targets=torch.randint(0, V, (M,), generator=g).to(dev))
    for n in ("nll", "lse", "tgt"):
        t[n] = torch.full((M,), -3.5, dtype=torch.float32, device=dev)
    t["argmax"] = torch.full((M,), -9, dtype=torch.int32, device=dev)
    return t


def _call(lib, t, M, V, K, dtype, ws, nbytes):
    return lib.qt_lm_head_nll(t["H"].data_ptr(), K, t["W"].data_ptr(), K, QT_BF16 if dtype == torch.bfloat16 else QT_F16,
                              M, K, V, t["targets"].data_ptr(), 8, t["nll"].data_ptr(), t["lse"].data_ptr(),
                              t["tgt"].data_ptr(), t["argmax"].data_ptr(), ws, nbytes,
                              torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("offset", [0, 16])
@pytest.mark.parametrize("M,V,K,dtype,branch", CASES, ids=[c[4].split(":")[0].split(",")[0] for c in CASES])
def test_no_write_outside_the_workspace(ops, dev, M, V, K, dtype, branch, offset):
    lib = _lib.load()
    t = _make(M, V, K, dtype, dev)
    need = int(lib.qt_lm_head_nll_workspace_size(M, V))
    tiles_n = (V + 255) // 256
    assert need == 16 * M * tiles_n + 4 * M and need > 0
    guard = (max(1 << 20, need) + 255) // 256 * 256
    start = guard + offset
    buf = torch.full((start + need + guard,), PATTERN, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 256 == 0
    ws = buf.data_ptr() + start
    before = {n: t[n].clone() for n in OUTS}
    torch.cuda.synchronize()

    # refusals: nothing may be launched
    assert _call(lib, t, M, V, K, dtype, ws, need - 1) == QT_ERR_WORKSPACE
    assert _call(lib, t, M, V, K, dtype, None, need) == QT_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert _first_bad(buf) is None, "a refused call wrote to the workspace buffer"
    for n in OUTS:
        assert torch.equal(t[n], before[n]), f"a refused call wrote to {n}"

    # the guarded call
    rc = _call(lib, t, M, V, K, dtype, ws, need)
    assert rc == QT_OK, lib.qt_last_error()
    torch.cuda.synchronize()
    lo, hi = _first_bad(buf[:start]), _first_bad(buf[start + need:])
    assert hi is None, f"[{branch}] wrote past the {need} bytes it asked for: {hi}"
    assert lo is None, f"[{branch}] wrote in front of the workspace: {lo}"
    # every record and every target logit has a writer: nothing of the pattern is left but the records' fourth word
    mid = buf[start:start + need]
    recs = mid[:16 * M * tiles_n].view(-1, 16)
    assert not bool((recs[:, :12] == PATTERN).all(dim=1).any()), "a record was never written"

    # the same call through ops, on fresh copies of the same inputs
    t2 = _make(M, V, K, dtype, dev)
    nll, lse, argmax, tgt = ops.lm_head_nll(t2["H"], t2["W"], t2["targets"], return_target_logit=True)
    for n, got in zip(("nll", "lse", "argmax", "tgt"), (nll, lse, argmax, tgt)):
        a, b = t[n], got
        if a.dtype == torch.float32:
            a, b = a.view(torch.int32), b.view(torch.int32)
        assert torch.equal(a, b), f"{n} differs from the call through ops"
