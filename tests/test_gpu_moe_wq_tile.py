"""``qt_moe_gemm_wq_tile`` on the GPU: every expert's rows bit for bit against ``qt_gemm_wq_tile`` on the gathered rows and
inside the fp64 bound, a caller-owned pitched Y with markers, the identity gather, an ``offsets`` table that must not be
trusted, the raw ABI's refusals, and ``WeightOnlyExperts`` with ``tile_max_tokens`` against the fp64 routed MLP."""
import pytest
import torch

from tests.test_gpu_moe import _random_routing
from tests.test_gpu_wq_experts import _acts, _experts
from tests.test_gpu_wq_linear import _bits_equal, _check_bound, _dev_args, _ref_w, _weight

pytestmark = pytest.mark.gpu

COUNTS = (129, 0, 1, 128)       # a slot pair whose second tile has one row, an empty expert, one row, a full tile
OFF = (0, 129, 129, 130, 258)
R, X_ROWS = 258, 300
BF, HF = torch.bfloat16, torch.float16
#        N    K    bits zp     grouped dtype     N: a ragged second column tile; K: two K-tiles (prologue and drain only)
CASES = [(129, 128, 4, False, True, BF),        # and ten (every ring slot and both images reused)
         (200, 640, 4, True, True, HF),
         (129, 640, 8, False, False, HF),
         (200, 128, 8, True, True, BF),
         (200, 640, 4, False, False, BF),
         (129, 640, 8, True, False, BF)]


def _bank(dev, N, K, bits, zp, grouped):
    """(Wq [E, N, .], s_w [E, N, G], zp_w or None, the checkpoint leaves per expert) from four seeded weights."""
    ts = [_weight(N, K, bits, zp=zp, grouped=grouped, seed=N + K + 5 * e)[0] for e in range(len(COUNTS))]
    per = [_dev_args(t, dev) for t in ts]
    return (torch.stack([p[0] for p in per]), torch.stack([p[1] for p in per]),
            torch.stack([p[2] for p in per]) if zp else None, ts)


def _gather(dev, K, dtype):
    g = torch.Generator().manual_seed(K)
    row_idx = torch.randint(0, X_ROWS, (R,), generator=g).to(torch.int32)      # permuted, with repeats
    return _acts(X_ROWS, K, dtype, dev, seed=K + 1), row_idx.to(dev)


def _raw(X, code, K, ldx, row_idx, R_, off, E, Wq, fmt, N, s, G, zp, g_idx, Y, ldy, x_rows):
    from quantool_amd.hip import _lib

    p = lambda v: None if v is None else v.data_ptr()       # noqa: E731
    _lib.check("qt_moe_gemm_wq_tile", _lib.load().qt_moe_gemm_wq_tile(
        p(X), code, K, ldx, p(row_idx), R_, p(off), E, p(Wq), fmt, N, p(s), G, p(zp), p(g_idx), p(Y), ldy, x_rows,
        torch.cuda.current_stream().cuda_stream))


def _into_marked_y(X, row_idx, off, Wq, s, z, N, K):
    """The raw call into a Y of R + 3 rows and pitch N + 20 pre-filled with 7: (the buffer, its [R + 3, N + 20] view)."""
    from quantool_amd.hip import _lib

    ldy, rows = N + 20, R + 3
    buf = torch.full((rows * ldy + 64,), 7.0, dtype=X.dtype, device=X.device)
    fmt = _lib.QT_W_INT4_PACKED if Wq.dtype == torch.int32 else _lib.QT_W_INT8
    _raw(X, _lib.QT_BF16 if X.dtype == BF else _lib.QT_F16, K, X.stride(0), row_idx, R, off, Wq.shape[0], Wq, fmt, N, s,
         s.shape[2], z, None, buf, ldy, X.shape[0])
    torch.cuda.synchronize()
    return buf, buf[:rows * ldy].view(rows, ldy)


@pytest.mark.parametrize("N,K,bits,zp,grouped,dtype", CASES)
def test_rows_equal_the_dense_tile_and_hold_the_fp64_bound(ops, dev, N, K, bits, zp, grouped, dtype):
    Wq, s, z, ts = _bank(dev, N, K, bits, zp, grouped)
    X, row_idx = _gather(dev, K, dtype)
    off = torch.tensor(OFF, dtype=torch.int32, device=dev)
    buf, grid = _into_marked_y(X, row_idx, off, Wq, s, z, N, K)
    _bits_equal(_into_marked_y(X, row_idx, off, Wq, s, z, N, K)[0], buf)               # two runs, the same bits
    assert (grid[:R, N:] == 7).all() and (grid[R:] == 7).all() and (buf[grid.numel():] == 7).all()
    _bits_equal(ops.moe_gemm_wq_tile(X, Wq, s, off, row_idx=row_idx, zp_w=z), grid[:R, :N].contiguous())
    for e, count in enumerate(COUNTS):
        if count:
            lo, hi = OFF[e], OFF[e + 1]
            rows = X[row_idx[lo:hi].long()]
            Y = grid[lo:hi, :N].contiguous()
            _bits_equal(Y, ops.gemm_wq_tile(rows, Wq[e], s[e], zp_w=None if z is None else z[e]))
            _check_bound(Y, rows, _ref_w(ts[e], dtype))


def test_identity_gather_and_untrusted_offsets(ops, dev):
    N, K, bits, zp, grouped, dtype = CASES[1]
    Wq, s, z, _ = _bank(dev, N, K, bits, zp, grouped)
    X, row_idx = _gather(dev, K, dtype)
    off = torch.tensor(OFF, dtype=torch.int32, device=dev)
    want = ops.moe_gemm_wq_tile(X, Wq, s, off, row_idx=row_idx, zp_w=z)
    _bits_equal(ops.moe_gemm_wq_tile(X[row_idx.long()].contiguous(), Wq, s, off, zp_w=z), want)
    # a descending entry and an entry past R: clamped into [0, R] and made ascending, not followed; and row_idx values
    # outside X's rows are clamped likewise
    bad = torch.tensor((0, 200, 100, 400, R), dtype=torch.int32, device=dev)
    wild = row_idx.clone()
    wild[::7] = X_ROWS + 1000
    wild[3::7] = -5
    buf, grid = _into_marked_y(X, wild, bad, Wq, s, z, N, K)
    assert (grid[:R, N:] == 7).all() and (grid[R:] == 7).all() and (buf[grid.numel():] == 7).all()
    assert torch.isfinite(grid[:R, :N].float()).all()


def test_raw_abi_refusals_launch_nothing(ops, dev):
    from quantool_amd.hip._lib import QT_BF16, QT_ERR_INVALID, QT_F32, QT_W_INT8, HipBackendError

    E, N, K, R_ = 2, 32, 1024, 40
    Wq = torch.zeros(E, N, K, dtype=torch.int8, device=dev)
    xbuf = torch.zeros(R_ * K + 8, dtype=BF, device=dev)
    X, X_off = xbuf[:R_ * K].view(R_, K), xbuf[1:1 + R_ * K].view(R_, K)
    s = torch.ones(E, N, 8, device=dev)
    gi = torch.zeros(E, K, dtype=torch.int32, device=dev)
    off = torch.tensor([0, 17, R_], dtype=torch.int32, device=dev)
    Y = torch.full((R_, N), 7.0, dtype=BF, device=dev)
    i8, bf = QT_W_INT8, QT_BF16
    #       0  1     2  3    4        5   6        7  8   9    10 11   12 13  14     15 16   17
    base = [X, bf, K, K, None, R_, off, E, Wq, i8, N, s, 1, None, None, Y, N, R_]      # ..., G, zp, g_idx, Y, ldy, x_rows
    cases = {"g_idx": ({12: 8, 14: gi}, "g_idx is not taken"), "K = 192": ({2: 192}, "not a multiple of the k-unit"),
             "X shifted": ({0: X_off}, "16-byte aligned"), "G = 3": ({12: 3}, "G must be 1 or K / 128 = 8"),
             "fp32 X": ({1: QT_F32}, "must be bf16 or fp16"),
             # x_rows ldx 2 = 2^32 (a row_idx pointer that is never read: refused first)
             "2^32 bytes": ({4: off, 17: (1 << 32) // (2 * K)}, "2\\^32"),
             "E past the limit": ({7: ops.MOE_WQ_TILE_MAX_E + 1}, "bad sizes")}
    for what, (change, reason) in cases.items():
        with pytest.raises(HipBackendError, match=reason) as e:
            _raw(*[change.get(i, v) for i, v in enumerate(base)])
        assert e.value.status == QT_ERR_INVALID, what
    torch.cuda.synchronize()
    assert (Y == 7).all()
    _raw(*[8 if i == 12 else v for i, v in enumerate(base)])                            # and the same call, accepted
    torch.cuda.synchronize()
    assert (Y == 0).all()


def _mlp64(ref, x, idx, w):
    """The routed MLP of the dense bank ``ref`` in fp64 on the CPU."""
    x, w, idx = x.cpu().double(), w.cpu().double(), idx.cpu()
    out = torch.zeros_like(x)
    for e in range(ref.gate_up_proj.shape[0]):
        tok, pos = torch.where(idx == e)
        gate, up = (x[tok] @ ref.gate_up_proj[e].cpu().double().T).chunk(2, dim=-1)
        out.index_add_(0, tok, (torch.nn.functional.silu(gate) * up) @ ref.down_proj[e].cpu().double().T * w[tok, pos, None])
    return out


@pytest.mark.parametrize("bits,zp", [(4, True), (8, False)])
def test_module_runs_the_tile_range_when_asked(ops, dev, monkeypatch, bits, zp):
    """Both paths against the fp64 routed MLP: inside 2^-4 of the output scale (the end-to-end tests' bound), the new one
    no further than twice the dequantise path's own distance plus one bf16 ulp; neither is the other's reference."""
    T, k = 200, 2
    woe, ref = _experts(dev, 4, 256, 384, bits, zp, False, seed=bits + 2)
    x = _acts(T, woe.hidden_dim, BF, dev, seed=T)
    idx = _random_routing(T, k, woe.num_experts, seed=T + 1).to(dev)
    w = torch.softmax(torch.randn(T, k, generator=torch.Generator().manual_seed(T)), -1).to(BF).to(dev)
    calls = []
    real = ops.moe_gemm_wq_tile
    monkeypatch.setattr(ops, "moe_gemm_wq_tile", lambda *a, **kw: calls.append(a[0].shape[0]) or real(*a, **kw))
    with torch.no_grad():
        dequantised = woe(x, idx, w)
        assert calls == [] and "tile_max_tokens=0" in repr(woe)
        woe.tile_max_tokens = 256
        got = woe(x, idx, w)
        assert calls == [T, T * k]                      # gate_up on the tokens it gathers, down on the routed rows
        woe.tile_max_tokens = T - 1
        _bits_equal(woe(x, idx, w), dequantised)        # past the range: the dequantise path again
    want = _mlp64(ref, x, idx, w)
    scale = want.abs().max().item()
    d_deq = (dequantised.cpu().double() - want).abs().max().item()
    d_new = (got.cpu().double() - want).abs().max().item()
    ulp = 2.0 ** (torch.tensor(scale).log2().floor().item() - 7)
    print(f"bits={bits} zp={zp}: scale {scale:.4g}, dequantise path {d_deq:.4g}, tile path {d_new:.4g}, ulp {ulp:.4g}")
    assert d_deq <= 2.0 ** -4 * scale and d_new <= 2.0 ** -4 * scale
    assert d_new <= 2 * d_deq + ulp
