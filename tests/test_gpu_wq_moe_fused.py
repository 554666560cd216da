"""``qt_gemm_wq_grouped_act_mul`` / ``qt_moe_gemm_wq_wide_act_mul`` on the GPU: H bit for bit against SiLU(g) * u of
``qt_gemm_wq_grouped``'s two halves (and the wide form against the decode form) at the column, expert, k-block and
m-tile edges; one fp64 check per dtype; ``load_quantized(..., a16_experts_fused_act=True)`` against the unfused bank; the
raw ABI's refusals."""
import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_wq_linear import _bits_equal, _ref_w
from tests.test_gpu_wq_moe_wide import _bank, _offsets

pytestmark = pytest.mark.gpu

UNROLL = 4                                      # WQ_UNROLL of csrc/wq_stream_tile.h
# (I, K): the gate / up boundary inside the last column tile (8 live columns), two k-blocks (two idle waves); the
# expert boundary next to the tile, five k-blocks (uneven waves); one k-block past a full batch of every wave
SHAPES = [(40, 256), (16, 640), (40, 128 * (4 * UNROLL + 1))]
# (bits, zero-point, G = K / 128): int4 symmetric at both group counts, int4 with a zero-point, int8 channel-wise
SCHEMES = [(4, False, True), (4, False, False), (4, True, True), (8, False, False)]
# rows per expert -> the m-tiles the host picks.  {0, 1, 16, 17}: an empty expert, one row, a full slot, a second slot
# of one live row, and two surplus slots; the others: a ragged last tile and an expert of two slots at 2, 4 and 8 m-tiles
DECODE = [0, 1, 16, 17]
WIDE = [([0, 1, 40, 27], 2), ([70, 0, 33, 37], 4), ([130, 3], 8)]


def _case(dev, counts, I, K, bits, zp, grouped, dtype):
    """A gate_up bank [E, 2I, .], X and a top-2 style row_idx (every token twice) for sum(counts) routed rows."""
    E, R = len(counts), sum(counts)
    Wq, s, z, ts = _bank(dev, E, 2 * I, K, bits, zp, grouped, seed=I + K + bits)
    g = torch.Generator().manual_seed(R + K)
    X = torch.randn((R + 1) // 2, K, generator=g).to(dtype).to(dev)
    row_idx = (torch.randperm(R, generator=g) // 2).to(torch.int32).to(dev)
    return X, row_idx, _offsets(counts, dev), Wq, s, z, ts


def _unfused(ops, X, row_idx, off, Wq, s, z, K):
    Y = ops.gemm_wq_grouped(X, Wq, s, off, row_idx=row_idx, K=K, zp_w=z)
    I = Y.shape[1] // 2
    return F.silu(Y[:, :I]) * Y[:, I:]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("bits,zp,grouped", SCHEMES, ids=["w4-g128", "w4-chan", "w4-zp", "w8-chan"])
@pytest.mark.parametrize("I,K", SHAPES)
def test_both_forms_equal_the_unfused_composition(ops, dev, I, K, bits, zp, grouped, dtype):
    X, row_idx, (_, off), Wq, s, z, _ = _case(dev, DECODE, I, K, bits, zp, grouped, dtype)
    want = _unfused(ops, X, row_idx, off, Wq, s, z, K)
    H = ops.gemm_wq_grouped_act_mul(X, Wq, s, off, row_idx=row_idx, K=K, zp_w=z)
    assert H.shape == (sum(DECODE), I) and H.dtype == dtype
    _bits_equal(H, want)
    _bits_equal(ops.moe_gemm_wq_wide_act_mul(X, Wq, s, off, row_idx=row_idx, K=K, zp_w=z), want)


@pytest.mark.parametrize("bits,zp,grouped,dtype", [s + (d,) for s, d in zip(SCHEMES, [torch.bfloat16, torch.float16] * 2)],
                         ids=["w4-g128-bf16", "w4-chan-fp16", "w4-zp-bf16", "w8-chan-fp16"])
@pytest.mark.parametrize("counts,mt", WIDE, ids=["mt2", "mt4", "mt8"])
def test_wide_form_at_several_m_tiles(ops, dev, counts, mt, bits, zp, grouped, dtype):
    I, K = 40, 640
    assert ops.moe_wq_wide_mtiles(sum(counts), len(counts)) == mt
    X, row_idx, (_, off), Wq, s, z, _ = _case(dev, counts, I, K, bits, zp, grouped, dtype)
    H = ops.moe_gemm_wq_wide_act_mul(X, Wq, s, off, row_idx=row_idx, K=K, zp_w=z)
    _bits_equal(H, _unfused(ops, X, row_idx, off, Wq, s, z, K))
    _bits_equal(H, ops.gemm_wq_grouped_act_mul(X, Wq, s, off, row_idx=row_idx, K=K, zp_w=z))
    # without row_idx: routed row m reads X[m]
    Xr = X[row_idx.long()].contiguous()
    _bits_equal(ops.moe_gemm_wq_wide_act_mul(Xr, Wq, s, off, K=K, zp_w=z), H)
    _bits_equal(ops.gemm_wq_grouped_act_mul(Xr, Wq, s, off, K=K, zp_w=z), H)


@pytest.mark.parametrize("dtype,bits,zp", [(torch.bfloat16, 4, False), (torch.float16, 4, True)], ids=["bf16", "fp16"])
def test_fp64_bound(ops, dev, dtype, bits, zp):
    """|h - h64| <= 1.05 u (1.1 |g64 u64| + 3 |h64|) + 2^-22 (|u64| sum|x w_g| + sum|x w_u|) + the smallest subnormal,
    h64 = silu(g64) u64 from the dequantised bank in fp64, u the unit roundoff: one rounding each of g, u, SiLU's result
    and the product, |SiLU'| <= 1.1, and the fp32 sums.  Random inputs (no exactly summable generator here builds a packed
    bank), so the last term stays.  A 16-bit emulation of the unfused path on the CPU is held to the rounding terms
    first: if it left them, the bound would be wrong, not the kernel."""
    I, K = SHAPES[1]
    X, row_idx, (off_l, off), Wq, s, z, ts = _case(dev, DECODE, I, K, bits, zp, True, dtype)
    H = ops.gemm_wq_grouped_act_mul(X, Wq, s, off, row_idx=row_idx, K=K, zp_w=z).cpu().double()
    H2 = ops.moe_gemm_wq_wide_act_mul(X, Wq, s, off, row_idx=row_idx, K=K, zp_w=z).cpu().double()
    unit, tiny = (2.0 ** -8, 2.0 ** -133) if dtype == torch.bfloat16 else (2.0 ** -11, 2.0 ** -24)
    x = X.cpu().double()[row_idx.cpu().long()]
    for e in range(len(DECODE)):
        lo, hi = off_l[e], off_l[e + 1]
        w = _ref_w(ts[e], dtype).double()
        g64, u64 = x[lo:hi] @ w[:I].T, x[lo:hi] @ w[I:].T
        mag_g, mag_u = x[lo:hi].abs() @ w[:I].abs().T, x[lo:hi].abs() @ w[I:].abs().T
        h64 = F.silu(g64) * u64
        rounding = 1.05 * unit * (1.1 * (g64 * u64).abs() + 3 * h64.abs()) + tiny
        emulated = (F.silu(g64.to(dtype)) * u64.to(dtype)).double()
        assert ((emulated - h64).abs() <= rounding).all()
        bound = rounding + 2.0 ** -22 * (u64.abs() * mag_g + mag_u)
        for got in (H[lo:hi], H2[lo:hi]):
            err = (got - h64).abs()
            print(f"expert {e}: max err / bound {(err / bound).max().item() if hi > lo else 0.0:.3f}")
            assert (err <= bound).all()


def test_loaded_bank_equals_the_unfused_bank(ops, dev, tmp_path, monkeypatch):
    from quantool_amd.engine.qlinear import load_quantized
    from tests.test_moe_loader import BANK, _write

    _write(tmp_path, "W4A16")
    kw = dict(device=dev, a16="packed", a16_experts="packed")
    plain = load_quantized(tmp_path, **kw).get_submodule(BANK)
    fused = load_quantized(tmp_path, a16_experts_fused_act=True, **kw).get_submodule(BANK)
    assert fused.fused_act and not plain.fused_act
    calls = []
    for name in ("gemm_wq_grouped_act_mul", "moe_gemm_wq_wide_act_mul"):
        def counting(*a, _real=getattr(ops, name), _name=name, **k):
            calls.append(_name)
            return _real(*a, **k)
        monkeypatch.setattr(ops, name, counting)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for T in (3, 100):                      # the decode form; from wide_min_tokens = 96 the wide form
            x = torch.randn(T, plain.hidden_dim, generator=g).to(torch.bfloat16).to(dev)
            idx = torch.stack([torch.randperm(plain.num_experts, generator=g)[:2] for _ in range(T)]).to(dev)
            w = torch.softmax(torch.randn(T, 2, generator=g), -1).to(torch.bfloat16).to(dev)
            want = plain(x, idx, w)
            assert calls == []
            _bits_equal(fused(x, idx, w), want)
            assert calls == ["gemm_wq_grouped_act_mul" if T == 3 else "moe_gemm_wq_wide_act_mul"]
            del calls[:]


@pytest.mark.parametrize("name", ["qt_gemm_wq_grouped_act_mul", "qt_moe_gemm_wq_wide_act_mul"])
def test_raw_abi_refusals_launch_nothing(dev, name):
    from quantool_amd.hip import _lib

    E, I, K, R = 2, 16, 1024, 40
    Wq = torch.zeros(E, 2 * I, K, dtype=torch.int8, device=dev)
    xbuf = torch.zeros(R * K + 8, dtype=torch.bfloat16, device=dev)
    X, X_off = xbuf[:R * K].view(R, K), xbuf[1:1 + R * K].view(R, K)
    s = torch.ones(E, 2 * I, 8, device=dev)
    gi = torch.zeros(E, K, dtype=torch.int32, device=dev)
    off = torch.tensor([0, 17, R], dtype=torch.int32, device=dev)
    H = torch.full((R, I), 7.0, dtype=torch.bfloat16, device=dev)
    #        X, K, G, g_idx
    cases = {"g_idx": (X, K, 8, gi, "g_idx is not taken"), "K = 192": (X, 192, 1, None, "not a multiple of the k-unit"),
             "X shifted": (X_off, K, 1, None, "16-byte aligned"), "G = 3": (X, K, 3, None, "G must be 1 or K / 128 = 8")}

    def raw(Xa, Ka, G, g_idx):
        _lib.check(name, getattr(_lib.load(), name)(
            Xa.data_ptr(), _lib.QT_BF16, Ka, K, None, R, off.data_ptr(), E, Wq.data_ptr(), _lib.QT_W_INT8, I,
            s.data_ptr(), G, None, None if g_idx is None else g_idx.data_ptr(), H.data_ptr(), I, R,
            torch.cuda.current_stream().cuda_stream))

    for what, (*args, reason) in cases.items():
        with pytest.raises(_lib.HipBackendError, match=f"{name}: .*{reason}") as e:
            raw(*args)
        assert e.value.status == _lib.QT_ERR_INVALID, what
    torch.cuda.synchronize()
    assert (H == 7).all()
    raw(X, K, 8, None)                          # and the same call, accepted: SiLU(0) * 0
    torch.cuda.synchronize()
    assert (H == 0).all()
