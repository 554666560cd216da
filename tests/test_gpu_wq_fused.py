"""The fused A16 decode forms on the GPU: ``qt_gemm_wq_skinny_act_mul`` against the dequantised weights
(one-hot rows), against fp64 (exact inputs) and against the composition it replaces; ``qt_gemm_wq_skinny_multi``
against separate skinny launches and the header's fp64 bound; ``qt_rmsnorm`` against ``qt_rmsnorm_quantize_i8``; the
raw ABI's refusals; and ``load_quantized(..., a16_fused_act / a16_fused_norm)`` end to end on a tiny Llama."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_qlinear import _eval_ids, _quantize_and_save
from tests.test_gpu_wq_linear import _check_bound, _dev_args, _greedy_logits, _ref_w, _weight

pytestmark = pytest.mark.gpu

BF, HF = torch.bfloat16, torch.float16
# (M, k-blocks, I or N, bits, zero-point, grouped, dtype): every M with every k-block count (1: three waves have no
# block; 5: ragged batches; 33: one block past two full batches), the column counts so that the last tile is full, has
# one column, or half; formats, zero-points, grouping and dtypes cycled over the cells
CELLS = [(1, 1, 16, 4, False, True, BF), (1, 5, 17, 8, True, False, HF), (1, 33, 40, 4, True, True, HF),
         (7, 1, 17, 8, False, True, HF), (7, 5, 40, 4, True, False, BF), (7, 33, 16, 8, False, False, BF),
         (16, 1, 40, 8, True, True, BF), (16, 5, 16, 4, False, False, HF), (16, 33, 17, 4, False, True, BF)]


def _bits(t):
    return t.contiguous().view(torch.int16)


def _x(M, K, dtype, dev, seed):
    return (torch.randn(M, K, generator=torch.Generator().manual_seed(seed)) * 0.5).to(dtype).to(dev)


def _pair(I, K, bits, zp, grouped, dev, seed, **kw):
    """(gate, up): each ((Wq, s_w, zp_w) on the device, its checkpoint leaves)."""
    out = []
    for i in range(2):
        t, _ = _weight(I, K, bits, zp=zp, grouped=grouped, seed=seed + i, **kw)
        out.append((_dev_args(t, dev)[:3], t))
    return out


@pytest.mark.parametrize("dtype", [BF, HF])
@pytest.mark.parametrize("bits,zp", [(4, False), (4, True), (8, False)])
def test_act_mul_one_hot_rows_read_both_weights(ops, dev, dtype, bits, zp):
    I, K = 33, 384
    (g, tg), (u, tu) = _pair(I, K, bits, zp, True, dev, seed=bits + zp)
    Wg, Wu = (_ref_w(t, dtype).to(dev).t().contiguous() for t in (tg, tu))            # [K, I]
    for M in (1, 7, 16):
        rows = torch.arange(M, device=dev)
        for off in range(0, 130):                                         # a whole k-block and the block boundary
            X = torch.zeros(M, K, dtype=dtype, device=dev)
            X[rows, off + rows] = 1
            H = ops.gemm_wq_skinny_act_mul(X, g, u)
            assert torch.equal(_bits(H), _bits(F.silu(Wg[off:off + M]) * Wu[off:off + M])), (M, off)


# |x| <= 4, |q - zp| <= 16 (int4) or 136 (int8), scales 2^0 .. 2^-4: every partial sum is a multiple of 2^-4 below 2^20
# (int4, K <= 4096; int8, K <= 1024), so exact in fp32 (test_gpu_wq_stream.py's argument): g and u are the fp64
# products rounded once
@pytest.mark.parametrize("dtype", [BF, HF])
@pytest.mark.parametrize("bits,zp,I,K", [(4, False, 40, 4096), (4, True, 17, 640), (8, True, 40, 1024), (8, False, 17, 640)])
def test_act_mul_exact_inputs_bit_exact(ops, dev, dtype, bits, zp, I, K):
    (g, tg), (u, tu) = _pair(I, K, bits, zp, True, dev, seed=3 * I + K, pow2_scales=True)
    Wg, Wu = (_ref_w(t, dtype).double() for t in (tg, tu))
    gen = torch.Generator().manual_seed(K)
    for M in (1, 7, 16):
        X = torch.randint(-4, 5, (M, K), generator=gen).to(dtype)
        gr, ur = (((X.double() @ W.T) + 0.0).to(dtype).to(dev) for W in (Wg, Wu))     # the kernel sums from +0
        H = ops.gemm_wq_skinny_act_mul(X.to(dev), g, u)
        assert torch.equal(_bits(H), _bits(F.silu(gr) * ur)), M


@pytest.mark.parametrize("M,kbs,I,bits,zp,grouped,dtype", CELLS)
def test_act_mul_equals_the_composition(ops, dev, M, kbs, I, bits, zp, grouped, dtype):
    K = 128 * kbs
    (g, _), (u, _) = _pair(I, K, bits, zp, grouped, dev, seed=M + kbs)
    X = _x(M, K, dtype, dev, seed=I)
    want = F.silu(ops.gemm_wq_skinny(X, g[0], g[1], zp_w=g[2])) * ops.gemm_wq_skinny(X, u[0], u[1], zp_w=u[2])
    H = ops.gemm_wq_skinny_act_mul(X, g, u)
    assert H.shape == (M, I) and H.dtype == dtype and torch.equal(_bits(H), _bits(want))
    assert torch.equal(_bits(ops.gemm_wq_skinny_act_mul(X, g, u)), _bits(H))          # two runs, the same bits


@pytest.mark.parametrize("M,kbs,N,bits,zp,grouped,dtype", CELLS)
def test_multi_equals_separate_launches_and_the_fp64_bound(ops, dev, M, kbs, N, bits, zp, grouped, dtype):
    K = 128 * kbs
    Ns = (N, 16 + N, 3 * N + 1, 5)                                        # the fourth: fewer columns than a tile
    X = _x(M, K, dtype, dev, seed=N)
    ts = [_weight(n, K, bits, zp=zp, grouped=grouped, seed=n)[0] for n in Ns]
    bias = (torch.randn(Ns[1], generator=torch.Generator().manual_seed(1)) * 0.1).to(dtype).to(dev)
    ws = [(*_dev_args(t, dev)[:3], bias if i == 1 else None) for i, t in enumerate(ts)]
    for count in (3, 4):
        Ys = ops.gemm_wq_skinny_multi(X, ws[:count])
        again = ops.gemm_wq_skinny_multi(X, ws[:count])
        assert len(Ys) == count
        for (Wq, s, z, b), t, Y, Y2 in zip(ws, ts, Ys, again):
            assert torch.equal(_bits(Y), _bits(ops.gemm_wq_skinny(X, Wq, s, zp_w=z, bias=b)))
            assert torch.equal(_bits(Y), _bits(Y2))
            _check_bound(Y, X, _ref_w(t, dtype), b)


@pytest.mark.parametrize("dtype", [BF, HF])
@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("K", [8, 136, 4096, 4100])
def test_rmsnorm_is_the_quantising_kernels_y(ops, dev, dtype, M, K):
    gen = torch.Generator().manual_seed(K + M)
    wide = (torch.randn(M, K + 24, generator=gen) * 3).to(dtype).to(dev)
    w = (1 + 0.1 * torch.randn(K, generator=gen)).to(dtype).to(dev)
    for X in (wide[:, :K].contiguous(), wide[:, 8:8 + K], wide[:, 1:1 + K]):          # dense, pitched, misaligned
        Yq, _, _, _, rq = ops.rmsnorm_quantize_i8(X, w, 1e-5, return_rstd=True)
        Y, r = ops.rmsnorm(X, w, 1e-5, return_rstd=True)
        assert torch.equal(_bits(Y), _bits(Yq)) and torch.equal(r, rq)
        assert torch.equal(_bits(ops.rmsnorm(X, w, 1e-5)), _bits(Yq))


def test_raw_abi_refusals_launch_nothing(ops, dev):
    from quantool_amd.hip import _lib
    from quantool_amd.hip._lib import QT_BF16, QT_ERR_INVALID, QT_W_INT4_PACKED, QT_W_INT8, HipBackendError, WqWeight

    N, K = 32, 1024
    wbuf = torch.zeros(N * K + 16, dtype=torch.int8, device=dev)
    Wq, Wq_off = wbuf[:N * K].view(N, K), wbuf[4:4 + N * K].view(N, K)
    W4 = torch.zeros(N, K // 8, dtype=torch.int32, device=dev)
    xbuf = torch.zeros(17 * K + 8, dtype=torch.bfloat16, device=dev)
    X, X_off = xbuf[:17 * K].view(17, K), xbuf[1:1 + 16 * K].view(16, K)
    s, zp = torch.ones(N, 8, device=dev), torch.zeros(N, 8, dtype=torch.int8, device=dev)
    gi = torch.zeros(K, dtype=torch.int32, device=dev)
    out = torch.full((3, 17, N), 7.0, dtype=torch.bfloat16, device=dev)
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream

    def weight(Wq=Wq, fmt=QT_W_INT8, G=8, zp=None, g_idx=None, Y=None):
        p = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        return WqWeight(p(Wq), fmt, N, s.data_ptr(), G, p(zp), p(g_idx), None, p(Y), N)

    def act_mul(x=X, M=16, k=K, gate=None, up=None):
        g, u = gate or weight(), up or weight()
        return lib.qt_gemm_wq_skinny_act_mul(x.data_ptr(), QT_BF16, M, k, K, ctypes.byref(g), ctypes.byref(u), 0,
                                             out[0].data_ptr(), N, stream)

    def multi(x=X, M=16, k=K, **second):
        table = (WqWeight * 2)(weight(Y=out[1]), weight(Y=out[2], **second))
        return lib.qt_gemm_wq_skinny_multi(x.data_ptr(), QT_BF16, M, k, K, table, 2, stream)

    for call, second in ((act_mul, "up"), (multi, None)):
        kw = (lambda **w: {second: weight(**w)}) if second else (lambda **w: w)
        cases = {"g_idx": (kw(g_idx=gi), "g_idx is not taken"),
                 "K = 130": ({"k": 130}, "not a multiple of the k-unit"),
                 "M = 17": ({"M": 17}, "1 <= M <= 16"),
                 "mixed formats": (kw(Wq=W4, fmt=QT_W_INT4_PACKED), "in format"),
                 "mixed G": (kw(G=1), "in format"),
                 "mixed zero-points": (kw(zp=zp), "in format"),
                 "X shifted": ({"x": X_off}, "16-byte aligned"),
                 "Wq shifted": (kw(Wq=Wq_off), "16-byte aligned")}
        for what, (args, reason) in cases.items():
            with pytest.raises(HipBackendError, match=reason) as e:
                _lib.check(what, call(**args))
            assert e.value.status == QT_ERR_INVALID, what
    torch.cuda.synchronize()
    assert (out == 7).all()
    assert act_mul() == 0 and multi() == 0                                 # and the same calls, accepted
    assert (out[:, :16] == 0).all() and (out[:, 16:] == 7).all()


def test_end_to_end_fused_flags(ops, dev, tmp_path, monkeypatch):
    from quantool_amd.engine.qlinear import SharedOutputs, WeightOnlyMLP, WeightOnlyRMSNorm, load_quantized

    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(SharedOutputs, "max_m", 16)               # the hand-off under test, whatever the measured bound
    ckpt = tmp_path / "ckpt"
    _quantize_and_save("gptq", "W4A16", dev, ckpt)
    plain = load_quantized(ckpt, device=dev, a16="packed")
    act = load_quantized(ckpt, device=dev, a16="packed", a16_fused_act=True)
    norm = load_quantized(ckpt, device=dev, a16="packed", a16_fused_norm=True)
    assert list(act.state_dict()) == list(norm.state_dict()) == list(plain.state_dict())
    assert sum(isinstance(m, WeightOnlyMLP) for m in act.modules()) == 2
    norms = {n: m for n, m in norm.named_modules() if isinstance(m, WeightOnlyRMSNorm)}
    assert len(norms) == 4 and act._qt_checkpoint["a16_fused_act"] and norm._qt_checkpoint["a16_fused_norm"]

    calls = {"act_mul": 0, "multi": 0}
    for name in calls:
        def counting(*a, _real=getattr(ops, f"gemm_wq_skinny_{name}"), _name=name, **k):
            calls[_name] += 1
            return _real(*a, **k)
        monkeypatch.setattr(ops, f"gemm_wq_skinny_{name}", counting)
    with torch.no_grad():
        for rows in (1, 16):                                              # one decode step of `rows` sequences
            ids = _eval_ids()[:1, :rows].reshape(rows, 1).to(dev)
            assert torch.equal(act(input_ids=ids).logits, plain(input_ids=ids).logits), rows
        assert calls == {"act_mul": 4, "multi": 4}                        # two layers, two forwards
        shared = {id(m.outputs_from): m.outputs_from for m in act.modules() if getattr(m, "outputs_from", None)}
        assert len(shared) == 2 and not any(s.holds_tensors for s in shared.values())

        seen = []
        hooks = [m.register_forward_hook(lambda mod, inp, out: seen.append((mod, inp[0], out))) for m in norms.values()]
        prompt = _eval_ids()[:1, :24].to(dev)
        ref, toks = _greedy_logits(plain, prompt, 8)
        got, toks_norm = _greedy_logits(norm, prompt, 8)
        for h in hooks:
            h.remove()
    assert len(seen) == 4 * 9
    for mod, x, y in seen:
        K = x.shape[-1]
        Yq = ops.rmsnorm_quantize_i8(x.reshape(-1, K), mod.weight, mod.variance_epsilon)[0]
        assert torch.equal(_bits(y), _bits(Yq.reshape(y.shape)))
    # the kernel's sum over K runs in its own order: tokens agree up to the first near-tie (reported, as decode_bench's
    # tokens_agree is; DESIGN.md 4.21 asserts finite logits and nothing about the tokens)
    agree = 0
    for a, b in zip(toks, toks_norm):
        if not torch.equal(a, b):
            break
        agree += 1
    print(f"tokens_agree {agree} of {len(toks)}; logits max abs diff {(got - ref).abs().max().item():.4g}")
    assert torch.isfinite(got).all()
