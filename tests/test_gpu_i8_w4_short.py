"""qt_w4_short_gemm_i8 (R 3, L 2): bits of the tiled qt_gemm_i8, and fp64 within ``gemm_i8_tolerance`` with G groups."""
import numpy as np
import pytest
import torch

from tests import ckpt_reference as cr
from tests.test_gpu_i8_ring import _raw_ring
from tests.test_gpu_i8_ring_w4 import _case, _fold32
from tests.test_gpu_i8_skinny import _bias, _same_bits, _sentinel, _untouched
from tests.test_gpu_runtime_edges import _leaves, _levels, _qweight, cr_wsum

pytestmark = pytest.mark.gpu
NAME = "qt_w4_short_gemm_i8"


def _check(ops, c, asym, dt, bias, what):
    Xq, s_x, zp_x, y64, mag = c[asym]
    kw = dict(K=c["K"], zp_x=zp_x, wsum=c["wsum"] if asym else None, bias=bias, out_dtype=dt)
    want = ops.gemm_i8(Xq, s_x, c["Wq"], c["s_w"], **kw)
    got = ops.gemm_i8_w4_short(Xq, s_x, c["Wq"], c["s_w"], **kw)
    _same_bits(got, want, what)
    if bias is not None:
        b = bias.cpu().double()
        y64, mag = y64 + b, mag + b.abs()
    cr.assert_within(got, y64, cr.gemm_i8_tolerance(got.cpu(), mag, c["G"]), f"{what} vs fp64")


@pytest.mark.parametrize("tiles", range(1, 10))
def test_pipeline_depth(ops, dev, tiles):
    """K/128 from L - 1 = 1 to 2 R + 3 = 9: the prologue alone, no issue inside the loop, the first refill of a slot,
    up to three trips round the ring with every remainder; 2 x 2 ragged tiles.  Both template instances at every
    depth; the output type and the bias alternate with the depth and the instance."""
    M, N, K = 200, 130, 128 * tiles
    c = _case(ops, dev, M, N, K, seed=K)
    for asym in (False, True):
        dt = (torch.bfloat16, torch.float16)[(tiles + asym) % 2]
        bias = _bias(N, dt, dev, seed=N) if (tiles // 2 + asym) % 2 else None
        _check(ops, c, asym, dt, bias, f"K={K} asym={asym} {dt} bias={bias is not None}")


@pytest.mark.parametrize("M,N,K", [(129, 128, 640), (128, 129, 640), (257, 257, 640), (1024, 8448, 128)])
def test_edges_and_a_grid_larger_than_residency(ops, dev, M, N, K):
    """One row or column over a tile, both over two, and 8 x 66 = 528 tiles: more than the 512 resident workgroups."""
    c = _case(ops, dev, M, N, K, seed=M + N)
    _check(ops, c, True, torch.bfloat16, _bias(N, torch.bfloat16, dev, seed=M), f"M={M} N={N}")


def test_groups_are_folded_in_ascending_order(ops, dev):
    """5 groups, s_w = 2^u with u in [-8, 8] (five 17-bit terms over fewer binades leave most fp32 sums exact), one
    activation row repeated, bias[n] = -(the ascending fold of column n in fp16): y + bias is the fp32 residual, and the
    ascending and descending folds differ in over 1 % of the fp16 outputs (asserted on the CPU).  The kernel matches
    the ascending fold, and the tiled kernel, to the bit."""
    G, M, N = 5, 200, 384
    K = G * 128
    g = torch.Generator().manual_seed(1)
    q = torch.randint(-8, 8, (N, K), generator=g, dtype=torch.int8)
    Xq = torch.randint(-128, 128, (1, K), generator=g, dtype=torch.int8).repeat(M, 1).contiguous()
    s_w = torch.exp2(torch.randint(-8, 9, (N, G), generator=g).float())
    zp_x, s_x = torch.full((M,), 37, dtype=torch.int32), torch.full((M,), 0.0123, dtype=torch.float32)
    wsum = cr_wsum(q, G)
    xi, qi = Xq[:1].numpy().astype(np.int64), q.numpy().astype(np.int64)
    t = np.stack([xi[:, j * 128:(j + 1) * 128] @ qi[:, j * 128:(j + 1) * 128].T
                  - 37 * wsum[:, j].numpy().astype(np.int64)[None, :] for j in range(G)], 2)
    fold = lambda b, order: _fold32(t, s_w.numpy(), s_x[:1].numpy(), b, order)   # noqa: E731
    bias = -torch.from_numpy(fold(np.zeros(N, np.float32), range(G))[0]).to(torch.float16)
    asc = torch.from_numpy(fold(bias.float().numpy(), range(G))).to(torch.float16)
    desc = torch.from_numpy(fold(bias.float().numpy(), range(G - 1, -1, -1))).to(torch.float16)
    differ = (asc.view(torch.int16) != desc.view(torch.int16)).float().mean().item()
    assert differ >= 0.01, differ
    kw = dict(K=K, zp_x=zp_x.to(dev), wsum=wsum.to(dev), bias=bias.to(dev), out_dtype=torch.float16)
    args = (Xq.to(dev), s_x.to(dev), _qweight(_leaves(q, 4, G, seed=0), dev), s_w.to(dev))
    got = ops.gemm_i8_w4_short(*args, **kw)
    _same_bits(got, ops.gemm_i8(*args, **kw), "group order vs the tiled kernel")
    _same_bits(got.cpu(), asc.expand(M, N).contiguous(), "group order vs the ascending CPU fold")


@pytest.mark.parametrize("scales", ["unit", "g+1"])
def test_identity_activations_read_the_weight(ops, dev, scales):
    """Xq = identity: Y[m, n] = W[n, m] pins the nibble every A byte meets; s_w[n, g] = g + 1 pins the group of every k."""
    K, N, G = 4 * 128, 96, 4
    W = _levels((N, K), 4, seed=77)
    s_w = torch.ones(N, G) if scales == "unit" else (torch.arange(G).float() + 1).repeat(N, 1).contiguous()
    want = W.T.float() * (1.0 if scales == "unit" else (torch.arange(K) // 128 + 1).float()[:, None])
    Y = ops.gemm_i8_w4_short(torch.eye(K, dtype=torch.int8, device=dev), torch.ones(K, device=dev),
                             _qweight(_leaves(W, 4, G, seed=1), dev), s_w.to(dev), K=K, out_dtype=torch.float16)
    _same_bits(Y.cpu(), want.to(torch.float16).contiguous(), f"identity, {scales} scales")


def test_caller_owned_y_keeps_its_padding(ops, dev):
    from quantool_amd.hip import _lib

    M, N, K = 200, 130, 4 * 128
    ldy = N + 17
    c = _case(ops, dev, M, N, K, seed=4)
    Xq, s_x, zp_x, _, _ = c[True]
    bias, Ys = _bias(N, torch.bfloat16, dev, seed=5), {}
    for name in ("qt_gemm_i8", NAME):
        Ys[name] = _sentinel((M + 3, ldy), torch.bfloat16, dev)
        _raw_ring(ops, Xq.data_ptr(), M, K, c["Wq"].data_ptr(), _lib.QT_W_INT4_PACKED, N, s_x, zp_x, c["s_w"], c["G"],
                  c["wsum"], bias, Ys[name], ldy, name=name)
    torch.cuda.synchronize()
    assert _untouched(Ys[NAME][:, N:]) and _untouched(Ys[NAME][M:]) and not _untouched(Ys[NAME][:M, :N])
    _same_bits(Ys[NAME][:M, :N].contiguous(), Ys["qt_gemm_i8"][:M, :N].contiguous(), "ldy > N")


def test_module_is_the_same_with_and_without_it(ops, dev, tmp_path, monkeypatch):
    """A tiny Llama W4A8 checkpoint (2 and 4 groups) at 1 x 200 tokens: loaded with ``a8_w4_short_min_m=129`` every
    Linear runs the new kernel and the logits equal the default load's to the bit."""
    import quantool_amd.methods  # noqa: F401
    from quantool_amd.core import QuantizerRegistry
    from quantool_amd.engine.qlinear import load_quantized
    from transformers import LlamaConfig, LlamaForCausalLM

    monkeypatch.chdir(tmp_path)
    cfg = LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, vocab_size=512, max_position_embeddings=256, tie_word_embeddings=False)
    torch.manual_seed(0)
    dense = LlamaForCausalLM(cfg).to(torch.bfloat16).to(dev)
    g = torch.Generator().manual_seed(2)
    data = [{"input_ids": torch.randint(0, 512, (48,), generator=g)} for _ in range(8)]
    q = QuantizerRegistry.create("smoothquant", model_id="synthetic/tiny-llama")
    q.quantize(model=dense, level="W4A8", dataset=data, num_calibration_samples=8, max_seq_length=64,
               shuffle_calibration_samples=False)
    q.save_pretrained(str(tmp_path / "ckpt"))
    calls = []
    real = ops.gemm_i8_w4_short
    monkeypatch.setattr(ops, "gemm_i8_w4_short", lambda *a, **kw: calls.append(a[0].shape[0]) or real(*a, **kw))
    ids = torch.randint(0, 512, (1, 200), generator=torch.Generator().manual_seed(11)).to(dev)
    logits, used = {}, {}
    for min_m in (0, 129):
        model = load_quantized(tmp_path / "ckpt", device=dev, a8_w4_short_min_m=min_m)
        with torch.no_grad():
            logits[min_m] = model(input_ids=ids).logits
        used[min_m], calls[:] = list(calls), []
    assert used[0] == [] and used[129] == [200] * 14
    _same_bits(logits[129], logits[0], "W4A8 logits, a8_w4_short_min_m 129 vs 0")
