"""Packed A16 expert banks on the GPU: ``qt_gemm_wq_grouped`` bit for bit against per-expert ``qt_gemm_wq_skinny``,
``WeightOnlyExperts`` on both of its paths against a torch restatement and the dense bank, no host sync at decode, and
``load_quantized(..., a16="packed", a16_experts="packed")`` end to end on a tiny Mixtral."""
import math

import pytest
import torch

from tests.test_gpu_moe import _random_routing, ref_combine
from tests.test_gpu_wq_linear import _bits_equal, _greedy_logits, _weight

pytestmark = pytest.mark.gpu


def _bank(dev, E, N, K, bits, zp, g_idx, seed):
    """(Wq [E, N, .], s_w [E, N, G], zp_w [E, N, G] or None, g_idx [E, K] or None) on ``dev``, experts all different."""
    ts = [_weight(N, K, bits, zp=zp, g_idx=g_idx, seed=seed + 7 * e)[0] for e in range(E)]
    leaf = "weight_packed" if bits == 4 else "weight"
    Wq = torch.stack([t[leaf] for t in ts]).to(dev)
    s = torch.stack([t["weight_scale"] for t in ts]).to(dev)
    z = torch.stack([t["weight_zero_point"] for t in ts]).to(dev) if zp else None
    gi = torch.stack([t["weight_g_idx"] for t in ts]).to(dev) if g_idx else None
    return Wq, s, z, gi


def _acts(M, K, dtype, dev, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(M, K, generator=g).to(dtype).to(dev)


def _per_expert(ops, X, src, off, Wq, s, zp, gi):
    """Per-expert ``gemm_wq_skinny`` on each expert's gathered rows, 16 rows at a time: [(lo, hi, Y rows)]."""
    out = []
    for e in range(len(off) - 1):
        for lo in range(off[e], off[e + 1], 16):
            hi = min(lo + 16, off[e + 1])
            rows = X[src[lo:hi]].contiguous()
            out.append((lo, hi, ops.gemm_wq_skinny(rows, Wq[e], s[e], zp_w=None if zp is None else zp[e],
                                                   g_idx=None if gi is None else gi[e])))
    return out


def _raw_grouped(X, Wq, s, off, K, row_idx, zp, gi, Y):
    """``qt_gemm_wq_grouped`` into a caller's Y (the wrapper allocates its own)."""
    from quantool_amd.hip import _lib, ops

    fmt = _lib.QT_W_INT4_PACKED if Wq.dtype == torch.int32 else _lib.QT_W_INT8
    R = row_idx.numel() if row_idx is not None else X.shape[0]
    _lib.check("qt_gemm_wq_grouped", _lib.load().qt_gemm_wq_grouped(
        X.data_ptr(), ops._dtype_code(X), K, X.stride(0), ops._ptr(row_idx), R, off.data_ptr(), Wq.shape[0],
        Wq.data_ptr(), fmt, Wq.shape[1], s.data_ptr(), s.shape[2], ops._ptr(zp), ops._ptr(gi), Y.data_ptr(),
        Y.stride(0), ops._stream()))


# ---- qt_gemm_wq_grouped ---------------------------------------------------------------------------------------------
GROUPED_CASES = [
    # E, rows per expert (17 and 33 span several row tiles), N, K
    (1, [33], 80, 1024),
    (4, [17, 0, 1, 33], 96, 520),             # K off 128 and off the 16-byte path
    (8, [0, 17, 2, 0, 33, 16, 1, 0], 48, 1056),
]


@pytest.mark.parametrize("E,counts,N,K", GROUPED_CASES)
@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("zp,g_idx", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("gather", [True, False])
def test_grouped_equals_per_expert_skinny(ops, dev, E, counts, N, K, bits, zp, g_idx, dtype, gather):
    seed = sum(counts) + K + bits
    Wq, s, z, gi = _bank(dev, E, N, K, bits, zp, g_idx, seed)
    off_l = [0]
    for c in counts:
        off_l.append(off_l[-1] + c)
    off = torch.tensor(off_l, dtype=torch.int32, device=dev)
    R = off_l[-1]
    if gather:
        T = 40
        X = _acts(T, K, dtype, dev, seed)
        row_idx = torch.randint(0, T, (R,), generator=torch.Generator().manual_seed(seed)).to(torch.int32).to(dev)
        Y = ops.gemm_wq_grouped(X, Wq, s, off, row_idx=row_idx, K=K, zp_w=z, g_idx=gi)
        src = row_idx.long()
    else:
        X = _acts(R, K, dtype, dev, seed)
        Y = ops.gemm_wq_grouped(X, Wq, s, off, K=K, zp_w=z, g_idx=gi)
        src = torch.arange(R, device=dev)
    assert Y.shape == (R, N) and Y.dtype == dtype
    for lo, hi, want in _per_expert(ops, X, src, off_l, Wq, s, z, gi):
        torch.cuda.synchronize()
        _bits_equal(Y[lo:hi], want)


@pytest.mark.parametrize("bits,zp,g_idx", [(4, False, False), (8, True, True)])
def test_grouped_is_deterministic_and_leaves_rows_past_the_routed_ones(ops, dev, bits, zp, g_idx):
    E, N, K, T = 4, 72, 1024, 24
    Wq, s, z, gi = _bank(dev, E, N, K, bits, zp, g_idx, seed=5)
    off = torch.tensor([0, 3, 3, 20, 21], dtype=torch.int32, device=dev)
    R = 30                                                   # rows [21, 30) belong to no expert
    X = _acts(T, K, torch.bfloat16, dev, seed=6)
    row_idx = torch.randint(0, T, (R,), generator=torch.Generator().manual_seed(7)).to(torch.int32).to(dev)
    runs = []
    for _ in range(2):
        Y = torch.full((R, N), float("nan"), dtype=torch.bfloat16, device=dev)
        _raw_grouped(X, Wq, s, off, K, row_idx, z, gi, Y)
        runs.append(Y)
    torch.cuda.synchronize()
    _bits_equal(runs[0], runs[1])
    assert torch.isnan(runs[0][21:].float()).all()
    assert torch.isfinite(runs[0][:21].float()).all()
    _bits_equal(runs[0][:21], ops.gemm_wq_grouped(X, Wq, s, off, row_idx=row_idx, K=K, zp_w=z, g_idx=gi)[:21])


@pytest.mark.parametrize("N,K", [(28672, 4096), (4096, 14336)])
@pytest.mark.parametrize("T", [1, 16])
def test_grouped_mixtral_shapes(ops, dev, N, K, T):
    """Mixtral-8x7B's gate_up (2 x 14336 rows over 4096) and down (4096 over 14336), int4 g128, top-2 of 8."""
    E, k = 8, 2
    g = torch.Generator(device=dev).manual_seed(N + T)
    Kw = (K + 7) // 8
    Wq = torch.randint(-2 ** 31, 2 ** 31 - 1, (E, N, Kw), generator=g, dtype=torch.int32, device=dev)
    s = torch.rand(E, N, (K + 127) // 128, generator=g, device=dev) * 0.01 + 1e-3
    X = _acts(T, K, torch.bfloat16, dev, seed=T)
    idx = _random_routing(T, k, E, seed=T).to(dev)
    off, src_token, _, _ = ops.moe_route(idx, E)
    Y = ops.gemm_wq_grouped(X, Wq, s, off, row_idx=src_token, K=K)
    torch.cuda.synchronize()
    off_l = off.cpu().tolist()
    assert off_l[-1] == T * k
    for lo, hi, want in _per_expert(ops, X, src_token.long(), off_l, Wq, s, None, None):
        torch.cuda.synchronize()
        _bits_equal(Y[lo:hi], want)


def test_grouped_refuses_bad_shapes(ops, dev):
    E, N, K = 2, 32, 256
    Wq, s, _, _ = _bank(dev, E, N, K, 4, False, False, seed=1)
    X = torch.zeros(4, K, dtype=torch.bfloat16, device=dev)
    off = torch.tensor([0, 2, 4], dtype=torch.int32, device=dev)
    with pytest.raises(ValueError):
        ops.gemm_wq_grouped(X, Wq, s, off, K=K - 8)                             # K is X's column count
    with pytest.raises(ValueError):
        ops.gemm_wq_grouped(X, Wq[0], s[0], off, K=K)                           # no leading E
    with pytest.raises(ValueError):
        ops.gemm_wq_grouped(X, Wq, s[:1], off, K=K)                             # scales of 1 expert
    with pytest.raises(ValueError):
        ops.gemm_wq_grouped(X, Wq, torch.ones(E, N, 3, device=dev), off, K=K)   # neither 1 nor K/128 groups
    with pytest.raises(ValueError):
        ops.gemm_wq_grouped(X, Wq, s, off[:2], K=K)                             # offsets not [E + 1]
    with pytest.raises(TypeError):
        ops.gemm_wq_grouped(X, Wq, s, off.long(), K=K)
    with pytest.raises(ValueError):
        ops.gemm_wq_grouped(X[:, :200], Wq, s, off, K=200)                      # packed width != ceil(K/8)
    with pytest.raises(TypeError):
        ops.gemm_wq_grouped(X.float(), Wq, s, off, K=K)
    with pytest.raises(TypeError):
        ops.gemm_wq_grouped(X, Wq, s, off, K=K, zp_w=torch.zeros(E, N, 2, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        ops.gemm_wq_grouped(X, Wq, s, off, K=K, g_idx=torch.zeros(K, dtype=torch.int32, device=dev))  # not [E, K]
    with pytest.raises(ValueError):
        ops.gemm_wq_grouped(X, Wq, s, off, K=K, row_idx=torch.zeros(2, 4, dtype=torch.int32, device=dev))


# ---- WeightOnlyExperts ----------------------------------------------------------------------------------------------
def _experts(dev, E, H, I, bits, zp, g_idx, seed):
    """(WeightOnlyExperts, the dense transformers bank it restates) on ``dev``."""
    from transformers import MixtralConfig
    from transformers.models.mixtral.modeling_mixtral import MixtralExperts

    from quantool_amd.engine.qlinear import WeightOnlyExperts, dequantized_weight

    cfg = MixtralConfig(hidden_size=H, intermediate_size=I, num_local_experts=E, num_experts_per_tok=2)
    parts = {}
    dense = {}
    for part, (N, K) in (("gate_up", (2 * I, H)), ("down", (H, I))):
        ts = [_weight(N, K, bits, zp=zp, g_idx=g_idx, seed=seed + 13 * e + N)[0] for e in range(E)]
        dense[part] = torch.stack([dequantized_weight(part, t, torch.bfloat16) for t in ts]).to(dev)
        leaf = "weight_packed" if bits == 4 else "weight"
        parts[part] = (torch.stack([t[leaf] for t in ts]).to(dev), torch.stack([t["weight_scale"] for t in ts]).to(dev),
                       torch.stack([t["weight_zero_point"] for t in ts]).to(dev) if zp else None,
                       torch.stack([t["weight_g_idx"] for t in ts]).to(dev) if g_idx else None)
    ref = MixtralExperts(cfg).to(torch.bfloat16).to(dev)
    ref.gate_up_proj.data = dense["gate_up"]
    ref.down_proj.data = dense["down"]
    bank = MixtralExperts(cfg).to(torch.bfloat16).to(dev)
    (gw, gs, gz, gg), (dw, ds, dz, dg) = parts["gate_up"], parts["down"]
    woe = WeightOnlyExperts(bank, gw, gs, dw, ds, gate_up_zero_point=gz, gate_up_g_idx=gg, down_zero_point=dz,
                            down_g_idx=dg)
    return woe, ref


def _restated(ops, woe, x, idx, w):
    """moe_route, per-expert gemm_wq_skinny, act_fn(gate) * up, per-expert gemm_wq_skinny, transformers' combine."""
    E = woe.num_experts
    off, src, _, row_of = ops.moe_route(idx, E)
    off_l = off.cpu().tolist()
    R = idx.numel()
    gu = torch.zeros(R, 2 * woe.intermediate_dim, dtype=x.dtype, device=x.device)
    for lo, hi, y in _per_expert(ops, x, src.long(), off_l, woe.gate_up, woe.gate_up_scale, woe.gate_up_zero_point,
                                 woe.gate_up_g_idx):
        gu[lo:hi] = y
    gate, up = gu.chunk(2, dim=-1)
    h = woe.act_fn(gate) * up
    Y = torch.zeros(R, woe.hidden_dim, dtype=x.dtype, device=x.device)
    for lo, hi, y in _per_expert(ops, h, torch.arange(R, device=x.device), off_l, woe.down, woe.down_scale,
                                 woe.down_zero_point, woe.down_g_idx):
        Y[lo:hi] = y
    return ref_combine(Y, idx, w, E, row_of)


@pytest.mark.parametrize("bits,zp,g_idx", [(4, False, False), (4, True, True), (8, False, False), (8, True, False)])
@pytest.mark.parametrize("T", [1, 5, 16, "max"])
def test_module_decode_path_bit_exact(ops, dev, bits, zp, g_idx, T):
    E, H, I, k = 8, 256, 384, 2
    woe, _ = _experts(dev, E, H, I, bits, zp, g_idx, seed=bits)
    T = woe.grouped_max_tokens if T == "max" else T
    assert T <= woe.grouped_max_tokens
    x = _acts(T, H, torch.bfloat16, dev, seed=T)
    idx = _random_routing(T, k, E, seed=T + 1).to(dev)
    w = torch.softmax(torch.randn(T, k, generator=torch.Generator().manual_seed(T)), -1).to(torch.bfloat16).to(dev)
    with torch.no_grad():
        out = woe(x, idx, w)
        want = _restated(ops, woe, x, idx, w)
    torch.cuda.synchronize()
    _bits_equal(out, want)


@pytest.mark.parametrize("bits,zp,g_idx", [(4, False, False), (4, True, True), (8, False, False)])
@pytest.mark.parametrize("above", [1, 300])
def test_module_large_path_equals_the_dense_bank(dev, bits, zp, g_idx, above):
    E, H, I, k = 4, 256, 384, 2
    woe, ref = _experts(dev, E, H, I, bits, zp, g_idx, seed=bits + above)
    T = woe.grouped_max_tokens + above
    x = _acts(T, H, torch.bfloat16, dev, seed=T)
    idx = _random_routing(T, k, E, seed=T + 1).to(dev)
    w = torch.softmax(torch.randn(T, k, generator=torch.Generator().manual_seed(T)), -1).to(torch.bfloat16).to(dev)
    with torch.no_grad():
        assert torch.equal(woe.dense_weight("gate_up", torch.bfloat16), ref.gate_up_proj.data)
        assert torch.equal(woe.dense_weight("down", torch.bfloat16), ref.down_proj.data)
        assert torch.equal(woe(x, idx, w), ref(x, idx, w))
        woe.grouped_max_tokens = 0                  # the same path at a decode-sized T
        assert torch.equal(woe(x[:3], idx[:3], w[:3]), ref(x[:3], idx[:3], w[:3]))


def test_module_decode_path_makes_no_host_sync(ops, dev, monkeypatch):
    E, H, I, k, T = 8, 256, 384, 2, 4
    woe, ref = _experts(dev, E, H, I, 4, False, False, seed=3)
    x = _acts(T, H, torch.bfloat16, dev, seed=1)
    idx = _random_routing(T, k, E, seed=2).to(dev)
    w = torch.softmax(torch.randn(T, k, generator=torch.Generator().manual_seed(3)), -1).to(torch.bfloat16).to(dev)
    calls = {"route": 0, "grouped": 0}
    real_route, real_grouped = ops.moe_route, ops.gemm_wq_grouped

    def route(*a, **kw):
        calls["route"] += 1
        return real_route(*a, **kw)

    def grouped(*a, **kw):
        calls["grouped"] += 1
        return real_grouped(*a, **kw)

    def host_read(*a, **kw):
        raise AssertionError("host read on the decode path")

    with torch.no_grad():
        torch.cuda.synchronize()
        # the CUDA sync debug mode, where it reports on this runtime: probe that it flags a nonzero() first
        torch.cuda.set_sync_debug_mode("error")
        try:
            try:
                torch.ones(4, device=dev).nonzero()
                mode_works = False
            except RuntimeError:
                mode_works = True
            if mode_works:
                out_mode = woe(x, idx, w)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        monkeypatch.setattr(ops, "moe_route", route)
        monkeypatch.setattr(ops, "gemm_wq_grouped", grouped)
        for name in ("nonzero", "item", "tolist", "cpu"):
            monkeypatch.setattr(torch.Tensor, name, host_read)
        monkeypatch.setattr(torch, "nonzero", host_read)
        out = woe(x, idx, w)
        monkeypatch.undo()
    assert calls == {"route": 1, "grouped": 2}
    torch.cuda.synchronize()
    if mode_works:
        _bits_equal(out_mode, out)
    # the dense bank's loop does read the host: the same guard catches it
    with torch.no_grad(), pytest.raises(AssertionError, match="host read"):
        monkeypatch.setattr(torch.Tensor, "nonzero", host_read)
        ref(x, idx, w)
    monkeypatch.undo()


# ---- end to end -----------------------------------------------------------------------------------------------------
def _quantize_mixtral(dev, source, out_dir):
    import quantool_amd.methods  # noqa: F401
    from quantool_amd.core import QuantizerRegistry
    from tests.test_gpu_moe import _tiny_mixtral

    model = _tiny_mixtral(dev)
    g = torch.Generator().manual_seed(2)
    data = [{"input_ids": torch.randint(0, 512, (48,), generator=g)} for _ in range(8)]
    if source == "oneshot_group":
        from quantool_amd.engine.modifiers import GPTQModifier
        from quantool_amd.engine.oneshot import oneshot

        oneshot(model=model, dataset=data, recipe=GPTQModifier(scheme="W4A16", actorder="group"),
                output_dir=str(out_dir), num_calibration_samples=8, max_seq_length=64,
                shuffle_calibration_samples=False)
    else:
        q = QuantizerRegistry.create("gptq", model_id="synthetic/tiny-mixtral")
        q.quantize(model=model, level=source, dataset=data, num_calibration_samples=8, max_seq_length=64,
                   shuffle_calibration_samples=False)
        torch.cuda.synchronize()
        q.save_pretrained(str(out_dir))
    torch.cuda.synchronize()


@pytest.mark.parametrize("source", ["W4A16", "W4A16_ASYM", "oneshot_group"])
def test_end_to_end_packed_experts(dev, tmp_path, monkeypatch, source):
    from quantool_amd.engine.qlinear import WeightOnlyExperts, load_quantized
    from quantool_amd.engine.serialization import load_state
    from quantool_amd.evaluate import perplexity
    from quantool_amd.hip import ops
    from tests.test_gpu_qlinear import _eval_ids

    monkeypatch.chdir(tmp_path)
    ckpt = tmp_path / "ckpt"
    _quantize_mixtral(dev, source, ckpt)
    names = set(load_state(ckpt))
    expert_zp = any(".experts." in n and n.endswith(".weight_zero_point") for n in names)
    expert_gidx = any(".experts." in n and n.endswith(".weight_g_idx") for n in names)
    assert expert_zp == (source == "W4A16_ASYM")
    dense_bank = load_quantized(ckpt, device=dev, a16="packed")
    packed = load_quantized(ckpt, device=dev, a16="packed", a16_experts="packed")
    banks = [m for m in packed.modules() if isinstance(m, WeightOnlyExperts)]
    assert len(banks) == 2 and packed._qt_checkpoint["dense_expert_banks"] == []
    assert all((b.gate_up_zero_point is not None) == expert_zp for b in banks)
    assert all((b.gate_up_g_idx is not None) == expert_gidx for b in banks)
    # prefill-sized batches (4 x 96 tokens) take the dequantise path: the same bits as the dense bank
    ids = _eval_ids()
    assert 4 * ids.shape[1] > banks[0].grouped_max_tokens
    p_dense = perplexity(dense_bank, ids, batch_size=4)["perplexity"]
    p_packed = perplexity(packed, ids, batch_size=4)["perplexity"]
    assert math.isfinite(p_dense) and p_packed == p_dense, (p_packed, p_dense)

    # a KV-cached greedy decode: every single-token step runs the grouped GEMV pair per layer (and so does the 24-token
    # prompt when it is within grouped_max_tokens)
    calls = {"grouped": 0}
    real = ops.gemm_wq_grouped

    def grouped(*a, **k):
        calls["grouped"] += 1
        return real(*a, **k)

    prompt = ids[:1, :24].to(dev)
    steps = 16
    with torch.no_grad():
        ref, toks = _greedy_logits(dense_bank, prompt, steps)
        monkeypatch.setattr(ops, "gemm_wq_grouped", grouped)
        got, _ = _greedy_logits(packed, prompt, steps, feed=toks)
    assert calls["grouped"] == 2 * len(banks) * (steps + (prompt.shape[1] <= banks[0].grouped_max_tokens))
    # each grouped row is within one rounding plus the summation-order bound of the dense bank's F.linear row, as the
    # skinny GEMV is; through 2 layers these stay a few ulps.  A wrong weight, scale or routing moves logits by O(1).
    diff = (got - ref).abs().max().item()
    scale = ref.abs().max().item()
    assert diff <= 2.0 ** -4 * scale, (diff, scale)
    # every Linear and packed expert bank against what the checkpoint files define (fp64, no shared decoding): the
    # grouped GEMV and the dequantise paths
    from tests.test_gpu_ckpt_e2e import check_modules_against_files

    assert check_modules_against_files(packed, ckpt, dev, tokens=(1, 129, 200)) > 0
