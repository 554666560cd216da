"""``qt_gemm_wq_stream`` on the GPU: every row bit for bit against the skinny kernel, the fp64 bound, one-hot rows that pin
the lane / column map against the dequantised weight, exact inputs against the fp64 product, pitched and caller-owned
operands, the raw ABI's refusals, ``WeightOnlyLinear`` with ``stream_max_m`` and ``load_quantized(...,
a16_stream_rows=)`` end to end."""
import itertools

import pytest
import torch

from tests.test_gpu_qlinear import _eval_ids, _quantize_and_save
from tests.test_gpu_wq_linear import _bits_equal, _check_bound, _dev_args, _greedy_logits, _ref_w, _weight

pytestmark = pytest.mark.gpu

# one instance per tile count ceil(M / 16): every count 1 ... 8, at its first and (1, 2, 4, 8) last row
MS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 81, 97, 127, 128)
# k-blocks of 128 columns; wave w takes k-blocks w, w + 4, ... in batches of 8 (int4) or 4 (int8), then 4, 2 and 1 for
# the rest.  1, 3, 4, 5: waves with no k-block, one, two.  16 / 17: four each (int8: one batch; int4: the 4-path) / + 1.
# 27: 7, 7, 7, 6 (the 4-, 2- and 1-paths together).  32 / 33: int4's one batch / + 1; int8's two.  35: 9, 9, 9, 8, the
# largest the kernel's branches need but for one: a second full int4 batch in one wave takes 64 k-blocks, so 67 (17, 17,
# 17, 16) is here too -- at N <= 67 it costs nothing.
KBS = (1, 3, 4, 5, 16, 17, 27, 32, 33, 35, 67)
NS = (1, 15, 16, 17, 33, 67)        # a workgroup owns 16 columns: 33 and 67 are 3 and 5 column tiles, the last partial


def _case(i, j):
    """(M, k-blocks, N, bits, zp, grouped, bias, dtype) of cell (i, j) of MS x KBS: the other factors cycle so that every
    pair of values of any two factors meets (test_cases_cover_every_pair)."""
    c = len(KBS) * i + j
    return (MS[i], KBS[j], NS[(i + j) % 6], (4, 8)[(c >> 1) & 1], bool((c >> 2) & 1), bool((c >> 3) & 1),
            bool((i + j // 2) & 1), (torch.bfloat16, torch.float16)[(i // 2 + j) & 1])


CASES = [_case(i, j) for i in range(len(MS)) for j in range(len(KBS))]


def test_cases_cover_every_pair():
    values = [MS, KBS, NS, (4, 8), (False, True), (False, True), (False, True), (torch.bfloat16, torch.float16)]
    for a, b in itertools.combinations(range(len(values)), 2):
        seen = {(c[a], c[b]) for c in CASES}
        missing = [p for p in itertools.product(values[a], values[b]) if p not in seen]
        assert not missing, (a, b, missing)


def _slices(M):
    """Every aligned 16-row slice, and the last 16 rows (a slice that straddles two m-tiles)."""
    out = [(i, min(i + 16, M)) for i in range(0, M, 16)]
    if M > 16 and M % 16:
        out.append((M - 16, M))
    return out


def _x(M, K, dtype, dev, seed):
    return torch.randn(M, K, generator=torch.Generator().manual_seed(seed)).to(dtype).to(dev)


# ---- bits against the skinny kernel ---------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(MS)), ids=[f"M{m}" for m in MS])
def test_rows_equal_the_skinny_kernel(ops, dev, i):
    for j in range(len(KBS)):
        M, kbs, N, bits, zp, grouped, with_bias, dtype = _case(i, j)
        K = 128 * kbs
        t, _ = _weight(N, K, bits, zp=zp, grouped=grouped, seed=11 * i + j)
        Wq, s, z, _ = _dev_args(t, dev)
        X = _x(M, K, dtype, dev, seed=200 + 11 * i + j)
        bias = (torch.randn(N, generator=torch.Generator().manual_seed(j)) * 0.1).to(dtype).to(dev) if with_bias else None
        Y = ops.gemm_wq_stream(X, Wq, s, zp_w=z, bias=bias)
        Y2 = ops.gemm_wq_stream(X, Wq, s, zp_w=z, bias=bias)
        assert Y.shape == (M, N) and Y.dtype == dtype
        for lo, hi in _slices(M):
            ref = ops.gemm_wq_skinny(X[lo:hi], Wq, s, zp_w=z, bias=bias)
            assert torch.equal(Y[lo:hi].view(torch.int16), ref.view(torch.int16)), (_case(i, j), lo, hi)
        assert torch.equal(Y.view(torch.int16), Y2.view(torch.int16)), _case(i, j)       # two runs, the same bits


@pytest.mark.parametrize("M,N,kbs,bits,zp,dtype", [(17, 33, 5, 4, True, torch.bfloat16),
                                                   (64, 67, 17, 8, False, torch.float16),
                                                   (128, 17, 35, 4, False, torch.bfloat16)])
def test_random_inputs_within_the_fp64_bound(ops, dev, M, N, kbs, bits, zp, dtype):
    K = 128 * kbs
    t, _ = _weight(N, K, bits, zp=zp, seed=M + N)
    Wq, s, z, _ = _dev_args(t, dev)
    X = _x(M, K, dtype, dev, seed=5)
    bias = (torch.randn(N, generator=torch.Generator().manual_seed(6)) * 0.1).to(dtype)
    Y = ops.gemm_wq_stream(X, Wq, s, zp_w=z, bias=bias.to(dev))
    _check_bound(Y, X, _ref_w(t, dtype), bias)


# ---- one-hot rows: the lane / column map against the dequantised weight, without the skinny kernel -----------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("bits,zp", [(4, False), (4, True), (8, False)])
def test_one_hot_rows_read_the_weight(ops, dev, dtype, bits, zp):
    N, K = 33, 384
    t, _ = _weight(N, K, bits, zp=zp, seed=bits + zp)
    Wq, s, z, _ = _dev_args(t, dev)
    Wt = _ref_w(t, dtype).to(dev).t().contiguous().view(torch.int16)      # [K, N]
    for M in (32, 64, 128):                                               # every row of every m-tile: 2, 4, 8 tiles
        rows = torch.arange(M, device=dev)
        for off in range(0, 130):                                         # a whole k-block and the block boundary
            X = torch.zeros(M, K, dtype=dtype, device=dev)
            X[rows, off + rows] = 1
            Y = ops.gemm_wq_stream(X, Wq, s, zp_w=z)
            assert torch.equal(Y.view(torch.int16), Wt[off:off + M]), (M, off)


# ---- exact inputs ---------------------------------------------------------------------------------------------------
# |x| <= 4, |q - zp| <= 16 (int4) or 136 (int8), scales 2^0 .. 2^-4: every partial sum is a multiple of 2^-4 below 2^20
# (int4, K <= 4096; int8, K <= 1024), so exact in fp32 (test_skinny_exact_inputs_bit_exact's argument)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("zp", [False, True])
@pytest.mark.parametrize("bits,N,K", [(4, 96, 1024), (4, 33, 4096), (8, 96, 1024)])
def test_exact_inputs_bit_exact(ops, dev, dtype, zp, bits, N, K):
    t, _ = _weight(N, K, bits, zp=zp, seed=3 * N + K, pow2_scales=True)
    Wq, s, z, _ = _dev_args(t, dev)
    W = _ref_w(t, dtype).double()
    g = torch.Generator().manual_seed(K)
    bias = torch.randint(-8, 9, (N,), generator=g).to(dtype)
    for M in (17, 64, 128):
        X = torch.randint(-4, 5, (M, K), generator=g).to(dtype)
        for b in (None, bias):
            Y = ops.gemm_wq_stream(X.to(dev), Wq, s, zp_w=z, bias=None if b is None else b.to(dev))
            ref = X.double() @ W.T
            if b is not None:
                ref = ref + b.double()
            _bits_equal(Y, (ref + 0.0).to(dtype))     # the kernel sums from +0: an exactly zero output is +0


# ---- edges ----------------------------------------------------------------------------------------------------------
def _raw(ops, X, M, K, ldx, Wq, fmt, N, s, G, zp, g_idx, bias, Y, ldy, code=None):
    from quantool_amd.hip import _lib

    p = lambda v: None if v is None else (v if isinstance(v, int) else v.data_ptr())   # noqa: E731
    code = _lib.QT_BF16 if code is None else code
    _lib.check("qt_gemm_wq_stream", _lib.load().qt_gemm_wq_stream(
        p(X), code, M, K, ldx, p(Wq), fmt, N, p(s), G, p(zp), p(g_idx), p(bias), p(Y), ldy,
        torch.cuda.current_stream().cuda_stream))


def test_pitched_activations(ops, dev):
    t, _ = _weight(67, 1024, 4, seed=2)
    Wq, s, z, _ = _dev_args(t, dev)
    wide = _x(80, 1032, torch.bfloat16, dev, seed=1)
    X = wide[:, :1024]                                                    # ldx = K + 8
    assert X.stride(0) == 1032 and ops.gemm_wq_stream_supported(X, Wq, s)
    Y = ops.gemm_wq_stream(X, Wq, s)
    _bits_equal(Y, ops.gemm_wq_stream(X.contiguous(), Wq, s))
    for lo in range(0, 80, 16):
        _bits_equal(Y[lo:lo + 16], ops.gemm_wq_skinny(X[lo:lo + 16], Wq, s))


@pytest.mark.parametrize("bits", [4, 8])
def test_caller_owned_output_keeps_its_sentinels(ops, dev, bits):
    from quantool_amd.hip import _lib

    M, N, K = 33, 67, 640
    t, _ = _weight(N, K, bits, zp=True, seed=4)
    # operands as exact-size allocations: each ends with its storage
    Wq, s, z, _ = (None if v is None else v.clone() for v in _dev_args(t, dev))
    X = _x(M, K, torch.bfloat16, dev, seed=3).clone()
    bias = (torch.randn(N, generator=torch.Generator().manual_seed(1)) * 0.1).to(torch.bfloat16).to(dev)
    for v in (Wq, s, z, X, bias):
        assert v.untyped_storage().nbytes() == v.numel() * v.element_size()
    ldy, rows = N + 17, M + 3
    buf = torch.full((rows * ldy + 64,), 7.0, dtype=torch.bfloat16, device=dev)
    fmt = _lib.QT_W_INT4_PACKED if bits == 4 else _lib.QT_W_INT8
    _raw(ops, X, M, K, K, Wq, fmt, N, s, s.shape[1], z, None, bias, buf, ldy)
    grid = buf[:rows * ldy].view(rows, ldy)
    _bits_equal(grid[:M, :N].contiguous(), ops.gemm_wq_stream(X, Wq, s, zp_w=z, bias=bias))
    assert (grid[:M, N:] == 7).all() and (grid[M:] == 7).all() and (buf[rows * ldy:] == 7).all()


def test_raw_abi_refusals_launch_nothing(ops, dev):
    from quantool_amd.hip._lib import QT_BF16, QT_ERR_INVALID, QT_F32, QT_W_INT4_PACKED, QT_W_INT8, HipBackendError

    N, K = 32, 1024
    wbuf = torch.zeros(N * K + 16, dtype=torch.int8, device=dev)
    Wq, Wq_off = wbuf[:N * K].view(N, K), wbuf[4:4 + N * K].view(N, K)
    xbuf = torch.zeros(129 * (K + 8) + 8, dtype=torch.bfloat16, device=dev)
    X, X_off = xbuf[:129 * K].view(129, K), xbuf[1:1 + 128 * K].view(128, K)
    s = torch.ones(N, 8, device=dev)
    gi = torch.zeros(K, dtype=torch.int32, device=dev)
    Y = torch.full((129, N), 7.0, dtype=torch.bfloat16, device=dev)
    i8 = QT_W_INT8
    #        X, M, K, ldx, Wq, fmt, N, s_w, G, zp, g_idx, bias, Y, ldy
    cases = {
        "g_idx": ((X, 32, K, K, Wq, i8, N, s, 8, None, gi, None, Y, N), "actorder group runs on qt_dequantize_weight"),
        "ragged K": ((X, 32, 192, K, Wq, i8, N, s, 1, None, None, None, Y, N), "not a multiple of the k-unit"),
        "M = 0": ((X, 0, K, K, Wq, i8, N, s, 1, None, None, None, Y, N), "1 <= M <= 128"),
        "M = 129": ((X, 129, K, K, Wq, i8, N, s, 1, None, None, None, Y, N), "1 <= M <= 128"),
        "X shifted": ((X_off, 32, K, K, Wq, i8, N, s, 1, None, None, None, Y, N), "16-byte aligned"),
        "Wq shifted": ((X, 32, K, K, Wq_off, i8, N, s, 1, None, None, None, Y, N), "16-byte aligned"),
        "pitch K + 1": ((X, 32, K, K + 1, Wq, i8, N, s, 1, None, None, None, Y, N), "16-byte aligned"),
        "pitch below K": ((X, 32, K, K - 8, Wq, i8, N, s, 1, None, None, None, Y, N), "ldx >= K"),
        "ldy below N": ((X, 32, K, K, Wq, i8, N, s, 1, None, None, None, Y, N - 1), "ldy >= N"),
        "null X": ((None, 32, K, K, Wq, i8, N, s, 1, None, None, None, Y, N), "null pointer"),
        "null Wq": ((X, 32, K, K, None, i8, N, s, 1, None, None, None, Y, N), "null pointer"),
        "null s_w": ((X, 32, K, K, Wq, i8, N, None, 1, None, None, None, Y, N), "null pointer"),
        "null Y": ((X, 32, K, K, Wq, i8, N, s, 1, None, None, None, None, N), "null pointer"),
        "G = 3": ((X, 32, K, K, Wq, i8, N, s, 3, None, None, None, Y, N), "G must be 1 or K / 128 = 8"),
        "w_format": ((X, 32, K, K, Wq, 99, N, s, 1, None, None, None, Y, N), "w_format 99"),
    }
    for what, (args, reason) in cases.items():
        with pytest.raises(HipBackendError, match=reason) as e:
            _raw(ops, *args)
        assert e.value.status == QT_ERR_INVALID, what
    with pytest.raises(HipBackendError, match="must be bf16 or fp16") as e:
        _raw(ops, X, 32, K, K, Wq, QT_W_INT4_PACKED, N, s, 8, None, None, None, Y, N, code=QT_F32)
    assert e.value.status == QT_ERR_INVALID
    torch.cuda.synchronize()
    assert (Y == 7).all()
    _raw(ops, X, 32, K, K, Wq, i8, N, s, 8, None, None, None, Y, N, code=QT_BF16)       # and the same call, accepted
    assert (Y[:32] == 0).all() and (Y[32:] == 7).all()


# ---- WeightOnlyLinear -----------------------------------------------------------------------------------------------
def test_module_paths(dev, ops, monkeypatch):
    import torch.nn.functional as F

    from quantool_amd.engine.qlinear import WeightOnlyLinear, weight_only_linear_from_tensors

    # the dispatch rules under test, whatever the measured size bounds are
    monkeypatch.setattr(WeightOnlyLinear, "stream_max_n", 0)
    monkeypatch.setattr(WeightOnlyLinear, "stream_min_k", 0)
    N, K = 384, 1024
    bias = (torch.randn(N, generator=torch.Generator().manual_seed(0)) * 0.1).to(torch.bfloat16).to(dev)
    big = _x(80, K, torch.bfloat16, dev, seed=1).reshape(2, 40, K)
    for bits, zp in ((4, False), (4, True), (8, False)):
        t, _ = _weight(N, K, bits, zp=zp, seed=bits + 10 * zp)
        m = weight_only_linear_from_tensors("m", {k: v.to(dev) for k, v in t.items()}, bias=bias)
        W = _ref_w(t, torch.bfloat16).to(dev)
        Wq, s, z, _ = _dev_args(t, dev)
        with torch.no_grad():
            assert m.stream_max_m == 0
            assert torch.equal(m(big), F.linear(big, W, bias))               # the default: dequantise + F.linear
            m.stream_max_m = 128
            y = m(big)
            assert y.shape == (2, 40, N)
            _bits_equal(y.reshape(80, N), ops.gemm_wq_stream(big.reshape(80, K), Wq, s, zp_w=z, bias=bias))
            for lo in range(0, 80, 16):
                _bits_equal(y.reshape(80, N)[lo:lo + 16],
                            ops.gemm_wq_skinny(big.reshape(80, K)[lo:lo + 16], Wq, s, zp_w=z, bias=bias))
            m.stream_max_m = 64
            assert torch.equal(m(big), F.linear(big, W, bias))               # 80 rows > 64
            m.stream_max_m, m.stream_max_n = 128, N - 1
            assert torch.equal(m(big), F.linear(big, W, bias))               # out_features past stream_max_n
            m.stream_max_n, m.stream_min_k = 0, K + 128
            assert torch.equal(m(big), F.linear(big, W, bias))               # in_features below stream_min_k
    t, _ = _weight(N, K, 4, g_idx=True, seed=9)
    m = weight_only_linear_from_tensors("m", {k: v.to(dev) for k, v in t.items()}, bias=bias)
    m.stream_max_m = 128
    with torch.no_grad():
        assert torch.equal(m(big), F.linear(big, _ref_w(t, torch.bfloat16).to(dev), bias))   # g_idx: never the kernel


# ---- end to end -----------------------------------------------------------------------------------------------------
def test_end_to_end_stream_rows(dev, tmp_path, monkeypatch):
    from quantool_amd.engine.qlinear import WeightOnlyLinear, load_quantized
    from quantool_amd.hip import ops

    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(WeightOnlyLinear, "stream_max_n", 0)     # the tiny model's Linears are 256 and 512 wide
    monkeypatch.setattr(WeightOnlyLinear, "stream_min_k", 0)
    ckpt = tmp_path / "ckpt"
    _quantize_and_save("gptq", "W4A16", dev, ckpt)
    dense = load_quantized(ckpt, device=dev)
    packed = load_quantized(ckpt, device=dev, a16="packed", a16_stream_rows=128)
    wols = [m for m in packed.modules() if isinstance(m, WeightOnlyLinear)]
    assert len(wols) == 14 and all(m.stream_max_m == 128 for m in wols)
    assert packed._qt_checkpoint["a16_stream_rows"] == 128

    calls = {"skinny": 0, "stream": 0, "dequant": 0}

    def counting(name, real):
        def f(*a, **k):
            calls[name] += 1
            return real(*a, **k)
        return f

    prompt = _eval_ids()[:1, :24].to(dev)
    steps = 4
    with torch.no_grad():
        ref, toks = _greedy_logits(dense, prompt, steps)
        monkeypatch.setattr(ops, "gemm_wq_skinny", counting("skinny", ops.gemm_wq_skinny))
        monkeypatch.setattr(ops, "gemm_wq_stream", counting("stream", ops.gemm_wq_stream))
        monkeypatch.setattr(ops, "dequantize_weight", counting("dequant", ops.dequantize_weight))
        first = packed(input_ids=prompt, use_cache=True)
        assert calls == {"skinny": 0, "stream": 14, "dequant": 0}            # the 24-token prompt
        del first
        calls["stream"] = 0
        got, _ = _greedy_logits(packed, prompt, steps, feed=toks)
    assert calls == {"skinny": 14 * steps, "stream": 14, "dequant": 0}       # decode steps stay on the skinny kernel
    # test_end_to_end_packed_model's bound and argument: each output is within about one bf16 ulp of the dense Linear's
    diff = (got - ref).abs().max().item()
    scale = ref.abs().max().item()
    assert diff <= 2.0 ** -4 * scale, (diff, scale)
