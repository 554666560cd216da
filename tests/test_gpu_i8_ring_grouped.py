"""qt_gemm_i8_ring_grouped: the 256 x 256 LDS-ring int8 GEMM over an expert bank (W8A8 / INT8 prefill).

Its contract is bit equality with the tiled qt_gemm_i8_grouped on the same arguments, so every comparison here is on bit
patterns (``.view(torch.int16)`` + ``torch.equal``), against two yardsticks: ``ops.gemm_i8_grouped`` and one
``ops.gemm_i8`` per expert on that expert's gathered rows.  That alone would pass kernels wrong in the same way, so the
same cases also go against the fp64 reference of tests/ckpt_reference.py within the project's own bound for this
sequence (``gemm_i8_tolerance``), and an identity test pins the expert and the gathered row of every output row.
Shapes are in the kernel's own constants: U = the k-unit, R = the ring's slots, L = its lead."""
import pytest
import torch

from tests import ckpt_reference as cr
from tests.test_gpu_i8_ring import _url
from tests.test_gpu_i8_skinny import _same_bits, _sentinel, _untouched
from tests.test_gpu_runtime_edges import _levels

pytestmark = pytest.mark.gpu


def _offsets(counts, dev):
    return torch.tensor([0] + torch.tensor(counts).cumsum(0).tolist(), dtype=torch.int32, device=dev)


def _acts(T, K, dev, seed):
    """T activation rows with outlier channels, an all-zero row (the eps clamp) and an all-positive one."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, K, generator=g)
    x[:, torch.randperm(K, generator=g)[: max(1, K // 64)]] *= 10
    x[T // 2] = 0.0
    x[T // 3] = x[T // 3].abs() + 0.5
    return x.to(torch.bfloat16).to(dev)


def _twice(n_rows, seed):
    """row_idx for n_rows routed rows: every source row twice (one of them once when n_rows is odd), out of order."""
    T = (n_rows + 1) // 2
    src = torch.cat([torch.arange(T), torch.arange(T)])[:n_rows]
    src = src[torch.randperm(n_rows, generator=torch.Generator().manual_seed(seed))].to(torch.int32)
    assert not torch.equal(src, src.sort().values) and int(src.bincount().min()) >= (2 if n_rows % 2 == 0 else 1)
    return T, src


def _case(ops, dev, counts, N, K, seed):
    """An int8 bank, a routing with ``counts`` rows per expert and both quantisations of the source rows, with the fp64
    reference of every routed row (computed once per case)."""
    E, n_rows = len(counts), sum(counts)
    q8 = _levels((E, N, K), 8, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    s_w = (torch.rand(E, N, 1, generator=g) * 0.02 + 1e-4).to(torch.bfloat16).float()
    T, src = _twice(n_rows, seed + 2)
    X = _acts(T, K, dev, seed + 3)
    out = {"E": E, "rows": n_rows, "N": N, "K": K, "counts": counts, "Wq": q8.to(dev), "s_w": s_w.to(dev),
           "wsum": q8.to(torch.int64).sum(-1, keepdim=True).to(torch.int32).to(dev), "offsets": _offsets(counts, dev),
           "src": src.to(dev)}
    off = [0] + torch.tensor(counts).cumsum(0).tolist()
    for asym in (False, True):
        Xq, s_x, zp_x = ops.quantize_tokens_i8(X, symmetric=not asym)
        y64, mag = torch.zeros(n_rows, N, dtype=torch.float64), torch.zeros(n_rows, N, dtype=torch.float64)
        for e in range(E):
            lo, hi = off[e], off[e + 1]
            if hi > lo:
                rows = src[lo:hi].long()
                t = {"weight": q8[e], "weight_scale": s_w[e], "weight_shape": torch.tensor([N, K])}
                y64[lo:hi], mag[lo:hi] = cr.a8_linear(Xq.cpu()[rows], s_x.cpu()[rows],
                                                      None if zp_x is None else zp_x.cpu()[rows], t)
        out[asym] = (Xq, s_x, zp_x, y64, mag)
    return out


def _check(ops, c, asym, dt, gather, what):
    Xq, s_x, zp_x, y64, mag = c[asym]
    src = c["src"].long()
    if gather:
        A, sa, za, ri = Xq, s_x, zp_x, c["src"]
    else:
        A, sa, ri = Xq[src].contiguous(), s_x[src].contiguous(), None
        za = None if zp_x is None else zp_x[src].contiguous()
    ws = c["wsum"] if asym else None
    kw = dict(row_idx=ri, zp_x=za, wsum=ws, out_dtype=dt)
    want = ops.gemm_i8_grouped(A, sa, c["Wq"], c["s_w"], c["offsets"], **kw)
    got = ops.gemm_i8_ring_grouped(A, sa, c["Wq"], c["s_w"], c["offsets"], **kw)
    torch.cuda.synchronize()
    assert got.shape == (c["rows"], c["N"])
    _same_bits(got, want, f"{what} vs gemm_i8_grouped")
    off = c["offsets"].cpu().tolist()
    for e in range(c["E"]):                      # the second yardstick: one dense GEMM per expert on its gathered rows
        lo, hi = off[e], off[e + 1]
        if hi > lo:
            r = src[lo:hi]
            one = ops.gemm_i8(Xq[r].contiguous(), s_x[r].contiguous(), c["Wq"][e], c["s_w"][e],
                              zp_x=None if zp_x is None else zp_x[r].contiguous(), wsum=None if ws is None else ws[e],
                              out_dtype=dt)
            _same_bits(got[lo:hi], one, f"{what} expert {e} vs gemm_i8")
    cr.assert_within(got, y64, cr.gemm_i8_tolerance(got.cpu(), mag, 1), f"{what} vs fp64")
    return got


def _all_forms(ops, c, what):
    for asym in (False, True):
        for dt in (torch.bfloat16, torch.float16):
            for gather in (True, False):
                _check(ops, c, asym, dt, gather, f"{what} asym={asym} {dt} gather={gather}")


# ---- 1: ragged experts ----------------------------------------------------------------------------------------------
def test_ragged_experts(ops, dev):
    """Empty experts first, in the middle and last; one row; exactly one tile; a tile and one row; a tile and 44 rows."""
    U, R, L = _url()
    c = _case(ops, dev, (0, 1, 256, 257, 0, 300, 0), 384, (R + 1) * U, seed=1)
    _all_forms(ops, c, "ragged")


# ---- 2: the ring's depth --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("units", ["1", "L", "R+1", "2R+3"])
def test_ring_depth(ops, dev, units):
    U, R, L = _url()
    K = U * {"1": 1, "L": L, "R+1": R + 1, "2R+3": 2 * R + 3}[units]
    c = _case(ops, dev, (130, 0, 300), 300, K, seed=K)
    _all_forms(ops, c, f"K={K}")


# ---- 3: the tile walk -----------------------------------------------------------------------------------------------
def test_many_small_experts(ops, dev):
    """E = 64 with 3 rows each: every tile clamps 253 of its rows to its own expert's last row, and the B base moves by
    e N K from tile to tile."""
    U, R, L = _url()
    c = _case(ops, dev, (3,) * 64, 130, (R + 1) * U, seed=3)
    _all_forms(ops, c, "E=64")


def test_one_expert_owns_all_rows(ops, dev):
    """700 rows on expert 5 of 8: 3 of the 3 + 8 m-tile slots work, the other 8 exit."""
    U, R, L = _url()
    c = _case(ops, dev, (0, 0, 0, 0, 0, 700, 0, 0), 200, (R + 1) * U, seed=4)
    _all_forms(ops, c, "one expert")


def test_more_than_group_m_tile_slots(ops, dev):
    """16 + 0 + 18 tiles in 34 + 3 = 37 slots: more than the 32 that walk the n-tiles together, over 2 n-tiles."""
    U, R, L = _url()
    c = _case(ops, dev, (4000, 0, 4500), 300, U, seed=5)
    for asym, dt, gather in ((True, torch.bfloat16, True), (False, torch.float16, False)):
        _check(ops, c, asym, dt, gather, f"37 slots asym={asym} gather={gather}")


def _raw(ops, name, Xq_ptr, K, row_idx, n_rows, offsets, E, Wq_ptr, fmt, N, s_x, zp_x, s_w, G, wsum, Y, ldy, x_rows):
    from quantool_amd.hip import _lib

    extra = (x_rows,) if name == "qt_gemm_i8_ring_grouped" else ()
    _lib.check(name, getattr(_lib.load(), name)(
        Xq_ptr, K, ops._ptr(row_idx), n_rows, offsets.data_ptr(), E, Wq_ptr, fmt, N, s_x.data_ptr(), ops._ptr(zp_x),
        s_w.data_ptr(), G, ops._ptr(wsum), Y.data_ptr(), ops._dtype_code(Y), ldy, *extra, ops._stream()))


def test_an_all_empty_table_writes_nothing(ops, dev):
    from quantool_amd.hip import _lib

    U, R, L = _url()
    E, n_rows, N, K = 5, 300, 260, 2 * U
    Xq = torch.ones(n_rows, K, dtype=torch.int8, device=dev)
    Wq = torch.ones(E, N, K, dtype=torch.int8, device=dev)
    s_x, s_w = torch.ones(n_rows, device=dev), torch.ones(E, N, 1, device=dev)
    for table in ([0] * (E + 1), [7] * (E + 1), [9, 5, 5, 2, 0, 0]):       # empty, empty at 7, descending: clamped empty
        Y = _sentinel((n_rows, N), torch.bfloat16, dev)
        offsets = torch.tensor(table, dtype=torch.int32, device=dev)
        _raw(ops, "qt_gemm_i8_ring_grouped", Xq.data_ptr(), K, None, n_rows, offsets, E, Wq.data_ptr(), _lib.QT_W_INT8,
             N, s_x, None, s_w, 1, None, Y, N, n_rows)
        torch.cuda.synchronize()
        assert _untouched(Y), table


# ---- 4: lane, slot, expert and row maps -----------------------------------------------------------------------------
def test_identity_activations_read_the_expert_and_the_row(ops, dev):
    """Xq = the K x K identity, unit scales, no zero-point: Y[r, n] = (float)W[e(r)][n, src(r)] exactly, which pins the
    expert, the gathered row and the weight byte every A slot multiplies."""
    U, R, L = _url()
    K, N, counts = (R + 1) * U, 96, (300, 0, 515, 1)
    E, n_rows = len(counts), sum(counts)
    W = _levels((E, N, K), 8, seed=77)
    assert len({tuple(r) for r in W.reshape(E * N, K).tolist()}) == E * N and not torch.equal(W[0], W[2])
    src = torch.randperm(K, generator=torch.Generator().manual_seed(6))[:n_rows].to(torch.int32)
    assert n_rows < K and not torch.equal(src, src.sort().values)
    expert = torch.repeat_interleave(torch.arange(E), torch.tensor(counts))
    want = W[expert, :, src.long()].to(torch.float16)                   # [rows, N]
    Xq = torch.eye(K, dtype=torch.int8, device=dev)
    Y = ops.gemm_i8_ring_grouped(Xq, torch.ones(K, device=dev), W.to(dev), torch.ones(E, N, 1, device=dev),
                                 _offsets(counts, dev), row_idx=src.to(dev), out_dtype=torch.float16)
    torch.cuda.synchronize()
    _same_bits(Y.cpu(), want.contiguous(), "identity")


def test_row_indices_are_clamped_into_xq(ops, dev):
    """An index below 0 reads row 0, one past the end reads the last row (the tiled kernel leaves this to the caller)."""
    U, R, L = _url()
    c = _case(ops, dev, (40, 270), 64, 2 * U, seed=8)
    Xq, s_x, zp_x, _, _ = c[True]
    T = Xq.shape[0]
    wild = c["src"].clone()
    tame = c["src"].clone()
    wild[::3], tame[::3] = -5, 0
    wild[1::3], tame[1::3] = 2 ** 31 - 1, T - 1
    kw = dict(zp_x=zp_x, wsum=c["wsum"])
    got = ops.gemm_i8_ring_grouped(Xq, s_x, c["Wq"], c["s_w"], c["offsets"], row_idx=wild, **kw)
    want = ops.gemm_i8_grouped(Xq, s_x, c["Wq"], c["s_w"], c["offsets"], row_idx=tame, **kw)
    torch.cuda.synchronize()
    _same_bits(got, want, "clamped row_idx")


def test_gathered_rows_past_2_31_bytes(ops, dev):
    """Xq of exactly 2^32 bytes: a gathered row's 32-bit byte offset is unsigned, so rows on both sides of 2^31 and the
    very last row are read where the tiled kernel's 64-bit addresses read them."""
    K, N, counts = 4096, 48, (19, 21)
    x_rows = 2 ** 32 // K
    picks = torch.tensor([0, 1, x_rows // 2 - 1, x_rows // 2, x_rows // 2 + 5, x_rows - 2, x_rows - 1])
    Xq = torch.zeros(x_rows, K, dtype=torch.int8, device=dev)
    Xq[picks.to(dev)] = _levels((len(picks), K), 8, seed=9).to(dev)
    g = torch.Generator().manual_seed(10)
    src = picks[torch.randint(0, len(picks), (sum(counts),), generator=g)].to(torch.int32)
    s_x = (torch.rand(x_rows, generator=g) * 1e-2 + 1e-3).to(dev)
    q8 = _levels((2, N, K), 8, seed=11)
    s_w = (torch.rand(2, N, 1, generator=g) * 0.02 + 1e-4).to(dev)
    offsets = _offsets(counts, dev)
    assert ops.gemm_i8_ring_grouped_supported(Xq, q8.to(dev), s_w, src.to(dev))
    got = ops.gemm_i8_ring_grouped(Xq, s_x, q8.to(dev), s_w, offsets, row_idx=src.to(dev))
    want = ops.gemm_i8_grouped(Xq, s_x, q8.to(dev), s_w, offsets, row_idx=src.to(dev))
    torch.cuda.synchronize()
    _same_bits(got, want, "2^32-byte Xq")
    rows = Xq[src.long().to(dev)].cpu()
    for e, (lo, hi) in enumerate(((0, counts[0]), (counts[0], sum(counts)))):
        t = {"weight": q8[e], "weight_scale": s_w[e].cpu(), "weight_shape": torch.tensor([N, K])}
        y64, mag = cr.a8_linear(rows[lo:hi], s_x.cpu()[src.long()[lo:hi]], None, t)
        cr.assert_within(got[lo:hi], y64, cr.gemm_i8_tolerance(got[lo:hi].cpu(), mag, 1), f"expert {e} vs fp64")


# ---- 5: raw C ABI calls ---------------------------------------------------------------------------------------------
def test_caller_owned_y_keeps_its_padding(ops, dev):
    """ldy = N + 17, offsets[E] < R and rows behind R: everything outside Y[r < offsets[E], n < N] keeps its sentinel."""
    from quantool_amd.hip import _lib

    U, R, L = _url()
    counts, N, K = (257, 0, 130), 200, (R + 1) * U
    c = _case(ops, dev, counts, N, K, seed=12)
    Xq, s_x, zp_x, _, _ = c[True]
    live, ldy = sum(counts), N + 17
    n_rows = live + 40                                           # 40 dropped routing slots
    row_idx = torch.cat([c["src"], torch.zeros(40, dtype=torch.int32, device=dev)])
    Ys = {}
    for name in ("qt_gemm_i8_grouped", "qt_gemm_i8_ring_grouped"):
        Ys[name] = _sentinel((n_rows + 3, ldy), torch.bfloat16, dev)
        _raw(ops, name, Xq.data_ptr(), K, row_idx, n_rows, c["offsets"], c["E"], c["Wq"].data_ptr(), _lib.QT_W_INT8, N,
             s_x, zp_x, c["s_w"], 1, c["wsum"], Ys[name], ldy, Xq.shape[0])
    torch.cuda.synchronize()
    Y = Ys["qt_gemm_i8_ring_grouped"]
    assert _untouched(Y[:, N:]) and _untouched(Y[live:]) and not _untouched(Y[:live, :N])
    _same_bits(Y[:live, :N].contiguous(), Ys["qt_gemm_i8_grouped"][:live, :N].contiguous(), "ldy > N")
    _same_bits(Y, Ys["qt_gemm_i8_grouped"], "the whole buffer")


def test_refusals_write_nothing_and_name_the_reason(ops, dev):
    from quantool_amd.hip import _lib
    from quantool_amd.hip._lib import QT_ERR_INVALID, HipBackendError

    U, R, L = _url()
    E, M, N, K = 2, 20, 32, 4 * 128
    Kbig = 32768 + U
    assert K % U == 0
    # every pointer below lies inside one of these buffers with room for the whole operand behind it; the cases whose
    # sizes are numbers only (2^32, E, tiles) come with an all-zero offsets table and row_idx
    xbuf = torch.ones(M * Kbig + 32, dtype=torch.int8, device=dev)
    wbuf = torch.zeros(E * N * Kbig + 32, dtype=torch.int8, device=dev)
    assert xbuf.data_ptr() % 16 == 0 and wbuf.data_ptr() % 16 == 0
    s_x = torch.ones(M, device=dev)
    s_w = torch.ones(E * N * (K // 128), device=dev)
    offsets = torch.tensor([0, 8, M], dtype=torch.int32, device=dev)
    zeros = torch.zeros(4098, dtype=torch.int32, device=dev)
    row_idx = torch.zeros(M, dtype=torch.int32, device=dev)
    Y = _sentinel((M, N), torch.bfloat16, dev)
    X, W, I8, I4 = xbuf.data_ptr(), wbuf.data_ptr(), _lib.QT_W_INT8, _lib.QT_W_INT4_PACKED
    cases = {     # (Xq, K, row_idx, R, offsets, E, Wq, format, N, G, x_rows), reason
        "int4 format": ((X, K, None, M, offsets, E, W, I4, N, 1, M), "int8 weights only"),
        "G > 1": ((X, K, None, M, offsets, E, W, I8, N, K // 128, M), "one scale group"),
        "K % U != 0": ((X, K + 16, None, M, offsets, E, W, I8, N, 1, M), "not a multiple of the k-unit"),
        "K > 32768": ((X, Kbig, None, M, offsets, E, W, I8, N, 1, M), "32768"),
        "Xq misaligned": ((X + 1, K, None, M, offsets, E, W, I8, N, 1, M), "Xq is not 16-byte aligned"),
        "Wq misaligned": ((X, K, None, M, offsets, E, W + 1, I8, N, 1, M), "Wq is not 16-byte aligned"),
        "x_rows K > 2^32": ((X, K, row_idx, M, zeros, E, W, I8, N, 1, 2 ** 32 // K + 1), "2^32"),
        "E > 4096": ((X, K, None, M, zeros, 4097, W, I8, N, 1, M), "4096"),
        "too many tiles": ((X, K, None, 2 ** 31 - 1, zeros, E, W, I8, 2 ** 20, 1, 2 ** 31 - 1), "too many tiles"),
        "x_rows < R": ((X, K, None, M, offsets, E, W, I8, N, 1, M - 1), "without row_idx"),
    }
    for what, ((xq, k, ri, n_rows, off, e, wq, fmt, n, G, x_rows), reason) in cases.items():
        with pytest.raises(HipBackendError) as err:
            _raw(ops, "qt_gemm_i8_ring_grouped", xq, k, ri, n_rows, off, e, wq, fmt, n, s_x, None, s_w, G, None, Y,
                 max(n, N), x_rows)
        assert err.value.status == QT_ERR_INVALID, what
        assert reason in str(err.value), (what, str(err.value))
    torch.cuda.synchronize()
    assert _untouched(Y)
    # the same operands, legal: the call goes through (so the refusals above were about what they name)
    _raw(ops, "qt_gemm_i8_ring_grouped", X, K, row_idx, M, offsets, E, W, I8, N, s_x, None, s_w, 1, None, Y, N,
         2 ** 32 // K)
    torch.cuda.synchronize()
    assert not _untouched(Y)


# ---- 6: the module, end to end --------------------------------------------------------------------------------------
class _Counter:
    def __init__(self, monkeypatch, ops, name):
        self.n = 0
        real = getattr(ops, name)

        def counted(*a, **kw):
            self.n += 1
            return real(*a, **kw)

        monkeypatch.setattr(ops, name, counted)


@pytest.mark.parametrize("level", ["W8A8", "W4A8"])
def test_tiny_mixtral_is_the_same_with_and_without_the_ring(ops, dev, tmp_path, monkeypatch, level):
    import quantool_amd.methods  # noqa: F401
    from quantool_amd.core import QuantizerRegistry
    from quantool_amd.engine.qlinear import QuantizedExperts, load_quantized
    from quantool_amd.evaluate import perplexity
    from tests.test_gpu_moe import _tiny_mixtral

    monkeypatch.chdir(tmp_path)
    model = _tiny_mixtral(dev)
    g = torch.Generator().manual_seed(2)
    data = [{"input_ids": torch.randint(0, 512, (48,), generator=g)} for _ in range(8)]
    q = QuantizerRegistry.create("smoothquant", model_id="synthetic/tiny-mixtral")
    q.quantize(model=model, level=level, dataset=data, num_calibration_samples=8, max_seq_length=64,
               shuffle_calibration_samples=False)
    torch.cuda.synchronize()
    q.save_pretrained(str(tmp_path / "ckpt"))
    del q, model
    model = load_quantized(tmp_path / "ckpt", device=dev)
    banks = [m for m in model.modules() if isinstance(m, QuantizedExperts)]
    assert len(banks) == 2 and all(b.int4 == (level == "W4A8") for b in banks)
    ids = torch.randint(0, 512, (6, 96), generator=torch.Generator().manual_seed(11))
    counter = _Counter(monkeypatch, ops, "gemm_i8_ring_grouped")
    logits, ppl, calls = {}, {}, {}
    for setting in (0, 1):
        monkeypatch.setattr(QuantizedExperts, "ring_min_rows_per_expert", setting)
        before = counter.n
        with torch.no_grad():
            logits[setting] = model(input_ids=ids[:2].to(dev)).logits
        ppl[setting] = perplexity(model, ids, batch_size=4)["perplexity"]
        torch.cuda.synchronize()
        calls[setting] = counter.n - before
    assert calls[0] == 0
    if level == "W8A8":
        assert calls[1] >= 2 * len(banks) * 3          # both products of both banks, in the forward and both batches
    else:                                              # packed int4, G = K/128: never the ring
        assert calls[1] == 0
    assert torch.isfinite(logits[1].float()).all()
    _same_bits(logits[1], logits[0], f"{level} logits, ring_min_rows_per_expert 1 vs 0")
    assert ppl[1] == ppl[0]
