"""qt_moe_gemm_i8_wide: qt_gemm_i8_mid's weight-streaming 16-column tile over an A8 expert bank.

Its contract is bit equality with the tiled qt_gemm_i8_grouped on the same arguments, so every comparison here is on bit
patterns (``.view(torch.int16)`` + ``torch.equal``), against two yardsticks: ``ops.gemm_i8_grouped`` on the same bank and
one dense ``ops.gemm_i8`` per expert on that expert's gathered rows.  Those would pass kernels wrong in the same way, so
the same cases also go against the fp64 reference of tests/ckpt_reference.py within the project's own bound for this
sequence (``gemm_i8_tolerance``); an identity test pins the expert, the m-tile and the row every routed row reads.  Shapes
are the smallest at which the kernel takes another path: MT = 2 / 4 / 8 m-tiles (R <= 32, <= 64, more), experts of one,
two and three 128-row slots, k-blocks of 128 around the four waves and around a batch (16 k-blocks at MT <= 4, 8 at
MT = 8), column tiles of 16."""
import pytest
import torch

from tests import ckpt_reference as cr
from tests.test_gpu_i8_ring_grouped import _acts, _offsets, _twice
from tests.test_gpu_i8_skinny import _Counter, _greedy_logits, _same_bits, _sentinel, _untouched
from tests.test_gpu_runtime_edges import _leaves, _levels, _qweight, cr_wsum

pytestmark = pytest.mark.gpu

NAME = "qt_moe_gemm_i8_wide"
KB = 128
BANKS = [(8, False), (8, True), (4, False), (4, True)]          # (bits, one scale per 128 columns)
# (asymmetric activations, output dtype, gathered rows): every value of each, not their product
SOME = [(False, torch.bfloat16, True), (True, torch.float16, True), (True, torch.bfloat16, False),
        (False, torch.float16, False)]
ALL = [(a, d, g) for a in (False, True) for d in (torch.bfloat16, torch.float16) for g in (True, False)]


def _bank(q, bits, G, seed, dev):
    """Checkpoint leaves per expert and the stacked device operands of the levels q int8 [E, N, K]."""
    E = q.shape[0]
    leaves = [_leaves(q[e], bits, G, seed=seed + e) for e in range(E)]
    Wq = torch.stack([_qweight(t, "cpu") for t in leaves]).contiguous().to(dev)
    s_w = torch.stack([t["weight_scale"] for t in leaves]).contiguous().to(dev)
    wsum = torch.stack([cr_wsum(q[e], G) for e in range(E)]).contiguous().to(dev)
    return leaves, Wq, s_w, wsum


def _case(ops, dev, counts, N, K, bits, grouped, seed):
    """A bank, a routing with ``counts`` rows per expert and both quantisations of the source rows, with the fp64
    reference of every routed row (computed once per case)."""
    E, n_rows = len(counts), sum(counts)
    G = K // KB if grouped else 1
    q = _levels((E, N, K), bits, seed=seed)
    leaves, Wq, s_w, wsum = _bank(q, bits, G, seed + 100, dev)
    T, src = _twice(n_rows, seed + 2)
    X = _acts(T, K, dev, seed + 3)
    out = {"E": E, "rows": n_rows, "N": N, "K": K, "G": G, "counts": counts, "Wq": Wq, "s_w": s_w, "wsum": wsum,
           "offsets": _offsets(counts, dev), "src": src.to(dev)}
    off = [0] + torch.tensor(counts).cumsum(0).tolist()
    for asym in (False, True):
        Xq, s_x, zp_x = ops.quantize_tokens_i8(X, symmetric=not asym)
        y64, mag = torch.zeros(n_rows, N, dtype=torch.float64), torch.zeros(n_rows, N, dtype=torch.float64)
        for e in range(E):
            lo, hi = off[e], off[e + 1]
            if hi > lo:
                rows = src[lo:hi].long()
                y64[lo:hi], mag[lo:hi] = cr.a8_linear(Xq.cpu()[rows], s_x.cpu()[rows],
                                                      None if zp_x is None else zp_x.cpu()[rows], leaves[e])
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
    kw = dict(row_idx=ri, K=c["K"], zp_x=za, wsum=ws, out_dtype=dt)
    assert ops.moe_gemm_i8_wide_supported(A, c["Wq"], c["s_w"], ri)
    want = ops.gemm_i8_grouped(A, sa, c["Wq"], c["s_w"], c["offsets"], **kw)
    got = ops.moe_gemm_i8_wide(A, sa, c["Wq"], c["s_w"], c["offsets"], **kw)
    torch.cuda.synchronize()
    assert got.shape == (c["rows"], c["N"]) and got.dtype == dt
    _same_bits(got, want, f"{what} vs gemm_i8_grouped")
    off = c["offsets"].cpu().tolist()
    for e in range(c["E"]):                      # the second yardstick: the dense tiled kernel per expert
        lo, hi = off[e], off[e + 1]
        if hi > lo:
            r = src[lo:hi]
            one = ops.gemm_i8(Xq[r].contiguous(), s_x[r].contiguous(), c["Wq"][e], c["s_w"][e], K=c["K"],
                              zp_x=None if zp_x is None else zp_x[r].contiguous(),
                              wsum=None if ws is None else ws[e], out_dtype=dt)
            _same_bits(got[lo:hi], one, f"{what} expert {e} vs gemm_i8")
    cr.assert_within(got, y64, cr.gemm_i8_tolerance(got.cpu(), mag, c["G"]), f"{what} vs fp64")


def _forms(ops, c, forms, what):
    for asym, dt, gather in forms:
        _check(ops, c, asym, dt, gather, f"{what} asym={asym} {dt} gather={gather}")


# ---- 1: the expert walk and the three instances ---------------------------------------------------------------------
COUNTS = {
    "tiles of one expert": (0, 1, 15, 16, 17, 0, 33, 0),                    # R = 82: MT = 8
    "one, two, three slots": (0, 127, 128, 129, 0, 300),                    # R = 684
    "R=17": (0, 1, 0, 0, 16, 0), "R=32": (0, 15, 0, 0, 17, 0),              # MT = 2
    "R=33": (0, 16, 0, 0, 17, 0), "R=64": (0, 31, 0, 0, 33, 0),             # MT = 4
    "R=65": (0, 32, 0, 0, 33, 0),                                           # MT = 8
    "E=1": (40,), "E=64": (3,) * 64,
}


@pytest.mark.parametrize("bits,grouped", BANKS)
@pytest.mark.parametrize("counts", list(COUNTS))
def test_ragged_experts(ops, dev, counts, bits, grouped):
    """Empty experts first, last and adjacent; one row; a tile less one, exactly one tile, a tile and one row; experts of
    one, two and three 128-row slots; every total at which the host picks another instance."""
    c = _case(ops, dev, COUNTS[counts], 33, 5 * KB, bits, grouped, seed=len(counts) + bits)
    _forms(ops, c, ALL if counts == "tiles of one expert" else SOME, counts)


# ---- 2: K around the waves and the batches --------------------------------------------------------------------------
@pytest.mark.parametrize("bits,grouped", BANKS)
@pytest.mark.parametrize("kblocks", [1, 3, 4, 5, 8, 9, 16, 17])
def test_k_blocks(ops, dev, kblocks, bits, grouped):
    """k-blocks of 128: fewer than the waves, the waves, one more; one batch and one more, for the batch of 16 (MT = 4,
    R = 33) and the batch of 8 (MT = 8, R = 90)."""
    for counts in ((3, 0, 30), (70, 0, 20)):
        c = _case(ops, dev, counts, 17, kblocks * KB, bits, grouped, seed=kblocks + sum(counts))
        _forms(ops, c, SOME, f"K={kblocks * KB} R={sum(counts)}")


# ---- 3: N around the column tile ------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,grouped", BANKS)
@pytest.mark.parametrize("N", [1, 15, 16, 17, 33])
def test_column_tiles(ops, dev, N, bits, grouped):
    c = _case(ops, dev, (0, 20, 45), N, 3 * KB, bits, grouped, seed=N)
    _forms(ops, c, SOME, f"N={N}")


# ---- 4: which expert, m-tile and row a routed row reads -------------------------------------------------------------
@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("counts", [(5, 0, 11), (5, 0, 40, 19), (0, 130, 3)])
def test_one_hot_rows_read_their_experts_weights(ops, dev, counts, bits):
    """Xq = the K x K identity, unit s_x, no zero-point: routed row r of expert e, gathered from source row k, is
    s_w[e, n, k // 128] (float)W[e][n, k] exactly.  The weights differ per expert and per row and s_w[e, n, g] =
    e G + g + 1 differs per (expert, group), so a row routed to the wrong expert, m-tile or source row changes a
    value."""
    K, N = 4 * KB, 20
    E, n_rows, G = len(counts), sum(counts), K // KB
    W = _levels((E, N, K), bits, seed=77)
    assert len({tuple(r) for r in W.reshape(E * N, K).tolist()}) == E * N
    s_w = (torch.arange(E)[:, None, None] * G + torch.arange(G)[None, None, :] + 1).float().expand(E, N, G).contiguous()
    leaves, Wq, _, _ = _bank(W, bits, G, 1, dev)
    src = torch.randperm(K, generator=torch.Generator().manual_seed(6))[:n_rows].to(torch.int32)
    assert not torch.equal(src, src.sort().values)
    expert = torch.repeat_interleave(torch.arange(E), torch.tensor(counts))
    want = W[expert, :, src.long()].float() * s_w[expert, :, src.long() // KB]          # [rows, N]
    assert float(want.abs().max()) <= 2048                                             # exact in fp16
    Xq = torch.eye(K, dtype=torch.int8, device=dev)
    Y = ops.moe_gemm_i8_wide(Xq, torch.ones(K, device=dev), Wq, s_w.to(dev), _offsets(counts, dev),
                             row_idx=src.to(dev), K=K, out_dtype=torch.float16)
    torch.cuda.synchronize()
    _same_bits(Y.cpu(), want.to(torch.float16).contiguous(), f"identity, counts {counts}")


# ---- 5: raw C ABI calls: nothing outside Y[m < offsets[E], n < N] is written ------------------------------------------
def _raw(ops, name, Xq, K, row_idx, n_rows, offsets, E, Wq, N, s_x, zp_x, s_w, G, wsum, Y, ldy, x_rows):
    from quantool_amd.hip import _lib

    fmt = _lib.QT_W_INT4_PACKED if Wq.dtype == torch.int32 else _lib.QT_W_INT8
    extra = (x_rows,) if name == NAME else ()
    _lib.check(name, getattr(_lib.load(), name)(
        Xq.data_ptr(), K, ops._ptr(row_idx), n_rows, offsets.data_ptr(), E, Wq.data_ptr(), fmt, N, s_x.data_ptr(),
        ops._ptr(zp_x), s_w.data_ptr(), G, ops._ptr(wsum), Y.data_ptr(), ops._dtype_code(Y), ldy, *extra, ops._stream()))


@pytest.mark.parametrize("bits,grouped", BANKS)
def test_caller_owned_y_keeps_its_padding(ops, dev, bits, grouped):
    """Y is a view into a larger buffer with ldy = N + 17: the gaps, the rows >= offsets[E] (40 dropped routing slots)
    and everything in front of and behind the view keep their sentinel."""
    counts, N, K = (129, 0, 17, 1), 33, 5 * KB
    c = _case(ops, dev, counts, N, K, bits, grouped, seed=12)
    Xq, s_x, zp_x, _, _ = c[True]
    live, ldy = sum(counts), N + 17
    n_rows = live + 40
    row_idx = torch.cat([c["src"], torch.zeros(40, dtype=torch.int32, device=dev)])
    Ys = {}
    for name in ("qt_gemm_i8_grouped", NAME):
        buf = _sentinel((n_rows + 6, ldy), torch.bfloat16, dev)
        Ys[name] = buf
        _raw(ops, name, Xq, K, row_idx, n_rows, c["offsets"], c["E"], c["Wq"], N, s_x, zp_x, c["s_w"], c["G"],
             c["wsum"], buf[3:], ldy, Xq.shape[0])
    torch.cuda.synchronize()
    Y = Ys[NAME]
    assert _untouched(Y[:3]) and _untouched(Y[3 + live:]) and _untouched(Y[:, N:]) and not _untouched(Y[3:3 + live, :N])
    _same_bits(Y, Ys["qt_gemm_i8_grouped"], "the whole buffer")


@pytest.mark.parametrize("bits,grouped", BANKS)
def test_indices_and_offsets_are_clamped(ops, dev, bits, grouped):
    """Xq, s_x and zp_x are the first x_rows rows of larger allocations whose rest would change the result; some
    row_idx entries lie at or past x_rows or below 0, and the offsets table runs past R.  The result is the tiled
    kernel's on the clamped indices and the clamped table, and Y's sentinels are intact: an index that was not clamped
    would show as a wrong number."""
    counts, N, K = (20, 0, 45), 17, 3 * KB
    c = _case(ops, dev, counts, N, K, bits, grouped, seed=8)
    Xq, s_x, zp_x, _, _ = c[True]
    x_rows, R = Xq.shape[0], sum(counts)
    big_x = torch.full((x_rows + 64, K), 77, dtype=torch.int8, device=dev)
    big_s = torch.full((x_rows + 64,), 1e3, device=dev)
    big_z = torch.full((x_rows + 64,), -99, dtype=torch.int32, device=dev)
    big_x[:x_rows], big_s[:x_rows], big_z[:x_rows] = Xq, s_x, zp_x
    Xv, sv, zv = big_x[:x_rows], big_s[:x_rows], big_z[:x_rows]
    assert Xv.data_ptr() % 16 == 0
    wild, tame = c["src"].clone(), c["src"].clone()
    wild[::3], tame[::3] = -5, 0
    wild[1::3], tame[1::3] = x_rows, x_rows - 1
    wild[4::9], tame[4::9] = 2 ** 31 - 1, x_rows - 1
    off_wild = torch.tensor([0, 20, 20, R + 50], dtype=torch.int32, device=dev)
    want = ops.gemm_i8_grouped(Xq, s_x, c["Wq"], c["s_w"], c["offsets"], row_idx=tame, K=K, zp_x=zp_x, wsum=c["wsum"])
    ldy = N + 17
    buf = _sentinel((R + 6, ldy), torch.bfloat16, dev)
    _raw(ops, NAME, Xv, K, wild, R, off_wild, c["E"], c["Wq"], N, sv, zv, c["s_w"], c["G"], c["wsum"], buf[3:], ldy,
         x_rows)
    torch.cuda.synchronize()
    assert _untouched(buf[:3]) and _untouched(buf[3 + R:]) and _untouched(buf[:, N:])
    _same_bits(buf[3:3 + R, :N].contiguous(), want, "clamped row_idx and offsets")
    # through the wrapper: x_rows is the view's row count
    got = ops.moe_gemm_i8_wide(Xv, sv, c["Wq"], c["s_w"], off_wild, row_idx=wild, K=K, zp_x=zv, wsum=c["wsum"])
    torch.cuda.synchronize()
    _same_bits(got, want, "clamped, through ops")


def test_an_all_empty_table_writes_nothing(ops, dev):
    E, n_rows, N, K = 5, 70, 20, 2 * KB
    Xq = torch.ones(n_rows, K, dtype=torch.int8, device=dev)
    Wq = torch.ones(E, N, K, dtype=torch.int8, device=dev)
    s_x, s_w = torch.ones(n_rows, device=dev), torch.ones(E, N, 1, device=dev)
    for table in ([0] * (E + 1), [7] * (E + 1), [9, 5, 5, 2, 0, 0]):       # empty, empty at 7, descending: clamped empty
        Y = _sentinel((n_rows, N), torch.bfloat16, dev)
        offsets = torch.tensor(table, dtype=torch.int32, device=dev)
        _raw(ops, NAME, Xq, K, None, n_rows, offsets, E, Wq, N, s_x, None, s_w, 1, None, Y, N, n_rows)
        torch.cuda.synchronize()
        assert _untouched(Y), table


def test_refusals_write_nothing_and_name_the_reason(ops, dev):
    from quantool_amd.hip._lib import QT_ERR_INVALID, HipBackendError

    E, M, N, K = 2, 20, 32, 4 * KB
    Kbig = 32768 + KB
    xbuf = torch.ones(M * Kbig + 32, dtype=torch.int8, device=dev)
    wbuf = torch.zeros(E * N * Kbig + 32, dtype=torch.int8, device=dev)
    assert xbuf.data_ptr() % 16 == 0 and wbuf.data_ptr() % 16 == 0
    s_x = torch.ones(M, device=dev)
    s_w = torch.ones(E * N * (Kbig // KB), device=dev)
    zp = torch.zeros(M, dtype=torch.int32, device=dev)
    offsets = torch.tensor([0, 8, M], dtype=torch.int32, device=dev)
    zeros = torch.zeros(4098, dtype=torch.int32, device=dev)
    row_idx = torch.zeros(M, dtype=torch.int32, device=dev)
    Y = _sentinel((M, N), torch.bfloat16, dev)
    X, W = xbuf[:M * K].view(M, K), wbuf[:E * N * K].view(E, N, K)
    X1, W4 = xbuf[1:M * K + 1].view(M, K), wbuf[4:E * N * K + 4].view(E, N, K)
    Xb, Wb = xbuf[:M * Kbig].view(M, Kbig), wbuf[:E * N * Kbig].view(E, N, Kbig)
    G = K // KB
    big_r = 128 * 65534 + 1
    cases = {     # (Xq, K, row_idx, R, offsets, E, Wq, zp_x, G, x_rows), reason
        "K % 128 != 0": ((X, K + 16, None, M, offsets, E, W, None, G, M), "not a multiple of the k-unit"),
        "K > 32768": ((Xb, Kbig, None, M, offsets, E, Wb, None, 1, M), "32768"),
        "G == 2": ((X, K, None, M, offsets, E, W, None, 2, M), "must be 1 or K / 128"),
        "Xq misaligned": ((X1, K, None, M, offsets, E, W, None, G, M), "Xq is not 16-byte aligned"),
        "Wq misaligned": ((X, K, None, M, offsets, E, W4, None, G, M), "Wq is not 16-byte aligned"),
        "x_rows K > 2^32": ((X, K, row_idx, M, zeros, E, W, None, G, 2 ** 32 // K + 1), "2^32"),
        "E > 4096": ((X, K, None, M, zeros, 4097, W, None, G, M), "4096"),
        "R > 2^31 - 1": ((X, K, None, 2 ** 31, zeros, E, W, None, G, 2 ** 31), "too large"),
        "too many slots": ((X, K, None, big_r, zeros, E, W, None, G, big_r), "row-tile slots"),
        "x_rows < R": ((X, K, None, M, offsets, E, W, None, G, M - 1), "without row_idx"),
        "zp_x without wsum": ((X, K, None, M, offsets, E, W, zp, G, M), "zp_x needs wsum"),
    }
    for what, ((xq, k, ri, n_rows, off, e, wq, z, g, x_rows), reason) in cases.items():
        with pytest.raises(HipBackendError) as err:
            _raw(ops, NAME, xq, k, ri, n_rows, off, e, wq, N, s_x, z, s_w, g, None, Y, N, x_rows)
        assert err.value.status == QT_ERR_INVALID, what
        assert reason in str(err.value) and str(err.value).count(NAME), (what, str(err.value))
    torch.cuda.synchronize()
    assert _untouched(Y)
    # the same operands, legal: the call goes through (so the refusals above were about what they name)
    _raw(ops, NAME, X, K, row_idx, M, offsets, E, W, N, s_x, None, s_w, G, None, Y, N, 2 ** 32 // K)
    torch.cuda.synchronize()
    assert not _untouched(Y)


# ---- 6: the module, end to end --------------------------------------------------------------------------------------
WIDE_ATTRS = ("wide_max_rows_per_expert", "wide_w4_max_rows_per_expert")


@pytest.mark.parametrize("int4", [False, True])
def test_quantized_experts_forward_is_the_same_with_and_without_the_form(ops, dev, monkeypatch, int4):
    import torch.nn as nn

    from quantool_amd.engine.qlinear import QuantizedExperts, pack_int4

    Hd, I, E, k = 512, 640, 4, 2
    bits = 4 if int4 else 8
    gu, dn = _levels((E, 2 * I, Hd), bits, seed=1), _levels((E, Hd, I), bits, seed=2)
    g = torch.Generator().manual_seed(3)
    s_gu = torch.rand(E, 2 * I, Hd // 128 if int4 else 1, generator=g) * 1e-2 + 1e-4
    s_dn = torch.rand(E, Hd, I // 128 if int4 else 1, generator=g) * 1e-2 + 1e-4
    if int4:
        gu, dn = torch.stack([pack_int4(w) for w in gu]), torch.stack([pack_int4(w) for w in dn])
    qe = QuantizedExperts(Hd, I, gu, s_gu, dn, s_dn, nn.SiLU(), act_symmetric=not int4).to(dev)
    monkeypatch.setattr(QuantizedExperts, "wide_min_k", 512)
    monkeypatch.setattr(QuantizedExperts, "wide_max_n", 0)
    monkeypatch.setattr(QuantizedExperts, "grouped_max_tokens", 16)
    counter = _Counter(monkeypatch, ops, "moe_gemm_i8_wide")
    for T in (17, 40, 130):
        gt = torch.Generator().manual_seed(T)
        x = (torch.randn(T, Hd, generator=gt) * 2).to(torch.bfloat16).to(dev)
        idx = torch.stack([torch.randperm(E, generator=gt)[:k] for _ in range(T)]).to(dev)
        w = torch.softmax(torch.randn(T, k, generator=gt), -1).to(dev)
        outs = {}
        for setting in (0, 10 ** 6):
            for name in WIDE_ATTRS:
                monkeypatch.setattr(QuantizedExperts, name, setting)
            before = counter.n
            with torch.no_grad():
                outs[setting] = qe(x, idx, w)
            assert counter.n - before == (2 if setting else 0)
        torch.cuda.synchronize()
        assert torch.isfinite(outs[0].float()).all() and bool(outs[0].any())
        assert torch.equal(outs[10 ** 6], outs[0]), f"T={T}"


@pytest.mark.parametrize("level", ["W8A8", "W4A8"])
def test_tiny_mixtral_is_the_same_with_and_without_the_form(ops, dev, tmp_path, monkeypatch, level):
    """The tiny Mixtral checkpoint (H = I = 256, so ``wide_min_k`` is lowered to 256 here): the perplexity and a 16-step
    greedy decode of 24 sequences at once, tokens and every step's logits, are the same with both banks' products on the
    new form and with none on it."""
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
    ids = torch.randint(0, 512, (24, 40), generator=torch.Generator().manual_seed(11))
    prompt = ids[:, :5].to(dev)
    assert prompt.shape[0] > QuantizedExperts.grouped_max_tokens
    monkeypatch.setattr(QuantizedExperts, "wide_min_k", 256)
    monkeypatch.setattr(QuantizedExperts, "wide_max_n", 0)
    counter = _Counter(monkeypatch, ops, "moe_gemm_i8_wide")
    ppl, logits, tokens, calls = {}, {}, {}, {}
    for setting in (0, 10 ** 6):
        for name in WIDE_ATTRS:
            monkeypatch.setattr(QuantizedExperts, name, setting)
        before = counter.n
        ppl[setting] = perplexity(model, ids[:6], batch_size=3)["perplexity"]
        logits[setting], tokens[setting] = _greedy_logits(model, prompt, 16)
        torch.cuda.synchronize()
        calls[setting] = counter.n - before
    assert calls[0] == 0
    assert calls[10 ** 6] >= 2 * len(banks) * (2 + 17)     # both products of both banks: two batches, prompt + 16 steps
    assert ppl[10 ** 6] == ppl[0]
    assert torch.equal(tokens[10 ** 6], tokens[0])
    for step, (a, b) in enumerate(zip(logits[10 ** 6], logits[0])):
        _same_bits(a, b, f"{level} logits of step {step}")
