"""tests/ckpt_reference.py, the independent checkpoint reader, against fixtures and hand-built words -- and the loader's
own decoding (``dequantized_weight``, ``QuantizedLinear``'s permuted buffers, ``load_quantized`` on the CPU) against it
at widths that are not multiples of 128 or of 8.  No GPU."""
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import ckpt_reference as cr

GOLD = Path(__file__).resolve().parent / "golden"


def _leaves(q, s, zp=None, g_idx=None, bits=4):
    N, K = q.shape
    t = {"weight_scale": torch.as_tensor(s, dtype=torch.float32), "weight_shape": torch.tensor([N, K])}
    if bits == 4:
        t["weight_packed"] = torch.from_numpy(cr.encode_int4(np.asarray(q), pad_nibble=0xF))
    else:
        t["weight"] = torch.as_tensor(np.asarray(q), dtype=torch.int8)
    if zp is not None:
        t["weight_zero_point"] = torch.as_tensor(zp, dtype=torch.int8)
    if g_idx is not None:
        t["weight_g_idx"] = torch.as_tensor(g_idx, dtype=torch.int32)
    return t


def test_decoder_reproduces_the_gptq_fixture():
    with np.load(GOLD / "gptq_w4a16_asym_static_16x256.npz") as z:
        g = {k: z[k] for k in z.files}
    N, K = g["q"].shape
    assert np.array_equal(cr.decode_int4(g["packed"], K), g["q"])
    t = {"weight_packed": torch.from_numpy(g["packed"]), "weight_shape": torch.tensor([N, K]),
         "weight_scale": torch.from_numpy(g["scale"]), "weight_zero_point": torch.from_numpy(g["zp"])}
    w = cr.contract_weight(t, torch.float32).numpy()
    # equal values; the fixture's oracle writes a zero weight as -0 where its q - zp is a negative zero
    assert np.array_equal(w, g["w_dq"])
    assert np.array_equal(w.view(np.int32)[w != 0], g["w_dq"].view(np.int32)[w != 0])


def test_hand_built_words_decode():
    # nibble j = j: levels j - 8, column j first
    assert cr.decode_int4(np.array([[0x76543210]], np.uint32).view(np.int32), 8).tolist() == [[-8, -7, -6, -5, -4, -3,
                                                                                                -2, -1]]
    # a word with the sign bit set (int32 -0x01234568): nibbles 8 .. F, levels 0 .. 7
    assert cr.decode_int4(np.array([[0xFEDCBA98]], np.uint32).view(np.int32), 8).tolist() == [list(range(8))]
    # K = 77: ten words, the last holding 5 columns; its 3 high nibbles are 0xF and must be ignored
    rng = np.random.default_rng(0)
    q = rng.integers(-8, 8, (3, 77))
    words = np.zeros((3, 10), np.int64)
    for k in range(80):
        nib = q[:, k] + 8 if k < 77 else np.full(3, 0xF)
        words[:, k // 8] |= nib.astype(np.int64) << (4 * (k % 8))
    words = words.astype(np.uint32).view(np.int32)
    assert np.array_equal(cr.decode_int4(words, 77), q)
    assert np.array_equal(cr.encode_int4(q, pad_nibble=0xF), words)


def test_group_of_a_column_picks_its_scale():
    K = 300                                           # G = 3, the last group 44 columns
    N = 4
    q = np.ones((N, K), np.int64)
    s = np.array([[2.0 ** -(1 + g + 3 * n) for g in range(3)] for n in range(N)], np.float32)
    w = cr.contract_weight(_leaves(q, s, bits=8), torch.float32).numpy()
    assert np.array_equal(w[:, :128], np.repeat(s[:, :1], 128, 1))
    assert np.array_equal(w[:, 256:], np.repeat(s[:, 2:], 44, 1))
    g_idx = (np.arange(K) // 128)[np.random.default_rng(1).permutation(K)]
    w = cr.contract_weight(_leaves(q, s, g_idx=g_idx, bits=4), torch.float32).numpy()
    assert np.array_equal(w, s[:, g_idx])
    zp = np.array([[1, -2, 3]] * N)
    w = cr.contract_weight(_leaves(q, s, zp=zp, g_idx=g_idx, bits=4), torch.float32).numpy()
    assert np.array_equal(w, ((1 - zp[:, g_idx]) * s[:, g_idx]).astype(np.float32))
    ch = cr.contract_weight(_leaves(q, s[:, :1], bits=8), torch.float32).numpy()
    assert np.array_equal(ch, np.repeat(s[:, :1], K, 1))


def _random_leaves(N, K, bits, zp, g_idx, grouped, seed):
    rng = np.random.default_rng(seed)
    G = -(-K // 128) if grouped else 1
    q = rng.integers(-8, 8, (N, K)) if bits == 4 else rng.integers(-128, 128, (N, K))
    s = torch.from_numpy((rng.uniform(0.5, 1.5, (N, G)) * 1e-2).astype(np.float32)).to(torch.bfloat16).float()
    z = rng.integers(-3, 4, (N, G)) if zp else None
    gi = (np.arange(K) // 128)[rng.permutation(K)] if g_idx else None
    return _leaves(q, s, z, gi, bits)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("bits,zp,g_idx,grouped", [(4, False, False, True), (4, True, False, True),
                                                   (4, True, True, True), (8, False, False, False),
                                                   (8, True, False, True)])
@pytest.mark.parametrize("K", [1, 77, 129, 200, 330, 1001])
def test_loader_dequantized_weight_equals_the_reference(dtype, bits, zp, g_idx, grouped, K):
    from quantool_amd.engine.qlinear import dequantized_weight

    t = _random_leaves(9, K, bits, zp, g_idx, grouped, seed=K + bits)
    got = dequantized_weight("m", t, dtype)
    assert torch.equal(got.view(torch.int16), cr.contract_weight(t, dtype).view(torch.int16))


@pytest.mark.parametrize("bits,g_idx", [(8, False), (4, False), (4, True), (8, True)])
@pytest.mark.parametrize("K", [77, 200, 330, 1001])
def test_quantized_linear_buffers_compute_the_files_product(bits, g_idx, K):
    """The A8 loader's buffers (columns permuted by col_perm, groups of 128 contiguous permuted columns, wsum) restated
    in fp64 give the product the file defines, for symmetric and asymmetric activation levels."""
    from quantool_amd.engine.qlinear import quantized_linear_from_tensors, unpack_int4

    t = _random_leaves(11, K, bits, False, g_idx, True, seed=3 * K + bits)
    m = quantized_linear_from_tensors("m", t, act_symmetric=False)
    rng = np.random.default_rng(K)
    Xq = torch.from_numpy(rng.integers(-128, 128, (5, K)).astype(np.int8))
    s_x = torch.from_numpy(rng.uniform(1e-3, 1e-2, 5).astype(np.float32))
    zp_x = torch.from_numpy(rng.integers(-128, 128, 5).astype(np.int32))
    want, _ = cr.a8_linear(Xq, s_x, zp_x, t)
    q = (unpack_int4(m.weight, K) if m.int4 else m.weight).double()
    xp = Xq.double() if m.col_perm is None else Xq.double()[:, m.col_perm.long()]
    G = m.weight_scale.shape[1]
    step = K if G == 1 else 128
    y = torch.zeros(5, 11, dtype=torch.float64)
    for g in range(G):
        acc = xp[:, g * step:(g + 1) * step] @ q[:, g * step:(g + 1) * step].T
        tg = acc - zp_x.double()[:, None] * m.wsum.double()[None, :, g]
        y = y + m.weight_scale.double()[None, :, g] * tg
    y = s_x.double()[:, None] * y
    assert torch.allclose(y, want, rtol=1e-12, atol=0)


def _cpu_llama(hidden, inter, seed=0):
    from transformers import LlamaConfig, LlamaForCausalLM

    cfg = LlamaConfig(hidden_size=hidden, intermediate_size=inter, num_hidden_layers=1, num_attention_heads=4,
                      num_key_value_heads=2, vocab_size=128, max_position_embeddings=64, tie_word_embeddings=False,
                      attention_bias=True)
    torch.manual_seed(seed)
    return LlamaForCausalLM(cfg).to(torch.bfloat16).eval()


@pytest.mark.parametrize("a16", ["dequantized", "packed"])
@pytest.mark.parametrize("bits,zp,g_idx", [(4, False, False), (4, True, True), (8, True, False)])
def test_load_quantized_on_cpu_matches_the_files(tmp_path, a16, bits, zp, g_idx):
    """A synthetic grouped checkpoint of a Llama 200 wide with intermediate 330 (a partial packed word, ragged last
    groups), loaded on the CPU: every quantized module's output against fp64 on the file's own decoding."""
    from quantool_amd.engine.qlinear import load_quantized

    model = _cpu_llama(200, 330)
    sd = model.state_dict()
    linears = {n: tuple(m.weight.shape) for n, m in model.named_modules()
               if isinstance(m, torch.nn.Linear) and n.startswith("model.layers.")}
    dense = {k: v for k, v in sd.items() if k.rpartition(".")[0] not in linears or not k.endswith(".weight")}
    cfg = model.config.to_dict()
    written = cr.write_synthetic(tmp_path / "ckpt", cfg, dense, linears, bits=bits, zero_point=zp, g_idx=g_idx,
                                 seed=bits)
    loaded = load_quantized(tmp_path / "ckpt", device="cpu", a16=a16)
    seen = {}
    mods = {n: loaded.get_submodule(n) for n in written}
    handles = [m.register_forward_hook(lambda mod, i, o, n=n: seen.__setitem__(n, (i[0].detach(), o.detach())))
               for n, m in mods.items()]
    ids = torch.randint(0, 128, (2, 9), generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        loaded(input_ids=ids)
    for h in handles:
        h.remove()
    assert set(seen) == set(written)
    for n, (x, y) in seen.items():
        K = written[n]["weight_shape"][1].item()
        bias = getattr(mods[n], "bias", None)
        y64, mag = cr.a16_linear(x.reshape(-1, K), written[n], bias)
        y2 = y.reshape(y64.shape)
        cr.assert_within(y2, y64, cr.gemv_tolerance(y2, mag, K), n)
