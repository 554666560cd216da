"""``StoredWeight`` (engine/stored_weight.py) on the CPU: what ``from_leaves`` and ``require_kernel_layout`` refuse, the
round trip through ``leaves``, and a bank [E, ...] against its experts one by one.  No GPU call."""
import pytest
import torch

from quantool_amd.engine.qlinear import quantized_linear_from_tensors, weight_only_linear_from_tensors
from quantool_amd.engine.stored_weight import StoredWeight, group_sums, pack_int4, unpack_int4

N, K = 6, 300          # 38 packed words, the last one partial; 3 groups, the last one ragged
G = (K + 127) // 128


def _leaves(seed, int4=True, zp=False, g_idx=False):
    g = torch.Generator().manual_seed(seed)
    q = torch.randint(-8, 8, (N, K), generator=g, dtype=torch.int8)
    t = {"weight_scale": (torch.rand(N, G, generator=g) * 0.02 + 1e-3).to(torch.bfloat16),
         "weight_shape": torch.tensor([N, K])}
    t["weight_packed" if int4 else "weight"] = pack_int4(q) if int4 else q
    if zp:
        t["weight_zero_point"] = torch.randint(-3, 4, (N, G), generator=g, dtype=torch.int8)
    if g_idx:
        t["weight_g_idx"] = (torch.arange(K) // 128)[torch.randperm(K, generator=g)].to(torch.int32)
    return t, q


def test_from_leaves_checks_the_levels_and_the_column_groups():
    t, _ = _leaves(0, g_idx=True)
    w = StoredWeight.from_leaves("m", t)
    assert (w.N, w.K, w.G, w.int4) == (N, K, G, True)
    assert w.scale.dtype == torch.float32 and w.g_idx.dtype == torch.int32 and w.zero_point is None
    with pytest.raises(ValueError, match="weight_packed must be int32"):
        StoredWeight.from_leaves("m", {**t, "weight_packed": t["weight_packed"][:, :-1]})
    with pytest.raises(ValueError, match="without weight_shape"):
        StoredWeight.from_leaves("m", {k: v for k, v in t.items() if k != "weight_shape"})
    with pytest.raises(ValueError, match="expected an int8 weight"):
        StoredWeight.from_leaves("m", {k: v for k, v in t.items() if k != "weight_packed"})
    with pytest.raises(ValueError, match="weight_g_idx does not match"):
        StoredWeight.from_leaves("m", {**t, "weight_g_idx": t["weight_g_idx"] + 1})
    with pytest.raises(ValueError, match="weight_g_idx does not match"):
        StoredWeight.from_leaves("m", {**t, "weight_g_idx": t["weight_g_idx"][:-1]})
    # any scale layout is read: the dequantised load takes what the kernels would not
    odd = StoredWeight.from_leaves("m", {**t, "weight_scale": torch.ones(N, G + 2), "weight_g_idx": t["weight_g_idx"]})
    assert odd.dequantize(torch.float32).shape == (N, K)


@pytest.mark.parametrize("build,hint", [(lambda t: quantized_linear_from_tensors("m", t, True), False),
                                        (lambda t: weight_only_linear_from_tensors("m", t), True)])
def test_kernel_layout_refusals(build, hint):
    t, _ = _leaves(1)
    build(t)
    build({**t, "weight_scale": t["weight_scale"][:, :1]})
    for bad in (torch.ones(N, 2), torch.ones(N + 1, G), torch.ones(N, G, 1)):
        with pytest.raises(ValueError, match="neither channel-wise nor groups of 128") as e:
            build({**t, "weight_scale": bad})
        assert ("a16='dequantized'" in str(e.value)) == hint


def test_zero_points_are_checked_where_they_are_taken():
    t, _ = _leaves(2, zp=True)
    with pytest.raises(ValueError, match="the int8 GEMM has no weight zero-point"):
        quantized_linear_from_tensors("m", t, True)
    assert weight_only_linear_from_tensors("m", t).weight_zero_point.dtype == torch.int8
    for bad in (torch.zeros(N, G), torch.full((N, G), 128, dtype=torch.int32), torch.zeros(N, 1, dtype=torch.int8)):
        with pytest.raises(ValueError, match="weight_zero_point must be integers"):
            weight_only_linear_from_tensors("m", {**t, "weight_zero_point": bad})


@pytest.mark.parametrize("int4", [True, False])
def test_leaves_round_trip(int4):
    t, q = _leaves(3, int4=int4, zp=True, g_idx=True)
    w = StoredWeight.from_leaves("m", t)
    back = StoredWeight.from_leaves("m", w.leaves())
    assert all(torch.equal(a, b) for a, b in zip(w[:4], back[:4])) and w[4:] == back[4:]
    s = t["weight_scale"].float()[:, t["weight_g_idx"].long()]
    z = t["weight_zero_point"].float()[:, t["weight_g_idx"].long()]
    assert torch.equal(w.dequantize(torch.bfloat16), ((q.float() - z) * s).to(torch.bfloat16))


@pytest.mark.parametrize("zp,g_idx", [(False, False), (True, True)])
def test_a_bank_is_its_experts(zp, g_idx):
    E = 3
    experts = []
    for e in range(E):
        a = StoredWeight.from_leaves("a", _leaves(10 + e, zp=zp, g_idx=g_idx)[0])
        b = StoredWeight.from_leaves("b", _leaves(20 + e, zp=zp)[0])._replace(g_idx=a.g_idx)
        experts.append([a, b])
    bank = StoredWeight.stack("bank", experts).require_kernel_layout("bank")
    assert (bank.N, bank.K, bank.G) == (2 * N, K, G) and tuple(bank.levels.shape) == (E, 2 * N, (K + 7) // 8)
    dense = bank.dequantize(torch.bfloat16)
    for e, (a, b) in enumerate(experts):
        assert torch.equal(dense[e], torch.cat([a.dequantize(torch.bfloat16), b.dequantize(torch.bfloat16)]))
    q = unpack_int4(bank.levels, K)
    assert all(torch.equal(q[e], unpack_int4(bank.levels[e], K)) for e in range(E))
    for groups in (1, G):
        sums = group_sums(q, groups)
        assert all(torch.equal(sums[e], group_sums(q[e], groups)) for e in range(E))
    with pytest.raises(ValueError, match="mix formats or group counts"):
        StoredWeight.stack("bank", [experts[0], [experts[1][0], experts[1][1]._replace(zero_point=None if zp else
                                                                                     torch.zeros(N, G))]])
    if g_idx:
        with pytest.raises(ValueError, match="group their columns differently"):
            StoredWeight.stack("bank", [[experts[0][0], experts[0][1]._replace(g_idx=experts[1][0].g_idx)]])
