"""``qt_moe_gemm_wq_wide``'s surface without a GPU: the header, the ctypes table, the built library and the resource
table carry it, ``ops.moe_gemm_wq_wide_supported`` / ``ops.moe_gemm_wq_wide`` refuse what the kernel does not take
before they touch the library, ``WeightOnlyExperts`` dispatches on ``wide_min_tokens`` / ``wide_max_tokens``, and
``load_quantized(..., a16_experts_wide_tokens=)`` switches the extended range on.

One refusal of the C contract has no form at the ``ops`` surface: without ``row_idx`` the wrapper passes R = X's row
count, so ``x_rows < R`` cannot be asked for; tests/test_gpu_wq_moe_wide.py holds the raw ABI to it."""
import re

import pytest
import torch
import torch.nn as nn

from tests.i8_fake_ops import aligned_i8, aligned_i32, check_surface, header_constants, header_text
from tests.test_moe_loader import BANK, _write
from tests.test_wq_stream_dispatch import _no_library, _x

NAME = "qt_moe_gemm_wq_wide"
CSRC = __import__("pathlib").Path(__file__).resolve().parent.parent / "quantool_amd" / "csrc"
MT_INSTANCES = (1, 2, 4, 8)


# ---- surface --------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_point_and_the_constants():
    from quantool_amd.hip import ops

    check_surface("header", NAME)
    assert header_constants("QT_MOE_WQ_WIDE_") == {"QT_MOE_WQ_WIDE_K_UNIT": ops.MOE_WQ_WIDE_K_UNIT,
                                                   "QT_MOE_WQ_WIDE_MAX_E": ops.MOE_WQ_WIDE_MAX_E,
                                                   "QT_MOE_WQ_WIDE_MAX_SLOTS": ops.MOE_WQ_WIDE_MAX_SLOTS}
    assert ops.MOE_WQ_WIDE_K_UNIT == 128 and ops.MOE_WQ_WIDE_MAX_SLOTS == 65535


def test_header_paragraph_states_the_contract():
    raw = header_text()[0]
    para = raw[raw.index(f"/* {NAME}:"):]
    para = " ".join(para[:para.index("*/")].replace("*", " ").split())
    for phrase in ("Every row of Y is bit-identical to qt_gemm_wq_grouped's row on the same arguments",
                   "rows >= offsets[E] are not written",
                   "row_idx values are clamped into [0, x_rows), not followed",
                   "65535",
                   "returns QT_ERR_INVALID before any launch",
                   "the smallest of 1, 2, 4, 8 with 16 MT >= ceil(R / E)"):
        assert phrase in para, phrase


def test_ctypes_signature_is_the_grouped_one_plus_x_rows():
    from ctypes import c_int64

    from quantool_amd.hip import _lib

    res, args = _lib.SIGNATURES[NAME]
    gres, gargs = _lib.SIGNATURES["qt_gemm_wq_grouped"]
    assert res == gres and args == gargs[:-1] + [c_int64] + gargs[-1:]      # x_rows in front of the stream


def test_library_exports_it_and_no_workspace_function_was_added():
    from quantool_amd.hip import _lib

    check_surface("library", NAME)
    assert len([n for n in _lib.SIGNATURES if n.endswith("_workspace_bytes")]) == 14
    assert not [n for n in _lib.SIGNATURES if ("stream" in n or "mid" in n) and n not in
                ("qt_gemm_wq_stream", "qt_gemm_i8_mid")]


def _resources(stem):
    from quantool_amd.csrc import build

    res = build.OBJ_DIR / f"{stem}.resources.txt"
    if not res.exists():
        import __graft_entry__ as g

        g.build()
    return res.read_text().splitlines()


def test_every_instance_is_free_of_scratch_and_spills():
    from quantool_amd.csrc import build

    rows = [line for line in _resources("wq_moe_wide") if "moe_gemm_wq_wide_kernel" in line]
    assert len(rows) == len(MT_INSTANCES) * 2 * 2 * 2           # m-tiles x int4 / int8 x bf16 / fp16 x zp / none
    for row in rows:
        assert "wq_stream_kernel" not in row
        assert "scratch 0\t" in row and "vgpr_spill 0\t" in row, row
        assert int(re.search(r"lds (\d+)", row).group(1)) <= 65536, row
    for mt in MT_INSTANCES:                                     # the last template argument is the tile count
        assert len([r for r in rows if re.search(rf"ELi{mt}EEEv", r)]) == 8, mt
    assert "moe_gemm_wq_wide_kernel" in build.NO_SPILL_KERNELS


def test_the_dense_kernels_kept_their_object():
    assert len([line for line in _resources("wq") if "wq_stream_kernel" in line]) == 64
    assert not [line for line in _resources("wq") if "moe_gemm_wq_wide_kernel" in line]


def test_both_kernels_include_the_tile():
    for src in ("wq.hip", "wq_moe_wide.hip"):
        text = (CSRC / src).read_text()
        assert '#include "wq_stream_tile.h"' in text and '#include "wq_stream_tile_body.h"' in text, src
    # stated once: neither file restates the batch
    body = (CSRC / "wq_stream_tile_body.h").read_text()
    assert body.count("auto batch = [&]") == 1
    for src in ("wq.hip", "wq_moe_wide.hip"):
        assert "auto batch" not in (CSRC / src).read_text(), src


# ---- refusals before the library ------------------------------------------------------------------------------------
E0, N0 = 2, 8


def _w4(K, shift=0, E=E0):
    return aligned_i32(E * N0, K // 8, shift // 4).view(E, N0, K // 8)


def _w8(K, E=E0):
    return aligned_i8(E * N0, K).view(E, N0, K)


def _s(G, E=E0):
    return torch.ones(E, N0, G)


def _meta(*shape, dtype=torch.bfloat16):
    return torch.empty(shape, dtype=dtype, device="meta")       # shapes and strides only; its address reads as 0


REFUSED = {
    "g_idx given": (lambda: (_x(32, 1024), _w4(1024), _s(8)), dict(g_idx=torch.zeros(E0, 1024, dtype=torch.int32)),
                    "g_idx is not taken"),
    "K = 192": (lambda: (_x(32, 192), _w8(192), _s(1)), {}, "not a multiple of the k-unit 128"),
    "X shifted by 2 bytes": (lambda: (_x(32, 1024, shift=2), _w4(1024), _s(8)), {}, "16-byte aligned"),
    "Wq shifted by 4 bytes": (lambda: (_x(32, 1024), _w4(1024, shift=4), _s(8)), {}, "16-byte aligned"),
    "a pitch of K + 1": (lambda: (_x(32, 1024, pitch=1025), _w4(1024), _s(8)), {}, "16-byte aligned"),
    "G = 3 at K = 1024": (lambda: (_x(32, 1024), _w4(1024), _s(3)), {}, "G must be 1 or K / 128 = 8"),
    "fp32 X": (lambda: (_x(32, 1024, dtype=torch.float32), _w4(1024), _s(8)), {}, "bf16 or fp16"),
    "float weights": (lambda: (_x(32, 1024), torch.zeros(E0, N0, 1024), _s(8)), {}, "weights only"),
    "E past the limit": (lambda: (_x(32, 128), _meta(4097, 1, 16, dtype=torch.int32), _meta(4097, 1, 1,
                                                                                           dtype=torch.float32)),
                         {}, "E=4097 experts are more than 4096"),
    # 8 m-tiles: floor(R / 128) + E = 65536 + 2 slots
    "too many slots": (lambda: (_x(32, 1024), _w4(1024), _s(8)), dict(row_idx=_meta(128 * 65536, dtype=torch.int32)),
                       "65538 row-tile slots"),
    "the 2^32 bound": (lambda: (_meta(1 << 21, 1024), _w4(1024), _s(8)), {}, "reaches 2\\^32 bytes"),
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_unsupported_operands_are_refused_before_the_library(monkeypatch, case):
    ops = _no_library(monkeypatch)
    make, kw, reason = REFUSED[case]
    X, Wq, s_w = make()
    assert ops.moe_gemm_wq_wide_supported(X, Wq, s_w, None, kw.get("g_idx"), kw.get("row_idx")) is False
    with pytest.raises(ValueError, match="moe_gemm_wq_wide: .*" + reason):
        ops.moe_gemm_wq_wide(X, Wq, s_w, torch.zeros(Wq.shape[0] + 1, dtype=torch.int32), **kw)


def test_supported_operands(monkeypatch):
    ops = _no_library(monkeypatch)
    zp = torch.zeros(E0, N0, 8, dtype=torch.int8)
    for M in (1, 17, 128, 2048):
        for dtype in (torch.bfloat16, torch.float16):
            assert ops.moe_gemm_wq_wide_supported(_x(M, 1024, dtype=dtype), _w4(1024), _s(8)) is True
        assert ops.moe_gemm_wq_wide_supported(_x(M, 1024), _w4(1024), _s(1), zp[:, :, :1]) is True
        assert ops.moe_gemm_wq_wide_supported(_x(M, 1024), _w8(1024), _s(8), zp, None) is True
        assert ops.moe_gemm_wq_wide_supported(_x(M, 1024, pitch=1032), _w8(1024), _s(1)) is True
        row_idx = torch.zeros(2 * M, dtype=torch.int32)
        assert ops.moe_gemm_wq_wide_supported(_x(M, 1024), _w4(1024), _s(8), None, None, row_idx) is True
    # the last sizes inside the bounds
    assert ops.moe_gemm_wq_wide_supported(_meta((1 << 21) - 2, 1024), _w4(1024), _s(8)) is True
    assert ops.moe_gemm_wq_wide_supported(_x(32, 1024), _w4(1024), _s(8), None, None,
                                          _meta(128 * 65533 + 127, dtype=torch.int32)) is True


def test_the_host_rule_for_the_tile_count():
    from quantool_amd.hip import ops

    for E in (1, 3, 8, 64):
        for per, mt in ((1, 1), (16, 1), (17, 2), (32, 2), (33, 4), (64, 4), (65, 8), (128, 8), (1000, 8)):
            assert ops.moe_wq_wide_mtiles(per * E, E) == mt, (E, per)
            assert ops.moe_wq_wide_mtiles((per - 1) * E + 1, E) == mt, (E, per)     # ceil(R / E)
    # the slot count bounds the tiles of any routing: all rows on one expert, and one row on each of the others
    for R, E in ((300, 8), (129, 4), (40, 64)):
        q = 16 * ops.moe_wq_wide_mtiles(R, E)
        slots = R // q + min(E, R)
        for counts in ([R] + [0] * (E - 1), [R - (E - 1)] + [1] * (E - 1) if R >= E else [1] * R):
            assert sum(-(-c // q) for c in counts) <= slots, (R, E, counts)


# ---- WeightOnlyExperts -----------------------------------------------------------------------------------------------
class _Bank(nn.Module):
    """The dense bank's stand-in: its forward marks the dequantise path."""

    def __init__(self, E, H, I):
        super().__init__()
        self.gate_up_proj = nn.Parameter(torch.zeros(E, 2 * I, H, dtype=torch.bfloat16), requires_grad=False)
        self.down_proj = nn.Parameter(torch.zeros(E, H, I, dtype=torch.bfloat16), requires_grad=False)
        self.act_fn = nn.SiLU()
        self.calls = 0

    def forward(self, hidden_states, top_k_index, top_k_weights):
        self.calls += 1
        assert self.gate_up_proj.numel() and self.down_proj.numel()      # the dequantised banks stand in
        return hidden_states * 0


class _OnDevice(torch.Tensor):
    """A CPU tensor that calls itself a device tensor, so that ``forward`` takes the device branches."""
    is_cuda = True


def _experts(g_idx=False, K_ragged=False):
    from quantool_amd.engine.qmodules import WeightOnlyExperts

    E, H, I = 4, 256, 384 + (64 if K_ragged else 0)
    gi = (torch.zeros(E, H, dtype=torch.int32), torch.zeros(E, I, dtype=torch.int32)) if g_idx else (None, None)
    bank = _Bank(E, H, I)
    woe = WeightOnlyExperts(bank, torch.zeros(E, 2 * I, H // 8, dtype=torch.int32), torch.ones(E, 2 * I, H // 128),
                            torch.zeros(E, H, (I + 7) // 8, dtype=torch.int32), torch.ones(E, H, (I + 127) // 128),
                            gate_up_g_idx=gi[0], down_g_idx=gi[1])
    return woe, bank


@pytest.fixture
def recorded(monkeypatch):
    """``ops`` with the routing steps and both product forms replaced by recording fakes, and no library."""
    ops = _no_library(monkeypatch)
    log = []

    def product(name):
        def f(X, Wq, s_w, offsets, *, row_idx=None, K=None, zp_w=None, g_idx=None):
            R = X.shape[0] if row_idx is None else row_idx.numel()
            log.append((name, "gate_up" if row_idx is not None else "down", R))
            return torch.zeros(R, Wq.shape[1], dtype=X.dtype)
        return f

    def route(top_k_index, num_experts):
        R = top_k_index.numel()
        src = torch.arange(R, dtype=torch.int32) // top_k_index.shape[1]
        return torch.zeros(num_experts + 1, dtype=torch.int32), src, None, torch.zeros(R, dtype=torch.int32)

    monkeypatch.setattr(ops, "gemm_wq_grouped", product("grouped"))
    monkeypatch.setattr(ops, "moe_gemm_wq_wide", product("wide"))
    monkeypatch.setattr(ops, "moe_route", route)
    monkeypatch.setattr(ops, "moe_combine", lambda Y, row_of, w: Y[:w.shape[0]])
    return ops, log


def _run(woe, T, k=2):
    x = torch.zeros(T, woe.hidden_dim, dtype=torch.bfloat16).as_subclass(_OnDevice)
    idx = torch.zeros(T, k, dtype=torch.int64)
    return woe(x, idx, torch.ones(T, k, dtype=torch.bfloat16))


def test_class_defaults():
    from quantool_amd.engine.qmodules import WeightOnlyExperts

    assert WeightOnlyExperts.wide_max_tokens == 0 and WeightOnlyExperts.grouped_max_tokens == 128
    lo = WeightOnlyExperts.wide_min_tokens
    assert type(lo) is int and (lo == 0 or 17 <= lo <= 128)
    woe, _ = _experts()
    assert f"wide_min_tokens={lo}" in repr(woe) and "wide_max_tokens=0" in repr(woe)
    woe.wide_min_tokens, woe.wide_max_tokens = 64, 512
    assert "wide_min_tokens=64" in repr(woe) and "wide_max_tokens=512" in repr(woe)


def test_defaults_leave_large_calls_on_the_dequantise_path(recorded):
    _, log = recorded
    woe, bank = _experts()
    for T in (129, 300, 2048):
        _run(woe, T)
    assert bank.calls == 3 and log == []


def test_wide_min_tokens_picks_the_form_inside_the_routed_forward(recorded, monkeypatch):
    ops, log = recorded
    woe, bank = _experts()
    woe.wide_min_tokens = 0
    for T in (1, 17, 128):
        _run(woe, T)
    assert [name for name, _, _ in log] == ["grouped"] * 6            # 0: never
    del log[:]
    woe.wide_min_tokens = 40
    for T in (39, 40, 41, 128):
        _run(woe, T)
    assert log == [("grouped", "gate_up", 78), ("grouped", "down", 78), ("wide", "gate_up", 80), ("wide", "down", 80),
                   ("wide", "gate_up", 82), ("wide", "down", 82), ("wide", "gate_up", 256), ("wide", "down", 256)]
    del log[:]
    _run(woe, 129)                                                      # past the routed range: wide_min_tokens is not read
    assert bank.calls == 1 and log == []
    # a bank the kernel does not take stays on the grouped GEMV
    g_woe, _ = _experts(g_idx=True)
    g_woe.wide_min_tokens = 40
    _run(g_woe, 64)
    assert [name for name, _, _ in log] == ["grouped"] * 2
    # with the attribute 0 the wide names are not read at all
    del log[:]
    monkeypatch.delattr(ops, "moe_gemm_wq_wide")
    monkeypatch.delattr(ops, "moe_gemm_wq_wide_supported")
    woe.wide_min_tokens = 0
    _run(woe, 64)
    _run(woe, 129)
    assert [name for name, _, _ in log] == ["grouped"] * 2 and bank.calls == 2


def test_wide_max_tokens_extends_the_routed_forward(recorded):
    _, log = recorded
    woe, bank = _experts()
    woe.wide_min_tokens, woe.wide_max_tokens = 0, 300
    for T in (128, 129, 300, 301):
        _run(woe, T)
    assert log == [("grouped", "gate_up", 256), ("grouped", "down", 256), ("wide", "gate_up", 258),
                   ("wide", "down", 258), ("wide", "gate_up", 600), ("wide", "down", 600)]
    assert bank.calls == 1                                              # 301
    del log[:]
    for kw in (dict(g_idx=True), dict(K_ragged=True)):                  # a bank with an unsupported product: as before
        other, other_bank = _experts(**kw)
        other.wide_max_tokens = 300
        _run(other, 200)
        assert other_bank.calls == 1 and log == [], kw


# ---- load_quantized -------------------------------------------------------------------------------------------------
def test_loader_sets_wide_tokens(tmp_path):
    from quantool_amd.engine.qlinear import A16_EXPERTS_WIDE_MAX_TOKENS, WeightOnlyExperts, load_quantized

    _write(tmp_path, "W4A16")
    kw = dict(device="cpu", a16="packed", a16_experts="packed")
    model = load_quantized(tmp_path, **kw)
    assert model.get_submodule(BANK).wide_max_tokens == 0 and model._qt_checkpoint["a16_experts_wide_tokens"] == 0
    model = load_quantized(tmp_path, a16_experts_wide_tokens=512, **kw)
    woe = model.get_submodule(BANK)
    assert isinstance(woe, WeightOnlyExperts) and woe.wide_max_tokens == 512 and "wide_max_tokens" in vars(woe)
    assert WeightOnlyExperts.wide_max_tokens == 0                        # an instance attribute: the class keeps 0
    assert model._qt_checkpoint["a16_experts_wide_tokens"] == 512 and "wide_max_tokens=512" in repr(woe)
    for ok in (129, A16_EXPERTS_WIDE_MAX_TOKENS):
        assert load_quantized(tmp_path, a16_experts_wide_tokens=ok, **kw).get_submodule(BANK).wide_max_tokens == ok
    for bad in (1, 128, A16_EXPERTS_WIDE_MAX_TOKENS + 1, -1, 256.0):
        with pytest.raises(ValueError, match="a16_experts_wide_tokens"):
            load_quantized(tmp_path, a16_experts_wide_tokens=bad, **kw)
    with pytest.raises(ValueError, match="needs a16_experts='packed'"):
        load_quantized(tmp_path, device="cpu", a16="packed", a16_experts_wide_tokens=512)
    assert "a16_experts_wide_tokens" not in load_quantized(tmp_path, device="cpu", a16="packed")._qt_checkpoint


def test_a8_checkpoints_ignore_wide_tokens(tmp_path):
    from quantool_amd.engine.qlinear import WeightOnlyExperts, load_quantized

    _write(tmp_path, "W4A8")
    model = load_quantized(tmp_path, device="cpu", a16="packed", a16_experts="packed", a16_experts_wide_tokens=512)
    assert not any(isinstance(m, WeightOnlyExperts) for m in model.modules())
    assert "a16_experts_wide_tokens" not in model._qt_checkpoint
