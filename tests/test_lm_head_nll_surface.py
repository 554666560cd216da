"""``qt_lm_head_nll`` without a GPU: the header declares both functions and states the contract, the ctypes table holds
them and the built library exports them; called through ctypes with host buffers, every argument the header lists as
refused returns ``QT_ERR_INVALID`` (or ``QT_ERR_WORKSPACE``) before any launch, with ``qt_last_error`` naming the
argument; ``ops.lm_head_nll`` refuses what the kernel does not take before it touches the library; and
``evaluate.perplexity`` knows its ``head`` keyword."""
import ctypes
import re

import pytest
import torch

from tests.i8_fake_ops import check_surface, header_text

NAME = "qt_lm_head_nll"
WS_NAME = "qt_lm_head_nll_workspace_size"


def test_header_declares_them():
    check_surface("header", NAME)
    check_surface("header", WS_NAME)
    text = header_text()[1]
    args = [a.strip() for a in re.search(NAME + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")]
    assert args == ["const void* H", "int64_t ldh", "const void* W", "int64_t ldw", "int dtype", "int64_t M", "int K",
                    "int V", "const void* targets", "int target_bytes", "float* nll", "float* lse", "float* tgt",
                    "int32_t* argmax", "void* workspace", "size_t workspace_bytes", "qt_stream_t stream"]
    ws_args = [a.strip() for a in re.search(WS_NAME + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")]
    assert ws_args == ["int64_t M", "int V"]
    assert re.search(r"QT_PROF_LM_HEAD_NLL\s*=\s*2", text)


def test_header_states_the_contract():
    raw = re.sub(r" +", " ", re.sub(r"\s*\n\s*\*\s*", " ", header_text()[0]))
    para = raw[raw.index(NAME + ":"):raw.index("#define QT_LM_HEAD_K_UNIT")]
    for must in ("the fp32 accumulator of the target column, to the bit", "the lowest v of maximal x[m, v]",
                 "nll[m] = lse[m] - tgt[m]", "targets[m] < 0 (the ignore index): nll[m] = 0 and tgt[m] = 0",
                 "lse[m] and argmax[m] are still written", "targets[m] >= V: nll[m] and tgt[m] are NaN",
                 "The [M, V] logits are never written", "the k order of one accumulator is fixed",
                 "the xor steps 16, 8, 4, 2, 1", "the four column waves in ascending order",
                 "the vocabulary tiles in ascending order", "ties of the maximum going to the lower index",
                 "Row m's four outputs depend only on H[m, :], W, V, K and targets[m]",
                 "not on M, the row's index, the pitches or the alignment of H", "Deterministic, no atomics",
                 "16 M ceil(V / 256) bytes of records + 4 M bytes of target logits",
                 "QT_ERR_WORKSPACE with nothing launched", "M = 0 returns QT_OK and touches nothing",
                 "QT_ERR_INVALID before any launch", "fp32 operands are not taken", "QT_LM_HEAD_MIN_K = 128",
                 "QT_LM_HEAD_MAX_K = 32768", "ldh < K or ldw < K", "V < 1", "fetched clamped"):
        assert must in para, must


def test_ctypes_table_holds_them():
    from quantool_amd.hip import _lib

    p, i, l, z = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t
    assert _lib.SIGNATURES[NAME] == (ctypes.c_int, [p, l, p, l, i, l, i, i, p, i, p, p, p, p, p, z, p])
    assert _lib.SIGNATURES[WS_NAME] == (z, [l, i])


def test_library_exports_them():
    check_surface("library", NAME)
    check_surface("library", WS_NAME)


def test_the_ring_headers_are_included_not_copied():
    from quantool_amd.csrc import build

    src = (build.CSRC / "lm_head_nll.hip").read_text()
    assert '#include "i8_ring_tile.h"' in src
    for shared in ("glds16_pair(", "ring_sync_math(", "ring_drain_wait<", "ring_stagger_begin(", "ring_body<8>(",
                   "i8_ring_tile_of(", "i8_ring_cd_row(", "mfma16<F16>("):
        assert shared in src, shared
    for own in ("global_load_lds", "s_waitcnt", "s_barrier()", "atomicAdd", "atomicMax"):
        assert own not in src, own
    assert "RAW:" in src and "WAR:" in src
    assert '"lm_head_nll.hip"' in (build.CSRC / "build.py").read_text()


def test_the_kernels_have_no_scratch():
    from quantool_amd.csrc import build

    res = build.OBJ_DIR / "lm_head_nll.resources.txt"
    if not res.exists():
        import __graft_entry__ as g

        g.build()
    rows = res.read_text().splitlines()
    assert sum("lm_head_nll_kernel" in r for r in rows) == 2          # bf16, fp16
    assert sum("lm_head_reduce_kernel" in r for r in rows) == 1
    for row in rows:
        assert "scratch 0\t" in row and "vgpr_spill 0\t" in row, row


def test_workspace_bytes():
    from quantool_amd.hip import _lib

    lib = _lib.load()
    assert lib.qt_lm_head_nll_workspace_size(257, 513) == 16 * 257 * 3 + 4 * 257
    assert lib.qt_lm_head_nll_workspace_size(1, 256) == 16 + 4
    assert lib.qt_lm_head_nll_workspace_size(16384, 128256) == 16 * 16384 * 501 + 4 * 16384
    assert lib.qt_lm_head_nll_workspace_size(0, 513) == 0


# ---- refusals before any launch -------------------------------------------------------------------------------------
QT_BF16, QT_F16, QT_F32 = 1, 2, 0
M0, K0, V0 = 3, 128, 5
NEED = 16 * M0 + 4 * M0

# case -> (overrides of the good call, expected status name, what qt_last_error must name)
BAD = {
    "null H": (dict(H=None), "INVALID", r"\bH\b"),
    "null W": (dict(W=None), "INVALID", r"\bW\b"),
    "null targets": (dict(targets=None), "INVALID", r"\btargets\b"),
    "null nll": (dict(nll=None), "INVALID", r"\bnll\b"),
    "null lse": (dict(lse=None), "INVALID", r"\blse\b"),
    "null tgt": (dict(tgt=None), "INVALID", r"\btgt\b"),
    "null argmax": (dict(argmax=None), "INVALID", r"\bargmax\b"),
    "fp32 operands": (dict(dtype=QT_F32), "INVALID", r"\bdtype\b"),
    "unknown dtype": (dict(dtype=7), "INVALID", r"\bdtype\b"),
    "K = 64": (dict(K=64, ldh=64, ldw=64), "INVALID", r"\bK\b.*128"),
    "K = 0": (dict(K=0), "INVALID", r"\bK\b"),
    "K = 192": (dict(K=192, ldh=192, ldw=192), "INVALID", r"\bK\b.*multiple"),
    "K = 32896": (dict(K=32896, ldh=32896, ldw=32896), "INVALID", r"32768"),
    "ldh below K": (dict(ldh=K0 - 8), "INVALID", r"\bldh\b"),
    "ldw below K": (dict(ldw=K0 - 8), "INVALID", r"\bldw\b"),
    "ldh breaks 16-byte alignment": (dict(ldh=K0 + 4), "INVALID", r"\bldh\b"),
    "ldw breaks 16-byte alignment": (dict(ldw=K0 + 4), "INVALID", r"\bldw\b"),
    "H base off 16 bytes": (dict(H_shift=2), "INVALID", r"\bH\b.*aligned"),
    "W base off 16 bytes": (dict(W_shift=8), "INVALID", r"\bW\b.*aligned"),
    "V = 0": (dict(V=0), "INVALID", r"\bV\b"),
    "M < 0": (dict(M=-1), "INVALID", r"\bM\b"),
    "M past INT32_MAX": (dict(M=2 ** 31), "INVALID", r"\bM\b.*too large"),
    "target_bytes = 2": (dict(target_bytes=2), "INVALID", r"\btarget_bytes\b"),
    "short workspace": (dict(workspace_bytes=NEED - 1), "WORKSPACE", r"\bworkspace\b"),
    "null workspace": (dict(workspace=None), "WORKSPACE", r"\bworkspace\b"),
}


@pytest.fixture(scope="module")
def lib():
    from quantool_amd.hip import _lib

    return _lib.load()


def _call(lib, a):
    return lib.qt_lm_head_nll(a["H"], a["ldh"], a["W"], a["ldw"], a["dtype"], a["M"], a["K"], a["V"], a["targets"],
                              a["target_bytes"], a["nll"], a["lse"], a["tgt"], a["argmax"], a["workspace"],
                              a["workspace_bytes"], None)


def _good():
    names = ("H", "W", "targets", "nll", "lse", "tgt", "argmax", "workspace")
    bufs = {n: ctypes.create_string_buffer(96) for n in names}
    addr = {n: (ctypes.addressof(b) + 15) // 16 * 16 for n, b in bufs.items()}
    a = dict(H=addr["H"], ldh=K0, W=addr["W"], ldw=K0, dtype=QT_BF16, M=M0, K=K0, V=V0, targets=addr["targets"],
             target_bytes=8, nll=addr["nll"], lse=addr["lse"], tgt=addr["tgt"], argmax=addr["argmax"],
             workspace=addr["workspace"], workspace_bytes=NEED)
    return bufs, a


@pytest.mark.parametrize("case", list(BAD))
def test_bad_arguments_are_refused_before_any_launch(lib, case):
    """The pointers are host buffers: a refusal never reads them, and nothing here reaches a launch."""
    from quantool_amd.hip import _lib

    bufs, a = _good()
    over, status, names = BAD[case]
    over = dict(over)
    for n in ("H", "W"):
        a[n] += over.pop(n + "_shift", 0)
    a.update(over)
    st = _call(lib, a)
    assert st == getattr(_lib, "QT_ERR_" + status)
    msg = lib.qt_last_error().decode()
    assert msg.startswith(NAME + ":") and re.search(names, msg), msg
    assert all(b.raw == bytes(96) for b in bufs.values())


def test_m_zero_is_ok_and_touches_nothing(lib):
    from quantool_amd.hip import _lib

    bufs, a = _good()
    a.update(M=0, workspace=None, workspace_bytes=0)
    assert _call(lib, a) == _lib.QT_OK
    assert all(b.raw == bytes(96) for b in bufs.values())


# ---- ops ------------------------------------------------------------------------------------------------------------
def test_ops_refuses_cpu_tensors():
    from quantool_amd.hip import ops

    with pytest.raises(ValueError, match="device tensor"):
        ops.lm_head_nll(torch.zeros(2, 128, dtype=torch.bfloat16), torch.zeros(5, 128, dtype=torch.bfloat16),
                        torch.zeros(2, dtype=torch.int64))


@pytest.fixture
def pretend_device(monkeypatch):
    """Host tensors that answer ``is_cuda`` with True, and a library that must not be reached: ``ops``' own checks run
    on them as on device tensors, and every one of them comes before the first pointer is read."""
    from quantool_amd.hip import ops

    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))

    def unreachable():
        raise AssertionError("ops reached the library")

    monkeypatch.setattr(ops, "load", unreachable)
    return ops


def _al(t):
    """A copy of t that starts on a 16-byte boundary."""
    buf = torch.zeros(t.numel() + 16, dtype=t.dtype)
    off = ((-buf.data_ptr()) % 16) // t.element_size()
    return buf[off:off + t.numel()].view(t.shape)


def test_ops_refuses_what_the_kernel_does_not_take(pretend_device):
    ops = pretend_device
    bf, fp = torch.bfloat16, torch.float16
    H, W, tg = _al(torch.zeros(3, 128, dtype=bf)), _al(torch.zeros(5, 128, dtype=bf)), torch.zeros(3, dtype=torch.int64)
    with pytest.raises(TypeError, match="bf16 or fp16"):
        ops.lm_head_nll(H.float(), W.float(), tg)
    with pytest.raises(TypeError, match="W must be of H's dtype"):
        ops.lm_head_nll(H, W.to(fp), tg)
    with pytest.raises(TypeError, match="W must be of H's dtype"):
        ops.lm_head_nll(H, W.float(), tg)
    for K in (64, 192, 32896):
        with pytest.raises(ValueError, match=f"K {K} unsupported"):
            ops.lm_head_nll(torch.zeros(3, K, dtype=bf), torch.zeros(5, K, dtype=bf), tg)
    with pytest.raises(ValueError, match=r"W must be \[V, 128\]"):
        ops.lm_head_nll(H, torch.zeros(5, 256, dtype=bf), tg)
    with pytest.raises(ValueError, match="unit column stride"):
        ops.lm_head_nll(torch.zeros(128, 3, dtype=bf).t(), W, tg)
    with pytest.raises(ValueError, match="unit column stride"):
        ops.lm_head_nll(H, torch.zeros(128, 5, dtype=bf).t(), tg)
    with pytest.raises(TypeError, match="targets must be torch.int32 or torch.int64"):
        ops.lm_head_nll(H, W, tg.float())
    with pytest.raises(ValueError, match=r"targets must be contiguous \[3\]"):
        ops.lm_head_nll(H, W, tg[:2])
    with pytest.raises(ValueError, match="row pitch 132"):
        ops.lm_head_nll(_al(torch.zeros(3, 132, dtype=bf))[:, :128], W, tg)
    with pytest.raises(ValueError, match="16-byte boundary"):
        ops.lm_head_nll(_al(torch.zeros(3, 136, dtype=bf))[:, 4:132], W, tg)
    with pytest.raises(AssertionError, match="reached the library"):     # and a good call passes every check
        ops.lm_head_nll(H, W, tg.int())
    with pytest.raises(AssertionError, match="reached the library"):
        ops.lm_head_nll(_al(torch.zeros(3, 136, dtype=bf))[:, :128], W, tg)


# ---- evaluate -------------------------------------------------------------------------------------------------------
def _tiny_llama(**over):
    from transformers import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(0)
    cfg = LlamaConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=4,
                      num_key_value_heads=4, vocab_size=131, max_position_embeddings=64, **over)
    return LlamaForCausalLM(cfg).to(torch.bfloat16).eval()


def test_perplexity_refuses_an_unknown_head():
    from quantool_amd.evaluate import perplexity

    with pytest.raises(ValueError, match="head must be one of"):
        perplexity(torch.nn.Linear(2, 2), torch.zeros(1, 4, dtype=torch.long), head="bogus")


def test_fused_head_on_a_cpu_model_raises_the_eligibility_error():
    from quantool_amd.evaluate import perplexity

    ids = torch.arange(24).reshape(2, 12) % 131
    with pytest.raises(ValueError, match=r'head="fused" is not available for this model: .*not on a GPU'):
        perplexity(_tiny_llama(), ids, head="fused")
    base = perplexity(_tiny_llama(), ids)
    assert set(base) == {"perplexity", "nll", "tokens"}                  # the default path gains no key
    assert perplexity(_tiny_llama(), ids, head="logits") == base


def test_the_eligibility_error_names_the_reason():
    from quantool_amd.evaluate import fused_head_parts

    with pytest.raises(ValueError, match="no base_model"):
        fused_head_parts(torch.nn.Linear(2, 2))
    m = _tiny_llama()
    m.lm_head = torch.nn.Linear(128, 131, bias=True).to(torch.bfloat16)
    with pytest.raises(ValueError, match="has a bias"):
        fused_head_parts(m)
    m = _tiny_llama()
    m.config.final_logit_softcapping = 30.0
    with pytest.raises(ValueError, match="soft-capping"):
        fused_head_parts(m)
    m = _tiny_llama().float()
    with pytest.raises(ValueError, match="not bf16 or fp16"):
        fused_head_parts(m)
    m = _tiny_llama()
    m.lm_head = torch.nn.Linear(64, 131, bias=False).to(torch.bfloat16)
    with pytest.raises(ValueError, match="hidden size 64 is outside the kernel's range"):
        fused_head_parts(m)
    m = _tiny_llama()
    m.lm_head = torch.nn.Sequential(torch.nn.Linear(128, 131, bias=False))
    with pytest.raises(ValueError, match="not a plain nn.Linear"):
        fused_head_parts(m)
