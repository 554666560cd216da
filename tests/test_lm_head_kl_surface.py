"""``qt_lm_head_kl`` without a GPU: the header declares both functions and states the contract, the ctypes table holds
them and the built library exports them; the kernels have no scratch; the record code lives in one header that both
LM-head files include; called through ctypes with host buffers, every argument the header lists as refused returns
``QT_ERR_INVALID`` (or ``QT_ERR_WORKSPACE``) before any launch, with ``qt_last_error`` naming the argument;
``ops.lm_head_kl`` refuses what the kernel does not take before it touches the library; and ``evaluate.divergence`` names
the reason a pair of models is not eligible."""
import ctypes
import re

import pytest
import torch

from tests.i8_fake_ops import check_surface, header_text

NAME = "qt_lm_head_kl"
WS_NAME = "qt_lm_head_kl_workspace_size"


def test_header_declares_them():
    check_surface("header", NAME)
    check_surface("header", WS_NAME)
    text = header_text()[1]
    args = [a.strip() for a in re.search(NAME + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")]
    assert [re.sub(r"\s+", " ", a) for a in args] == [
        "const void* Hp", "int64_t ldhp", "const void* Hq", "int64_t ldhq", "const void* W", "int64_t ldw", "int dtype",
        "int64_t M", "int K", "int V", "const void* targets", "int target_bytes", "float* kl", "float* nll_p",
        "float* nll_q", "float* lse_p", "float* lse_q", "int32_t* argmax_p", "int32_t* argmax_q", "void* workspace",
        "size_t workspace_bytes", "qt_stream_t stream"]
    ws_args = [a.strip() for a in re.search(WS_NAME + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")]
    assert ws_args == ["int64_t M", "int V"]
    assert re.search(r"QT_PROF_LM_HEAD_NLL\s*=\s*2", text)
    assert len(re.findall(r"#define QT_LM_HEAD_(K_UNIT|MIN_K|MAX_K)\b", text)) == 3      # reused, not redefined


def test_header_states_the_contract():
    raw = re.sub(r" +", " ", re.sub(r"\s*\n\s*\*\s*", " ", header_text()[0]))
    para = raw[raw.index(NAME + ":"):raw.index("size_t " + WS_NAME)]
    for must in ("kl[m] = KL(P || Q)", "t / s_a - lse_p[m] + lse_q[m]", "not clamped at 0",
                 "t = sum_v exp(a[m, v] - max_a) (a[m, v] - b[m, v])", "the lowest v of maximal a[m, v]",
                 "nll_p[m] = lse_p[m] - a[m, targets[m]]", "nll_q[m] = lse_q[m] - b[m, targets[m]]",
                 "targets[m] < 0 (the ignore index) gives nll_p[m] = nll_q[m] = 0", "targets[m] >= V gives NaN in both",
                 "kl, both lse and both argmax are still written", "to the bit",
                 "the lane's two columns (c, c + 128 of the tile)", "the xor steps 16, 8, 4, 2, 1",
                 "the four column waves in ascending order", "the vocabulary tiles in ascending order",
                 "{a, 1, v, a - b}", "{-inf, 0, v, 0}", "t merges with the weights of s",
                 "Row m's seven outputs depend only on Hp[m, :], Hq[m, :], W, V, K and targets[m]",
                 "not on M, the row's index, the pitches or the alignment of Hp and Hq", "Deterministic, no atomics",
                 "32 M ceil(V / 256) bytes of records + 8 M bytes of target logits",
                 "QT_ERR_WORKSPACE with nothing launched", "M = 0 returns QT_OK and touches nothing",
                 "QT_ERR_INVALID before any launch", "the refusals of qt_lm_head_nll, for both hidden-state operands",
                 "fp32 operands are not taken", "ldhp < K, ldhq < K or ldw < K", "V < 1", "fetched clamped",
                 "row M - 1 on each side"):
        assert must in para, must


def test_ctypes_table_holds_them():
    from quantool_amd.hip import _lib

    p, i, l, z = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t
    assert _lib.SIGNATURES[NAME] == (ctypes.c_int, [p, l, p, l, p, l, i, l, i, i, p, i, p, p, p, p, p, p, p, p, z, p])
    assert _lib.SIGNATURES[WS_NAME] == (z, [l, i])


def test_library_exports_them():
    check_surface("library", NAME)
    check_surface("library", WS_NAME)


def test_the_record_code_is_shared_not_copied():
    from quantool_amd.csrc import build

    hdr = (build.CSRC / "lm_head_rec.h").read_text()
    for defined in ("struct Rec {", "struct RecT {", " rec_merge(const Rec& lo", " rec_merge(const RecT& lo",
                    " void rec_scatter_step(", " load_target(", " rec_pack(const Rec& o", "constexpr int LMH_MIN_K"):
        assert defined in hdr, defined
    for name in ("lm_head_nll.hip", "lm_head_kl.hip"):
        src = (build.CSRC / name).read_text()
        assert '#include "lm_head_rec.h"' in src and '#include "i8_ring_tile.h"' in src, name
        for defined in ("struct Rec", "Rec rec_merge(", "void rec_scatter_step(", "int64_t load_target(", "constexpr int LMH_", "LMH_MAX_PITCH ="):
            assert defined not in src, (name, defined)
        for used in ("rec_merge(", "rec_scatter_step<16, 16>(", "load_target(", "rec_pack(", "rec_unpack("):
            assert used in src, (name, used)
    kl = (build.CSRC / "lm_head_kl.hip").read_text()
    for shared in ("glds16_pair(", "ring_sync_math(", "ring_drain_wait<", "ring_stagger_begin(", "ring_body<8>(",
                   "i8_ring_tile_of(", "i8_ring_cd_row(", "mfma16<F16>("):
        assert shared in kl, shared
    for own in ("global_load_lds", "s_waitcnt", "s_barrier()", "atomicAdd", "atomicMax"):
        assert own not in kl, own
    assert "RAW:" in kl and "WAR:" in kl
    text = (build.CSRC / "build.py").read_text()
    assert '"lm_head_kl.hip"' in text and '"lm_head_kl_kernel"' in text


def test_the_kernels_have_no_scratch():
    from quantool_amd.csrc import build

    res = build.OBJ_DIR / "lm_head_kl.resources.txt"
    if not res.exists():
        import __graft_entry__ as g

        g.build()
    rows = res.read_text().splitlines()
    assert sum("lm_head_kl_kernel" in r for r in rows) == 2           # bf16, fp16
    assert sum("lm_head_kl_reduce_kernel" in r for r in rows) == 1
    assert len(rows) == 3
    for row in rows:
        assert "scratch 0\t" in row and "vgpr_spill 0\t" in row, row


def test_workspace_size():
    from quantool_amd.hip import _lib

    lib = _lib.load()
    assert lib.qt_lm_head_kl_workspace_size(257, 513) == 32 * 257 * 3 + 8 * 257
    assert lib.qt_lm_head_kl_workspace_size(1, 256) == 32 + 8
    assert lib.qt_lm_head_kl_workspace_size(1, 257) == 64 + 8
    assert lib.qt_lm_head_kl_workspace_size(16384, 128256) == 32 * 16384 * 501 + 8 * 16384
    assert lib.qt_lm_head_kl_workspace_size(16384, 128256) == 2 * lib.qt_lm_head_nll_workspace_size(16384, 128256)
    assert lib.qt_lm_head_kl_workspace_size(0, 513) == 0
    assert lib.qt_lm_head_kl_workspace_size(-1, 513) == 0
    assert lib.qt_lm_head_kl_workspace_size(5, 0) == 0


# ---- refusals before any launch -------------------------------------------------------------------------------------
QT_BF16, QT_F16, QT_F32 = 1, 2, 0
M0, K0, V0 = 3, 128, 5
NEED = 32 * M0 + 8 * M0
POINTERS = ("Hp", "Hq", "W", "targets", "kl", "nll_p", "nll_q", "lse_p", "lse_q", "argmax_p", "argmax_q")
ORDER = ("Hp", "ldhp", "Hq", "ldhq", "W", "ldw", "dtype", "M", "K", "V", "targets", "target_bytes", "kl", "nll_p",
         "nll_q", "lse_p", "lse_q", "argmax_p", "argmax_q", "workspace", "workspace_bytes")

# case -> (overrides of the good call, expected status name, what qt_last_error must name)
BAD = {f"null {n}": ({n: None}, "INVALID", rf"\b{n}\b") for n in POINTERS}
BAD.update({
    "fp32 operands": (dict(dtype=QT_F32), "INVALID", r"\bdtype\b"),
    "unknown dtype": (dict(dtype=7), "INVALID", r"\bdtype\b"),
    "K = 64": (dict(K=64, ldhp=64, ldhq=64, ldw=64), "INVALID", r"\bK\b.*128"),
    "K = 0": (dict(K=0), "INVALID", r"\bK\b"),
    "K = 192": (dict(K=192, ldhp=192, ldhq=192, ldw=192), "INVALID", r"\bK\b.*multiple"),
    "K = 32896": (dict(K=32896, ldhp=32896, ldhq=32896, ldw=32896), "INVALID", r"32768"),
    "ldhp below K": (dict(ldhp=K0 - 8), "INVALID", r"\bldhp\b"),
    "ldhq below K": (dict(ldhq=K0 - 8), "INVALID", r"\bldhq\b"),
    "ldw below K": (dict(ldw=K0 - 8), "INVALID", r"\bldw\b"),
    "ldhp breaks 16-byte alignment": (dict(ldhp=K0 + 4), "INVALID", r"\bldhp\b"),
    "ldhq breaks 16-byte alignment": (dict(ldhq=K0 + 4), "INVALID", r"\bldhq\b"),
    "ldw breaks 16-byte alignment": (dict(ldw=K0 + 4), "INVALID", r"\bldw\b"),
    "ldhp past 2^22": (dict(ldhp=(1 << 22) + 8), "INVALID", r"\bldhp\b"),
    "ldhq past 2^22": (dict(ldhq=(1 << 22) + 8), "INVALID", r"\bldhq\b"),
    "Hp base off 16 bytes": (dict(Hp_shift=2), "INVALID", r"\bHp\b.*aligned"),
    "Hq base off 16 bytes": (dict(Hq_shift=4), "INVALID", r"\bHq\b.*aligned"),
    "W base off 16 bytes": (dict(W_shift=8), "INVALID", r"\bW\b.*aligned"),
    "V = 0": (dict(V=0), "INVALID", r"\bV\b"),
    "M < 0": (dict(M=-1), "INVALID", r"\bM\b"),
    "M past INT32_MAX": (dict(M=2 ** 31), "INVALID", r"\bM\b.*too large"),
    "target_bytes = 2": (dict(target_bytes=2), "INVALID", r"\btarget_bytes\b"),
    "short workspace": (dict(workspace_bytes=NEED - 1), "WORKSPACE", r"\bworkspace\b"),
    "the NLL call's workspace": (dict(workspace_bytes=16 * M0 + 4 * M0), "WORKSPACE", r"\bworkspace\b"),
    "null workspace": (dict(workspace=None), "WORKSPACE", r"\bworkspace\b"),
    "workspace off 16 bytes": (dict(workspace_shift=8, workspace_bytes=NEED), "WORKSPACE", r"\bworkspace\b"),
})


@pytest.fixture(scope="module")
def lib():
    from quantool_amd.hip import _lib

    return _lib.load()


def _call(lib, a):
    return lib.qt_lm_head_kl(*(a[n] for n in ORDER), None)


def _good():
    names = POINTERS + ("workspace",)
    bufs = {n: ctypes.create_string_buffer(160) for n in names}
    addr = {n: (ctypes.addressof(b) + 15) // 16 * 16 for n, b in bufs.items()}
    a = dict(addr, ldhp=K0, ldhq=K0, ldw=K0, dtype=QT_BF16, M=M0, K=K0, V=V0, target_bytes=8, workspace_bytes=NEED)
    return bufs, a


@pytest.mark.parametrize("case", list(BAD))
def test_bad_arguments_are_refused_before_any_launch(lib, case):
    """The pointers are host buffers: a refusal never reads them, and nothing here reaches a launch."""
    from quantool_amd.hip import _lib

    bufs, a = _good()
    over, status, names = BAD[case]
    over = dict(over)
    for n in ("Hp", "Hq", "W", "workspace"):
        a[n] += over.pop(n + "_shift", 0)
    a.update(over)
    st = _call(lib, a)
    assert st == getattr(_lib, "QT_ERR_" + status)
    msg = lib.qt_last_error().decode()
    assert msg.startswith(NAME + ":") and re.search(names, msg), msg
    assert all(b.raw == bytes(160) for b in bufs.values())


def test_m_zero_is_ok_and_touches_nothing(lib):
    from quantool_amd.hip import _lib

    bufs, a = _good()
    a.update(M=0, workspace=None, workspace_bytes=0)
    assert _call(lib, a) == _lib.QT_OK
    assert all(b.raw == bytes(160) for b in bufs.values())


# ---- ops ------------------------------------------------------------------------------------------------------------
def test_ops_refuses_cpu_tensors():
    from quantool_amd.hip import ops

    z = torch.zeros(2, 128, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="device tensor"):
        ops.lm_head_kl(z, z, torch.zeros(5, 128, dtype=torch.bfloat16), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="device tensor"):
        ops.lm_head_kl(z, z, torch.zeros(5, 128, dtype=torch.bfloat16))


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
    H2 = _al(torch.zeros(3, 128, dtype=bf))
    with pytest.raises(TypeError, match="bf16 or fp16"):
        ops.lm_head_kl(H.float(), H2.float(), W.float(), tg)
    with pytest.raises(TypeError, match="Hq must be of Hp's dtype"):
        ops.lm_head_kl(H, H2.to(fp), W, tg)
    with pytest.raises(TypeError, match="bf16 or fp16"):
        ops.lm_head_kl(H, H2.float(), W, tg)
    with pytest.raises(ValueError, match=r"Hq must be of Hp's shape \(3, 128\)"):
        ops.lm_head_kl(H, _al(torch.zeros(4, 128, dtype=bf)), W, tg)
    with pytest.raises(ValueError, match=r"Hq must be of Hp's shape \(3, 128\)"):
        ops.lm_head_kl(H, _al(torch.zeros(3, 256, dtype=bf)), W, tg)
    with pytest.raises(TypeError, match="W must be of Hp's dtype"):
        ops.lm_head_kl(H, H2, W.to(fp), tg)
    for K in (64, 192, 32896):
        z = torch.zeros(3, K, dtype=bf)
        with pytest.raises(ValueError, match=f"K {K} unsupported"):
            ops.lm_head_kl(z, z, torch.zeros(5, K, dtype=bf), tg)
    with pytest.raises(ValueError, match=r"W must be \[V, 128\]"):
        ops.lm_head_kl(H, H2, torch.zeros(5, 256, dtype=bf), tg)
    with pytest.raises(ValueError, match="Hp must be 2-d .* unit column stride"):
        ops.lm_head_kl(torch.zeros(128, 3, dtype=bf).t(), H2, W, tg)
    with pytest.raises(ValueError, match="Hq must be 2-d .* unit column stride"):
        ops.lm_head_kl(H, torch.zeros(128, 3, dtype=bf).t(), W, tg)
    with pytest.raises(ValueError, match="unit column stride"):
        ops.lm_head_kl(H, H2, torch.zeros(128, 5, dtype=bf).t(), tg)
    with pytest.raises(TypeError, match="targets must be torch.int32 or torch.int64"):
        ops.lm_head_kl(H, H2, W, tg.float())
    with pytest.raises(ValueError, match=r"targets must be contiguous \[3\]"):
        ops.lm_head_kl(H, H2, W, tg[:2])
    with pytest.raises(ValueError, match="Hp: row pitch 132"):
        ops.lm_head_kl(_al(torch.zeros(3, 132, dtype=bf))[:, :128], H2, W, tg)
    with pytest.raises(ValueError, match="Hq: row pitch 132"):
        ops.lm_head_kl(H, _al(torch.zeros(3, 132, dtype=bf))[:, :128], W, tg)
    with pytest.raises(ValueError, match="Hq must start on a 16-byte boundary"):
        ops.lm_head_kl(H, _al(torch.zeros(3, 136, dtype=bf))[:, 4:132], W, tg)
    with pytest.raises(ValueError, match="Hp must start on a 16-byte boundary"):
        ops.lm_head_kl(_al(torch.zeros(3, 136, dtype=bf))[:, 4:132], H2, W, tg)
    for good in ((H, H2, W, tg.int()), (H, H2, W), (H, H, W, tg),     # and a good call passes every check
                 (_al(torch.zeros(3, 136, dtype=bf))[:, :128], _al(torch.zeros(3, 144, dtype=bf))[:, :128], W, tg)):
        with pytest.raises(AssertionError, match="reached the library"):
            ops.lm_head_kl(*good)


def test_the_named_tuple():
    from quantool_amd.hip import ops

    assert ops.LmHeadKl._fields == ("kl", "nll_p", "nll_q", "lse_p", "lse_q", "argmax_p", "argmax_q")


# ---- evaluate -------------------------------------------------------------------------------------------------------
def _tiny_llama(seed=0, **over):
    from transformers import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(seed)
    cfg = LlamaConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=4,
                      num_key_value_heads=4, vocab_size=131, max_position_embeddings=64, **over)
    return LlamaForCausalLM(cfg).to(torch.bfloat16).eval()


IDS = torch.arange(24).reshape(2, 12) % 131


def test_divergence_names_a_cpu_model():
    from quantool_amd.evaluate import divergence

    with pytest.raises(ValueError, match=r"divergence: the reference: .*not on a GPU"):
        divergence(_tiny_llama(), _tiny_llama(), IDS)


def test_divergence_names_a_head_with_bias(pretend_device):
    from quantool_amd.evaluate import divergence

    m = _tiny_llama()
    m.lm_head = torch.nn.Linear(128, 131, bias=True).to(torch.bfloat16)
    with pytest.raises(ValueError, match=r"divergence: the model: .*its head has a bias"):
        divergence(_tiny_llama(), m, IDS)
    with pytest.raises(ValueError, match=r"divergence: the reference: .*its head has a bias"):
        divergence(m, _tiny_llama(), IDS)


def test_divergence_names_heads_that_differ(pretend_device):
    from quantool_amd.evaluate import divergence

    why = "the two models' LM heads differ: one head weight is what the kernel takes"
    with pytest.raises(ValueError, match=why + r" \(the weights are not equal\)"):
        divergence(_tiny_llama(0), _tiny_llama(1), IDS)
    m = _tiny_llama()
    m.lm_head = torch.nn.Linear(128, 140, bias=False).to(torch.bfloat16)
    with pytest.raises(ValueError, match=why + r" \(reference \(131, 128\)"):
        divergence(_tiny_llama(), m, IDS)
    m = _tiny_llama().to(torch.float16)
    with pytest.raises(ValueError, match=why + r" \(reference .*bfloat16, model .*float16"):
        divergence(_tiny_llama(), m, IDS)
    with pytest.raises(AssertionError, match="reached the library"):     # equal heads pass every check
        divergence(_tiny_llama(0), _tiny_llama(0), IDS)


def test_divergence_refuses_a_directory_that_is_not_a_checkpoint(tmp_path):
    from quantool_amd.evaluate import divergence

    with pytest.raises(ValueError, match="not a local checkpoint directory"):
        divergence(tmp_path, _tiny_llama(), IDS)


def test_perplexity_is_unchanged():
    from quantool_amd.evaluate import perplexity

    assert set(perplexity(_tiny_llama(), IDS)) == {"perplexity", "nll", "tokens"}
