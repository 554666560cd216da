"""``qt_rmsnorm_quantize_i8`` without a GPU: the header declares it and states its sequence, the ctypes table holds it
and the built library exports it; called through ctypes with host buffers, every argument the header lists as refused
returns ``QT_ERR_INVALID`` before any launch, with ``qt_last_error`` naming the argument; and ``ops`` refuses what the
kernel does not take before it touches the library."""
import ctypes
import re

import pytest
import torch

from tests.i8_fake_ops import check_surface, header_text

NAME = "qt_rmsnorm_quantize_i8"


def test_header_declares_it():
    check_surface("header", NAME)
    text = header_text()[1]
    args = [a.strip() for a in re.search(NAME + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")]
    assert args == ["const void* X", "int64_t ldx", "const void* weight", "int x_dtype", "int64_t M", "int K",
                    "float eps", "const int32_t* col_perm", "int symmetric", "int8_t* Xq", "float* s_x",
                    "int32_t* zp_x", "void* Y", "int64_t ldy", "float* rstd", "qt_stream_t stream"]
    assert text.index("qt_act_mul_quantize_i8(") < text.index(NAME + "(") < text.index("qt_gemm_i8(")


def test_header_states_the_sequence():
    raw = re.sub(r" +", " ", re.sub(r"\s*\n\s*\*\s*", " ", header_text()[0]))
    para = raw[raw.index(NAME + ":"):raw.index("enum qt_act")]
    for must in ("1. sq_k = x_k * x_k", "owns the 8-element chunks c = t (mod 256)", "in ascending k, starting from 0.0f",
                 "the element-load path walks the same chunks", "xor butterfly 32, 16, ..., 1",
                 "sum = ((wave0 + wave1) + wave2) + wave3", "mean = sum * (1.0f / (float)K)",
                 "v = mean + eps", "r = (float)(1.0 / sqrt((double)v))", "the correctly rounded fp32 value of 1 / sqrt(v)",
                 "rstd[m] = r", "n_k = (x_k * r) rounded once to x_dtype (RNE)",
                 "y_k = ((float)w_k * (float)n_k) rounded once to x_dtype (RNE)",
                 "exactly qt_quantize_tokens_i8's row sequence on y", "Xq[m, k] = q(y[m, col_perm[k]])",
                 "not on alignment, pitch, M or the row's index", "QT_ERR_INVALID before any launch", "K > 32768",
                 "an eps that is negative or not finite", "no atomics, no workspace"):
        assert must in para, must


def test_ctypes_table_holds_it():
    from quantool_amd.hip import _lib

    res, args = _lib.SIGNATURES[NAME]
    p, i, l, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    assert res is ctypes.c_int
    assert args == [p, l, p, i, l, i, f, p, i, p, p, p, p, l, p, p]


def test_library_exports_it():
    check_surface("library", NAME)


def test_the_quantiser_constants_keep_their_one_home():
    from quantool_amd.csrc import build

    shared = (build.CSRC / "i8_quant.h").read_text()
    assert "kActSymDivisor = 127.5f" in shared and "q_one(" in shared and "qt_i8_row_qparams(" in shared
    src = (build.CSRC / "rmsnorm_quant.hip").read_text()
    assert '#include "i8_quant.h"' in src
    for own in ("127.5f", "255.0f", "int q_one(", "FLT_EPSILON", "-128.0f"):
        assert own not in src, own
    assert "qt_i8_row_qparams(mn, mx, symmetric, s, zp)" in src and "q_eight(" in src and "q_one(" in src


def test_the_kernel_has_no_scratch():
    from quantool_amd.csrc import build

    res = build.OBJ_DIR / "rmsnorm_quant.resources.txt"
    if not res.exists():
        import __graft_entry__ as g

        g.build()
    rows = [r for r in res.read_text().splitlines() if "rmsnorm_quantize_kernel" in r]
    assert len(rows) == 4                                   # bf16 / fp16 x 16-byte / element loads
    for row in rows:
        assert "scratch 0\t" in row and "vgpr_spill 0\t" in row, row


# ---- refusals before any launch -------------------------------------------------------------------------------------
QT_BF16, QT_F16, QT_F32 = 1, 2, 0
M0, K0 = 3, 64

# case -> (overrides of the good call, what qt_last_error must name)
BAD = {
    "null X": (dict(X=None), r"\bX\b"),
    "null weight": (dict(weight=None), r"\bweight\b"),
    "null Xq": (dict(Xq=None), r"\bXq\b"),
    "null s_x": (dict(s_x=None), r"\bs_x\b"),
    "M = 0": (dict(M=0), r"\bM\b"),
    "M < 0": (dict(M=-1), r"\bM\b"),
    "M past INT32_MAX": (dict(M=2 ** 31), r"\bM\b.*too large"),
    "K = 0": (dict(K=0), r"\bK\b"),
    "K < 0": (dict(K=-8), r"\bK\b"),
    "K = 32769": (dict(K=32769, ldx=32769, ldy=32769), r"32768"),
    "ldx below K": (dict(ldx=K0 - 1), r"\bldx\b"),
    "ldy below K": (dict(Y=True, ldy=K0 - 1), r"\bldy\b"),
    "fp32 rows": (dict(x_dtype=QT_F32), r"\bx_dtype\b"),
    "unknown dtype": (dict(x_dtype=7), r"\bx_dtype\b"),
    "asymmetric without zp_x": (dict(symmetric=0, zp_x=None), r"\bzp_x\b"),
    "eps < 0": (dict(eps=-1e-6), r"\beps\b"),
    "eps = inf": (dict(eps=float("inf")), r"\beps\b"),
    "eps = nan": (dict(eps=float("nan")), r"\beps\b"),
}


@pytest.fixture(scope="module")
def lib():
    from quantool_amd.hip import _lib

    return _lib.load()


@pytest.mark.parametrize("case", list(BAD))
def test_bad_arguments_are_refused_before_any_launch(lib, case):
    """The pointers are host buffers: a refusal never reads them, and nothing here reaches a launch."""
    from quantool_amd.hip import _lib

    bufs = {n: ctypes.create_string_buffer(64) for n in ("X", "weight", "Xq", "s_x", "zp_x", "Y", "rstd")}
    addr = {n: ctypes.addressof(b) for n, b in bufs.items()}
    a = dict(X=addr["X"], ldx=K0, weight=addr["weight"], x_dtype=QT_BF16, M=M0, K=K0, eps=1e-6, col_perm=None,
             symmetric=1, Xq=addr["Xq"], s_x=addr["s_x"], zp_x=addr["zp_x"], Y=None, ldy=K0, rstd=addr["rstd"])
    over, names = BAD[case]
    a.update(over)
    if a["Y"] is True:
        a["Y"] = addr["Y"]
    st = lib.qt_rmsnorm_quantize_i8(a["X"], a["ldx"], a["weight"], a["x_dtype"], a["M"], a["K"], a["eps"],
                                    a["col_perm"], a["symmetric"], a["Xq"], a["s_x"], a["zp_x"], a["Y"], a["ldy"],
                                    a["rstd"], None)
    assert st == _lib.QT_ERR_INVALID
    msg = lib.qt_last_error().decode()
    assert msg.startswith(NAME + ":") and re.search(names, msg), msg
    assert all(b.raw == bytes(64) for b in bufs.values())


# ---- ops ------------------------------------------------------------------------------------------------------------
def test_ops_refuses_cpu_tensors():
    from quantool_amd.hip import ops

    x = torch.zeros(2, 8, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="device tensor"):
        ops.rmsnorm_quantize_i8(x, torch.ones(8, dtype=torch.bfloat16), 1e-6)


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


def test_ops_refuses_what_the_kernel_does_not_take(pretend_device):
    ops = pretend_device
    bf, fp = torch.bfloat16, torch.float16
    x, w = torch.zeros(3, 16, dtype=bf), torch.ones(16, dtype=bf)
    perm = torch.arange(16, dtype=torch.int32)
    with pytest.raises(TypeError, match="weight must be of X's dtype"):
        ops.rmsnorm_quantize_i8(x, w.to(fp), 1e-6)
    with pytest.raises(TypeError, match="weight must be of X's dtype"):
        ops.rmsnorm_quantize_i8(x, w.float(), 1e-6)
    with pytest.raises(TypeError, match="bf16 or fp16"):
        ops.rmsnorm_quantize_i8(x.float(), w.float(), 1e-6)
    with pytest.raises(ValueError, match="X's device"):
        ops.rmsnorm_quantize_i8(x, torch.ones(16, dtype=bf, device="meta"), 1e-6)
    with pytest.raises(ValueError, match="unit column stride"):
        ops.rmsnorm_quantize_i8(torch.zeros(16, 3, dtype=bf).t(), w, 1e-6)
    with pytest.raises(ValueError, match="unit column stride"):
        ops.rmsnorm_quantize_i8(torch.zeros(2, 3, 16, dtype=bf), w, 1e-6)
    for empty, we in ((torch.zeros(0, 16, dtype=bf), w), (torch.zeros(3, 0, dtype=bf), w[:0])):
        with pytest.raises(ValueError, match="non-empty"):
            ops.rmsnorm_quantize_i8(empty, we, 1e-6)
    for bad_w in (torch.ones(15, dtype=bf), torch.ones(1, 16, dtype=bf), torch.ones(32, dtype=bf)[::2]):
        with pytest.raises(ValueError, match=r"weight must be contiguous \[16\]"):
            ops.rmsnorm_quantize_i8(x, bad_w, 1e-6)
    for bad_perm in (torch.arange(32, dtype=torch.int32)[::2], perm[:15]):
        with pytest.raises(ValueError, match=r"col_perm must be contiguous int32 \[16\]"):
            ops.rmsnorm_quantize_i8(x, w, 1e-6, col_perm=bad_perm)
    with pytest.raises(TypeError, match="col_perm must be torch.int32"):
        ops.rmsnorm_quantize_i8(x, w, 1e-6, col_perm=perm.long())
    for bad_eps in (-1e-6, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="eps must be finite and not negative"):
            ops.rmsnorm_quantize_i8(x, w, bad_eps)
    with pytest.raises(AssertionError, match="reached the library"):     # and a good call passes every check
        ops.rmsnorm_quantize_i8(x, w, 1e-6, col_perm=perm)
