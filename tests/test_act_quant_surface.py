"""``qt_act_mul_quantize_i8`` without a GPU: the header declares it, the ctypes table holds it and the built library
exports it; and, called through ctypes with host buffers, every argument the header lists as refused returns
``QT_ERR_INVALID`` before any launch, with ``qt_last_error`` naming the argument."""
import ctypes
import re

import pytest

from tests.i8_fake_ops import check_surface, header_text

NAME = "qt_act_mul_quantize_i8"


def test_header_declares_it():
    check_surface("header", NAME)
    text = header_text()[1]
    args = [a.strip() for a in re.search(NAME + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")]
    assert args == ["const void* gate", "int64_t ldg", "const void* up", "int64_t ldu", "int x_dtype", "int64_t M",
                    "int K", "int act", "const int32_t* col_perm", "int symmetric", "int8_t* Xq", "float* s_x",
                    "int32_t* zp_x", "void* H", "int64_t ldh", "qt_stream_t stream"]
    assert re.search(r"enum\s+qt_act\s*\{\s*QT_ACT_SILU\s*=\s*0\s*\}", text)


def test_header_states_the_sequence():
    raw = re.sub(r" +", " ", re.sub(r"\s*\n\s*\*\s*", " ", header_text()[0]))
    para = raw[raw.index(NAME + ":"):raw.index("enum qt_act")]
    for must in ("a = g / (1.0f + expf(-g)) IEEE division", "rounded once to x_dtype (RNE)", "p = (float)a' * u",
                 "exactly qt_quantize_tokens_i8's row sequence on h", "Xq[m, k] = q(h[m, col_perm[k]])",
                 "QT_ERR_INVALID before any launch", "K > 32768", "no atomics, no workspace",
                 "outside [0, K) is clamped into the row here"):
        assert must in para, must


def test_ctypes_table_holds_it():
    from quantool_amd.hip import _lib

    res, args = _lib.SIGNATURES[NAME]
    p, i, l = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert res is ctypes.c_int
    assert args == [p, l, p, l, i, l, i, i, p, i, p, p, p, p, l, p]


def test_library_exports_it():
    check_surface("library", NAME)


def test_the_quantiser_constants_have_one_home():
    from quantool_amd.csrc import build

    shared = (build.CSRC / "i8_quant.h").read_text()
    assert "kActSymDivisor = 127.5f" in shared and "q_one(" in shared
    for stem in ("qlinear", "act_quant"):
        src = (build.CSRC / f"{stem}.hip").read_text()
        assert '#include "i8_quant.h"' in src, stem
        assert "127.5f" not in src and "int q_one(" not in src, stem


def test_the_kernel_has_no_scratch():
    from quantool_amd.csrc import build

    res = build.OBJ_DIR / "act_quant.resources.txt"
    if not res.exists():
        import __graft_entry__ as g

        g.build()
    rows = [r for r in res.read_text().splitlines() if "act_mul_quantize_kernel" in r]
    assert len(rows) == 4                                   # bf16 / fp16 x 16-byte / element loads
    for row in rows:
        assert "scratch 0\t" in row and "vgpr_spill 0\t" in row, row


# ---- refusals before any launch -------------------------------------------------------------------------------------
QT_BF16, QT_F16, QT_F32 = 1, 2, 0
M0, K0 = 3, 64

# case -> (overrides of the good call, what qt_last_error must name)
BAD = {
    "null gate": (dict(gate=None), r"\bgate\b"),
    "null up": (dict(up=None), r"\bup\b"),
    "null Xq": (dict(Xq=None), r"\bXq\b"),
    "null s_x": (dict(s_x=None), r"\bs_x\b"),
    "M = 0": (dict(M=0), r"\bM\b"),
    "M < 0": (dict(M=-1), r"\bM\b"),
    "K = 0": (dict(K=0), r"\bK\b"),
    "K < 0": (dict(K=-8), r"\bK\b"),
    "ldg below K": (dict(ldg=K0 - 1), r"\bldg\b"),
    "ldu below K": (dict(ldu=K0 - 1), r"\bldu\b"),
    "ldh below K": (dict(H=True, ldh=K0 - 1), r"\bldh\b"),
    "fp32 rows": (dict(x_dtype=QT_F32), r"\bx_dtype\b"),
    "unknown dtype": (dict(x_dtype=7), r"\bx_dtype\b"),
    "unknown act": (dict(act=1), r"\bact\b"),
    "asymmetric without zp_x": (dict(symmetric=0, zp_x=None), r"\bzp_x\b"),
    "K = 32769": (dict(K=32769, ldg=32769, ldu=32769, ldh=32769), r"32768"),
    "M past INT32_MAX": (dict(M=2 ** 31), r"\bM\b.*too large"),
}


@pytest.fixture(scope="module")
def lib():
    from quantool_amd.hip import _lib

    return _lib.load()


@pytest.mark.parametrize("case", list(BAD))
def test_bad_arguments_are_refused_before_any_launch(lib, case):
    """The pointers are host buffers: a refusal never reads them, and nothing here reaches a launch."""
    from quantool_amd.hip import _lib

    bufs = {n: ctypes.create_string_buffer(64) for n in ("gate", "up", "Xq", "s_x", "zp_x", "H")}
    addr = {n: ctypes.addressof(b) for n, b in bufs.items()}
    a = dict(gate=addr["gate"], ldg=K0, up=addr["up"], ldu=K0, x_dtype=QT_BF16, M=M0, K=K0, act=0, col_perm=None,
             symmetric=1, Xq=addr["Xq"], s_x=addr["s_x"], zp_x=addr["zp_x"], H=None, ldh=K0)
    over, names = BAD[case]
    a.update(over)
    if a["H"] is True:
        a["H"] = addr["H"]
    st = lib.qt_act_mul_quantize_i8(a["gate"], a["ldg"], a["up"], a["ldu"], a["x_dtype"], a["M"], a["K"], a["act"],
                                    a["col_perm"], a["symmetric"], a["Xq"], a["s_x"], a["zp_x"], a["H"], a["ldh"], None)
    assert st == _lib.QT_ERR_INVALID
    msg = lib.qt_last_error().decode()
    assert msg.startswith(NAME + ":") and re.search(names, msg), msg
    assert all(b.raw == bytes(64) for b in bufs.values())


def test_ops_refuses_what_the_kernel_does_not_take(monkeypatch):
    """``ops.act_mul_quantize_i8`` checks as ``quantize_tokens_i8`` does: device tensors only."""
    import torch

    from quantool_amd.hip import ops

    g = torch.zeros(2, 8, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="device tensor"):
        ops.act_mul_quantize_i8(g, g)
    assert ops.ACTS == {"silu": 0}
