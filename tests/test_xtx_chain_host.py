"""``chain_tokens`` -- the bound on an fp32 accumulator chain inside a Gram launch -- on the host side (no GPU): the two
entry points exist in the header, the library and the ctypes table; a bound that is no multiple of 640 is refused
before anything else is looked at; ``QT_XTX_CHAIN_TOKENS`` is parsed as documented; ``HessianAccumulator`` hands the
value to the 16-bit Gram calls and to nothing else."""
import ctypes
import re
import subprocess
from pathlib import Path

import pytest
import torch

from quantool_amd.engine import gptq_linear as gl

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("qt_xtx_accumulate_chained", "qt_xtx_accumulate_batched_chained")
QT_ERR_INVALID = -1


@pytest.fixture(scope="module")
def lib():
    from quantool_amd.hip import _lib

    if not _lib.LIB_PATH.exists():
        import __graft_entry__ as g

        g.build()
    raw = ctypes.CDLL(str(_lib.LIB_PATH))          # loading needs no GPU
    for name in NAMES:
        fn = getattr(raw, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    raw.qt_last_error.restype = ctypes.c_char_p
    return raw


def test_names_in_header_exports_and_ctypes_table(lib):
    from quantool_amd.hip import _lib

    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "quantool_amd.h").read_text(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in the header"
        assert name in exported, f"{name} is not exported"
        assert name in _lib.SIGNATURES
    # the chained calls take the unchained calls' arguments plus one int64 in front of the workspace
    for name in NAMES:
        plain = _lib.SIGNATURES[name[:-len("_chained")]][1]
        assert _lib.SIGNATURES[name][1] == plain[:-3] + [ctypes.c_int64] + plain[-3:]
    assert header.count("_workspace_bytes(") == sum(n.endswith("_workspace_bytes") for n in _lib.SIGNATURES)
    assert not any("chain" in n and n.endswith("_workspace_bytes") for n in _lib.SIGNATURES)


@pytest.mark.parametrize("chain", [-640, 1, 639, 1000])
def test_bad_chain_tokens_is_refused_before_anything_else(lib, chain):
    """Every other argument is NULL / 0 here, so a check that ran after them, or after a device call, would report
    something else (or fail on a machine without a device)."""
    rc = lib.qt_xtx_accumulate_chained(None, 1, 128, 256, 256, None, chain, None, 0, None)
    assert rc == QT_ERR_INVALID
    msg = lib.qt_last_error()
    assert b"chain_tokens" in msg and b"qt_xtx_accumulate_chained" in msg, msg
    rc = lib.qt_xtx_accumulate_batched_chained(None, 1, None, None, 256, None, 2, chain, None, 0, None)
    assert rc == QT_ERR_INVALID
    msg = lib.qt_last_error()
    assert b"chain_tokens" in msg and b"qt_xtx_accumulate_batched_chained" in msg, msg


def test_a_good_bound_reaches_the_other_checks(lib):
    """640 passes the bound's check; the NULL pointers are then what is refused (still before any device call)."""
    assert lib.qt_xtx_accumulate_chained(None, 1, 128, 256, 256, None, 640, None, 0, None) == QT_ERR_INVALID
    assert b"chain_tokens" not in lib.qt_last_error() and b"null pointer" in lib.qt_last_error()
    assert lib.qt_xtx_accumulate_chained(None, 1, 0, 256, 256, None, 1280, None, 0, None) == 0      # no tokens: nothing to do


@pytest.mark.parametrize("text,want", [("1300", 1280), ("639", 0), ("x", 0), (None, 0), ("640", 640), ("30720", 30720),
                                       ("-5", 0), ("", 0)])
def test_environment_parsing(monkeypatch, text, want):
    if text is None:
        monkeypatch.delenv("QT_XTX_CHAIN_TOKENS", raising=False)
    else:
        monkeypatch.setenv("QT_XTX_CHAIN_TOKENS", text)
    assert gl._chain_token_limit() == want


def test_ops_refuse_a_bad_bound_without_a_device():
    from quantool_amd.hip import ops

    X, G = torch.zeros(64, 64, dtype=torch.bfloat16), torch.zeros(64, 64)
    for bad in (-640, 1, 639, 1000):
        with pytest.raises(ValueError, match="chain_tokens"):
            ops.xtx_accumulate(X, G, chain_tokens=bad)
        with pytest.raises(ValueError, match="chain_tokens"):
            ops.xtx_accumulate_batched([X], [G], chain_tokens=bad)


@pytest.fixture
def calls(monkeypatch):
    """a recording stand-in for ``ops``: (which, rows, keyword arguments) per Gram call"""
    log = []
    monkeypatch.setattr(gl.ops, "xtx_accumulate", lambda rows, G, **kw: log.append(("single", rows.shape[0], kw)))
    monkeypatch.setattr(gl.ops, "xtx_accumulate_f32", lambda rows, G, **kw: log.append(("f32", rows.shape[0], kw)))
    monkeypatch.setattr(gl.ops, "xtx_accumulate_batched",
                        lambda Xs, Gs, **kw: log.append(("batched", [x.shape[0] for x in Xs], kw)))
    for v in ("QT_XTX_LAUNCH_TOKENS", "QT_FP32_ACTIVATIONS", "QT_XTX_CHAIN_TOKENS", "QT_XTX_BATCHED"):
        monkeypatch.delenv(v, raising=False)
    return log


def _acc(K, rows, dtype=torch.bfloat16):
    acc = gl.HessianAccumulator(K, "cpu", stage_tokens=4096)
    acc.add(torch.ones(rows, K, dtype=dtype))
    return acc


def test_gram_forwards_the_bound_on_16_bit_rows_only(monkeypatch, calls):
    monkeypatch.setenv("QT_XTX_CHAIN_TOKENS", "1300")
    for dtype in (torch.bfloat16, torch.float16):
        _acc(512, 100, dtype).flush()
    _acc(512, 100, torch.float32).flush()
    assert calls == [("single", 100, {"chain_tokens": 1280}), ("single", 100, {"chain_tokens": 1280}), ("f32", 100, {})]


def test_launch_splitting_comes_first_and_each_launch_is_chained(monkeypatch, calls):
    monkeypatch.setenv("QT_XTX_CHAIN_TOKENS", "640")
    monkeypatch.setenv("QT_XTX_LAUNCH_TOKENS", "1500")           # 1472 per launch
    _acc(512, 3000).flush()
    assert calls == [("single", 1472, {"chain_tokens": 640}), ("single", 1472, {"chain_tokens": 640}),
                     ("single", 56, {"chain_tokens": 640})]


def test_flush_many_forwards_the_bound_to_the_batched_call(monkeypatch, calls):
    monkeypatch.setenv("QT_XTX_BATCHED", "1")
    monkeypatch.setenv("QT_XTX_CHAIN_TOKENS", "30720")
    gl.HessianAccumulator.flush_many([_acc(512, 100), _acc(512, 200), _acc(1024, 70)])
    assert calls == [("single", 70, {"chain_tokens": 30720}), ("batched", [100, 200], {"chain_tokens": 30720})]


@pytest.mark.parametrize("text", [None, "0", "639", "x"])
def test_unset_the_calls_carry_no_bound(monkeypatch, calls, text):
    if text is not None:
        monkeypatch.setenv("QT_XTX_CHAIN_TOKENS", text)
    monkeypatch.setenv("QT_XTX_BATCHED", "1")
    _acc(512, 100).flush()
    gl.HessianAccumulator.flush_many([_acc(512, 100), _acc(512, 200)])
    assert [c[0] for c in calls] == ["single", "batched"]
    assert all(c[2].get("chain_tokens", 0) == 0 for c in calls)
