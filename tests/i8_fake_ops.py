"""What the int8 dispatch tests (test_i8_*_dispatch.py, test_i8_forms.py) share: a recording stand-in for
``quantool_amd.hip.ops`` that carries every name ``QuantizedLinear`` / ``QuantizedExperts`` may read, the fixture that
installs it, aligned and shifted CPU buffers, and the header / ctypes table / library checks of an entry point."""
import re
import subprocess
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
DENSE = ("gemm_i8", "gemm_i8_skinny", "gemm_i8_mid", "gemm_i8_ring", "gemm_i8_ring_w4")
GROUPED = ("gemm_i8_grouped", "gemm_i8_skinny_grouped", "gemm_i8_ring_grouped")
SUPPORTED = ("gemm_i8_mid_supported", "gemm_i8_ring_supported", "gemm_i8_ring_w4_supported",
             "gemm_i8_ring_grouped_supported")


class Recorder:
    """Stands in for quantool_amd.hip.ops: the eight GEMMs record (name, rows) in ``calls``; every ``*_supported``
    records its call in ``queries[name]`` (the rows of row_idx, or None) and answers ``answers[name]``; the I8_*
    constants are the real ones; the passes around the GEMMs return tensors of the right shapes on the CPU.
    ``asked`` / ``supported`` speak of the one ``*_supported`` a test file watches."""

    def __init__(self, watch=None):
        from quantool_amd.hip import ops as real

        for name in dir(real):
            if name.startswith("I8_"):
                setattr(self, name, getattr(real, name))
        self.calls = []
        self.watch = watch
        self.answers = {name: True for name in SUPPORTED}
        self.queries = {name: [] for name in SUPPORTED}
        for name in DENSE + GROUPED + SUPPORTED:
            setattr(self, name, getattr(self, "_grouped" if name in GROUPED else "_supported" if name in SUPPORTED
                                        else "_dense")(name))

    @property
    def asked(self):
        """How often the watched function was asked; for the grouped one, with how many rows of row_idx each time."""
        q = self.queries[self.watch]
        return q if self.watch == "gemm_i8_ring_grouped_supported" else len(q)

    @property
    def supported(self):
        return self.answers[self.watch]

    @supported.setter
    def supported(self, value):
        self.answers[self.watch] = value

    def _dense(self, name):
        def gemm(Xq, s_x, Wq, s_w, **kw):
            self.calls.append((name, Xq.shape[0]))
            return torch.zeros(Xq.shape[0], Wq.shape[-2], dtype=kw["out_dtype"])

        return gemm

    def _grouped(self, name):
        def gemm(Xq, s_x, Wq, s_w, offsets, **kw):
            rows = kw["row_idx"].numel() if kw.get("row_idx") is not None else Xq.shape[0]
            self.calls.append((name, rows))
            return torch.zeros(rows, Wq.shape[-2], dtype=kw["out_dtype"])

        return gemm

    def _supported(self, name):
        def supported(Xq, Wq, s_w, row_idx=None):
            self.queries[name].append(None if row_idx is None else row_idx.numel())
            return self.answers[name]

        return supported

    def quantize_tokens_i8(self, X, symmetric=True, col_perm=None):
        M = X.shape[0]
        zp = None if symmetric else torch.zeros(M, dtype=torch.int32)
        return torch.zeros(X.shape, dtype=torch.int8), torch.ones(M), zp

    def moe_route(self, top_k_index, num_experts):
        R = top_k_index.numel()
        z = torch.zeros(R, dtype=torch.int32)
        return torch.zeros(num_experts + 1, dtype=torch.int32), z, z, z

    def moe_combine(self, Y, row_of, top_k_weights):
        return torch.zeros(top_k_weights.shape[0], Y.shape[1], dtype=Y.dtype)


@pytest.fixture
def fake_ops(request, monkeypatch):
    """A Recorder in the place of quantool_amd.hip.ops.  The test module may name the ``*_supported`` it watches
    (``WATCH``) and the QuantizedLinear attributes its dispatch rules assume (``LINEAR_ATTRS``), whatever the measured
    class defaults are."""
    import quantool_amd.hip as hip
    from quantool_amd.engine.qmodules import QuantizedLinear
    from quantool_amd.hip import ops as real   # noqa: F401  (the attribute the modules import must exist first)

    rec = Recorder(getattr(request.module, "WATCH", None))
    monkeypatch.setattr(hip, "ops", rec)
    for name, value in getattr(request.module, "LINEAR_ATTRS", {}).items():
        monkeypatch.setattr(QuantizedLinear, name, value)
    return rec


def _aligned(dtype, rows, cols, shift):
    size = torch.empty(0, dtype=dtype).element_size()
    buf = torch.zeros(rows * cols + 32, dtype=dtype)
    off = ((-buf.data_ptr()) % 16) // size + shift
    return buf[off:off + rows * cols].view(rows, cols)


def aligned_i8(rows, cols, shift=0):
    """A zero int8 matrix whose first byte lies ``shift`` bytes behind a 16-byte boundary."""
    return _aligned(torch.int8, rows, cols, shift)


def aligned_i32(rows, cols, shift=0):
    """A zero int32 matrix whose first word lies ``shift`` words behind a 16-byte boundary."""
    return _aligned(torch.int32, rows, cols, shift)


def header_text():
    """include/quantool_amd.h: (as it is, without its comments)."""
    raw = (ROOT / "include" / "quantool_amd.h").read_text()
    return raw, re.sub(r"/\*.*?\*/", "", raw, flags=re.S)


def header_constants(prefix):
    """The header's ``#define <prefix>NAME <int>`` lines as a dict."""
    return {k: int(v) for k, v in re.findall(rf"#define\s+({prefix}[A-Z_]+)\s+(\d+)", header_text()[1])}


def check_surface(part, name, like=None):
    """One part of an entry point's surface: the "header" declares it, the "ctypes" table holds it with the signature
    of ``like`` (the tiled or the grouped entry point), the built "library" exports it."""
    from quantool_amd.hip import _lib

    if part == "header":
        assert name in set(re.findall(r"\b(qt_[a-z0-9_]+)\s*\(", header_text()[1]))
    elif part == "ctypes":
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[like]
    elif part == "library":
        if not _lib.LIB_PATH.exists():
            import __graft_entry__ as g

            g.build()
        out = subprocess.check_output(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], text=True)
        assert name in {line.split()[-1] for line in out.splitlines() if " T " in line}
    else:
        raise KeyError(part)
