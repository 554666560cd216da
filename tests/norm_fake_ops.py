"""What the fused-norm tests (test_a8_fused_norm_dispatch.py, test_rmsnorm_quant_surface.py,
test_gpu_a8_fused_norm_modules.py) share: a ``Recorder`` (tests/i8_fake_ops.py) whose quantiser computes on the CPU
and names its caller, with ``rmsnorm_quantize_i8`` as the five-line torch sequence plus that quantiser; the tagging of a
model's ``QuantizedLinear``s; and the list of a model's eligible norms."""
import torch

from tests.i8_fake_ops import Recorder


def torch_rmsnorm(x, weight, eps):
    """``LlamaRMSNorm.forward`` of the installed transformers, line by line."""
    input_dtype = x.dtype
    hidden_states = x.to(torch.float32)
    variance = hidden_states.pow(2).mean(-1, keepdim=True)
    hidden_states = hidden_states * torch.rsqrt(variance + eps)
    return weight * hidden_states.to(input_dtype)


def torch_quantize_tokens(X, symmetric=True, col_perm=None):
    """``qt_quantize_tokens_i8`` in torch (include/quantool_amd.h): min / max including 0, s, zp, q, the gather."""
    x = X.to(torch.float32)
    zero = torch.zeros((), dtype=torch.float32, device=x.device)
    mn = torch.minimum(x.amin(1), zero)
    mx = torch.maximum(x.amax(1), zero)
    eps = torch.tensor(torch.finfo(torch.float32).eps, device=x.device)
    if symmetric:
        s = torch.maximum(torch.maximum(-mn, mx) / 127.5, eps)
        zp = torch.zeros_like(s)
    else:
        s = torch.maximum((mx - mn) / 255.0, eps)
        zp = torch.clamp(torch.round(-128.0 - mn / s), -128.0, 127.0)
    q = torch.round(torch.clamp(x / s[:, None] + zp[:, None], -128.0, 127.0)).to(torch.int8)
    if col_perm is not None:
        q = q[:, col_perm.long()]
    return q.contiguous(), s, None if symmetric else zp.to(torch.int32)


class NormRecorder(Recorder):
    """``Recorder`` with the names the fused switches read.  ``quantised`` lists (caller, shape) of every
    ``quantize_tokens_i8`` call (``caller`` is what ``tag_linears`` set, or None), ``norms`` (shape, symmetric,
    col_perm) of every ``rmsnorm_quantize_i8`` call, ``fused`` the shape of every ``act_mul_quantize_i8`` input."""

    def __init__(self):
        super().__init__()
        self.quantised, self.norms, self.fused = [], [], []
        self.caller = None

    def clear(self):
        self.calls.clear()
        self.quantised.clear()
        self.norms.clear()
        self.fused.clear()

    def quantize_tokens_i8(self, X, symmetric=True, col_perm=None):
        self.quantised.append((self.caller, tuple(X.shape)))
        return torch_quantize_tokens(X, symmetric, col_perm)

    def act_mul_quantize_i8(self, gate, up, symmetric=True, col_perm=None, act="silu", return_h=False):
        assert act == "silu" and not return_h
        self.fused.append(tuple(gate.shape))
        return torch_quantize_tokens(torch.nn.functional.silu(gate) * up, symmetric, col_perm)

    def rmsnorm_quantize_i8(self, X, weight, eps, symmetric=True, col_perm=None, return_rstd=False):
        assert X.dim() == 2 and X.stride(1) == 1 and not return_rstd
        self.norms.append((tuple(X.shape), symmetric, col_perm))
        Y = torch_rmsnorm(X, weight, eps)
        return (Y,) + torch_quantize_tokens(Y, symmetric, col_perm)


def tag_linears(model, rec):
    """Every ``QuantizedLinear``'s ``quantize_rows`` names the Linear in ``rec.caller`` while it runs."""
    from quantool_amd.engine.qmodules import QuantizedLinear

    def tagged(name, inner):
        def quantize_rows(x):
            rec.caller = name
            try:
                return inner(x)
            finally:
                rec.caller = None

        return quantize_rows

    for name, m in model.named_modules():
        if isinstance(m, QuantizedLinear):
            m.quantize_rows = tagged(name, m.quantize_rows)


def quantizing_norms(model):
    from quantool_amd.engine.qmodules import QuantizingRMSNorm

    return {n: m for n, m in model.named_modules() if isinstance(m, QuantizingRMSNorm)}
