"""The workspace contract of the C ABI: an entry point writes no scratch outside ``(workspace, workspace_bytes)`` when
the caller passes exactly what the matching ``*_workspace_bytes()`` returns.

The rest of the suite cannot see a breach: it goes through ``ops.workspace()``, a grow-only buffer that is soon larger
than any later call asks for.  Here the library is called directly (``_lib.load()``, raw pointers) on a workspace the
test owns: ``guard + need + guard`` bytes of one byte pattern, the middle ``need`` bytes handed over.  After the call

* both guards still hold the pattern, byte for byte (a stray write lands in the test's own memory, not in a fault);
* every output is bit-identical to the same call made through ``ops`` (all of these entry points are documented as
  deterministic);
* ``workspace_bytes = need - 1`` and a NULL workspace are refused with ``QT_ERR_WORKSPACE`` and leave the outputs and
  the whole buffer untouched (nothing was launched).

Every entry point aligns the workspace pointer up to 256 itself and its size carries the slack (read in csrc/: xtx.hip,
gemm3_tn.hip, stats.hip, hessian.hip, cholesky.hip, sweep.hip, awq.hip, sgemm_tn.hip), so every case also runs with the
pointer 16 bytes off a 256-byte boundary.

Shapes come from the planners, one case per branch of a size computation; each case names its branch.  The Cholesky
chain and the gemm3 test face have fixed shares of 128 MiB (split-K slabs / slab area), so their workspaces are not
small whatever K is; the guard is as large as the workspace in every case.
"""
import ctypes

import numpy as np
import pytest
import torch

from quantool_amd.hip import _lib
from quantool_amd.hip._lib import QT_BF16, QT_ERR_WORKSPACE, QT_F16, QT_F32, QT_OK

pytestmark = pytest.mark.gpu

PATTERN = 0xA5
CODES = {torch.float32: QT_F32, torch.bfloat16: QT_BF16, torch.float16: QT_F16}


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Case:
    """One entry point at one shape.  ``host``: numpy inputs, built once; ``make(dev)``: fresh device tensors from them
    (a dict; the outputs included, initialised as the caller must); ``need(lib, t)``; ``call(lib, t, ws, nbytes)`` -> the
    status; ``via_ops(ops, t)``; ``outs``: names of the tensors the call writes."""

    def __init__(self, name, branch, make, need, call, via_ops, outs, env=None):
        self.name, self.branch, self.make, self.need, self.call, self.via_ops, self.outs = (
            name, branch, make, need, call, via_ops, outs)
        self.env = env or {}


def _first_bad(region: torch.Tensor):
    bad = (region != PATTERN).nonzero()
    return None if bad.numel() == 0 else (int(bad[0]), int(bad[-1]), int(bad.numel()))


def _run(case: Case, dev, ops, monkeypatch, offset: int):
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    lib = _lib.load()
    t = case.make(dev)
    need = int(case.need(lib, t))
    assert need > 0, "the case must need a workspace"
    guard = (max(1 << 20, need) + 255) // 256 * 256
    start = guard + offset
    buf = torch.full((start + need + guard,), PATTERN, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 256 == 0
    ws = buf.data_ptr() + start
    before = {n: t[n].clone() for n in case.outs}
    torch.cuda.synchronize()

    # refusals: nothing may be launched
    rc = case.call(lib, t, ws, need - 1)
    assert rc == QT_ERR_WORKSPACE, f"{case.name}: workspace_bytes = need - 1 returned {rc}"
    rc = case.call(lib, t, None, need)
    assert rc == QT_ERR_WORKSPACE, f"{case.name}: NULL workspace returned {rc}"
    torch.cuda.synchronize()
    assert _first_bad(buf) is None, f"{case.name}: a refused call wrote to the workspace buffer"
    for n in case.outs:
        assert torch.equal(t[n], before[n]), f"{case.name}: a refused call wrote to {n}"

    # the guarded call
    rc = case.call(lib, t, ws, need)
    assert rc == QT_OK, f"{case.name}: status {rc}: {lib.qt_last_error()}"
    torch.cuda.synchronize()
    lo, hi = _first_bad(buf[:start]), _first_bad(buf[start + need:])
    assert hi is None, (f"{case.name} [{case.branch}]: wrote past the {need} bytes it asked for: first / last bad byte "
                        f"{hi[0]} / {hi[1]} bytes behind the end, {hi[2]} bytes changed")
    assert lo is None, (f"{case.name} [{case.branch}]: wrote in front of the workspace: first bad byte at "
                        f"{lo[0] - start} relative to it, {lo[2]} bytes changed")

    # the same call through ops, on fresh copies of the same inputs
    t2 = case.make(dev)
    case.via_ops(ops, t2)
    torch.cuda.synchronize()
    for n in case.outs:
        assert torch.equal(t[n], t2[n]), f"{case.name}: {n} differs from the call through ops"
    del buf


def _rng(seed):
    return np.random.default_rng(seed)


def _dev(a, dev, dtype=None):
    x = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return x if dtype is None else x.to(dtype)


# ---------------------------------------------------------------------------------------------------- a7: Gram sums
def _xtx(n, K, dtype, pad, branch):
    host = (_rng(n + K).standard_normal((n, K + pad)) * 0.5).astype(np.float32)

    def make(dev):
        X = _dev(host, dev, dtype)
        return dict(X=X[:, :K] if pad else X, G=torch.zeros((K, K), dtype=torch.float32, device=dev))

    return Case(
        f"qt_xtx_accumulate n={n} K={K} ldx={K + pad} {str(dtype)[6:]}", branch, make,
        lambda lib, t: lib.qt_xtx_workspace_bytes(n, K),
        lambda lib, t, ws, nb: lib.qt_xtx_accumulate(t["X"].data_ptr(), CODES[dtype], n, K, K + pad, t["G"].data_ptr(), ws,
                                                     nb, _stream()),
        lambda ops, t: ops.xtx_accumulate(t["X"], t["G"]), ["G"])


def _xtx_f32(n, K, branch):
    host = _rng(n * 3 + K).standard_normal((n, K)).astype(np.float32)

    def make(dev):
        return dict(X=_dev(host, dev), G=torch.zeros((K, K), dtype=torch.float32, device=dev))

    return Case(
        f"qt_xtx_accumulate_f32 n={n} K={K}", branch, make,
        lambda lib, t: lib.qt_xtx_accumulate_f32_workspace_bytes(n, K),
        lambda lib, t, ws, nb: lib.qt_xtx_accumulate_f32(t["X"].data_ptr(), n, K, K, t["G"].data_ptr(), ws, nb, _stream()),
        lambda ops, t: ops.xtx_accumulate_f32(t["X"], t["G"]), ["G"])


def _xtx_dot(n, K, branch):
    r = _rng(n + 7 * K)
    hx = (r.standard_normal((n, K)) * 0.5).astype(np.float32)
    hh = r.standard_normal((K, K)).astype(np.float32)

    def make(dev):
        return dict(X=_dev(hx, dev, torch.bfloat16), H=_dev(hh, dev), out=torch.zeros(1, dtype=torch.float32, device=dev))

    return Case(
        f"qt_xtx_dot n={n} K={K}", branch, make,
        lambda lib, t: lib.qt_xtx_dot_workspace_bytes(n, K),
        lambda lib, t, ws, nb: lib.qt_xtx_dot(t["X"].data_ptr(), QT_BF16, n, K, K, t["H"].data_ptr(), 0.125,
                                              t["out"].data_ptr(), 0, ws, nb, _stream()),
        lambda ops, t: ops.xtx_dot(t["X"], t["H"], 0.125, out=t["out"]), ["out"])


# ------------------------------------------------------------------------------------- a12 / a13: activation statistics
def _act_stats(n, K, branch):
    host = _rng(n + K + 1).standard_normal((n, K)).astype(np.float32)

    def make(dev):
        return dict(X=_dev(host, dev, torch.float16), s=torch.zeros(K, dtype=torch.float32, device=dev),
                    mn=torch.full((K,), float("inf"), dtype=torch.float32, device=dev),
                    mx=torch.full((K,), float("-inf"), dtype=torch.float32, device=dev))

    return Case(
        f"qt_act_stats_accumulate n={n} K={K}", branch, make,
        lambda lib, t: lib.qt_act_stats_workspace_bytes(n, K),
        lambda lib, t, ws, nb: lib.qt_act_stats_accumulate(t["X"].data_ptr(), QT_F16, n, K, K, t["s"].data_ptr(),
                                                           t["mn"].data_ptr(), t["mx"].data_ptr(), ws, nb, _stream()),
        lambda ops, t: ops.act_stats_accumulate(t["X"], t["s"], t["mn"], t["mx"]), ["s", "mn", "mx"])


# ----------------------------------------------------------------------------------------- a8 / a9: prepare, factorise
def _spd(K, seed):
    r = _rng(seed)
    M = r.standard_normal((K, 2 * K)).astype(np.float32)
    return (M @ M.T / np.float32(2 * K) + np.eye(K, dtype=np.float32)).astype(np.float32)


def _prepare(K, branch, env=None):
    hg = np.tril(_spd(K, K))
    hperm = _rng(K + 1).permutation(K).astype(np.int32)

    def make(dev):
        return dict(G=_dev(hg, dev), perm=_dev(hperm, dev), A=torch.zeros((K, K), dtype=torch.float32, device=dev),
                    dead=torch.zeros(K, dtype=torch.uint8, device=dev), diag=torch.zeros(K, dtype=torch.float32, device=dev))

    def via_ops(ops, t):
        _, dead, diag = ops.hessian_prepare(t["G"], 8, 0.01, t["perm"], A_out=t["A"])
        t["dead"], t["diag"] = dead, diag

    return Case(
        f"qt_hessian_prepare K={K}", branch, make,
        lambda lib, t: lib.qt_hessian_prepare_workspace_bytes(K),
        lambda lib, t, ws, nb: lib.qt_hessian_prepare(t["G"].data_ptr(), K, 8, 0.01, t["perm"].data_ptr(), t["A"].data_ptr(),
                                                      t["dead"].data_ptr(), t["diag"].data_ptr(), ws, nb, _stream()),
        via_ops, ["A", "dead", "diag"], env)


F32_CHAIN = {"QT_CHOL_G3": "0"}
BF16X3_CHAIN = {"QT_CHOL_G3": "1", "QT_CHOL_G3_MIN_CHUNKS": "1"}   # as test_cholesky_inverse_upper_bf16x3_products


def _chol(K, env, branch):
    ha = _spd(K, 3 * K)

    def make(dev):
        return dict(A=_dev(ha, dev), U=torch.zeros((K, K), dtype=torch.float32, device=dev),
                    info=torch.full((1,), 7, dtype=torch.int32, device=dev))

    def via_ops(ops, t):
        _, t["info"] = ops.cholesky_inverse_upper(t["A"], U_out=t["U"])

    return Case(
        f"qt_cholesky_inverse_upper K={K} {'bf16x3' if env is BF16X3_CHAIN else 'f32'}", branch, make,
        lambda lib, t: lib.qt_cholesky_inverse_upper_workspace_bytes(K),
        lambda lib, t, ws, nb: lib.qt_cholesky_inverse_upper(t["A"].data_ptr(), K, t["U"].data_ptr(), t["info"].data_ptr(),
                                                             ws, nb, _stream()),
        via_ops, ["U", "info"], env)


def _chol_batched(K, n, env, branch):
    ha = np.stack([_spd(K, 5 * K + b) for b in range(n)])

    def make(dev):
        return dict(A=_dev(ha, dev), U=torch.zeros((n, K, K), dtype=torch.float32, device=dev),
                    info=torch.full((n,), 7, dtype=torch.int32, device=dev))

    def via_ops(ops, t):
        t["info"] = ops.cholesky_inverse_upper_batched(t["A"], t["U"])

    return Case(
        f"qt_cholesky_inverse_upper_batched K={K} n={n} {'bf16x3' if env is BF16X3_CHAIN else 'f32'}", branch, make,
        lambda lib, t: lib.qt_cholesky_inverse_upper_batched_workspace_bytes(K, n),
        lambda lib, t, ws, nb: lib.qt_cholesky_inverse_upper_batched(t["A"].data_ptr(), K * K, K, t["U"].data_ptr(), K * K,
                                                                     t["info"].data_ptr(), n, ws, nb, _stream()),
        via_ops, ["U", "info"], env)


# -------------------------------------------------------------------------------------------------------- a11: sweep
def _sweep_inputs(R, K, n_groups, seed):
    r = _rng(seed)
    W = (r.standard_normal((R, K)) * 0.02).astype(np.float32)
    U = np.stack([np.triu(r.standard_normal((K, K)) * 0.02, 1).astype(np.float32) +
                  np.diag(1.0 + r.random(K)).astype(np.float32) for _ in range(n_groups)])
    G = K // 128
    amax = np.abs(W.reshape(R, G, 128)).max(axis=2)
    scale_t = np.ascontiguousarray((amax / np.float32(7.5)).T.astype(np.float32))
    g_idx = np.tile((np.arange(K) // 128).astype(np.int32), (n_groups, 1))
    return W, U, scale_t, g_idx


def _sweep(R, K, env, branch):
    hW, hU, hs, hg = _sweep_inputs(R, K, 1, R + K)
    G = K // 128

    def make(dev):
        return dict(W=_dev(hW, dev), U=_dev(hU[0], dev), s=_dev(hs, dev), z=torch.zeros((G, R), dtype=torch.float32, device=dev),
                    g=_dev(hg[0], dev), Qt=torch.zeros((K, R), dtype=torch.int8, device=dev),
                    loss=torch.zeros(R, dtype=torch.float32, device=dev))

    def via_ops(ops, t):
        t["Qt"], t["loss"] = ops.gptq_sweep(t["W"], t["U"], t["s"], t["z"], t["g"], 128, 4)

    return Case(
        f"qt_gptq_sweep R={R} K={K}{' far=bf16x3' if env and 'QT_SWEEP_FAR' in env else ''}", branch, make,
        lambda lib, t: lib.qt_gptq_sweep_workspace_bytes(R, K, 128),
        lambda lib, t, ws, nb: lib.qt_gptq_sweep(t["W"].data_ptr(), R, K, t["U"].data_ptr(), t["s"].data_ptr(),
                                                 t["z"].data_ptr(), G, t["g"].data_ptr(), 128, 4, t["Qt"].data_ptr(),
                                                 t["loss"].data_ptr(), ws, nb, _stream()),
        via_ops, ["W", "Qt", "loss"], env)


def _sweep_grouped(R, K, row_end, branch, env=None):
    n = len(row_end)
    hW, hU, hs, hg = _sweep_inputs(R, K, n, R + K + n)
    G = K // 128
    ends = (ctypes.c_int32 * n)(*row_end)

    def make(dev):
        return dict(W=_dev(hW, dev), U=_dev(hU, dev), s=_dev(hs, dev), z=torch.zeros((G, R), dtype=torch.float32, device=dev),
                    g=_dev(hg, dev), Qt=torch.zeros((K, R), dtype=torch.int8, device=dev),
                    loss=torch.zeros(R, dtype=torch.float32, device=dev))

    def via_ops(ops, t):
        t["Qt"], t["loss"] = ops.gptq_sweep_grouped(t["W"], t["U"], row_end, t["s"], t["z"], t["g"], 128, 4)

    return Case(
        f"qt_gptq_sweep_grouped R={R} K={K} row_end={row_end}", branch, make,
        lambda lib, t: lib.qt_gptq_sweep_workspace_bytes(R, K, 128),
        lambda lib, t, ws, nb: lib.qt_gptq_sweep_grouped(
            t["W"].data_ptr(), R, K, t["U"].data_ptr(), K * K, n, ctypes.cast(ends, ctypes.c_void_p), t["s"].data_ptr(),
            t["z"].data_ptr(), G, t["g"].data_ptr(), 128, 4, t["Qt"].data_ptr(), t["loss"].data_ptr(), ws, nb, _stream()),
        via_ops, ["W", "Qt", "loss"], env)


# ---------------------------------------------------------------------------------------------------------- a12: AWQ
def _wmean(R, K, gs, dtype, branch):
    host = (_rng(R + K + gs).standard_normal((R, K)) * 0.05).astype(np.float32)

    def make(dev):
        return dict(W=_dev(host, dev, dtype), s=torch.zeros(K, dtype=torch.float32, device=dev))

    return Case(
        f"qt_awq_weight_mean_accumulate R={R} K={K} gs={gs} {str(dtype)[6:]}", branch, make,
        lambda lib, t: lib.qt_awq_weight_mean_workspace_bytes(R, K),
        lambda lib, t, ws, nb: lib.qt_awq_weight_mean_accumulate(t["W"].data_ptr(), CODES[dtype], R, K, K, gs,
                                                                 t["s"].data_ptr(), ws, nb, _stream()),
        lambda ops, t: ops.awq_weight_mean_accumulate(t["W"], gs, t["s"]), ["s"])


def _loss_inputs(R, K, n_grid, seed):
    r = _rng(seed)
    W = (r.standard_normal((R, K)) * 0.05).astype(np.float32)
    X = r.standard_normal((2 * K, K)).astype(np.float32)
    G = (X.T @ X).astype(np.float32)
    G = np.tril(G) + np.tril(G, -1).T
    s = (0.5 + r.random((n_grid, K))).astype(np.float32)
    return W, G, s


def _awq_loss(R, K, gs, exact, branch):
    hW, hG, hs = _loss_inputs(R, K, 1, R + K + exact)

    def make(dev):
        return dict(W=_dev(hW, dev, torch.bfloat16), G=_dev(hG, dev), s=_dev(hs[0], dev),
                    out=torch.full((1,), -1.0, dtype=torch.float32, device=dev))

    return Case(
        f"qt_awq_loss R={R} K={K} gs={gs} exact={exact}", branch, make,
        lambda lib, t: lib.qt_awq_loss_workspace_bytes(R, K),
        lambda lib, t, ws, nb: lib.qt_awq_loss(t["W"].data_ptr(), QT_BF16, R, K, K, t["s"].data_ptr(), gs, 1, 4,
                                               t["G"].data_ptr(), 2 * K, exact, 1.0, 0, t["out"].data_ptr(), ws, nb, _stream()),
        lambda ops, t: ops.awq_loss(t["W"], t["s"], gs, True, 4, t["G"], 2 * K, t["out"], exact=bool(exact)), ["out"])


def _awq_losses(R, K, n_grid, branch):
    hW, hG, hs = _loss_inputs(R, K, n_grid, R + K + n_grid)

    def make(dev):
        return dict(W=_dev(hW, dev, torch.bfloat16), G=_dev(hG, dev), s=_dev(hs, dev),
                    out=torch.full((n_grid,), -1.0, dtype=torch.float32, device=dev))

    return Case(
        f"qt_awq_losses R={R} K={K} n_grid={n_grid}", branch, make,
        lambda lib, t: lib.qt_awq_losses_workspace_bytes(R, K, n_grid),
        lambda lib, t, ws, nb: lib.qt_awq_losses(t["W"].data_ptr(), QT_BF16, R, K, K, t["s"].data_ptr(), n_grid, 128, 1, 4,
                                                 t["G"].data_ptr(), 2 * K, 1.0, 0, t["out"].data_ptr(), ws, nb, _stream()),
        lambda ops, t: ops.awq_losses(t["W"], t["s"], 128, True, 4, t["G"], 2 * K, t["out"]), ["out"])


# -------------------------------------------------------------------------------------------------- a13: SmoothQuant
def _col_absmax(R, K, dtype, branch):
    host = _rng(R + 2 * K).standard_normal((R, K)).astype(np.float32)

    def make(dev):
        return dict(W=_dev(host, dev, dtype), m=torch.zeros(K, dtype=torch.float32, device=dev))

    return Case(
        f"qt_col_absmax_accumulate R={R} K={K} {str(dtype)[6:]}", branch, make,
        lambda lib, t: lib.qt_col_absmax_workspace_bytes(R, K),
        lambda lib, t, ws, nb: lib.qt_col_absmax_accumulate(t["W"].data_ptr(), CODES[dtype], R, K, K, t["m"].data_ptr(), ws,
                                                            nb, _stream()),
        lambda ops, t: ops.col_absmax_accumulate(t["W"], t["m"]), ["m"])


# ------------------------------------------------------------------------------------------------ the GEMM test faces
def _sgemm(M, N, k, mode, branch):
    r = _rng(M + N + k)
    ha, hb, hc = (r.standard_normal(s).astype(np.float32) for s in ((k, M), (k, N), (M, N)))

    def make(dev):
        return dict(A=_dev(ha, dev), B=_dev(hb, dev), Cin=_dev(hc, dev), out=torch.zeros((M, N), dtype=torch.float32, device=dev))

    return Case(
        f"qt_sgemm_tn_f32 M={M} N={N} k={k} mode={mode} split-k", branch, make,
        lambda lib, t: lib.qt_sgemm_tn_f32_workspace_bytes(M, N),
        lambda lib, t, ws, nb: lib.qt_sgemm_tn_f32(t["A"].data_ptr(), M, t["B"].data_ptr(), N,
                                                   t["Cin"].data_ptr() if mode == 0 else None, N if mode == 0 else 0,
                                                   t["out"].data_ptr(), N, M, N, k, 0, mode, 1, ws, nb, _stream()),
        lambda ops, t: ops.sgemm_tn(t["A"], t["B"], t["Cin"] if mode == 0 else None, mode, allow_split_k=True, out=t["out"]),
        ["out"])


def _gemm3(M, N, k, kind, branch):
    r = _rng(M + N + k + kind)
    ha, hb, hc = (r.standard_normal(s).astype(np.float32) for s in ((k, M), (k, N), (M, N)))

    def make(dev):
        return dict(A=_dev(ha, dev), B=_dev(hb, dev), C=_dev(hc, dev))

    return Case(
        f"qt_gemm3_tn_f32 M={M} N={N} k={k} kind={kind}", branch, make,
        lambda lib, t: lib.qt_gemm3_tn_f32_workspace_bytes(M, N, k),
        lambda lib, t, ws, nb: lib.qt_gemm3_tn_f32(t["A"].data_ptr(), M, t["B"].data_ptr(), N, t["C"].data_ptr(), N, M, N, k,
                                                   kind, ws, nb, _stream()),
        lambda ops, t: ops.gemm3_tn(t["A"], t["B"], t["C"], kind), ["C"])


# (builder, arguments): built lazily so that collecting the file costs nothing
CASES = [
    # xtx_plan (xtx.hip): n_tt = ceil(n / 64) token tiles, 256 x 256 output tiles, leftover tiles cut into s2 slabs
    (_xtx, (256, 256, torch.bfloat16, 0, "xtx_plan: no token tail, n_tt = 4 < 8 so the leftover tile is not split (s2 = 1)")),
    (_xtx, (1024, 256, torch.float16, 0, "xtx_plan: no token tail, 1 leftover tile split into s2 = 4 slabs (n_tt = 16)")),
    (_xtx, (200, 520, torch.bfloat16, 0, "xtx_plan: ragged token tail (200 % 64) staged in the workspace, s2 = 1, ragged K")),
    (_xtx, (1000, 520, torch.bfloat16, 0, "xtx_plan: ragged token tail AND 6 leftover tiles in s2 = 4 slabs each")),
    (_xtx, (1000, 520, torch.bfloat16, 64, "xtx_plan: ldx > K with a tail: the two-launch form (full tiles at ldx, staged tail at K)")),
    (_xtx, (40, 256, torch.float16, 8, "xtx_plan: ldx > K, fewer than 64 tokens: the staged tail alone")),
    # qt_xtx_accumulate_f32 (gemm3_tn.hip): three plane copies of a chunk of <= 8192 tokens + two item-table slots
    (_xtx_f32, (300, 264, "xtx_f32: one ragged chunk, plane pitch 512 != K (planes zeroed first)")),
    (_xtx_f32, (8192 + 100, 256, "xtx_f32: a full 8192-token chunk, then a ragged one (both table slots), pitch == K")),
    (_xtx_dot, (256, 520, "frobenius plan: 6 whole tiles, one fp64 partial each (s2 = 1)")),
    (_xtx_dot, (1024, 256, "frobenius plan: one tile cut into s2 = 4 token chunks, one partial per chunk")),
    # stats_plan (stats.hip): min(2048 / strips, ceil(n / 16)) token chunks of 3 K floats
    (_act_stats, (10, 264, "stats_plan: fewer than 16 tokens, one chunk")),
    (_act_stats, (1000, 2056, "stats_plan: two 2048-channel strips, 63 chunks of 16 tokens")),
    # prepare_two_pass (hessian.hip): a symmetric copy of G from K = 2048
    (_prepare, (2040, "prepare: one pass below the threshold (512 bytes of statistics only)")),
    (_prepare, (2048, "prepare: two passes at the threshold K = 2048 (K * K * 4 bytes for the symmetric copy)")),
    (_prepare, (2048, "prepare: QT_PREPARE_TWO_PASS=0 keeps the one-pass size at K = 2048", {"QT_PREPARE_TWO_PASS": "0"})),
    # CholLayout (chol_layout.h, cholesky.hip)
    (_chol, (1000, F32_CHAIN, "chain: f32 products only (no plane copies), ragged K = 1000")),
    (_chol, (1000, BF16X3_CHAIN, "chain: bf16x3 block-row products forced at small K (plane copies, slabs, item tables), K = 1000")),
    (_chol, (384, F32_CHAIN, "chain: f32, K of three 128-blocks, two outer blocks")),
    (_chol_batched, (512, 3, F32_CHAIN, "batched chain: three problems' shares, f32 products")),
    (_chol_batched, (520, 3, BF16X3_CHAIN, "batched chain: three shares + ONE copy of the item tables behind them, ragged K")),
    # qt_gptq_sweep_workspace_bytes (sweep.hip): ErrT for 8 blocks; + the far-update plan under QT_SWEEP_FAR
    (_sweep, (300, 1024, None, "sweep: ErrT only (the default f32 far update), two batches of blocks")),
    (_sweep, (300, 1024, {"QT_SWEEP_FAR": "bf16x3"}, "sweep: far-update plan (U planes, error planes, item table)")),
    (_sweep_grouped, (300, 640, [128, 300], "grouped sweep: two row groups, ErrT spans the stacked rows")),
    # qt_awq_weight_mean_workspace_bytes (awq.hip): partial sums + the (row, group) maxima of the long-group path
    (_wmean, (64, 512, 32, torch.bfloat16, "weight mean: group 32 (short groups: no maxima table; 16 groups per row)")),
    (_wmean, (300, 1024, 32, torch.float16, "weight mean: group 32, five row chunks")),
    (_wmean, (300, 200, 40, torch.float32, "weight mean: group 40 at K = 200 (5 groups against ceil(200 / 64) = 4)")),
    (_wmean, (100, 1024, 128, torch.bfloat16, "weight mean: group 128, register path (no table)")),
    (_wmean, (100, 1024, 512, torch.bfloat16, "weight mean: group 512, the widest register path")),
    (_wmean, (100, 2048, 1024, torch.bfloat16, "weight mean: group 1024, long-group path with a [R, 2] maxima table")),
    (_wmean, (100, 1152, -1, torch.bfloat16, "weight mean: channel-wise (group = K = 1152), long-group path, [R, 1] table")),
    (_wmean, (130, 576, 72, torch.float32, "weight mean: group 72, long-group path with 8 groups per row against ceil(576 / 64) = 9")),
    (_wmean, (65, 320, 64, torch.float16, "weight mean: group 64 register path, one row in the second chunk")),
    # qt_awq_loss_workspace_bytes: D + C + row partials + the Gram kernel's share
    (_awq_loss, (128, 512, 128, 0, "loss: R % 64 == 0, bf16 D and the fused Frobenius epilogue in the Gram share")),
    (_awq_loss, (100, 512, 128, 0, "loss: R % 64 != 0, D^T D materialised in C through qt_xtx_accumulate (staged tail)")),
    (_awq_loss, (100, 264, -1, 1, "loss: exact, fp32 D (the full R * K * 4) and C from the f32 GEMM")),
    (_awq_loss, (128, 512, 64, 1, "loss: exact at R % 64 == 0")),
    (_awq_losses, (128, 512, 7, "losses: batched form (R % 64 == 0, bf16, g128): n_grid D matrices + one Gram launch")),
    (_awq_losses, (100, 512, 7, "losses: per-point fallback (R % 64 != 0) inside the batched size")),
    (_col_absmax, (300, 264, torch.bfloat16, "col absmax: three 128-row chunks")),
    (_col_absmax, (1, 8, torch.float32, "col absmax: one row, one chunk")),
    (_sgemm, (256, 256, 2048, 1, "sgemm: 4 tiles, k = 2048 split into 16 slabs of M * N floats")),
    (_sgemm, (200, 136, 1000, 0, "sgemm: ragged M / N / k, split-k with Cin - acc in the reduction")),
    (_gemm3, (260, 516, 512, 0, "gemm3 test face kind 0: whole tiles, planes + item table (slab area unused)")),
    (_gemm3, (260, 516, 512, 1, "gemm3 test face kind 1: every tile cut along k into slabs")),
    # qt_gptq_sweep_workspace_bytes again (appended: a case's id carries its index), on whole 128-tiles, where the sweep
    # takes the fused form: two error buffers of one batch each, the second at ErrT + sweep_fused_err_bytes
    # (FUSED_SWEEPS below holds each of these to the fused form's launch count)
    (_sweep, (256, 1152, None, "fused sweep: two buffers of the default 4 blocks inside the classic 8-block ErrT")),
    (_sweep, (256, 2304, {"QT_SWEEP_BATCH": "8"},
              "fused sweep: 8-block batches, the second buffer lies beyond the classic ErrT (the size doubles)")),
    (_sweep_grouped, (512, 768, [128, 384, 512], "fused grouped sweep: three row groups, 2-block batches, a far_rest with row groups",
                      {"QT_SWEEP_BATCH": "2"})),
]
FUSED_SWEEPS = CASES[-3:]


def _id(entry):
    builder, args = entry
    return builder.__name__.lstrip("_") + "-" + "-".join(
        str(a).replace("torch.", "") for a in args if isinstance(a, (int, torch.dtype)))


@pytest.mark.parametrize("offset", [0, 16], ids=["aligned", "off16"])
@pytest.mark.parametrize("entry", CASES, ids=[f"{i:02d}-{_id(e)}" for i, e in enumerate(CASES)])
def test_entry_point_stays_inside_the_workspace_it_asks_for(entry, offset, dev, ops, monkeypatch):
    """See the module docstring; the branch of the size computation a case exercises is its last string argument (it is
    printed with a failure)."""
    builder, args = entry
    _run(builder(*args), dev, ops, monkeypatch, offset)


@pytest.mark.parametrize("entry", FUSED_SWEEPS, ids=[_id(e) for e in FUSED_SWEEPS])
def test_fused_sweep_cases_take_the_fused_form(entry, dev, ops, monkeypatch):
    """The fused cases above are fused: through ``ops`` under their environment each makes ``ceil(K / (128 batch))``
    block-kernel launches, not the chain's ``K / 128``."""
    from tests.test_gpu_sweep_fused import chain_launches, default_batch, fused_launches, sweep_launches

    builder, args = entry
    case = builder(*args)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    K = args[1]
    batch = int(case.env.get("QT_SWEEP_BATCH", default_batch(K)))
    t = case.make(dev)
    _, launches = sweep_launches(lambda: case.via_ops(ops, t))
    assert launches == fused_launches(K, batch) != chain_launches(K), launches


def test_fused_sweep_doubles_the_workspace_only_for_8_block_batches(monkeypatch):
    """R = 256, K = 2304: with 8-block batches the fused form asks for more than the chain of launches
    (``QT_SWEEP_FUSED=0``), with 4-block batches for exactly as much."""
    lib = _lib.load()
    need = {}
    for batch in ("4", "8"):
        monkeypatch.setenv("QT_SWEEP_BATCH", batch)
        monkeypatch.delenv("QT_SWEEP_FUSED", raising=False)
        need[batch, "default"] = int(lib.qt_gptq_sweep_workspace_bytes(256, 2304, 128))
        monkeypatch.setenv("QT_SWEEP_FUSED", "0")
        need[batch, "chain"] = int(lib.qt_gptq_sweep_workspace_bytes(256, 2304, 128))
    assert need["4", "default"] == need["4", "chain"] == need["8", "chain"] > 0
    assert need["8", "default"] > need["8", "chain"]


def test_every_size_function_has_a_case():
    """The fourteen ``*_workspace_bytes`` of the C ABI, fifteen consumers: none may be added without a case here."""
    sized = sorted(n for n in _lib.SIGNATURES if n.endswith("_workspace_bytes"))
    assert len(sized) == 14
    import inspect

    src = inspect.getsource(inspect.getmodule(test_every_size_function_has_a_case))
    for name in sized:
        assert f"lib.{name}(" in src, name
    for consumer in ("qt_xtx_accumulate(", "qt_xtx_accumulate_f32(", "qt_act_stats_accumulate(", "qt_hessian_prepare(",
                     "qt_cholesky_inverse_upper(", "qt_cholesky_inverse_upper_batched(", "qt_gptq_sweep(",
                     "qt_gptq_sweep_grouped(", "qt_awq_weight_mean_accumulate(", "qt_awq_loss(", "qt_awq_losses(",
                     "qt_col_absmax_accumulate(", "qt_sgemm_tn_f32(", "qt_xtx_dot(", "qt_gemm3_tn_f32("):
        assert f"lib.{consumer}" in src, consumer
