"""Where the decoder layers live while the sequential driver calibrates them.

Resident: ``model.to(dev)``, the whole model in HBM next to the calibration working set (every model that fits).
Streamed: the model stays in host memory and each decoder layer visits the device for its own work only -- onloaded
while the layer before it calibrates, written back into the caller's host tensors behind its propagate pass
(``LayerMover``).  ``should_stream`` decides from what the code can observe: where the layers are, their shapes, the
scheme, the calibration token count and the free device memory.  DESIGN.md section 10 documents the formula and the
measurements it is checked against.
"""
from __future__ import annotations

import logging
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, Optional, Sequence

import torch
import torch.nn as nn

from .model_shapes import LayerShape

logger = logging.getLogger(__name__)


def free_device_bytes(dev) -> int:
    """The free-bytes probe of the decision (tests and tools substitute it)."""
    return int(torch.cuda.mem_get_info(dev)[0])


def layer_shape(layers: Sequence[nn.Module], name: str = "model") -> LayerShape:
    """The largest decoder layer as a ``LayerShape`` with one group per Linear (shared inputs are not known before a
    forward, so each Linear is counted with a Gram sum and a chain of its own: an upper bound).  A fused sparse-MoE
    bank (3-d ``gate_up_proj [E, 2I, H]`` / ``down_proj [E, H, I]``) counts as its experts' two matrices each."""
    best: Optional[LayerShape] = None
    for layer in layers:
        groups = []
        for n, m in layer.named_modules():
            if isinstance(m, nn.Linear):
                groups.append((n, m.in_features, ((n, m.out_features),)))
                continue
            gu, dn = getattr(m, "gate_up_proj", None), getattr(m, "down_proj", None)
            if isinstance(gu, nn.Parameter) and isinstance(dn, nn.Parameter) and gu.dim() == 3 and dn.dim() == 3:
                for e in range(int(gu.shape[0])):
                    groups.append((f"{n}.{e}.gate_up", int(gu.shape[2]), ((f"{n}.{e}.gate_up", int(gu.shape[1])),)))
                    groups.append((f"{n}.{e}.down", int(dn.shape[2]), ((f"{n}.{e}.down", int(dn.shape[1])),)))
        shape = LayerShape(name, len(layers), tuple(groups))
        if best is None or shape.weights_per_layer > best.weights_per_layer:
            best = shape
    return best


#: Tokens of one calibration forward (``QT_CALIB_BATCH_TOKENS``'s default in the driver).
FORWARD_TOKENS = 32768


def _stage_bytes(K: int, dtype_bytes: int) -> int:
    """A HessianAccumulator's token buffer (``gptq_linear.HessianAccumulator``: 1 GiB worth of rows, 4096..65536)."""
    return max(4096, min(65536, (1 << 30) // (2 * K))) * K * dtype_bytes


def result_bytes(weights: int, qargs, dtype_bytes: int = 2, detail_bytes: Optional[int] = None) -> int:
    """Device bytes of the results of ``weights`` quantised weights: packed levels (``num_bits`` / 8 per weight), per
    group a scale in the model dtype and in fp32 (and a zero point in int8 and fp32 when asymmetric), and up to
    ``RESULT_DETAIL_BYTES`` of detail (one int8 level per weight)."""
    from .sequential import RESULT_DETAIL_BYTES

    detail = RESULT_DETAIL_BYTES if detail_bytes is None else detail_bytes
    out = weights * qargs.num_bits // 8
    gs = qargs.group_size if (qargs.strategy == "group" and qargs.group_size) else None
    if gs:
        out += weights // gs * (dtype_bytes + 4 + (0 if qargs.symmetric else 5))
    return out + min(detail, weights)


def calibration_bytes(shape: LayerShape, hidden: int, tokens: int, qargs, *, dtype_bytes: int = 2,
                      with_results: bool = True) -> int:
    """Device bytes the driver needs next to the weights, for one decoder layer of ``shape`` (per input group of
    in_features K and out_features R_1..R_n) and ``tokens`` calibration tokens:

      Gram sums           4 K^2 per group (fp32)
      chain workspaces   24 K^2 per group (the batched factorisation's A and U in fp32, the Cholesky workspace's
                          bf16 planes and slabs)
      token buffers       one HessianAccumulator buffer per group (1 GiB worth of rows, 4096..65536 tokens)
      working copies      7 bytes per weight of the layer (the sweep's fp32 copy, the int8 levels, the dequantised
                          weight in the model dtype)
      activation caches   2 x tokens x hidden in the model dtype (the layer's inputs and the next layer's)
      forward transients  min(tokens, FORWARD_TOKENS) x sum over groups of (K + sum R) in the model dtype (every
                          Linear's input and output of one calibration forward, batch 0's kept alive)
      results             (``with_results``: resident) ``result_bytes`` of every layer's weights
    """
    gram = sum(4 * K * K for _, K, _ in shape.groups)
    chains = sum(24 * K * K for _, K, _ in shape.groups)
    stage = sum(_stage_bytes(K, dtype_bytes) for _, K, _ in shape.groups)
    sweep = 7 * shape.weights_per_layer
    acts = 2 * tokens * hidden * dtype_bytes
    fwd = min(tokens, FORWARD_TOKENS) * dtype_bytes * sum(K + sum(R for _, R in lins) for _, K, lins in shape.groups)
    total = gram + chains + stage + sweep + acts + fwd
    if with_results:
        total += result_bytes(shape.total_weights, qargs, dtype_bytes)
    return total


def should_stream(shape: LayerShape, hidden: int, param_bytes: int, qargs, tokens: int, free_bytes: int, *,
                  on_host: bool, dtype_bytes: int = 2) -> bool:
    """Stream the decoder layers from the host iff they arrive there (``on_host``) and the model's parameter bytes
    plus the resident working set (``calibration_bytes``) exceed the free device memory."""
    if not on_host:
        return False
    return param_bytes + calibration_bytes(shape, hidden, tokens, qargs, dtype_bytes=dtype_bytes) > free_bytes


def _slots(module: nn.Module) -> List[list]:
    """Every distinct parameter / buffer of ``module``: ``[tensor, [(owner, name, is_param), ...]]``."""
    by_id: Dict[int, list] = {}
    for mod in module.modules():
        for name, p in mod._parameters.items():
            if p is not None:
                by_id.setdefault(id(p), [p, []])[1].append((mod, name, True))
        for name, b in mod._buffers.items():
            if b is not None:
                by_id.setdefault(id(b), [b, []])[1].append((mod, name, False))
    return list(by_id.values())


def _point(slot, t: torch.Tensor) -> None:
    """Make every owner of ``slot`` hold ``t``: a parameter keeps its ``Parameter`` object (``.data``), so weights tied
    to it (``lm_head.weight`` is often the embedding's) stay tied; a buffer is replaced in its owners' tables."""
    obj, owners = slot
    if isinstance(obj, nn.Parameter):
        obj.data = t
    else:
        for mod, name, _ in owners:
            mod._buffers[name] = t
        slot[0] = t


class outside_layers_on_device:
    """Context: the parameters and buffers held by no decoder layer (embeddings, rotary buffers, the final norm,
    ``lm_head``) on the device for the first-layer capture; on exit every owner holds its original host tensor
    again (nothing outside the layers is changed by calibration, so nothing is copied back)."""

    def __init__(self, model: nn.Module, layers: Sequence[nn.Module], dev):
        inside = {id(t) for layer in layers for t, _ in _slots(layer)}
        self.slots = [s for s in _slots(model) if id(s[0]) not in inside]
        self.dev = dev
        self.host: List[torch.Tensor] = []

    def __enter__(self):
        for s in self.slots:
            h = s[0].data if isinstance(s[0], nn.Parameter) else s[0]
            self.host.append(h)
            _point(s, h.to(self.dev, copy=True))
        return self

    def __exit__(self, *exc):
        for s, h in zip(self.slots, self.host):
            _point(s, h)
        return False


def _pieces(sizes: Sequence[int], chunk: int):
    """Lay byte ranges of ``sizes`` one after another (256-byte aligned) over chunks of ``chunk`` bytes:
    ``(tensor index, offset in the tensor, chunk index, offset in the chunk, bytes)``."""
    pos = 0
    for i, n in enumerate(sizes):
        off = 0
        while off < n:
            c, co = divmod(pos, chunk)
            k = min(n - off, chunk - co)
            yield i, off, c, co, k
            off += k
            pos += k
        pos = (pos + 255) // 256 * 256


def _flat(t: torch.Tensor) -> torch.Tensor:
    if not t.is_contiguous():
        raise ValueError(f"streamed placement copies contiguous tensors only (got strides {t.stride()} for "
                         f"shape {tuple(t.shape)})")
    return t.reshape(-1).view(torch.uint8)


class _Staging:
    """Pinned host staging in CHUNK-byte blocks, grown on demand and kept for the run.  torch's pinned host allocator
    rounds every request up to a power of two (``CachingHostAllocator``), so a 1.7 GB layer as one buffer would pin
    2 GiB; chunks of a power-of-two size waste at most the last chunk's tail."""

    def __init__(self, chunk: int):
        self.chunk, self.bufs = chunk, []

    def ensure(self, nbytes: int) -> None:
        while len(self.bufs) * self.chunk < nbytes:
            self.bufs.append(torch.empty(self.chunk, dtype=torch.uint8, pin_memory=True))

    @property
    def nbytes(self) -> int:
        return len(self.bufs) * self.chunk


def _span(sizes: Sequence[int], chunk: int) -> int:
    end = 0
    for _i, _off, c, co, k in _pieces(sizes, chunk):
        end = c * chunk + co + k
    return end


class LayerMover:
    """Moves decoder layers between their host tensors and the device for the streamed driver (``_stream_layers``).

    ``stage(i)``     a worker thread copies layer i's host tensors into the onload staging (pinned)
    ``upload(i)``    device copies allocated on the H2D stream and filled from the staging, asynchronously
    ``attach(i)``    the current stream waits for the upload; layer i's parameters and buffers point at the copies
    ``writeback(i)`` behind the work queued so far (quantisation, propagate), the D2H stream copies layer i's tensors
                     and the new results' tensors into the write-back staging; the worker copies them on into the
                     caller's host tensors (parameters) or fresh host tensors (results) while the next layer runs
    ``release(i)``   every owner holds its host tensor again; the device copies are freed behind every stream that
                     read them (``record_stream``)

    The copy streams are the mover's own, not ``GroupStreams``'.  Host memory overhead: the two stagings, one layer for
    the onload and one layer plus its results for the write-back (Llama-3-70B-shaped: 4.75 GiB next to 1.59 GiB
    layers while the first layers keep their detail, ``RESULT_DETAIL_BYTES``)."""

    CHUNK = 256 << 20

    def __init__(self, layers: Sequence[nn.Module], dev, phases=None):
        self.layers, self.dev, self.ph = list(layers), torch.device(dev), phases
        self.h2d = torch.cuda.Stream(device=self.dev)
        self.d2h = torch.cuda.Stream(device=self.dev)
        self.main = torch.cuda.current_stream(self.dev)
        # one worker: its copies use torch's intra-op threads (OMP_NUM_THREADS), no pool of its own
        self.pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix="qt-layer-copy")
        self.on_stage, self.wb_stage = _Staging(self.CHUNK), _Staging(self.CHUNK)
        self.slots: Dict[int, List[list]] = {}
        self.host: Dict[int, List[torch.Tensor]] = {}
        self.devt: Dict[int, List[torch.Tensor]] = {}
        self.staged: Dict[int, object] = {}
        self.uploaded: Dict[int, torch.cuda.Event] = {}
        self.up_ev: Optional[torch.cuda.Event] = None      # the last upload's end: the onload staging is free after it
        self.wb_job = None
        self.copy_events: List[tuple] = []                  # (direction, start event, end event)
        self.stats = {"bytes_h2d": 0, "bytes_d2h": 0}

    # -- onload --
    def stage(self, i: int) -> None:
        slots = _slots(self.layers[i])
        host = [s[0].data if isinstance(s[0], nn.Parameter) else s[0] for s in slots]
        for h in host:
            if h.device.type != "cpu":
                raise ValueError(f"streamed placement: a tensor of decoder layer {i} is on {h.device}, not the host")
        self.slots[i], self.host[i] = slots, host
        sizes = [h.numel() * h.element_size() for h in host]
        self.on_stage.ensure(_span(sizes, self.CHUNK))
        flats = [_flat(h) for h in host]
        bufs, after = self.on_stage.bufs, self.up_ev

        def copy_in():
            if after is not None:
                after.synchronize()          # the previous upload still reads the staging
            for t, off, c, co, k in _pieces(sizes, self.CHUNK):
                bufs[c][co:co + k].copy_(flats[t][off:off + k])

        self.staged[i] = self.pool.submit(copy_in)

    def upload(self, i: int) -> None:
        self._timed("onload", self.staged.pop(i).result)
        host = self.host[i]
        sizes = [h.numel() * h.element_size() for h in host]
        bufs = self.on_stage.bufs
        with torch.cuda.stream(self.h2d):
            devt = [torch.empty_like(h, device=self.dev) for h in host]
            flats = [_flat(d) for d in devt]
            start = torch.cuda.Event(enable_timing=True)
            start.record(self.h2d)
            for t, off, c, co, k in _pieces(sizes, self.CHUNK):
                flats[t][off:off + k].copy_(bufs[c][co:co + k], non_blocking=True)
            end = torch.cuda.Event(enable_timing=True)
            end.record(self.h2d)
        self.copy_events.append(("h2d", start, end))
        self.stats["bytes_h2d"] += sum(sizes)
        self.devt[i], self.uploaded[i], self.up_ev = devt, end, end

    def attach(self, i: int) -> None:
        ev = self.uploaded.pop(i)
        self._timed("onload", lambda: self.main.wait_event(ev))
        for s, d in zip(self.slots[i], self.devt[i]):
            _point(s, d)

    # -- write-back --
    def writeback(self, i: int, results: Sequence[object] = ()) -> None:
        """Queue layer i's tensors and the tensor fields of ``results`` (replaced by host tensors at once, filled by the
        worker before ``finish`` returns) for the trip back."""
        import dataclasses

        src = list(self.devt[i])
        dst = list(self.host[i])
        for r in results:
            for f in dataclasses.fields(r):
                v = getattr(r, f.name)
                if isinstance(v, torch.Tensor) and v.device.type != "cpu":
                    h = torch.empty(v.shape, dtype=v.dtype)
                    src.append(v.contiguous())
                    dst.append(h)
                    setattr(r, f.name, h)
        sizes = [d.numel() * d.element_size() for d in dst]
        if self.wb_job is not None:       # the previous write-back still reads the staging
            self._timed("write-back", self.wb_job.result)
            self.wb_job = None
        self.wb_stage.ensure(_span(sizes, self.CHUNK))
        bufs = self.wb_stage.bufs
        queued = torch.cuda.Event()
        queued.record(self.main)
        self.d2h.wait_event(queued)
        with torch.cuda.stream(self.d2h):
            start = torch.cuda.Event(enable_timing=True)
            start.record(self.d2h)
            flats = [_flat(s) for s in src]
            for t, off, c, co, k in _pieces(sizes, self.CHUNK):
                bufs[c][co:co + k].copy_(flats[t][off:off + k], non_blocking=True)
            end = torch.cuda.Event(enable_timing=True)
            end.record(self.d2h)
        for s in src:
            s.record_stream(self.d2h)
        self.copy_events.append(("d2h", start, end))
        self.stats["bytes_d2h"] += sum(sizes)
        out = [_flat(d) for d in dst]

        def copy_out():
            end.synchronize()
            for t, off, c, co, k in _pieces(sizes, self.CHUNK):
                out[t][off:off + k].copy_(bufs[c][co:co + k])

        self.wb_job = self.pool.submit(copy_out)

    def release(self, i: int) -> None:
        for s, h in zip(self.slots.pop(i), self.host.pop(i)):
            _point(s, h)
        for d in self.devt.pop(i):
            d.record_stream(self.main)

    def finish(self) -> None:
        if self.wb_job is not None:
            self._timed("write-back", self.wb_job.result)
            self.wb_job = None
        self.d2h.synchronize()
        self.h2d.synchronize()
        self.pool.shutdown(wait=True)
        for d in ("h2d", "d2h"):
            self.stats[f"ms_{d}"] = sum(s.elapsed_time(e) for k, s, e in self.copy_events if k == d)
        self.stats["pinned_bytes"] = self.on_stage.nbytes + self.wb_stage.nbytes
        self.on_stage.bufs.clear()
        self.wb_stage.bufs.clear()

    def abort(self) -> None:
        """After a failure: wait for the copies in flight (they read or write tensors the caller still holds)."""
        for job in [self.wb_job] + list(self.staged.values()):
            if job is not None:
                try:
                    job.result()
                except Exception:  # noqa: BLE001
                    pass
        self.d2h.synchronize()
        self.h2d.synchronize()
        self.pool.shutdown(wait=True)

    def _timed(self, name: str, fn):
        if self.ph is None:
            return fn()
        self.ph.start()
        out = fn()
        self.ph.stop(name)
        return out
