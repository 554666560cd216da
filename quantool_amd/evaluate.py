"""Perplexity of a model or a saved checkpoint on token sequences.

The reference declares an evaluation step and enables it by default (``src/quantool/args/quantization_args.py:63-80``:
``enable_evaluation=True``, ``metrics=["perplexity"]``) but never runs one (``cli.py:413`` is commented out).  This is
that step for the checkpoints this backend writes: ``perplexity(path_or_model, input_ids)``.
"""
from __future__ import annotations

import math
from pathlib import Path
from typing import Iterable, List, Optional, Sequence, Union

import torch


def _sequences(input_ids) -> List[torch.Tensor]:
    if isinstance(input_ids, torch.Tensor):
        if input_ids.dim() == 1:
            return [input_ids]
        if input_ids.dim() != 2:
            raise ValueError(f"input_ids must be [B, T] or a list of 1-d tensors, got shape {tuple(input_ids.shape)}")
        return list(input_ids)
    out = []
    for s in input_ids:
        s = s["input_ids"] if isinstance(s, dict) else s
        s = torch.as_tensor(s)
        out.append(s.reshape(-1))
    return out


def _batches(seqs: Sequence[torch.Tensor], batch_size: int) -> Iterable[torch.Tensor]:
    """Consecutive sequences of equal length, up to ``batch_size`` per forward (no padding, so no attention mask)."""
    i = 0
    while i < len(seqs):
        j = i + 1
        while j < len(seqs) and j - i < batch_size and seqs[j].numel() == seqs[i].numel():
            j += 1
        yield torch.stack([s.long() for s in seqs[i:j]])
        i = j


def _logits(model, ids: torch.Tensor) -> torch.Tensor:
    out = model(input_ids=ids)
    if hasattr(out, "logits"):
        return out.logits
    if isinstance(out, (tuple, list)):
        return out[0]
    return out


def nll_sum(logits: torch.Tensor, targets: torch.Tensor, chunk_rows: int = 1024) -> float:
    """sum over rows of -log_softmax(logits[r])[targets[r]], log-softmax in fp32 over ``chunk_rows`` rows at a time
    (a 128 256-entry vocabulary never needs a whole [B, T, V] fp32 tensor); the sum is kept in fp64."""
    V = logits.shape[-1]
    lg = logits.reshape(-1, V)
    tg = targets.reshape(-1)
    tot = torch.zeros((), dtype=torch.float64, device=lg.device)
    for r0 in range(0, lg.shape[0], chunk_rows):
        lp = torch.log_softmax(lg[r0:r0 + chunk_rows].float(), dim=-1)
        tot -= lp.gather(1, tg[r0:r0 + chunk_rows].unsqueeze(1)).double().sum()
    return float(tot)


@torch.no_grad()
def perplexity(model, input_ids=None, *, batch_size: int = 8, device=None, chunk_rows: int = 1024,
               tokenizer=None, dataset=None, num_samples: int = 512, max_seq_length: int = 2048,
               text_column: str = "text", dtype: Optional[torch.dtype] = None) -> dict:
    """exp(sum NLL / predicted tokens) over the next-token predictions of every sequence.

    ``model``: an ``nn.Module`` (returns logits, or an object with ``.logits``) or a checkpoint directory, which goes
    through ``load_quantized``.  ``input_ids``: a [B, T] tensor or a list of 1-d tensors (sequences of equal length
    share a forward, up to ``batch_size``).  Text instead: ``dataset`` (rows, a ``datasets.Dataset`` or a local
    .json / .jsonl file) with a ``tokenizer``, through the calibration front-end (``build_batches``; nothing is
    fetched -- a dataset id is refused).  Returns ``{"perplexity", "nll", "tokens"}`` (``nll`` is the mean)."""
    if isinstance(model, (str, Path)):
        from .engine.qlinear import load_quantized

        model = load_quantized(model, device=device or "cuda", dtype=dtype)
    if input_ids is None:
        if dataset is None:
            raise ValueError("pass input_ids, or dataset= with tokenizer=")
        from .engine.sequential import build_batches

        input_ids = build_batches(dataset, tokenizer, num_samples, max_seq_length, False, 0, text_column)
    if device is None:
        p = next(iter(model.parameters()), None)
        device = p.device if p is not None else torch.device("cpu")
    seqs = [s for s in _sequences(input_ids) if s.numel() >= 2]
    if not seqs:
        raise ValueError("no sequence has two or more tokens: nothing to predict")
    if batch_size < 1:
        raise ValueError("batch_size must be >= 1")
    total, n = 0.0, 0
    for ids in _batches(seqs, batch_size):
        ids = ids.to(device)
        logits = _logits(model, ids)
        total += nll_sum(logits[:, :-1], ids[:, 1:], chunk_rows)
        n += ids.shape[0] * (ids.shape[1] - 1)
        del logits
    nll = total / n
    return {"perplexity": math.exp(nll), "nll": nll, "tokens": n}
