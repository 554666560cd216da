"""Perplexity of a model or a saved checkpoint on token sequences, and its divergence from the model it came from.

The reference declares an evaluation step and enables it by default (``src/quantool/args/quantization_args.py:63-80``:
``enable_evaluation=True``, ``metrics=["perplexity"]``) but never runs one (``cli.py:413`` is commented out).  This is
that step for the checkpoints this backend writes: ``perplexity(path_or_model, input_ids)``, and
``divergence(reference, path_or_model, input_ids)`` for the per-token KL and top-1 agreement of the two models.
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


HEADS = ("logits", "fused")
IGNORE_INDEX = -100


def fused_head_parts(model):
    """(decoder, LM-head weight) of a model whose head ``ops.lm_head_nll`` can stand in for, or ``ValueError`` naming
    why it cannot: the decoder is ``model.base_model`` (its output is the final norm's), the head a bias-free
    ``nn.Linear`` with a 16-bit weight on a GPU, applied to the hidden states as they are (no logit soft-capping)."""
    why = "head=\"fused\" is not available for this model: "
    base = getattr(model, "base_model", None)
    if base is None or base is model:
        raise ValueError(why + "it has no base_model (the decoder with its final norm) apart from itself")
    head = model.get_output_embeddings() if hasattr(model, "get_output_embeddings") else None
    if head is None:
        raise ValueError(why + "it has no output embedding (get_output_embeddings())")
    if type(head) is not torch.nn.Linear:
        raise ValueError(why + f"its head is a {type(head).__name__}, not a plain nn.Linear")
    if head.bias is not None:
        raise ValueError(why + "its head has a bias")
    config = getattr(model, "config", None)
    for name in ("final_logit_softcapping", "logit_softcapping", "logits_soft_cap"):
        if getattr(config, name, None):
            raise ValueError(why + f"its config sets logit soft-capping ({name}={getattr(config, name)})")
    W = head.weight
    if W.dtype not in (torch.bfloat16, torch.float16):
        raise ValueError(why + f"its head weight is {W.dtype}, not bf16 or fp16")
    from .hip import ops

    if not ops.lm_head_k_supported(W.shape[1]):
        raise ValueError(why + f"its hidden size {W.shape[1]} is outside the kernel's range (a multiple of "
                         f"{ops.LM_HEAD_K_UNIT} in [{ops.LM_HEAD_MIN_K}, {ops.LM_HEAD_MAX_K}])")
    if not W.is_cuda:
        raise ValueError(why + f"its head weight is on {W.device}, not on a GPU")
    return base, W


def _fused_batch(base, W, ids: torch.Tensor):
    """(sum of NLL in fp64, positions whose argmax is the target) of one batch through ``ops.lm_head_nll``.  Every row
    of the [B, T, K] hidden states goes to the kernel as it lies in memory (a view, no copy of the [:, :-1] rows); the
    last position of each sequence, which predicts nothing, carries the ignore index and contributes 0."""
    from .hip import ops

    out = base(input_ids=ids)
    hs = out.last_hidden_state if hasattr(out, "last_hidden_state") else out[0]
    if not hs.is_cuda or hs.dtype != W.dtype:
        raise ValueError(f"head=\"fused\" is not available for this model: its hidden states are {hs.dtype} on "
                         f"{hs.device}, the head weight {W.dtype} on {W.device}")
    B, T, K = hs.shape
    if not hs.is_contiguous():                 # a decoder that returns a transposed or sliced tensor: [B, T, K] rows once
        hs = hs.contiguous()
    tg = torch.full((B, T), IGNORE_INDEX, dtype=torch.int64, device=hs.device)
    tg[:, :-1] = ids[:, 1:]
    tg = tg.view(-1)
    nll, _, argmax = ops.lm_head_nll(hs.view(B * T, K), W, tg)
    return float(nll.double().sum()), int(((argmax == tg) & (tg >= 0)).sum())


@torch.no_grad()
def perplexity(model, input_ids=None, *, batch_size: int = 8, device=None, chunk_rows: int = 1024,
               tokenizer=None, dataset=None, num_samples: int = 512, max_seq_length: int = 2048,
               text_column: str = "text", dtype: Optional[torch.dtype] = None, head: str = "logits") -> dict:
    """exp(sum NLL / predicted tokens) over the next-token predictions of every sequence.

    ``model``: an ``nn.Module`` (returns logits, or an object with ``.logits``) or a checkpoint directory, which goes
    through ``load_quantized``.  ``input_ids``: a [B, T] tensor or a list of 1-d tensors (sequences of equal length
    share a forward, up to ``batch_size``).  Text instead: ``dataset`` (rows, a ``datasets.Dataset`` or a local
    .json / .jsonl file) with a ``tokenizer``, through the calibration front-end (``build_batches``; nothing is
    fetched -- a dataset id is refused).  Returns ``{"perplexity", "nll", "tokens"}`` (``nll`` is the mean).

    ``head="fused"``: the decoder (``model.base_model``) runs alone and ``ops.lm_head_nll`` takes its hidden states and
    the LM-head weight: the [B, T, V] logits are never formed and every logit stays in fp32.  ``ValueError`` when the
    model is not eligible (``fused_head_parts``).  The result then also carries ``"head"`` and ``"top1"``, the share of
    positions whose argmax is the target."""
    if head not in HEADS:
        raise ValueError(f"head must be one of {HEADS}, got {head!r}")
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
    if head == "fused":
        base, W = fused_head_parts(model)
        total, hits, n = 0.0, 0, 0
        for ids in _batches(seqs, batch_size):
            ids = ids.to(W.device)
            t, h = _fused_batch(base, W, ids)
            total, hits = total + t, hits + h
            n += ids.shape[0] * (ids.shape[1] - 1)
        nll = total / n
        return {"perplexity": math.exp(nll), "nll": nll, "tokens": n, "head": head, "top1": hits / n}
    total, n = 0.0, 0
    for ids in _batches(seqs, batch_size):
        ids = ids.to(device)
        logits = _logits(model, ids)
        total += nll_sum(logits[:, :-1], ids[:, 1:], chunk_rows)
        n += ids.shape[0] * (ids.shape[1] - 1)
        del logits
    nll = total / n
    return {"perplexity": math.exp(nll), "nll": nll, "tokens": n}


def load_side(side, device, dtype):
    """A module as it is; a directory through ``load_quantized`` when its config.json carries a quantization_config,
    else as a dense checkpoint through transformers with ``local_files_only=True`` (nothing is fetched)."""
    if not isinstance(side, (str, Path)):
        return side
    import json

    path = Path(side)
    cfg_file = path / "config.json"
    if not cfg_file.is_file():
        raise ValueError(f"{path}: not a local checkpoint directory (no config.json); nothing is fetched")
    if json.loads(cfg_file.read_text()).get("quantization_config"):
        from .engine.qlinear import load_quantized

        return load_quantized(path, device=device or "cuda", dtype=dtype)
    from transformers import AutoModelForCausalLM

    model = AutoModelForCausalLM.from_pretrained(str(path), local_files_only=True, dtype=dtype or "auto")
    return model.to(device or "cuda").eval()


def _hidden(base, ids, W):
    out = base(input_ids=ids)
    hs = out.last_hidden_state if hasattr(out, "last_hidden_state") else out[0]
    if not hs.is_cuda or hs.dtype != W.dtype:
        raise ValueError(f"divergence is not available for this pair: hidden states are {hs.dtype} on {hs.device}, "
                         f"the head weight {W.dtype} on {W.device}")
    return hs if hs.is_contiguous() else hs.contiguous()


DIVERGENCE_KEYS = ("tokens", "kl", "kl_max", "top1_agree", "nll_ref", "nll", "perplexity_ref", "perplexity", "top1_ref",
                   "top1")


@torch.no_grad()
def divergence(reference, model, input_ids=None, *, batch_size: int = 8, device=None,
               dtype: Optional[torch.dtype] = None, tokenizer=None, dataset=None, num_samples: int = 512,
               max_seq_length: int = 2048, text_column: str = "text") -> dict:
    """How far ``model`` (the quantised side, Q) moved from ``reference`` (the original, P) on the same tokens: the
    per-token KL(P || Q) and the top-1 agreement, beside both perplexities.

    Either side is an ``nn.Module`` or a local directory: one whose config.json has a ``quantization_config`` goes
    through ``load_quantized``, a dense one through transformers' ``from_pretrained(local_files_only=True)``.
    ``input_ids`` / ``dataset`` + ``tokenizer`` as in ``perplexity``.  Both decoders run on the same ids, and
    ``ops.lm_head_kl`` takes the two [B * T, K] hidden states and the one head weight: no logits are formed, and
    a - b is taken between fp32 accumulators.  The last position of each sequence carries the ignore index and is
    left out of every statistic, so the positions are exactly ``perplexity``'s.

    Eligible: both sides pass ``fused_head_parts`` and their head weights have one shape and dtype and are
    ``torch.equal``; anything else is a ``ValueError`` naming the reason.  Returns ``{"tokens", "kl" (mean), "kl_max",
    "top1_agree", "nll_ref", "nll", "perplexity_ref", "perplexity", "top1_ref", "top1"}``; sums are kept in fp64."""
    reference = load_side(reference, device, dtype)
    model = load_side(model, device, dtype)
    try:
        base_p, W = fused_head_parts(reference)
    except ValueError as e:
        raise ValueError(f"divergence: the reference: {e}") from None
    try:
        base_q, Wq = fused_head_parts(model)
    except ValueError as e:
        raise ValueError(f"divergence: the model: {e}") from None
    why = "the two models' LM heads differ: one head weight is what the kernel takes"
    if W.shape != Wq.shape or W.dtype != Wq.dtype:
        raise ValueError(f"divergence: {why} (reference {tuple(W.shape)} {W.dtype}, model {tuple(Wq.shape)} {Wq.dtype})")
    if W.device != Wq.device:
        raise ValueError(f"divergence: the two models are on different devices ({W.device}, {Wq.device})")
    if W.data_ptr() != Wq.data_ptr() and not torch.equal(W, Wq):
        raise ValueError(f"divergence: {why} (the weights are not equal)")
    if input_ids is None:
        if dataset is None:
            raise ValueError("pass input_ids, or dataset= with tokenizer=")
        from .engine.sequential import build_batches

        input_ids = build_batches(dataset, tokenizer, num_samples, max_seq_length, False, 0, text_column)
    seqs = [s for s in _sequences(input_ids) if s.numel() >= 2]
    if not seqs:
        raise ValueError("no sequence has two or more tokens: nothing to predict")
    if batch_size < 1:
        raise ValueError("batch_size must be >= 1")
    from .hip import ops

    dev = W.device
    sums = torch.zeros(3, dtype=torch.float64, device=dev)         # kl, nll_ref, nll
    hits = torch.zeros(3, dtype=torch.int64, device=dev)           # agree, top1_ref, top1
    kl_max = torch.full((), -math.inf, dtype=torch.float32, device=dev)
    n = 0
    for ids in _batches(seqs, batch_size):
        ids = ids.to(dev)
        hp = _hidden(base_p, ids, W)
        hq = _hidden(base_q, ids, W)
        B, T, K = hp.shape
        if hq.shape != hp.shape:
            raise ValueError(f"divergence: hidden states of {tuple(hp.shape)} and {tuple(hq.shape)}")
        tg = torch.full((B, T), IGNORE_INDEX, dtype=torch.int64, device=dev)
        tg[:, :-1] = ids[:, 1:]
        tg = tg.view(-1)
        r = ops.lm_head_kl(hp.view(B * T, K), hq.view(B * T, K), W, tg)
        keep = tg >= 0
        sums += torch.stack([r.kl[keep].double().sum(), r.nll_p.double().sum(), r.nll_q.double().sum()])
        hits += torch.stack([((r.argmax_p == r.argmax_q) & keep).sum(), ((r.argmax_p == tg) & keep).sum(),
                             ((r.argmax_q == tg) & keep).sum()])
        kl_max = torch.maximum(kl_max, r.kl[keep].max())
        n += B * (T - 1)
    kl, nll_ref, nll = (float(x) / n for x in sums)
    agree, top1_ref, top1 = (int(x) / n for x in hits)
    return {"tokens": n, "kl": kl, "kl_max": float(kl_max), "top1_agree": agree, "nll_ref": nll_ref, "nll": nll,
            "perplexity_ref": math.exp(nll_ref), "perplexity": math.exp(nll), "top1_ref": top1_ref, "top1": top1}
