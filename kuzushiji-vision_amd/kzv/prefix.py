"""Forced prefixes: decoding continues a line from given tokens (HF ``generate(input_ids=[BOS] + prefix)``; per image, since HF
needs equal-length prompts and a batch here may be ragged).

A prefix is 0 or more token ids per image, without BOS.  It costs one decoder step per forced token -- there is no prefill pass: at a
step whose chosen index cur = t + 1 satisfies cur <= prefix_len[image], the row of scores is replaced by -inf everywhere and 0 at the
forced token (HF's ForceTokensLogitsProcessor), AFTER the generation controls and the language model: the prompt is subject to neither.
Selection is untouched: arg-max picks the forced token with log-probability exactly 0; a beam search carries the prefix in all beams
at scores 0, -1e9, -1e9, .. -- HF's state after a prompt.  ``max_length``, ``min_length`` and the histories the controls and the
language model read all include the prefix; beam scores sum the log-probabilities of the generated tokens only, and the length
normalisation and the early-stop heuristic use the generated length (kzv/beam.py: ``prompt``).

``force_reference`` is the torch statement that csrc/force_prefix.hip (kzv_force_prefix) is pinned against bit for bit; ``normalise``
checks a request; ``Prefixes`` holds the tables on a device.
"""
from __future__ import annotations


def normalise(prefix_ids, batch: int, *, vocab: int, pad_id: int, bos_id: int, eos_id: int, max_length: int, limits=None):
    """``prefix_ids``: None, a list of ``batch`` id sequences (ragged; None or () = empty), or a [batch, P] integer tensor / array padded
    on the right with ``pad_id``.  Returns ``(prefix int64 [batch, P], prefix_len int32 [batch])`` as CPU tensors (P >= 1, padded with
    pad_id), or None when every prefix is empty (off).  ValueError -- before anything runs -- for BOS, EOS, padding or an id outside the
    vocabulary inside a prefix, and for 1 + len(prefix) > max_length - 1 (or the image's ``limits`` entry - 1): no token could be
    generated."""
    import torch
    if prefix_ids is None:
        return None
    if torch.is_tensor(prefix_ids) or hasattr(prefix_ids, "shape"):
        t = torch.as_tensor(prefix_ids)
        if t.dim() != 2 or t.dtype.is_floating_point or t.dtype == torch.bool:
            raise ValueError("prefix_ids: a [batch, P] integer tensor padded with pad_id, or a list of id sequences")
        t = t.cpu().long()
        n_rows, P = t.shape
        # a row's length: up to its last id that is no padding (padding INSIDE a prefix is then refused below)
        lens = ((t != pad_id).long() * torch.arange(1, P + 1).view(1, P)).max(dim=1)[0] if P else torch.zeros(n_rows, dtype=torch.int64)
    else:
        rows = [[] if r is None else [int(x) for x in (r.tolist() if hasattr(r, "tolist") else r)] for r in prefix_ids]
        n_rows = len(rows)
        lens = torch.tensor([len(r) for r in rows], dtype=torch.int64)
        P = int(lens.max()) if n_rows else 0
        t = torch.full((n_rows, max(P, 1)), pad_id, dtype=torch.int64)
        if P:
            t[torch.arange(max(P, 1)).view(1, -1) < lens.view(-1, 1)] = torch.tensor([x for r in rows for x in r], dtype=torch.int64)
    if n_rows != batch:
        raise ValueError(f"prefix_ids holds {n_rows} prefixes for {batch} images")
    cap = torch.full((batch,), int(max_length), dtype=torch.int64)
    if limits is not None:
        lim = torch.as_tensor(limits).reshape(-1).long().cpu()
        if lim.numel() != batch:
            raise ValueError("limits must hold one entry per image")
        cap = torch.minimum(cap, lim)
    P = int(lens.max()) if batch else 0
    if P == 0:
        return None
    t = t[:, :P]
    inside = torch.arange(P).view(1, P) < lens.view(-1, 1)
    bad = inside & ((t < 0) | (t >= vocab) | (t == bos_id) | (t == eos_id) | (t == pad_id))
    if bool(bad.any()):
        i, j = (int(v) for v in bad.nonzero()[0])
        x = int(t[i, j])
        if not 0 <= x < vocab:
            raise ValueError(f"prefix_ids[{i}]: id {x} outside the vocabulary 0..{vocab - 1}")
        raise ValueError(f"prefix_ids[{i}]: a prefix holds no BOS / EOS / padding (id {x}); BOS is added by the decoder")
    long = (lens > 0) & (1 + lens > cap - 1)
    if bool(long.any()):
        i = int(long.nonzero()[0])
        raise ValueError(f"prefix_ids[{i}]: BOS + {int(lens[i])} forced tokens leave no room under max_length / limit {int(cap[i])} "
                         f"(1 + len(prefix) <= {int(cap[i])} - 1)")
    return torch.where(inside, t, torch.full_like(t, pad_id)).contiguous(), lens.to(torch.int32)


def force_reference(scores, n, prefix, prefix_len):
    """The torch statement of kzv_force_prefix.  ``scores`` [R, V] fp32; ``n``: the history length of every row (an int, or an integer
    tensor [R]) -- the token being chosen has index cur = n; ``prefix`` int64 [R, P] and ``prefix_len`` [R]: every ROW's prefix (callers
    expand per-image tables to rows).  Rows with 1 <= cur <= prefix_len become -inf with 0 at prefix[row][cur - 1]; the others are
    returned as they are.  Returns a new tensor."""
    import torch
    R, V = scores.shape
    dev = scores.device
    cur = (torch.full((R,), int(n), dtype=torch.int64, device=dev) if not torch.is_tensor(n) else n.to(dev).long().reshape(R))
    plen = prefix_len.to(dev).long().reshape(R).clamp(max=prefix.shape[1])
    forced = (cur >= 1) & (cur <= plen)
    tok = prefix.to(dev).long().gather(1, (cur - 1).clamp(min=0, max=prefix.shape[1] - 1).view(R, 1))      # [R, 1]
    forced = forced & (tok[:, 0] >= 0) & (tok[:, 0] < V)
    hit = torch.arange(V, device=dev).view(1, V) == tok
    row = torch.where(hit, torch.zeros_like(scores), torch.full_like(scores, float("-inf")))
    return torch.where(forced.view(R, 1), row, scores)


def forced_logprob_reference(scores, n, prefix, prefix_len, normalised: bool = False):
    """What kzv_force_prefix writes to ``forced_logprob``: per row (value fp32 [R], forced bool [R]) -- the model's own log-probability
    of the forced token, log_softmax(scores)[f], or scores[f] when the rows are normalised already."""
    import torch
    R, V = scores.shape
    dev = scores.device
    cur = (torch.full((R,), int(n), dtype=torch.int64, device=dev) if not torch.is_tensor(n) else n.to(dev).long().reshape(R))
    plen = prefix_len.to(dev).long().reshape(R).clamp(max=prefix.shape[1])
    forced = (cur >= 1) & (cur <= plen)
    tok = prefix.to(dev).long().gather(1, (cur - 1).clamp(min=0, max=prefix.shape[1] - 1).view(R, 1)).clamp(min=0, max=V - 1)
    x = scores if normalised else torch.log_softmax(scores.float(), dim=-1)
    return x.gather(1, tok)[:, 0], forced


class Prefixes:
    """The tables of one call on a device: ``prefix`` int64 [n, P], ``prefix_len`` int32 [n] (kzv_force_prefix's), the CPU originals,
    and, on request, ``forced_logprob`` fp32 [n, P + 1] (zeros; column cur = the model's log-probability of the token forced there)."""

    def __init__(self, prefix, prefix_len, device, want_logprobs: bool = False):
        import torch
        self.host = prefix
        self.host_len = prefix_len
        self.prefix = prefix.to(device).contiguous()
        self.prefix_len = prefix_len.to(device).contiguous()
        self.forced_logprob = torch.zeros(prefix.shape[0], prefix.shape[1] + 1, dtype=torch.float32, device=device) if want_logprobs else None

    @property
    def n(self) -> int:
        return self.host.shape[0]

    @property
    def width(self) -> int:
        return self.host.shape[1]

    def rows(self, group: int):
        """(prefix, prefix_len) expanded to ``group`` rows per image: force_reference's operands for a beam search."""
        return self.prefix.repeat_interleave(group, dim=0), self.prefix_len.repeat_interleave(group, dim=0)

    def slice(self, a: int, b: int, device=None, want_logprobs: bool = False):
        """The prefixes of images a .. b - 1 as tables of their own (None when all of them are empty)."""
        ln = self.host_len[a:b]
        P = int(ln.max()) if ln.numel() else 0
        if P == 0:
            return None
        return Prefixes(self.host[a:b, :P].contiguous(), ln.contiguous(), self.prefix.device if device is None else device, want_logprobs)

    def select(self, index, want_logprobs: bool = False):
        """The prefixes of the images ``index`` (a CPU integer tensor), or None when all of them are empty."""
        ln = self.host_len[index]
        P = int(ln.max()) if ln.numel() else 0
        if P == 0:
            return None
        return Prefixes(self.host[index][:, :P].contiguous(), ln.contiguous(), self.prefix.device, want_logprobs)

    def keep(self):
        return [t for t in (self.prefix, self.prefix_len, self.forced_logprob) if t is not None]


def resolve(prefix_ids, batch: int, cfg, max_length: int, device, limits=None, want_logprobs: bool = False):
    """``generate``'s / ``generate_stream``'s ``prefix_ids`` as a ``Prefixes`` on ``device``, or None when off.  A ``Prefixes`` passes
    through (the fallbacks of generate_stream hand theirs on) after the same checks."""
    if isinstance(prefix_ids, Prefixes):
        prefix_ids = prefix_ids.host             # padded with pad_id, which no checked prefix holds: the lengths come out as they were
    got = normalise(prefix_ids, batch, vocab=cfg.vocab, pad_id=cfg.pad_id, bos_id=cfg.bos_id, eos_id=cfg.eos_id, max_length=max_length, limits=limits)
    if got is None:
        return None
    return Prefixes(got[0], got[1], device, want_logprobs)


def texts_to_ids(tokenizer, texts, n_special: int = 0):
    """``prefix_texts`` through the tokenizer, for one-character tokenizers only (kzv/metrics.py: is_one_char_tokenizer): a list of id
    lists without special tokens.  ValueError for any other tokenizer: a prefix of k characters must be k tokens."""
    from . import metrics as M
    if tokenizer is None:
        raise ValueError("prefix_texts needs a tokenizer (use prefix_ids)")
    if not M.is_one_char_tokenizer(tokenizer):
        raise ValueError("prefix_texts needs a one-character tokenizer (use prefix_ids)")
    out = []
    for s in texts:
        if not s:
            out.append([])
            continue
        ids = tokenizer.convert_tokens_to_ids(list(s))
        out.append([int(x) for x in ids])
    return out
