"""Generation controls: ``no_repeat_ngram_size``, ``repetition_penalty``, ``min_length`` and ``suppress_tokens`` with the semantics of
``transformers.generate`` (generation/logits_process.py: RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor,
MinLengthLogitsProcessor, SuppressTokensLogitsProcessor), plus ``allowed_tokens``, the complement form of a suppression.

``process_reference`` is the readable torch statement of the four rules; tests pin it against transformers' own processors on the CPU and
the device kernel (csrc/logits_process.hip: kzv_logits_process) against it bit for bit.  HF builds its processor list in the order
repetition penalty, n-gram ban, minimum length, suppression (GenerationMixin._get_logits_processor); the last three only write ``-inf``
and the penalty maps ``-inf`` to ``-inf``, so the order is immaterial for the result.

Where the controls act (generation/utils.py, ``_sample`` and ``_beam_search``): greedy decoding processes the raw logits, and arg-max /
log-sum-exp are then taken of the processed row; beam search processes ``log_softmax(logits)`` before the beam score is added and does
not normalise again.  A row's history is its ``input_ids``: BOS included, every token chosen so far.
"""
from __future__ import annotations

MAX_NGRAM = 8
MAX_VOCAB = 64 * 256          # the device kernel keeps two token bitmasks in LDS


class GenerationControls:
    """The four controls of one decode.  ``suppress_tokens``: ids that may never be chosen; ``allowed_tokens``: the complement form (every
    id NOT listed is suppressed; EOS is always kept); the two are mutually exclusive.  ``eos_id`` (optional here, required by ``mask``
    when a list is set): a list that suppresses EOS is refused, no line could end.  Every default is "off"."""

    def __init__(self, no_repeat_ngram_size: int = 0, repetition_penalty: float = 1.0, min_length: int = 0, suppress_tokens=None,
                 allowed_tokens=None, eos_id: int | None = None):
        g, p, ml = int(no_repeat_ngram_size or 0), float(repetition_penalty), int(min_length or 0)
        if not 0 <= g <= MAX_NGRAM:
            raise ValueError(f"no_repeat_ngram_size must be in 0..{MAX_NGRAM} (got {g})")
        if not p > 0.0:
            raise ValueError(f"repetition_penalty must be positive (got {p})")
        if ml < 0:
            raise ValueError("min_length must not be negative")
        if suppress_tokens is not None and allowed_tokens is not None:
            raise ValueError("suppress_tokens and allowed_tokens are mutually exclusive")
        self.no_repeat_ngram_size, self.repetition_penalty, self.min_length = g, p, ml
        self.suppress_tokens = None if suppress_tokens is None else sorted({int(v) for v in suppress_tokens})
        self.allowed_tokens = None if allowed_tokens is None else sorted({int(v) for v in allowed_tokens})
        for lst in (self.suppress_tokens, self.allowed_tokens):
            if lst and lst[0] < 0:
                raise ValueError("token ids must not be negative")
        if eos_id is not None and self.suppress_tokens and int(eos_id) in self.suppress_tokens:
            raise ValueError(f"suppress_tokens holds EOS ({int(eos_id)}): no line could end")

    @property
    def neutral(self) -> bool:
        """True when nothing would change a decode: the engine then launches nothing for the controls."""
        return (self.no_repeat_ngram_size == 0 and self.repetition_penalty == 1.0 and self.min_length == 0
                and not self.suppress_tokens and self.allowed_tokens is None)

    def suppressed(self, vocab: int, eos_id: int | None = None) -> list[int]:
        """The suppressed ids below ``vocab``, ascending.  ValueError for a listed id outside the vocabulary or a list that holds EOS."""
        vocab = int(vocab)
        lst = self.suppress_tokens if self.allowed_tokens is None else self.allowed_tokens
        if lst and lst[-1] >= vocab:
            raise ValueError(f"token id {lst[-1]} outside the vocabulary of {vocab}")
        if self.allowed_tokens is not None:
            if eos_id is None:
                raise ValueError("allowed_tokens needs eos_id: EOS is always kept")
            keep = set(self.allowed_tokens) | {int(eos_id)}
            return [v for v in range(vocab) if v not in keep]
        out = list(self.suppress_tokens or [])
        if eos_id is not None and int(eos_id) in out:
            raise ValueError(f"suppress_tokens holds EOS ({int(eos_id)}): no line could end")
        return out

    def check(self, vocab: int, eos_id: int, num_beams: int = 1) -> None:
        """ValueError for what a decode over ``vocab`` tokens cannot serve: a vocabulary beyond the kernel's bound, listed ids outside the
        vocabulary, a suppressed EOS, and for beam search a mask that leaves fewer than 2 tokens (a step ranks 2 * num_beams
        continuations of num_beams rows: with one token left they do not exist, and HF's own top-k then returns -inf entries)."""
        if int(vocab) > MAX_VOCAB:
            raise ValueError(f"generation controls serve vocabularies up to {MAX_VOCAB} tokens")
        left = int(vocab) - len(self.suppressed(vocab, eos_id))
        if int(num_beams) > 1 and left < 2:
            raise ValueError(f"the mask leaves {left} token(s): beam search needs at least 2 to rank 2 * num_beams continuations")

    def mask(self, vocab: int, eos_id: int | None = None):
        """The suppression as bit words for the device: int32 tensor of (vocab + 31) // 32 words (the bit pattern of uint32), bit v % 32
        of word v // 32 set for every suppressed id v; None when nothing is suppressed."""
        import torch
        ids = self.suppressed(vocab, eos_id)
        if not ids:
            return None
        words = [0] * ((int(vocab) + 31) // 32)
        for v in ids:
            words[v >> 5] |= 1 << (v & 31)
        return torch.tensor([w - (1 << 32) if w >= (1 << 31) else w for w in words], dtype=torch.int32)

    def hook(self, eos_id: int):
        """``process(scores [R, V], ids [R, >= n], n) -> scores``: the lockstep statements' hook (kzv/beam.py); history ids[:, :n]."""
        return lambda scores, ids, n: process_reference(scores, ids[:, :n], self, eos_id)

    def rows_hook(self, eos_id: int):
        """``process(scores [R, V], hist [R, L], lens [R], live [R]) -> scores``: the slot statements' hook (kzv/stream.py); row r has the
        history hist[r][:lens[r]], rows that are not live come back as they are."""
        return lambda scores, hist, lens, live=None: process_rows_reference(scores, hist, lens, self, eos_id, live)

    def __repr__(self):
        return (f"GenerationControls(no_repeat_ngram_size={self.no_repeat_ngram_size}, repetition_penalty={self.repetition_penalty}, "
                f"min_length={self.min_length}, suppress_tokens={self.suppress_tokens}, allowed_tokens={self.allowed_tokens})")


def from_kwargs(eos_id: int, no_repeat_ngram_size=0, repetition_penalty=1.0, min_length=0, suppress_tokens=None, allowed_tokens=None):
    """The controls of a ``generate`` call from its keywords: validated; None when every one is off."""
    c = GenerationControls(no_repeat_ngram_size, repetition_penalty, min_length, suppress_tokens, allowed_tokens, eos_id=eos_id)
    return None if c.neutral else c


def banned_ngram_tokens(history, g: int) -> list[int]:
    """The tokens the n-gram rule bans after ``history`` (a list of ints, BOS included): plain Python, the rule as process_reference's docstring states it."""
    n = len(history)
    if g <= 0 or n + 1 < g:
        return []
    tail = list(history[n - g + 1:n])
    return sorted({history[i + g - 1] for i in range(0, n - g + 1) if list(history[i:i + g - 1]) == tail})


def process_reference(scores, input_ids, controls: GenerationControls, eos_id: int):
    """The four rules on ``scores`` [R, V] (logits for greedy decoding, log-probabilities for beam search) given the histories
    ``input_ids`` [R, n]; returns a new tensor.
      repetition_penalty p: every distinct token v of the history once, x[v] = x[v] * p if x[v] < 0 else x[v] / p
      no_repeat_ngram_size g: nothing while n + 1 < g; else x[h[i + g - 1]] = -inf for every i in 0 .. n - g with
                              h[i : i + g - 1] == h[n - g + 1 : n]   (g = 1: every token of the history)
      min_length L: x[eos] = -inf while n < L
      suppress_tokens / allowed_tokens: x[v] = -inf for every suppressed v"""
    import torch
    x = scores.clone()
    R, V = x.shape
    n = int(input_ids.shape[1])
    ids = input_ids.to(x.device).long()
    p = controls.repetition_penalty
    if p != 1.0 and n:
        s = torch.gather(x, 1, ids)
        s = torch.where(s < 0, s * p, s / p)
        x = x.scatter(1, ids, s)
    g = controls.no_repeat_ngram_size
    if g:
        rows = ids.tolist()
        for r in range(R):
            ban = banned_ngram_tokens(rows[r], g)
            if ban:
                x[r, ban] = float("-inf")
    if n < controls.min_length:
        x[:, int(eos_id)] = float("-inf")
    sup = controls.suppressed(V, eos_id)
    if sup:
        x[:, sup] = float("-inf")
    return x


def process_rows_reference(scores, hist, lens, controls: GenerationControls, eos_id: int, live=None):
    """``process_reference`` where every row has its own history length: row r has hist[r][:lens[r]]; rows with live[r] false come back
    untouched."""
    x = scores.clone()
    ln = [int(v) for v in lens.tolist()]
    lv = [True] * len(ln) if live is None else [bool(v) for v in live.tolist()]
    for r in range(x.shape[0]):
        if lv[r]:
            x[r:r + 1] = process_reference(scores[r:r + 1], hist[r:r + 1, :ln[r]], controls, eos_id)
    return x


def has_repeated_ngram(tokens, g: int) -> bool:
    """Whether the token list holds some g-gram twice (what ``no_repeat_ngram_size=g`` rules out)."""
    seen = set()
    for i in range(len(tokens) - g + 1):
        k = tuple(tokens[i:i + g])
        if k in seen:
            return True
        seen.add(k)
    return False
