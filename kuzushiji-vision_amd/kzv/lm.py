"""A character n-gram language model fused into decoding (shallow fusion): every step's scores become
``score(v) + lm_weight * log p_lm(v | the last order - 1 tokens)``.

The training labels are one character per token, so the model is fitted on label ids in seconds (``NGramLM.fit``), or imported from an
ARPA file (``NGramLM.from_arpa``: KenLM / SRILM).  ``NGramLM.row`` is the readable fp32 statement of the evaluation and
``fuse_reference`` that of the fusion; the device kernel (csrc/lm_fusion.hip: kzv_lm_fuse) is pinned against them bit for bit.

The model.  Counts: for every position i >= 1 of a sequence (BOS ... EOS, no padding) and every k in 1..order with i - k + 1 >= 0,
c_k(ctx = s[i - k + 1 : i], v = s[i]); BOS is only ever a context, nothing crosses a sequence boundary.  Probabilities, interpolated
absolute discounting on the raw counts, in float64:
  P_1(v)     = max(c(v) - D, 0) / T + (D * n1 / T) / vocab            T predicted tokens, n1 distinct predicted tokens
  P_k(v | c) = max(c(c, v) - D, 0) / c(c) + g(c) * P_{k-1}(v | c[1:]),  g(c) = D * types(c) / c(c);  an unseen c: P_{k-1}(v | c[1:])
Stored, fp32 rounded once from float64, natural logarithms: uni[v] = log P_1(v); for every seen context of length 1..order - 1
bo = log g(c) and its seen successors (v, lp = log P_k(v | c)).

The evaluation rule (``row``), for a history h[0 .. n), BOS included, all in fp32 and in this order:
  acc = 0
  for k = min(order - 1, n) down to 1:
      if the context h[n - k : n] is in the table:
          for each of its successors (v, lp) not yet claimed:  lm[v] = acc + lp; claim v
          acc = acc + bo(context)
  for every unclaimed v:  lm[v] = acc + uni[v]
A context that holds a token outside [0, vocab) counts as not found; a found context whose shorter suffix is absent (an ARPA file
after dropped entries) simply skips that suffix.

Where the fusion acts -- one rule everywhere, after the generation controls (kzv/controls.py):
  greedy   raw logits -> controls (if any) -> + lm_weight * lm -> arg-max and log-sum-exp of the result; the log-probabilities and
           ``top_k`` alternatives of ``generate_stream`` are those of the fused row;
  beams    log_softmax(logits) -> controls -> + lm_weight * lm -> + beam score, ranked without a second normalisation;
  the repetition penalty acts on the model's score alone, and the -inf of a ban survives the addition;
  ``align`` / ``recognize``: the per-character values stay the model's own (a teacher-forced pass); the LM steers the decode only.

The flat layout (``tables``; the ``.npz`` of ``save`` holds exactly these arrays plus ``order`` and ``vocab``; include/kzv.h:
kzv_ngram_lm): ``uni`` fp32 [vocab]; per context length k = 1..3 ``keys{k}`` int64 ascending (the k tokens as one number in base
16384, oldest token most significant), ``bo{k}`` fp32, ``off{k}`` int32 [contexts + 1] CSR offsets into the shared ``succ_tok`` int32 /
``succ_lp`` fp32, a context's successors ascending by token.
"""
from __future__ import annotations

import math

import numpy as np

MAX_ORDER = 4
MAX_VOCAB = 64 * 256          # the device kernel keeps a claim bit per token in LDS
BASE = MAX_VOCAB


def _key(ctx) -> int:
    k = 0
    for v in ctx:
        k = k * BASE + int(v)
    return k


class NGramLM:
    """Backoff n-gram model over token ids, 1 <= order <= 4, vocab <= 16384.  ``NGramLM(order, vocab)`` is the uniform model (no
    contexts); ``fit``, ``from_tables``, ``from_arpa`` and ``load`` build the others."""

    def __init__(self, order: int, vocab: int):
        order, vocab = int(order), int(vocab)
        if not 1 <= order <= MAX_ORDER:
            raise ValueError(f"order must be in 1..{MAX_ORDER} (got {order})")
        if not 1 <= vocab <= MAX_VOCAB:
            raise ValueError(f"vocab must be in 1..{MAX_VOCAB} (got {vocab})")
        self.order, self.vocab = order, vocab
        self.uni = np.full(vocab, np.float32(-math.log(vocab)), dtype=np.float32)
        self.keys = [np.zeros(0, dtype=np.int64) for _ in range(MAX_ORDER - 1)]
        self.bo = [np.zeros(0, dtype=np.float32) for _ in range(MAX_ORDER - 1)]
        self.off = [np.zeros(1, dtype=np.int32) for _ in range(MAX_ORDER - 1)]
        self.succ_tok = np.zeros(0, dtype=np.int32)
        self.succ_lp = np.zeros(0, dtype=np.float32)
        self._counts = None                      # fitted models keep their counts: prob64
        self._discount = None
        self._device = {}

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_tables(cls, order: int, vocab: int, uni, contexts: dict):
        """``uni``: [vocab] log-probabilities; ``contexts``: {tuple of 1..order - 1 tokens: (bo, {v: lp})}.  Values are rounded to fp32
        once.  Nothing is checked for consistency: a context may lack its suffix (``row`` states what then happens)."""
        lm = cls(order, vocab)
        uni = np.asarray(uni, dtype=np.float64)
        if uni.shape != (lm.vocab,):
            raise ValueError(f"uni must hold {lm.vocab} values")
        lm.uni = uni.astype(np.float32)
        per = [[] for _ in range(MAX_ORDER - 1)]
        for ctx, (bo, succ) in contexts.items():
            ctx = tuple(int(v) for v in ctx)
            if not 1 <= len(ctx) <= lm.order - 1:
                raise ValueError(f"context {ctx}: an order-{lm.order} model holds contexts of 1..{lm.order - 1} tokens")
            if any(not 0 <= v < lm.vocab for v in ctx) or any(not 0 <= int(v) < lm.vocab for v in succ):
                raise ValueError(f"context {ctx}: token outside the vocabulary of {lm.vocab}")
            per[len(ctx) - 1].append((_key(ctx), float(bo), sorted((int(v), float(lp)) for v, lp in succ.items())))
        toks, lps, base = [], [], 0
        for k in range(MAX_ORDER - 1):
            per[k].sort(key=lambda e: e[0])
            lm.keys[k] = np.array([e[0] for e in per[k]], dtype=np.int64)
            lm.bo[k] = np.array([e[1] for e in per[k]], dtype=np.float64).astype(np.float32)
            off = [base]
            for e in per[k]:
                toks += [v for v, _ in e[2]]
                lps += [lp for _, lp in e[2]]
                base += len(e[2])
                off.append(base)
            lm.off[k] = np.array(off, dtype=np.int32)
        lm.succ_tok = np.array(toks, dtype=np.int32)
        lm.succ_lp = np.array(lps, dtype=np.float64).astype(np.float32)
        return lm

    @classmethod
    def fit(cls, sequences, order: int, vocab: int, discount: float = 0.75):
        """Fit on ``sequences`` (lists of ids, each BOS ... EOS without padding) by the rules of the module docstring."""
        lm = cls(order, vocab)
        D = float(discount)
        if not 0.0 < D < 1.0:
            raise ValueError("discount must lie strictly between 0 and 1")
        counts = [dict() for _ in range(lm.order)]       # counts[k - 1][ctx][v], ctx of k - 1 tokens
        for s in sequences:
            s = [int(v) for v in s]
            if any(not 0 <= v < lm.vocab for v in s):
                raise ValueError(f"token outside the vocabulary of {lm.vocab}")
            for i in range(1, len(s)):
                for k in range(1, lm.order + 1):
                    if i - k + 1 < 0:
                        break
                    d = counts[k - 1].setdefault(tuple(s[i - k + 1:i]), {})
                    d[s[i]] = d.get(s[i], 0) + 1
        if not counts[0]:
            raise ValueError("fit: no predicted token (every sequence needs BOS and at least one more token)")
        lm._counts, lm._discount = counts, D
        contexts = {}
        for k in range(2, lm.order + 1):
            for ctx, succ in counts[k - 1].items():
                total = sum(succ.values())
                lower = lm._p64(ctx[1:])
                g = D * len(succ) / total
                contexts[ctx] = (math.log(g), {v: math.log(max(c - D, 0.0) / total + g * lower[v]) for v, c in succ.items()})
        out = cls.from_tables(lm.order, lm.vocab, np.log(lm._p64(())), contexts)
        out._counts, out._discount = counts, D
        return out

    def _p64(self, ctx) -> np.ndarray:
        """P_{len(ctx) + 1}(. | ctx) in float64 from the counts (fitted models only)."""
        counts, D, V = self._counts, self._discount, self.vocab
        ctx = tuple(ctx)
        if not ctx:
            uni = counts[0][()]
            T = sum(uni.values())
            p = np.full(V, (D * len(uni) / T) / V, dtype=np.float64)
            for v, c in uni.items():
                p[v] += max(c - D, 0.0) / T
            return p
        lower = self._p64(ctx[1:])
        succ = counts[len(ctx)].get(ctx) if all(0 <= v < V for v in ctx) else None
        if not succ:
            return lower
        total = sum(succ.values())
        p = (D * len(succ) / total) * lower
        for v, c in succ.items():
            p[v] += max(c - D, 0.0) / total
        return p

    def prob64(self, history) -> np.ndarray:
        """The float64 model itself after ``history`` (BOS included): P_order(. | the last order - 1 tokens).  Fitted models only."""
        if self._counts is None:
            raise ValueError("prob64 needs the counts of a fitted model")
        h = [int(v) for v in history]
        return self._p64(h[max(0, len(h) - (self.order - 1)):] if self.order > 1 else ())

    # ------------------------------------------------------------------ evaluation
    def n_contexts(self) -> list[int]:
        """Contexts held per length 1..order - 1."""
        return [int(self.keys[k].size) for k in range(self.order - 1)]

    def _find(self, ctx) -> int:
        k = len(ctx)
        if any(not 0 <= v < self.vocab for v in ctx):
            return -1
        keys = self.keys[k - 1]
        key = _key(ctx)
        j = int(np.searchsorted(keys, key))
        return j if j < keys.size and int(keys[j]) == key else -1

    def row(self, history) -> np.ndarray:
        """fp32 [vocab]: log p_lm(v | history) by the evaluation rule of the module docstring -- what the device computes."""
        h = [int(v) for v in history]
        n = len(h)
        out = np.empty(self.vocab, dtype=np.float32)
        claimed = np.zeros(self.vocab, dtype=bool)
        acc = np.float32(0.0)
        for k in range(min(self.order - 1, n), 0, -1):
            j = self._find(h[n - k:])
            if j < 0:
                continue
            a, b = int(self.off[k - 1][j]), int(self.off[k - 1][j + 1])
            tok, lp = self.succ_tok[a:b], self.succ_lp[a:b]
            new = ~claimed[tok]
            out[tok[new]] = (acc + lp[new]).astype(np.float32)
            claimed[tok[new]] = True
            acc = np.float32(acc + self.bo[k - 1][j])
        rest = ~claimed
        out[rest] = (acc + self.uni[rest]).astype(np.float32)
        return out

    def logprob(self, sequence) -> float:
        """Sum over the predicted positions i >= 1 of row(sequence[:i])[sequence[i]], accumulated in float64."""
        s = [int(v) for v in sequence]
        return float(sum(float(self.row(s[:i])[s[i]]) for i in range(1, len(s))))

    def perplexity(self, sequences) -> float:
        """exp(- sum of logprob / number of predicted tokens) over ``sequences``."""
        total, n = 0.0, 0
        for s in sequences:
            total += self.logprob(s)
            n += max(0, len(s) - 1)
        if n == 0:
            raise ValueError("perplexity: no predicted token")
        return math.exp(-total / n)

    # ------------------------------------------------------------------ files
    def tables(self) -> dict:
        """The flat arrays of the module docstring (views, not copies)."""
        t = {"order": np.array(self.order, dtype=np.int32), "vocab": np.array(self.vocab, dtype=np.int32), "uni": self.uni,
             "succ_tok": self.succ_tok, "succ_lp": self.succ_lp}
        for k in range(MAX_ORDER - 1):
            t[f"keys{k + 1}"], t[f"bo{k + 1}"], t[f"off{k + 1}"] = self.keys[k], self.bo[k], self.off[k]
        return t

    def save(self, path: str) -> None:
        """``.npz`` of ``tables()``: arrays only."""
        with open(path, "wb") as f:
            np.savez(f, **self.tables())

    @classmethod
    def load(cls, path: str):
        with np.load(path, allow_pickle=False) as z:
            lm = cls(int(z["order"]), int(z["vocab"]))
            lm.uni = z["uni"].astype(np.float32, copy=True)
            lm.succ_tok, lm.succ_lp = z["succ_tok"].astype(np.int32, copy=True), z["succ_lp"].astype(np.float32, copy=True)
            for k in range(MAX_ORDER - 1):
                lm.keys[k] = z[f"keys{k + 1}"].astype(np.int64, copy=True)
                lm.bo[k] = z[f"bo{k + 1}"].astype(np.float32, copy=True)
                lm.off[k] = z[f"off{k + 1}"].astype(np.int32, copy=True)
        lm._validate()
        return lm

    def _validate(self) -> None:
        if self.uni.shape != (self.vocab,):
            raise ValueError("language model file: uni does not hold one value per token")
        for k in range(MAX_ORDER - 1):
            n = self.keys[k].size
            if k >= self.order - 1 and n:
                raise ValueError(f"language model file: contexts of {k + 1} tokens in a model of order {self.order}")
            if self.bo[k].size != n or self.off[k].size != n + 1 or np.any(np.diff(self.keys[k]) <= 0) or np.any(np.diff(self.off[k]) < 0):
                raise ValueError(f"language model file: inconsistent tables for contexts of {k + 1} tokens")
            if self.off[k][0] < 0 or self.off[k][-1] > self.succ_tok.size:
                raise ValueError("language model file: successor offsets outside the successor arrays")
        if self.succ_tok.size != self.succ_lp.size or (self.succ_tok.size and (self.succ_tok.min() < 0 or self.succ_tok.max() >= self.vocab)):
            raise ValueError("language model file: successor tokens outside the vocabulary")

    @classmethod
    def from_arpa(cls, text_or_path: str, token_to_id, bos_id: int, eos_id: int, vocab: int):
        """Import an ARPA file (or its text): log10 values become natural logarithms, ``<s>`` maps to BOS and ``</s>`` to EOS, other
        tokens through ``token_to_id`` (a dict or a callable returning None for unknown tokens); entries with an unmapped token are
        dropped; a token of the vocabulary without a unigram gets the ``<unk>`` value if the file has one, else the smallest unigram
        value.  An n-gram's back-off becomes the ``bo`` of the context it spells; a context listed without one has bo = 0."""
        import os
        text = text_or_path
        if "\n" not in text_or_path and os.path.exists(text_or_path):
            with open(text_or_path, encoding="utf-8") as f:
                text = f.read()
        look = token_to_id.get if isinstance(token_to_id, dict) else token_to_id
        ln10 = math.log(10.0)

        def tid(w):
            if w == "<s>":
                return int(bos_id)
            if w == "</s>":
                return int(eos_id)
            v = look(w)
            return None if v is None or not 0 <= int(v) < int(vocab) else int(v)

        section, grams, unk = 0, {}, None
        for line in text.splitlines():
            line = line.strip()
            if not line or line == "\\data\\" or line.startswith("ngram "):
                continue
            if line == "\\end\\":
                break
            if line.startswith("\\") and line.endswith("-grams:"):
                section = int(line[1:line.index("-")])
                continue
            if not section:
                continue
            f = line.split()
            if len(f) not in (section + 1, section + 2):
                raise ValueError(f"ARPA: cannot read {line!r} as a {section}-gram")
            lp = float(f[0]) * ln10
            bo = float(f[section + 1]) * ln10 if len(f) == section + 2 else None
            if section == 1 and f[1] == "<unk>" and tid("<unk>") is None:
                unk = lp
                continue
            ids = [tid(w) for w in f[1:section + 1]]
            if any(v is None for v in ids):
                continue
            grams.setdefault(section, {})[tuple(ids)] = (lp, bo)
        order = max(grams) if grams else 0
        if not 1 <= order <= MAX_ORDER:
            raise ValueError(f"ARPA: order {order} outside 1..{MAX_ORDER}")
        if not grams.get(1):
            raise ValueError("ARPA: no unigram of the vocabulary")
        fill = unk if unk is not None else min(lp for lp, _ in grams[1].values())
        uni = np.full(int(vocab), fill, dtype=np.float64)
        for (v,), (lp, _) in grams[1].items():
            uni[v] = lp
        contexts = {}
        for k in range(1, order):                # back-offs: a k-gram as the context of length k
            for ctx, (_, bo) in grams.get(k, {}).items():
                if bo is not None:
                    contexts[ctx] = [bo, {}]
        for k in range(2, order + 1):            # successors: a k-gram under its first k - 1 tokens
            for g, (lp, _) in grams.get(k, {}).items():
                contexts.setdefault(g[:-1], [0.0, {}])[1][g[-1]] = lp
        return cls.from_tables(order, int(vocab), uni, {c: (bo, succ) for c, (bo, succ) in contexts.items()})

    # ------------------------------------------------------------------ device
    def to_device(self, device="cuda"):
        """The device form: the flat tables as tensors on ``device`` plus the kzv_ngram_lm struct over them (``DeviceLM``; it keeps the
        tensors alive and is what the ``lm=`` keywords use).  Built once per device and kept for as long as this model lives: the model
        is FROZEN from its first ``to_device`` on -- a later edit of its arrays would not reach the copy; ``release_device()`` drops the
        copies (then the next call builds new ones from the arrays as they are)."""
        import torch
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        key = str(dev)
        if key not in self._device:
            self._device[key] = DeviceLM(self, dev)
        return self._device[key]

    def release_device(self) -> None:
        """Forget the device copies ``to_device`` made (their memory is freed once no decode holds them)."""
        self._device = {}

    def __repr__(self):
        return f"NGramLM(order={self.order}, vocab={self.vocab}, contexts={self.n_contexts()}, successors={int(self.succ_tok.size)})"


class DeviceLM:
    """An NGramLM's tables on a device and the C struct over them (include/kzv.h: kzv_ngram_lm).  ``host`` is the model itself."""

    def __init__(self, host: NGramLM, device):
        import torch
        from . import _lib as L
        self.host, self.device = host, device
        self.order, self.vocab = host.order, host.vocab
        t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in host.tables().items() if k not in ("order", "vocab")}
        self.tensors = t
        s = L.kzv_ngram_lm()
        s.order, s.vocab, s.reserved = host.order, host.vocab, 0
        for k in range(MAX_ORDER - 1):
            n = int(host.keys[k].size) if k < host.order - 1 else 0
            s.n_ctx[k] = n
            s.keys[k] = L.ptr(t[f"keys{k + 1}"]) if n else None
            s.bo[k] = L.ptr(t[f"bo{k + 1}"]) if n else None
            s.off[k] = L.ptr(t[f"off{k + 1}"]) if n else None
        s.uni = L.ptr(t["uni"])
        s.succ_tok = L.ptr(t["succ_tok"]) if host.succ_tok.size else None
        s.succ_lp = L.ptr(t["succ_lp"]) if host.succ_lp.size else None
        self.struct = s

    def keep(self) -> list:
        """The tensors a stream that reads the tables must keep alive."""
        return list(self.tensors.values())


def resolve(lm, lm_weight, vocab: int, device=None):
    """The ``lm=`` / ``lm_weight=`` keywords of a decode: (host NGramLM, DeviceLM or None, weight), or None when the fusion is off
    (``lm is None`` or ``lm_weight == 0``: nothing is built and nothing launched).  ValueError for a non-finite weight, a vocabulary
    that is not the model's, or something that is no language model."""
    w = float(lm_weight)
    if not math.isfinite(w):
        raise ValueError(f"lm_weight must be finite (got {lm_weight})")
    if lm is None or w == 0.0:
        return None
    host = lm.host if isinstance(lm, DeviceLM) else lm
    if not isinstance(host, NGramLM):
        raise ValueError("lm must be an NGramLM or its device form (NGramLM.to_device)")
    if host.vocab != int(vocab):
        raise ValueError(f"the language model's vocabulary ({host.vocab}) is not the model's ({int(vocab)})")
    if device is None:
        return host, (lm if isinstance(lm, DeviceLM) else None), w
    return host, host.to_device(device), w


def fuse_reference(scores, histories, lm: NGramLM, weight: float):
    """The torch statement of the fusion: ``scores`` [R, V] (logits for greedy decoding, processed log-probabilities for beam search),
    ``histories`` [R, n] token ids, BOS included; returns y = scores + weight * lm with two fp32 roundings (the multiply, then the
    add); -inf stays -inf."""
    import torch
    h = histories.tolist()
    rows = np.stack([lm.row(r) for r in h]) if h else np.zeros((0, lm.vocab), dtype=np.float32)
    t = torch.from_numpy(rows).to(scores.device)
    w = torch.tensor(float(weight), dtype=torch.float32, device=scores.device)
    return scores.float() + t * w


def fuse_rows_reference(scores, hist, lens, lm: NGramLM, weight: float, live=None):
    """``fuse_reference`` where every row has its own history length: row r has hist[r][:lens[r]]; rows with live[r] false come back
    untouched (the slot statements' hook: kzv/stream.py)."""
    x = scores.clone()
    ln = [int(v) for v in lens.tolist()]
    lv = [True] * len(ln) if live is None else [bool(v) for v in live.tolist()]
    for r in range(x.shape[0]):
        if lv[r]:
            x[r:r + 1] = fuse_reference(scores[r:r + 1], hist[r:r + 1, :ln[r]], lm, weight)
    return x


def hook(lm: NGramLM, weight: float, controls=None):
    """``process(scores [R, V], ids [R, >= n], n) -> scores`` for the lockstep statements (kzv/beam.py): ``controls`` (a hook of the same
    shape, GenerationControls.hook) first, then the fusion."""
    def process(scores, ids, n):
        if controls is not None:
            scores = controls(scores, ids, n)
        return fuse_reference(scores, ids[:, :n], lm, weight)
    return process


def rows_hook(lm: NGramLM, weight: float, controls=None):
    """``process(scores [R, V], hist [R, L], lens [R], live [R]) -> scores`` for the slot statements (kzv/stream.py): ``controls``
    (GenerationControls.rows_hook) first, then the fusion; rows that are not live come back as they are."""
    def process(scores, hist, lens, live=None):
        if controls is not None:
            scores = controls(scores, hist, lens, live)
        return fuse_rows_reference(scores, hist, lens, lm, weight, live)
    return process


def sweep_weight(model, pixel_values_or_loader, labels, lm, weights, **generate_kw) -> dict:
    """{weight: corpus CER} of ``model.evaluate_many`` over the images for every weight of ``weights`` -- how a user picks lm_weight on
    the validation split; the CER comes from the device.  A loader is read once and held (every weight decodes the same batches)."""
    import torch
    px = pixel_values_or_loader if torch.is_tensor(pixel_values_or_loader) else list(pixel_values_or_loader)
    lab = labels if torch.is_tensor(labels) else list(labels)
    return {float(w): model.evaluate_many(px, lab, lm=lm, lm_weight=float(w), **generate_kw)["cer_corpus"] for w in weights}


def wrap_sequence(ids, bos_id: int, eos_id: int) -> list[int]:
    """``ids`` as BOS ... EOS: the project's one-character tokenizer adds neither on encode (kzv/data.py), a decode's history starts
    with BOS and ends a line with EOS, so label ids are wrapped before ``fit`` sees them; ids that already hold them stay."""
    r = [int(v) for v in ids]
    if not r or r[0] != bos_id:
        r = [int(bos_id)] + r
    if r[-1] != eos_id:
        r = r + [int(eos_id)]
    return r


def sequences_from_labels(labels, pad_id: int, eos_id: int, bos_id: int | None = None) -> list[list[int]]:
    """Label rows (tokens and padding, with or without BOS / EOS) as the sequences ``fit`` takes: cut after the first EOS, padding
    dropped; with ``bos_id`` every row is wrapped as BOS ... EOS where it is not already (``wrap_sequence``).  Empty rows are left out."""
    out = []
    for r in labels:
        r = [int(v) for v in np.asarray(r).tolist()]
        if eos_id in r:
            r = r[:r.index(eos_id) + 1]
        r = [v for v in r if v != pad_id]
        if bos_id is not None and r:
            r = wrap_sequence(r, bos_id, eos_id)
        if len(r) >= 2:
            out.append(r)
    return out


def load_any(path: str, tokenizer=None, bos_id=None, eos_id=None, vocab=None) -> NGramLM:
    """``.arpa`` by extension (needs the tokenizer), anything else as the ``.npz`` of ``save``."""
    if path.lower().endswith(".arpa"):
        if tokenizer is None:
            raise ValueError("an ARPA file needs the tokenizer that maps its tokens to ids")
        return NGramLM.from_arpa(path, tokenizer.get_vocab(), bos_id, eos_id, vocab)
    return NGramLM.load(path)


def _main(argv=None) -> int:
    """python -m kzv.lm fit|info|perplexity: files of one label per line, tokenised by the tokenizer of a decoder directory."""
    import argparse
    p = argparse.ArgumentParser(prog="python -m kzv.lm", description=_main.__doc__)
    sub = p.add_subparsers(dest="cmd", required=True)
    f = sub.add_parser("fit", help="fit on a text file and write the .npz")
    f.add_argument("text")
    f.add_argument("--tokenizer", required=True)
    f.add_argument("--order", type=int, default=3)
    f.add_argument("--discount", type=float, default=0.75)
    f.add_argument("--out", required=True)
    i = sub.add_parser("info", help="order, vocabulary and context counts of an .npz")
    i.add_argument("lm")
    q = sub.add_parser("perplexity", help="perplexity of a text file under an .npz / .arpa")
    q.add_argument("lm")
    q.add_argument("text")
    q.add_argument("--tokenizer", required=True)
    a = p.parse_args(argv)
    if a.cmd == "info":
        print(NGramLM.load(a.lm))
        return 0
    from transformers import AutoTokenizer
    tok = AutoTokenizer.from_pretrained(a.tokenizer)
    with open(a.text, encoding="utf-8") as fh:
        lines = [ln.rstrip("\n") for ln in fh if ln.strip()]
    bos = tok.bos_token_id if tok.bos_token_id is not None else tok.cls_token_id
    eos = tok.eos_token_id if tok.eos_token_id is not None else tok.sep_token_id
    if bos is None or eos is None:
        raise SystemExit("the tokenizer names no BOS / EOS (bos_token or cls_token, eos_token or sep_token)")
    # the one-character tokenizer adds no BOS / EOS on encode: every line is wrapped, as a decode's history is
    seqs = [wrap_sequence(s, bos, eos) for s in (tok(ln)["input_ids"] for ln in lines) if len(s) >= 1]
    if a.cmd == "fit":
        lm = NGramLM.fit(seqs, a.order, len(tok), a.discount)
        lm.save(a.out)
        print(f"{lm} fitted on {len(seqs)} lines -> {a.out}")
        return 0
    lm = load_any(a.lm, tok, bos, eos, len(tok))
    print(f"perplexity {lm.perplexity(seqs):.4f} over {len(seqs)} lines ({lm})")
    return 0


if __name__ == "__main__":
    raise SystemExit(_main())
