"""Per-class weights of the TrOCR training loss (TrOCRModel(class_weights=...), python -m kzv.train --class_weights) from how often
each character is a TARGET of the training split.  The vocabulary is a few thousand single characters with a long tail: a handful of kana
are most targets, hundreds of kanji appear a few times per epoch.

  count_targets  what the loss scores: row[1:] != pad of every label row (the first id of a row is only ever an input), so an EOS in the
                 rows is counted and a BOS is not.
  from_counts    weights from those counts, n_c = max(count_c, 1) (a class never seen weighs like one seen once):
                   inv_pow    n_c ** -power                        (power 0.5: inverse square root)
                   effective  (1 - beta) / (1 - beta ** n_c)       (class-balanced loss: the inverse "effective number" of samples)
                 clamped into [min, min * cap] (min = the smallest raw weight, that of the commonest class) and scaled so that the
                 count-weighted mean is 1: sum_c count_c w_c == sum_c count_c.  The weight of an average training token is then 1, so
                 the loss, the clip threshold and the learning rate keep their meaning.
"""
from __future__ import annotations

import numpy as np

SCHEMES = ("inv_pow", "effective")


def count_targets(label_id_rows, vocab: int, pad_id: int) -> np.ndarray:
    """int64 [vocab]: how often each class is a scored target, over rows of label ids (lists, arrays or tensors, padded or not)."""
    counts = np.zeros(int(vocab), dtype=np.int64)
    for row in label_id_rows:
        ids = np.asarray(row, dtype=np.int64).reshape(-1)[1:]
        ids = ids[(ids != pad_id) & (ids >= 0) & (ids < vocab)]
        counts += np.bincount(ids, minlength=int(vocab))
    return counts


def from_counts(counts, scheme: str = "inv_pow", power: float = 0.5, beta: float = 0.999, cap: float = 10.0) -> np.ndarray:
    """float32 [V] weights from int counts [V] (module docstring).  cap >= 1 bounds max / min; 0 < beta < 1; power >= 0."""
    counts = np.asarray(counts, dtype=np.float64).reshape(-1)
    if counts.size == 0 or bool((counts < 0).any()):
        raise ValueError("counts must be a non-empty array of non-negative numbers")
    if not cap >= 1.0:
        raise ValueError(f"cap must be >= 1, not {cap!r}")
    n = np.maximum(counts, 1.0)
    if scheme == "inv_pow":
        if not power >= 0.0:
            raise ValueError(f"power must be >= 0, not {power!r}")
        raw = n ** -float(power)
    elif scheme == "effective":
        if not 0.0 < beta < 1.0:
            raise ValueError(f"beta must be in (0, 1), not {beta!r}")
        raw = (1.0 - beta) / -np.expm1(n * np.log(beta))       # 1 - beta ** n without the cancellation at small n (1 - beta)
    else:
        raise ValueError(f"scheme must be one of {SCHEMES}, not {scheme!r}")
    lo = float(raw.min())
    w = np.clip(raw, lo, lo * float(cap))
    total = float(counts.sum())
    if total > 0:
        w = w * (total / float((counts * w).sum()))
    return w.astype(np.float32)


def describe(w, cap: float | None = None) -> str:
    """One line for the training log: the range of the weights and how many classes sit at each clamp."""
    w = np.asarray(w, dtype=np.float64)
    lo, hi = float(w.min()), float(w.max())
    at_lo = int((w <= lo * (1 + 1e-6)).sum())
    at_hi = int((w >= hi * (1 - 1e-6)).sum())
    capped = "" if cap is None else f", cap {cap:g}"
    return f"min {lo:.4g} ({at_lo} classes), max {hi:.4g} ({at_hi} classes), max / min {hi / lo:.3g}{capped}"
