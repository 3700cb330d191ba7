"""Evaluation on the device: edit distance, CER, edit counts, alignment and per-character error tables of decoded lines against
their labels (include/kzv.h: kzv_edit_distance; csrc/edit_distance.hip).

The reference scores a line by ``tokenizer.batch_decode(skip_special_tokens=True)`` of both sides and ``calculate_cer`` on the two strings
(src/models/trocr_model.py:373-379, 400-410).  Its tokenizer is one character per token with the specials at ids 0..4 (kzv/data.py), so
the Levenshtein distance over the ids that are left once the specials are dropped equals the distance over the strings, and the ids are
already on the device when a decode ends.  ``is_one_char_tokenizer`` says whether that holds for a tokenizer; where it does not, callers
keep the string path.

``edit_stats`` is the device call, ``edit_stats_reference`` the numpy statement it is tested against: the full Wagner-Fischer matrix and
a walk back from its last cell under one fixed preference -- DIAGONAL (match or substitution) if it attains the cell's minimum, else UP
(deletion of a label token), else LEFT (insertion of a predicted token).  The rule is part of the contract: both sides report the same
alignment, not merely one of the optimal ones."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

MAX_WIDTH = 128          # columns of an id row (generate's max_length, the data loader's max_length)
MAX_SPECIAL = 8
STAT_COLUMNS = ("count", "correct", "substituted", "deleted", "inserted")


def _specials(special_ids) -> list[int]:
    out = sorted({int(s) for s in special_ids})
    if len(out) > MAX_SPECIAL:
        raise ValueError(f"at most {MAX_SPECIAL} special ids (got {len(out)})")
    return out


def _rows(x, what: str):
    """int64 device rows with unit column stride and a row stride >= the width, as the kernel reads them (no copy where they already are)."""
    import torch
    if x.dim() != 2:
        raise ValueError(f"{what} must be [N, width]")
    if not 1 <= x.shape[1] <= MAX_WIDTH:
        raise ValueError(f"{what}: width must be in 1..{MAX_WIDTH} (got {x.shape[1]})")
    if x.dtype != torch.int64:
        x = x.long()
    if x.shape[0] and (x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < x.shape[1])):
        x = x.contiguous()
    return x, (x.stride(0) if x.shape[0] > 1 else x.shape[1])


def edit_stats(pred_ids, ref_ids, special_ids, vocab, align=False, char_stats=None, ops=True):
    """One ``kzv_edit_distance`` over the pairs (pred_ids[i], ref_ids[i]): int64 device tensors [N, <= 128] each (row strides are honoured).
    ``special_ids`` (<= 8) are dropped by value wherever they stand, as is every id outside [0, vocab).  Returns a dict of device tensors:
    ``dist``, ``ref_len``, ``pred_len`` int32 [N]; ``ops`` int32 [N, 4] = correct, substituted, deleted, inserted (unless ``ops=False``);
    with ``align`` also ``ref_to_pred`` [N, ref width] and ``pred_to_ref`` [N, pred width] over COMPACTED indices (-1 deleted / inserted,
    -2 past the line's end); with ``char_stats`` -- an int32 [vocab, 5] device tensor that is ACCUMULATED into, or True for a fresh one --
    also ``char_stats`` (columns: STAT_COLUMNS).  With ``ops=False`` and neither of the others the distance-only kernel runs."""
    import torch
    vocab = int(vocab)
    if ref_ids.shape[0] != pred_ids.shape[0]:
        raise ValueError("pred_ids and ref_ids must hold the same number of rows")
    dev = pred_ids.device
    ref_ids = ref_ids.to(dev)
    pred, ld_pred = _rows(pred_ids, "pred_ids")
    ref, ld_ref = _rows(ref_ids, "ref_ids")
    sp = _specials(special_ids)
    n, wp, wr = pred.shape[0], pred.shape[1], ref.shape[1]
    out = {k: torch.empty(n, dtype=torch.int32, device=dev) for k in ("dist", "ref_len", "pred_len")}
    if ops:
        out["ops"] = torch.empty(n, 4, dtype=torch.int32, device=dev)
    ld_align = max(wp, wr)
    r2p = p2r = None
    if align:
        r2p = torch.empty(n, ld_align, dtype=torch.int32, device=dev)
        p2r = torch.empty(n, ld_align, dtype=torch.int32, device=dev)
        out["ref_to_pred"], out["pred_to_ref"] = r2p[:, :wr], p2r[:, :wp]
    if char_stats is True:
        char_stats = torch.zeros(vocab, 5, dtype=torch.int32, device=dev)
    if char_stats is not None:
        if char_stats.dtype != torch.int32 or tuple(char_stats.shape) != (vocab, 5) or not char_stats.is_contiguous() or char_stats.device != dev:
            raise ValueError("char_stats must be a contiguous int32 [vocab, 5] tensor on the ids' device")
        out["char_stats"] = char_stats
    a = L.kzv_edit_args(pred=L.ptr(pred), ld_pred=ld_pred, ref=L.ptr(ref), ld_ref=ld_ref, n=n, width_pred=wp, width_ref=wr, vocab=vocab,
                        n_special=len(sp), special=(C.c_int32 * 8)(*sp), dist=L.ptr(out["dist"]), ref_len=L.ptr(out["ref_len"]),
                        pred_len=L.ptr(out["pred_len"]), ops=L.ptr(out.get("ops")), ref_to_pred=L.ptr(r2p), pred_to_ref=L.ptr(p2r),
                        ld_align=ld_align, char_stats=L.ptr(char_stats))
    with torch.cuda.device(dev):
        L.check(L.load().kzv_edit_distance(C.byref(a), L.stream_handle()), "kzv_edit_distance")
    return out


def _np(x):
    return np.asarray(x.detach().cpu().numpy() if hasattr(x, "detach") else x)


def edit_stats_reference(pred_ids, ref_ids, special_ids, vocab, align=False, char_stats=None, ops=True):
    """``edit_stats`` stated in numpy (tensors or arrays in, numpy arrays out): per pair the full (m + 1) x (n + 1) Wagner-Fischer matrix
    with unit costs, then the walk back from (m, n) that prefers the diagonal where it attains the minimum, else up, else left.  A given
    ``char_stats`` is not modified: the returned table is its sum with this call's counts."""
    pred, ref = _np(pred_ids).astype(np.int64), _np(ref_ids).astype(np.int64)
    sp, vocab = _specials(special_ids), int(vocab)
    n, wp, wr = pred.shape[0], pred.shape[1], ref.shape[1]
    out = {k: np.zeros(n, dtype=np.int32) for k in ("dist", "ref_len", "pred_len")}
    op = np.zeros((n, 4), dtype=np.int32)
    r2p, p2r = np.full((n, wr), -2, dtype=np.int32), np.full((n, wp), -2, dtype=np.int32)
    stats = np.zeros((vocab, 5), dtype=np.int64)

    def line(row):
        return [int(t) for t in row if 0 <= t < vocab and int(t) not in sp]

    for k in range(n):
        r, p = line(ref[k]), line(pred[k])
        m, q = len(r), len(p)
        D = [[j if i == 0 else (i if j == 0 else 0) for j in range(q + 1)] for i in range(m + 1)]      # the whole matrix, Python ints
        for i in range(1, m + 1):
            for j in range(1, q + 1):
                D[i][j] = min(D[i - 1][j - 1] + (r[i - 1] != p[j - 1]), D[i - 1][j] + 1, D[i][j - 1] + 1)
        out["dist"][k], out["ref_len"][k], out["pred_len"][k] = D[m][q], m, q
        r2p[k, :m], p2r[k, :q] = -1, -1
        i, j = m, q
        while i > 0 or j > 0:
            if i > 0 and j > 0 and D[i][j] == D[i - 1][j - 1] + (r[i - 1] != p[j - 1]):
                same = r[i - 1] == p[j - 1]
                op[k, 0 if same else 1] += 1
                stats[r[i - 1], 1 if same else 2] += 1
                r2p[k, i - 1], p2r[k, j - 1] = j - 1, i - 1
                i, j = i - 1, j - 1
            elif i > 0 and D[i][j] == D[i - 1][j] + 1:
                op[k, 2] += 1
                stats[r[i - 1], 3] += 1
                i -= 1
            else:
                op[k, 3] += 1
                stats[p[j - 1], 4] += 1
                j -= 1
        for t in r:
            stats[t, 0] += 1
    if ops:
        out["ops"] = op
    if align:
        out["ref_to_pred"], out["pred_to_ref"] = r2p, p2r
    if char_stats is not None:
        base = 0 if char_stats is True else _np(char_stats).astype(np.int64)
        out["char_stats"] = (stats + base).astype(np.int32)
    return out


def cer_values(dist, ref_len, pred_len) -> list[float]:
    """Per-line CER by ``calculate_cer``'s rule (src/models/trocr_model.py:400-410) from the three integer arrays: dist / ref_len, 1.0 for
    an empty target with a non-empty prediction, 0.0 where both are empty.  Python int / int, the very division the string path performs,
    so the values are == to its values."""
    d, r, p = (_np(x).tolist() for x in (dist, ref_len, pred_len))
    return [(1.0 if pk > 0 else 0.0) if rk == 0 else dk / rk for dk, rk, pk in zip(d, r, p)]


def is_one_char_tokenizer(tok) -> bool:
    """True where the id-level distance equals the reference's string-level one: every non-special vocabulary entry is a single character,
    there are at most 8 special ids, and decoding joins the entries with the empty string and leaves them as they are (probed on the whole
    vocabulary in id order with a special in between; a tokenizer that cleans up spaces while holding a whitespace entry is refused)."""
    try:
        vocab = tok.get_vocab()
        special = {int(i) for i in tok.all_special_ids}
    except Exception:
        return False
    if not vocab or len(special) > MAX_SPECIAL:
        return False
    items = sorted(((i, t) for t, i in vocab.items() if i not in special), key=lambda e: e[0])
    if not items or any(len(t) != 1 for _, t in items):
        return False
    if getattr(tok, "clean_up_tokenization_spaces", False) and any(t.isspace() for _, t in items):
        return False
    probe = [i for i, _ in items]
    if special:
        probe.insert(len(probe) // 2, min(special))
    return tok.decode(probe, skip_special_tokens=True) == "".join(t for _, t in items)


def character_table(char_stats, tokenizer=None, top: int | None = 20) -> list[dict]:
    """The characters a model gets wrong, worst first: rows ``{char, id, count, correct, substituted, deleted, inserted, error_rate}`` of the
    ids that occur in ``char_stats`` [vocab, 5], sorted by errors (substituted + deleted + inserted) descending, ties by id; ``error_rate``
    = errors / max(count, 1).  ``top``: how many rows (None: all).  Without a tokenizer ``char`` is None."""
    st = _np(char_stats).astype(np.int64)
    err = st[:, 2] + st[:, 3] + st[:, 4]
    ids = [int(i) for i in np.flatnonzero((st[:, 0] > 0) | (st[:, 4] > 0))]
    ids.sort(key=lambda i: (-int(err[i]), i))
    if top is not None:
        ids = ids[:int(top)]
    chars = tokenizer.convert_ids_to_tokens(ids) if tokenizer is not None and ids else [None] * len(ids)
    return [{"char": ch, "id": i, "count": int(st[i, 0]), "correct": int(st[i, 1]), "substituted": int(st[i, 2]), "deleted": int(st[i, 3]),
             "inserted": int(st[i, 4]), "error_rate": float(err[i]) / max(int(st[i, 0]), 1)} for ch, i in zip(chars, ids)]
