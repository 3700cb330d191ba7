"""Host part of ``TrOCRModel.align`` / ``TrOCRModel.recognize``: from the padded per-position arrays the engine returns
(include/kzv.h: kzv_cross_attention, kzv_score_tokens) and the token ids to one record per image.  numpy only (torch only where a
caller hands tensors in), so it imports and runs without a GPU.

Indexing.  The decoder is teacher-forced on ``ids[:, :-1]`` and scored against ``ids[:, 1:]``: row ``t`` of every array belongs to
the token ``ids[:, t + 1]`` -- its log-probability, and the cross-attention of the position that EMITTED it.  Row ``t`` is live
when both ``ids[:, t]`` (the decoder input) and ``ids[:, t + 1]`` (the target) are real tokens.
"""
from __future__ import annotations

import math

import numpy as np


def live_mask(ids, pad_id: int):
    """[B, L] ids -> [B, L - 1] bool: decoder input and target both non-pad (works on numpy arrays and torch tensors)."""
    return (ids[:, :-1] != pad_id) & (ids[:, 1:] != pad_id)


def patch_to_pixel(rows_cols, patch_h: int, patch_w: int):
    """Patch-grid coordinates [..., 2] = (row, col), fractional allowed -> pixel coordinates (y, x) of that point, a patch's
    own (row, col) mapping to its centre: ((row + 0.5) * patch_h, (col + 0.5) * patch_w).  numpy or torch."""
    out = rows_cols + 0.5
    if isinstance(out, np.ndarray):
        return out * np.asarray([patch_h, patch_w], dtype=out.dtype)
    return out * out.new_tensor([patch_h, patch_w])


def peak_to_pixel(patch: int, grid_w: int, patch_h: int, patch_w: int) -> tuple[float, float]:
    """Centre (y, x) in pixels of patch index ``patch`` on a grid ``grid_w`` patches wide."""
    return ((patch // grid_w + 0.5) * patch_h, (patch % grid_w + 0.5) * patch_w)


def stats_from_map(amap, grid_w: int):
    """What kzv_attn_probs derives from a map, restated in torch for maps averaged on the host (several layers):
    amap [B, T, n_patches] -> (pos [B, T, 4] = (sum P row, sum P col, max P, sum P), peak [B, T] = first arg-max)."""
    import torch
    k = torch.arange(amap.shape[-1], device=amap.device)
    row = torch.div(k, grid_w, rounding_mode="floor").to(amap.dtype)
    col = (k % grid_w).to(amap.dtype)
    # the FIRST maximum, explicitly (torch.max / argmax do not promise which of several equal maxima they return)
    top = amap.max(dim=-1, keepdim=True).values
    peak = torch.where(amap == top, k, amap.shape[-1]).min(dim=-1).values
    pos = torch.stack(((amap * row).sum(-1), (amap * col).sum(-1), top.squeeze(-1), amap.sum(-1)), dim=-1)
    return pos, peak.to(torch.int32)


def pad_rows(x, width: int, fill=0):
    """[B, t, ...] torch tensor -> [B, width, ...] (t <= width), the new rows holding ``fill``."""
    if x.shape[1] == width:
        return x
    out = x.new_full((x.shape[0], width) + tuple(x.shape[2:]), fill)
    out[:, :x.shape[1]] = x
    return out


def build_records(ids, logprob, centroid, peak_patch, *, pad_id: int, bos_id: int, eos_id: int, texts=None, to_strings=None,
                  alternatives=None, forced=None, prefix_logprobs=None) -> list[dict]:
    """One record per image from ids [B, L] (BOS first, PAD after the end) and the per-position arrays [B, L - 1] (centroid
    [B, L - 1, 2] in pixels, (y, x)):

      tokens        the ids without BOS / EOS / PAD, in order
      token_strings ``to_strings(tokens)`` (a tokenizer's convert_ids_to_tokens), else None
      text          ``texts[b]`` (batch_decode(skip_special_tokens=True) of the ids), else None
      logprobs      log-probability of each of ``tokens`` (row t scores token t + 1)
      confidence    exp(mean log-probability over ``tokens`` AND the closing EOS when the sequence has one); 0.0 for a row
                    in which nothing was scored
      centroids     (y, x) in pixels per token; peak_patches: the arg-max patch per token

    A row stops at its first EOS or PAD target; a generation that is BOS, EOS only gives empty lists and the EOS's own
    probability as confidence.

    ``alternatives`` = (alt_ids, alt_logprob), [B, L - 1, k] each (kzv_score_tokens_topk / kzv_stream_topk: the k best tokens of
    every position, best first, -1 where there is none), adds two keys:

      alternatives  per token of ``tokens`` a list of up to k dicts {"token", "string", "logprob"} in rank order (entries with
                    id -1 dropped; ``string`` from ``to_strings``, else None)
      margins       per token the first alternative's log-probability minus the second's; inf with a single candidate

    ``forced`` = [B] ints (forced prefixes, kzv/prefix.py: the first forced[b] tokens after BOS were given, not read) adds ``forced``
    (the count) to every record; ``confidence`` is then taken over the FREE tokens only (EOS included), and the ``alternatives`` /
    ``margins`` of forced positions are emptied ([] / inf).  ``prefix_logprobs`` [B, >= forced + 1] (column t + 1 = the model's own
    log-probability of the token forced at row t; generate_stream(return_prefix_logprobs=True)) adds ``prefix_logprobs``, one value
    per forced token.  None: the records as they were."""
    ids = np.asarray(ids)
    logprob = np.asarray(logprob, dtype=np.float64)
    centroid = np.asarray(centroid, dtype=np.float64)
    peak_patch = np.asarray(peak_patch)
    B, L = ids.shape
    if logprob.shape != (B, L - 1) or peak_patch.shape != (B, L - 1) or centroid.shape != (B, L - 1, 2):
        raise ValueError(f"per-position arrays must be [B, L - 1] = {(B, L - 1)} (centroid [B, L - 1, 2]); got "
                         f"{logprob.shape}, {centroid.shape}, {peak_patch.shape}")
    if alternatives is not None:
        alt_ids, alt_lp = (np.asarray(a) for a in alternatives)
        if alt_ids.ndim != 3 or alt_ids.shape[:2] != (B, L - 1) or alt_lp.shape != alt_ids.shape:
            raise ValueError(f"alternatives must be two [B, L - 1, k] = {(B, L - 1, 'k')} arrays; got {alt_ids.shape}, {alt_lp.shape}")
    records = []
    for b in range(B):
        tokens, lps, cents, peaks, scored, alts, margins = [], [], [], [], [], [], []
        for t in range(L - 1):
            tok = int(ids[b, t + 1])
            if tok == pad_id or int(ids[b, t]) == pad_id:
                break
            is_forced = forced is not None and t < int(forced[b])
            if not is_forced:
                scored.append(float(logprob[b, t]))
            if tok == eos_id:
                break
            if tok == bos_id:            # a BOS past column 0 is a special token like any other: scored, not reported
                continue
            tokens.append(tok)
            lps.append(float(logprob[b, t]))
            cents.append((float(centroid[b, t, 0]), float(centroid[b, t, 1])))
            peaks.append(int(peak_patch[b, t]))
            if alternatives is not None:
                cand = [(int(i), float(p)) for i, p in zip(alt_ids[b, t], alt_lp[b, t]) if int(i) >= 0]
                strs = [None] * len(cand) if to_strings is None else list(to_strings([i for i, _ in cand]))
                if is_forced:            # the row was overwritten: its candidates say nothing about the model
                    alts.append([])
                    margins.append(math.inf)
                    continue
                alts.append([{"token": i, "string": s, "logprob": p} for (i, p), s in zip(cand, strs)])
                margins.append(cand[0][1] - cand[1][1] if len(cand) > 1 and cand[1][1] > -math.inf else math.inf)
        records.append({
            "text": None if texts is None else texts[b],
            "tokens": tokens,
            "token_strings": None if to_strings is None else list(to_strings(tokens)),
            "logprobs": lps,
            "confidence": math.exp(sum(scored) / len(scored)) if scored else 0.0,
            "centroids": cents,
            "peak_patches": peaks,
        })
        if alternatives is not None:
            records[-1]["alternatives"] = alts
            records[-1]["margins"] = margins
        if forced is not None:
            records[-1]["forced"] = int(forced[b])
            if prefix_logprobs is not None:
                records[-1]["prefix_logprobs"] = [float(prefix_logprobs[b][t + 1]) for t in range(int(forced[b]))]
    return records
