"""N-best lists and per-token log-probabilities of the device beam search: the host side (HF ``generate(num_return_sequences=n,
output_scores=True)`` + ``compute_transition_scores``).

Both beam searches keep an image's whole finished list -- num_beams hypotheses, best first, with scores and lengths -- on the device
through the search; kzv/beam.py and kzv/stream.py state how rows 0 .. n - 1 of it and their per-token log-probabilities leave
(``nbest_result``), csrc/token_search.hip does it (the LP / NBEST instances of the two update kernels).  What is here:

  * ``check_request``: the one refusal rule of ``generate`` / ``generate_stream`` / ``recognize_many`` / ``evaluate_many``;
  * ``WaveOutputs`` / ``static_wave``: the n-best buffers of one ``generate_stream`` wave (kzv_stream_set_nbest) and the same rows from
    lockstep ``generate`` for the two fallbacks;
  * ``records``: ``recognize_many``'s records with ``score`` and ``hypotheses``;
  * ``oracle_stats``: the oracle CER of an n-best table -- how much of the error the search already holds among its candidates, i.e. what
    a language model or a lexicon rescoring could win at most.

Rows are image-major, best first: row i * n + r is hypothesis r of image i, as HF lays ``sequences`` out."""
from __future__ import annotations

import numpy as np


def check_request(num_beams: int, num_return_sequences: int = 1, return_logprobs: bool = False, who: str = "generate") -> int:
    """``num_return_sequences`` as an int after the refusals: it must be in 1..num_beams, and more than one needs a beam search."""
    nb, n = int(num_beams), int(num_return_sequences)
    if nb < 1:
        raise ValueError(f"{who}: num_beams must be positive")
    if n < 1 or n > nb:
        if nb == 1 and n > 1:
            raise ValueError(f"{who}: num_return_sequences = {n} needs a beam search (num_beams >= {n}); greedy decoding has one reading per line")
        raise ValueError(f"{who}: num_return_sequences must be in 1..num_beams = {nb} (got {n})")
    return n


def check_done(lengths, who: str = "generate"):
    """Every returned row must be a finished hypothesis: a finished entry that never received one comes out with length 0."""
    if int(lengths.min()) < 1:
        bad = int((lengths < 1).sum())
        raise RuntimeError(f"{who}: {bad} of the {lengths.numel()} rows asked for never received a finished hypothesis (the search ended "
                           "with fewer than num_return_sequences of them)")


class WaveOutputs:
    """The n-best outputs of one wave of ``n_images`` images: ids [n_images * n, Lh] (BOS + padding), scores, lengths, and with
    ``want_lp`` log-probabilities (zeros) -- what kzv_stream_set_nbest writes into."""

    def __init__(self, n_images: int, n: int, Lh: int, pad_id: int, bos_id: int, device, want_lp: bool):
        import torch
        self.n = int(n)
        self.ids = torch.full((n_images * self.n, Lh), pad_id, dtype=torch.int64, device=device)
        self.ids[:, 0] = bos_id
        self.scores = torch.zeros(n_images * self.n, dtype=torch.float32, device=device)
        self.lengths = torch.zeros(n_images * self.n, dtype=torch.int32, device=device)
        self.logprobs = torch.zeros(n_images * self.n, Lh, dtype=torch.float32, device=device) if want_lp else None

    def arm(self, lib, handle, stream, check):
        """After kzv_stream_begin_beams and before kzv_stream_start."""
        Lh = self.ids.shape[1]
        check(lib.kzv_stream_set_nbest(handle, self.n, self.ids.data_ptr(), Lh, self.scores.data_ptr(), self.lengths.data_ptr(),
                                       None if self.logprobs is None else self.logprobs.data_ptr(), Lh, stream), "stream_set_nbest")

    def tensors(self):
        return [t for t in (self.ids, self.scores, self.lengths, self.logprobs) if t is not None]

    def result(self) -> dict:
        out = {"ids": self.ids, "scores": self.scores, "lengths": self.lengths.long()}
        if self.logprobs is not None:
            out["logprobs"] = self.logprobs
        return out


def static_wave(model, px, Lh: int, slots: int, lim, beams, n: int, want_lp: bool, generate_kw: dict, prefixes=None) -> dict:
    """The rows of a wave from lockstep ``generate(num_return_sequences=n, return_scores=True, return_logprobs=want_lp)`` over batches of
    ``slots`` (generate_stream's two fallbacks): the same dict as ``WaveOutputs.result``.  With limits, the images of every distinct limit
    are decoded with it as their max_length.  ``prefixes``: the wave's forced prefixes (kzv/prefix.py: Prefixes) or None; every batch gets
    those of its images."""
    import torch
    c = model.cfg
    nb, early, lpen = beams
    n_img, dev = px.shape[0], model.device
    out = WaveOutputs(n_img, n, Lh, c.pad_id, c.bos_id, dev, want_lp)
    lim = None if lim is None else lim.cpu().clamp(max=Lh)
    groups = [(Lh, torch.arange(n_img))] if lim is None else [(int(v), (lim == v).nonzero().reshape(-1)) for v in lim.unique().tolist()]
    hyp = torch.arange(n)
    for width, idx in groups:
        for a in range(0, idx.numel(), slots):
            sel = idx[a:a + slots]
            got = model.generate(px[sel.to(px.device)], max_length=width, num_beams=nb, early_stopping=early, length_penalty=lpen,
                                 num_return_sequences=n, return_scores=True, return_logprobs=want_lp,
                                 prefix_ids=None if prefixes is None else prefixes.select(sel), **generate_kw)
            rows = (sel.view(-1, 1) * n + hyp.view(1, n)).reshape(-1).to(dev)
            g = got[0]
            block = torch.full((rows.numel(), Lh), c.pad_id, dtype=torch.int64, device=dev)
            block[:, :g.shape[1]] = g
            out.ids[rows] = block
            out.scores[rows] = got[1]
            out.lengths[rows] = model.last_generate_lengths.to(torch.int32)
            if want_lp:
                lp = torch.zeros(rows.numel(), Lh, dtype=torch.float32, device=dev)
                lp[:, :g.shape[1]] = got[2]
                out.logprobs[rows] = lp
    return out.result()


def records(model, ids, scores, logprobs, n: int) -> list[dict]:
    """``recognize_many``'s records from the n-best rows of a beam search: per image the winner's ``text``, ``tokens``, ``token_strings``,
    ``logprobs``, ``confidence`` (align.build_records' definitions, from the search's own log-probabilities), its ``score`` (HF
    ``sequences_scores``) and ``hypotheses``: the n readings as such records, best first, entry 0 the winner."""
    from . import align as A
    c = model.cfg
    rows = ids.cpu().numpy()
    R, W = rows.shape
    tok = model.tokenizer
    recs = A.build_records(rows, logprobs[:, 1:].cpu().numpy(), np.zeros((R, W - 1, 2)), np.zeros((R, W - 1), dtype=np.int64),
                           pad_id=c.pad_id, bos_id=c.bos_id, eos_id=c.eos_id,
                           texts=None if tok is None else tok.batch_decode(ids, skip_special_tokens=True),
                           to_strings=None if tok is None else tok.convert_ids_to_tokens)
    sc = scores.cpu().tolist()
    out = []
    for r, s in zip(recs, sc):
        del r["centroids"], r["peak_patches"]
        r["score"] = float(s)
    for i in range(R // n):
        hyps = recs[i * n:(i + 1) * n]
        out.append(dict(hyps[0], hypotheses=hyps))
    return out


def oracle_stats(dist, ref_len, pred_len) -> dict:
    """The oracle CER of an n-best table: ``dist`` / ``pred_len`` int [N, n] (edit distance and length of hypothesis r of line i against
    label i), ``ref_len`` int [N].  Per line the hypothesis with the smallest CER (metrics.cer_values' rule) is the best reading, ties to
    the lower rank.  Returns ``cer_oracle`` (the mean over lines of the best reading's CER), ``cer_oracle_corpus`` (sum of the best
    readings' distances / sum of label lengths), ``oracle_rank`` (list of n counts: how often rank r held the best reading),
    ``cer_oracle_lines`` (the best reading's CER per line) and ``dist_nbest`` (the table, numpy)."""
    from . import metrics as M
    dist = np.asarray(dist).astype(np.int64)
    pred_len = np.asarray(pred_len).astype(np.int64)
    ref_len = np.asarray(ref_len).astype(np.int64).reshape(-1)
    if dist.ndim != 2 or pred_len.shape != dist.shape or ref_len.shape[0] != dist.shape[0]:
        raise ValueError(f"oracle_stats: dist and pred_len [N, n], ref_len [N]; got {dist.shape}, {pred_len.shape}, {ref_len.shape}")
    N, n = dist.shape
    cers = [M.cer_values(dist[:, r], ref_len, pred_len[:, r]) for r in range(n)]
    rank, best_cer, best_dist = [0] * n, [], 0
    for i in range(N):
        r = min(range(n), key=lambda k: (cers[k][i], k))         # ties to the lower rank
        rank[r] += 1
        best_cer.append(cers[r][i])
        best_dist += int(dist[i, r])
    chars = int(ref_len.sum())
    return {"cer_oracle": sum(best_cer) / N if N else 0.0, "cer_oracle_corpus": best_dist / chars if chars else 0.0,
            "oracle_rank": rank, "cer_oracle_lines": best_cer, "dist_nbest": dist}


def oracle_of_ids(model, ids_nbest, labels, n: int) -> dict:
    """``oracle_stats`` of the n-best rows ``ids_nbest`` [N * n, W] against ``labels`` [N, <= 128]: ONE more kzv_edit_distance (the
    distance-only instance), every hypothesis row against its line's label."""
    from . import metrics as M
    lab = labels.to(ids_nbest.device).repeat_interleave(n, dim=0)
    st = M.edit_stats(ids_nbest, lab, model._edit_special_ids(), model.cfg.vocab, ops=False)
    N = ids_nbest.shape[0] // n
    return oracle_stats(st["dist"].view(N, n).cpu().numpy(), st["ref_len"].view(N, n)[:, 0].cpu().numpy(), st["pred_len"].view(N, n).cpu().numpy())
