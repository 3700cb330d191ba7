"""Token-selection bookkeeping of ``decoder.generate`` as the reference calls it (src/models/trocr_model.py:306-316:
``max_length=128, num_beams=4, early_stopping=True, pad_token_id, eos_token_id``), separated from the engine so that it can
be pinned on the CPU against HF's own implementation (tests/test_host_cpu.py runs transformers' ``generate`` on a small
RobertaForCausalLM and this module on the same step logits).

``generate`` lives in a third-party dependency (transformers; the reference pins 4.57.0, this image holds 5.15.0), not
under /root/reference; what is restated here is its published algorithm, following transformers/generation/utils.py
``GenerationMixin._beam_search`` (:3208-3508) and its helpers ``_get_top_k_continuations`` (:3077-3129),
``_get_running_beams_for_next_iteration`` (:3131-3151), ``_update_finished_beams`` (:3153-3204),
``_check_early_stop_heuristic`` (:3008-3052), ``_beam_search_has_unfinished_sequences`` (:3055-3075), and the greedy
branch of ``_sample``:

  * every step ranks the 2*num_beams best continuations of [num_beams x vocab] accumulated log-probabilities;
  * a continuation "hits a stopping criterion" when its token is EOS or it reaches max_length; only those among the first
    num_beams ranks may enter the finished list, scored sum-log-prob / generated_length**length_penalty; the finished list
    keeps the best num_beams by score;
  * the running beams of the next step are the best num_beams continuations that did NOT hit a stopping criterion;
  * with early_stopping=True a batch element stops accepting hypotheses once it holds num_beams finished ones, and the
    loop ends when every batch element is full; with early_stopping=False the loop ends when, for every element, the best
    running score / current generated length cannot beat its worst finished score;
  * the result is the best finished hypothesis per element, cropped to the longest one, padded with pad_token_id.

Everything is torch tensor arithmetic on whatever device the logits live on (vectorised over the batch; one host
synchronisation per step for the loop condition).  ``step(t, flat_ids)`` must return the next-token logits [B*beams, V] of
position t given ids[:, :t+1]; ``reorder(flat_rows, t)`` is told which former row each row continues from (KV cache).
"""
from __future__ import annotations

NEG = -1.0e9


def _prefix_rows(prefix, batch: int, group: int, device):
    """``prefix`` = (ids int64 [batch, P], lengths [batch]) (kzv/prefix.py: normalise) on ``device``, expanded to ``group`` rows per
    image: (ids [batch * group, P], lengths int64 [batch * group], lengths per image int64 [batch, 1])."""
    pfx, plen = prefix
    pfx, plen = pfx.to(device).long(), plen.to(device).long().reshape(-1)
    if pfx.dim() != 2 or pfx.shape[0] != batch or plen.numel() != batch:
        raise ValueError(f"prefix: ids [batch, P] and lengths [batch] for batch = {batch}")
    return pfx.repeat_interleave(group, dim=0), plen.repeat_interleave(group), plen.view(batch, 1)


def greedy(step, batch: int, max_len: int, pad_id: int, bos_id: int, eos_id: int, device, update=None, process=None, prefix=None):
    """``num_beams=1``: argmax per step; finished rows emit padding; stops when every row has emitted EOS.
    ``update(logits, ids, t, done) -> running`` (optional, kzv_greedy_update): the selection in one launch; running[t] = rows
    still running after step t.
    ``process(logits, ids, n) -> logits`` (optional; kzv/controls.py: GenerationControls.hook): generation controls on the step's raw
    logits given the histories ids[:, :n] -- where HF's greedy loop applies its logits processors.  None: what this computed before.
    ``prefix`` = (ids [batch, P], lengths [batch]) (optional; kzv/prefix.py): every row's forced prefix, the prompt [BOS] + prefix of HF's
    ``generate(input_ids=...)``.  While the chosen index t + 1 lies inside a row's prefix its scores are replaced by force_reference's
    row AFTER ``process``, so arg-max takes the forced token; nothing else changes (a prefix holds no EOS).  A caller that forces inside
    ``step`` / ``process`` itself (the device kernel) passes None."""
    import torch
    ids = torch.full((batch, max_len), pad_id, dtype=torch.int64, device=device)
    ids[:, 0] = bos_id
    if process is not None:
        raw_step = step
        step = lambda t, ids_: process(raw_step(t, ids_), ids_, t + 1)      # noqa: E731
    if prefix is not None:
        from . import prefix as PF
        pfx_rows, plen_rows, _ = _prefix_rows(prefix, batch, 1, device)
        free_step = step
        step = lambda t, ids_: PF.force_reference(free_step(t, ids_).float(), t + 1, pfx_rows, plen_rows)      # noqa: E731
    if update is not None:
        # the stop test costs a host round trip: taken every 4th step; the steps run past the end only write padding, and the
        # per-step counters say where the end was
        done8 = torch.zeros(batch, dtype=torch.uint8, device=device)
        running = None
        for t in range(max_len - 1):
            running = update(step(t, ids), ids, t, done8)
            if t % 4 == 3 or t == max_len - 2:
                r = running[:t + 1].tolist()
                if 0 in r:
                    return ids[:, :r.index(0) + 2]
        return ids[:, :max_len]
    done = torch.zeros(batch, dtype=torch.bool, device=device)
    n = 1
    for t in range(max_len - 1):
        nxt = step(t, ids).argmax(-1)
        nxt = torch.where(done, torch.full_like(nxt, pad_id), nxt)
        ids[:, t + 1] = nxt
        n = t + 2
        done |= nxt == eos_id
        if bool(done.all()):
            break
    return ids[:, :n]


def nbest_result(fin_seq, fin_sc, fin_done, fin_len, fin_lp, n: int, bos_id: int, pad_id: int):
    """The first ``n`` rows of every image's finished list in HF's ``num_return_sequences`` layout (image-major, best first): a dict of
    ``ids`` int64 [B * n, width], width = the longest of those rows; ``scores`` fp32 [B * n] (HF ``sequences_scores``); ``lengths`` int64
    [B * n], tokens with BOS included; and, where ``fin_lp`` is given, ``logprobs`` fp32 [B * n, width]: column t holds the
    log-probability of the token in column t, 0 in column 0 and from the row's length on (generate_stream's conventions for greedy).
    A finished entry that never received a hypothesis (fin_done == 0) comes out as BOS + padding, score -1e9, length 0: what the slot
    kernel writes for it."""
    import torch
    B, _, L = fin_seq.shape
    done = fin_done[:, :n].bool()
    lengths = torch.where(done, fin_len[:, :n], torch.zeros_like(fin_len[:, :n]))
    width = max(2, int(lengths.max()))
    col = torch.arange(width, device=fin_seq.device).view(1, 1, width)
    keep = col < lengths.unsqueeze(-1)
    blank = torch.full_like(fin_seq[:, :n, :width], pad_id)
    blank[:, :, 0] = bos_id
    out = {"ids": torch.where(keep, fin_seq[:, :n, :width], blank).reshape(B * n, width),
           "scores": torch.where(done, fin_sc[:, :n], torch.full_like(fin_sc[:, :n], NEG)).reshape(B * n),
           "lengths": lengths.reshape(B * n)}
    if fin_lp is not None:
        lp = fin_lp[:, :n, :width]
        out["logprobs"] = torch.where(keep & (col >= 1), lp, torch.zeros_like(lp)).reshape(B * n, width)
    return out


def _check_nbest(num_return_sequences, num_beams):
    n = int(num_return_sequences)
    if not 1 <= n <= int(num_beams):
        raise ValueError(f"num_return_sequences must be in 1..num_beams = {int(num_beams)} (got {n})")
    return n


def beam_search(step, reorder, batch: int, num_beams: int, max_len: int, vocab: int, pad_id: int, bos_id: int, eos_id: int,
                device, early_stopping=True, length_penalty: float = 1.0, topk=None, update=None, process=None,
                num_return_sequences: int = 1, return_logprobs: bool = False, prefix=None):
    """``topk(logits [B * nb, vocab] fp32, run_sc [B, nb]) -> (top_lp [B, 2 nb], top_ix [B, 2 nb])``: optional fused ranking
    (kzv_beam_topk on the GPU); None = the torch expression of the same thing below.
    ``update``: optional fused bookkeeping (kzv_beam_update); with it the loop below is replaced by beam_search_fused.
    ``process(logp, ids, n) -> logp`` (optional; GenerationControls.hook): generation controls on ``log_softmax(logits)`` given the
    histories ids[:, :n], before the beam score is added and with no second normalisation -- where HF's beam search applies its logits
    processors.  It belongs to the torch expression: a caller that passes ``topk`` processes inside ``step`` and passes a ranking over
    log-probabilities (make_device_hooks(logprobs=True)).  None: what this computed before.
    ``num_return_sequences`` n in 1..num_beams / ``return_logprobs``: with n > 1 or log-probabilities asked for, the result is
    nbest_result's dict of the first n rows of the finished list instead of the winner's ids (HF ``generate(num_return_sequences=n)``).
    A token's log-probability is the fp32 difference ``top_lp[k] - run_sc[src[k]]``, the continuation's accumulated score minus its
    parent beam's, carried in run_lp / fin_lp [B, nb, max_len] through exactly the gathers of run_seq / fin_seq (HF
    ``compute_transition_scores``); under ``process`` it is therefore the processed row's value.
    ``prefix`` = (ids [B, P], lengths [B]) (optional; kzv/prefix.py): every image's forced prefix, so that its prompt is [BOS] + prefix
    and ``prompt`` below becomes 1 + lengths PER IMAGE.  While cur lies inside an image's prefix the processed log-probabilities of its
    rows are replaced by force_reference's rows (the torch ranking; with ``topk`` the caller forces inside ``step``), so all beams carry
    the prefix at scores 0, -1e9, -1e9, .. -- HF's state after a prompt.  Scores sum the generated tokens only (a forced token adds 0);
    a hypothesis is normalised by its generated length cur + 1 - prompt and the heuristic uses cur - prompt, both clamped to >= 1: inside
    a prefix nothing can finish (it holds no EOS and ends before max_len - 1), so a forced step only moves the running beams and the
    image stays unsatisfied, where 0 / 0 ** p would end the search.  The divisors are fp32 of n ** length_penalty computed in double
    (stream.divisor_table): what HF's tensor / Python float divides by.  With the device ``update`` the lengths live in that hook
    (make_device_hooks(prefix_len=...))."""
    import torch
    if process is not None and topk is not None:
        raise ValueError("beam_search: `process` belongs to the torch ranking; with `topk` process inside `step` and rank log-probabilities")
    if update is not None and topk is not None:
        return beam_search_fused(step, reorder, batch, num_beams, max_len, vocab, pad_id, bos_id, eos_id, device, early_stopping,
                                 length_penalty, topk, update, num_return_sequences=num_return_sequences, return_logprobs=return_logprobs)
    n_ret = _check_nbest(num_return_sequences, num_beams)
    B, nb, K = batch, num_beams, 2 * num_beams
    prompt = 1                                                    # decoder prompt = [BOS]
    pfx_rows = plen_rows = plen_img = div_tab = None
    if prefix is not None:                                        # per image: prompt = [BOS] + prefix
        from . import prefix as PF
        from .stream import divisor_table
        pfx_rows, plen_rows, plen_img = _prefix_rows(prefix, B, nb, device)
        div_tab = divisor_table(max_len, length_penalty, device)
    run_seq = torch.full((B, nb, max_len), pad_id, dtype=torch.int64, device=device)
    run_seq[:, :, 0] = bos_id
    fin_seq = run_seq.clone()
    run_sc = torch.zeros(B, nb, device=device)
    run_sc[:, 1:] = NEG                                           # only beam 0 is live at the first step
    fin_sc = torch.full((B, nb), NEG, device=device)
    fin_done = torch.zeros(B, nb, dtype=torch.bool, device=device)
    fin_len = torch.full((B, nb), prompt, dtype=torch.int64, device=device)
    run_lp = fin_lp = None
    if return_logprobs:
        run_lp = torch.zeros(B, nb, max_len, dtype=torch.float32, device=device)
        fin_lp = run_lp.clone()
    unsat = torch.ones(B, 1, dtype=torch.bool, device=device)     # "the open beams may still improve the finished ones"
    top_mask = (torch.arange(K, device=device) < nb).view(1, K)
    base = (torch.arange(B, device=device) * nb).view(B, 1)
    cur = prompt
    while True:
        raw = step(cur - 1, run_seq.view(B * nb, max_len))
        if topk is not None:
            top_lp, top_ix = topk(raw, run_sc)
        else:
            logp = torch.log_softmax(raw.float(), dim=-1)
            if process is not None:
                logp = process(logp, run_seq.view(B * nb, max_len), cur)
            if pfx_rows is not None:
                logp = PF.force_reference(logp, cur, pfx_rows, plen_rows)
            acc = logp.view(B, nb, vocab) + run_sc.unsqueeze(-1)
        # top K of the nb * vocab continuations in two stages (the K best overall are among each beam's K best): one
        # single-block top-k per beam row instead of a multi-pass radix select over nb * vocab entries per batch element
        if topk is not None:
            pass
        elif vocab > 4 * K:
            blp, bix = acc.topk(K, dim=2)                                  # [B, nb, K]
            top_lp, sel = blp.reshape(B, nb * K).topk(K, dim=1)
            top_ix = (bix + (torch.arange(nb, device=device) * vocab).view(1, nb, 1)).reshape(B, nb * K).gather(1, sel)
        else:
            top_lp, top_ix = acc.view(B, nb * vocab).topk(K, dim=1)
        src, tok = top_ix // vocab, top_ix % vocab
        cand = run_seq.gather(1, src.unsqueeze(-1).expand(B, K, max_len)).clone()
        cand[:, :, cur] = tok
        hits = (tok == eos_id) | (cur + 1 >= max_len)
        # running beams of the next step: the best nb continuations that did not stop
        nxt_ix = (top_lp + hits.float() * NEG).topk(nb, dim=1)[1]
        if run_lp is not None:                                    # the token's own log-probability, from the OLD running scores
            cand_lp = run_lp.gather(1, src.unsqueeze(-1).expand(B, K, max_len)).clone()
            cand_lp[:, :, cur] = top_lp.float() - run_sc.gather(1, src)
            run_lp = cand_lp.gather(1, nxt_ix.unsqueeze(-1).expand(B, nb, max_len))
        run_seq = cand.gather(1, nxt_ix.unsqueeze(-1).expand(B, nb, max_len))
        run_sc = (top_lp + hits.float() * NEG).gather(1, nxt_ix)
        rows = (base + src.gather(1, nxt_ix)).reshape(-1)
        # finished list: stopped continuations of rank < nb, normalised by the generated length
        just = hits & top_mask
        if plen_img is None:
            fsc = top_lp / float((cur + 1 - prompt) ** length_penalty)
        else:                                                     # the image's own generated length, >= 1 (a forced step finishes nothing)
            fsc = top_lp / div_tab[(cur - plen_img).clamp(min=1)]
        full = fin_done.all(dim=1, keepdim=True) & (early_stopping is True)
        fsc = fsc + full.float() * NEG + (~unsat).float() * NEG + (~just).float() * NEG
        m_sc = torch.cat((fin_sc, fsc), dim=1)
        m_ix = m_sc.topk(nb, dim=1)[1]
        fin_seq = torch.cat((fin_seq, cand), dim=1).gather(1, m_ix.unsqueeze(-1).expand(B, nb, max_len))
        if fin_lp is not None:
            fin_lp = torch.cat((fin_lp, cand_lp), dim=1).gather(1, m_ix.unsqueeze(-1).expand(B, nb, max_len))
        fin_sc = m_sc.gather(1, m_ix)
        fin_done = torch.cat((fin_done, just), dim=1).gather(1, m_ix)
        fin_len = torch.cat((fin_len, torch.full((B, K), cur + 1, dtype=torch.int64, device=device)), dim=1).gather(1, m_ix)
        cur += 1
        # stop test (one host synchronisation per step)
        if plen_img is None:
            best_open = run_sc[:, :1] / float((cur - prompt) ** length_penalty)
        else:
            best_open = run_sc[:, :1] / div_tab[(cur - 1 - plen_img).clamp(min=1)]
        worst_fin = torch.where(fin_done, fin_sc.min(dim=1, keepdim=True)[0], torch.full_like(fin_sc, NEG))
        unsat = unsat & (best_open > worst_fin).any(dim=-1, keepdim=True)
        go_on = unsat.any() & ~(fin_done.all() & (early_stopping is True)) & ~hits.all()
        if not bool(go_on):
            break
        reorder(rows, cur - 1)
    if n_ret > 1 or return_logprobs:
        return nbest_result(fin_seq, fin_sc, fin_done, fin_len, fin_lp, n_ret, bos_id, pad_id)
    width = int(fin_len[:, 0].max())
    return fin_seq[:, 0, :width]


def beam_search_fused(step, reorder, batch, num_beams, max_len, vocab, pad_id, bos_id, eos_id, device, early_stopping, length_penalty,
                      topk, update, return_state=False, num_return_sequences: int = 1, return_logprobs: bool = False):
    """The same loop with the two device kernels: ``topk`` ranks the continuations, ``update(state, top_lp, top_ix, cur) -> (rows,
    flags)`` does everything beam_search does between two steps (state: dict of the tensors below; token rows double-buffered).
    One host synchronisation per step (the three counters of ``flags``).  ``num_return_sequences`` / ``return_logprobs``: as
    beam_search's; the log-probability rows run_lp / fin_lp join the state (double-buffered like the token rows) only when asked for."""
    import torch
    n_ret = _check_nbest(num_return_sequences, num_beams)
    B, nb = batch, num_beams
    st = {"run_seq": [torch.full((B, nb, max_len), pad_id, dtype=torch.int64, device=device) for _ in range(2)],
          "fin_seq": [torch.full((B, nb, max_len), pad_id, dtype=torch.int64, device=device) for _ in range(2)],
          "run_sc": torch.zeros(B, nb, device=device), "fin_sc": torch.full((B, nb), NEG, device=device),
          "fin_done": torch.zeros(B, nb, dtype=torch.uint8, device=device),
          "fin_len": torch.full((B, nb), 1, dtype=torch.int64, device=device),
          "unsat": torch.ones(B, dtype=torch.uint8, device=device), "cur_buf": 0}
    for t in st["run_seq"] + st["fin_seq"]:
        t[:, :, 0] = bos_id
    st["run_sc"][:, 1:] = NEG
    if return_logprobs:
        st["run_lp"] = [torch.zeros(B, nb, max_len, dtype=torch.float32, device=device) for _ in range(2)]
        st["fin_lp"] = [torch.zeros(B, nb, max_len, dtype=torch.float32, device=device) for _ in range(2)]
    cur = 1
    while True:
        raw = step(cur - 1, st["run_seq"][st["cur_buf"]].view(B * nb, max_len))
        top_lp, top_ix = topk(raw, st["run_sc"])
        rows, flags = update(st, top_lp, top_ix, cur)
        st["cur_buf"] ^= 1
        cur += 1
        # the stop test is taken on the device (flags[3]); the host looks every 4th step -- updates issued past the end are no-ops
        if (cur - 1) % 4 == 0 or cur >= max_len:
            f = flags.tolist()
            if f[3]:
                st["cur_buf"] = f[4] & 1                               # the buffers written by the last update that was applied
                break
        reorder(rows, cur - 1)
    fin_seq = st["fin_seq"][st["cur_buf"]]
    if n_ret > 1 or return_logprobs:
        out = nbest_result(fin_seq, st["fin_sc"], st["fin_done"], st["fin_len"], st["fin_lp"][st["cur_buf"]] if return_logprobs else None,
                           n_ret, bos_id, pad_id)
        return (out, st) if return_state else out
    width = int(st["fin_len"][:, 0].max())
    out = fin_seq[:, 0, :width]
    return (out, st) if return_state else out


def make_device_hooks(batch, num_beams, max_len, vocab, eos_id, early_stopping, length_penalty, device, logprobs: bool = False, prefix_len=None):
    """(topk, update) for beam_search on the GPU: kzv_beam_topk and kzv_beam_update through the C ABI, on the current stream,
    writing into buffers allocated here once.  ``logprobs``: the step hands over processed log-probabilities (the normalising
    kzv_logits_process has run on them), so ``topk`` is kzv_beam_rank_logprobs, which does not normalise again.
    ``prefix_len`` (int32 [batch] on the device, or None): the images carry forced prefixes (the step forces them: kzv_force_prefix), so
    ``update`` is kzv_beam_update_prefix -- every image's own generated length, beam_search's rule."""
    import ctypes as C
    import torch
    from . import _lib as L
    lib = L.load()
    B, nb = batch, num_beams
    top_lp = torch.empty(B, 2 * nb, dtype=torch.float32, device=device)
    top_ix = torch.empty(B, 2 * nb, dtype=torch.int64, device=device)
    rows_buf = torch.empty(B * nb, dtype=torch.int64, device=device)
    flags_buf = torch.zeros(5, dtype=torch.int32, device=device)
    keep = {}
    if prefix_len is not None:
        from .stream import divisor_table
        if prefix_len.dtype != torch.int32 or prefix_len.numel() != B or not prefix_len.is_contiguous():
            raise ValueError("prefix_len: a contiguous int32 tensor [batch]")
        div_tab = divisor_table(max_len, length_penalty, device).contiguous()

    def topk(raw, run_sc):                # log_softmax + beam score + top 2 * nb per image in one launch
        sc = run_sc.contiguous()
        keep["sc"] = sc
        rank = lib.kzv_beam_rank_logprobs if logprobs else lib.kzv_beam_topk
        L.check(rank(raw.data_ptr(), raw.stride(0), sc.data_ptr(), B, nb, vocab, 2 * nb, top_lp.data_ptr(), top_ix.data_ptr(),
                     L.stream_handle()), "beam_rank_logprobs" if logprobs else "beam_topk")
        return top_lp, top_ix

    def update(st, lp, ix, cur):          # everything between two decoder steps in one launch
        a = st["cur_buf"]
        lp_rows = {} if "run_lp" not in st else dict(run_lp_in=st["run_lp"][a].data_ptr(), run_lp_out=st["run_lp"][a ^ 1].data_ptr(),
                                                     fin_lp_in=st["fin_lp"][a].data_ptr(), fin_lp_out=st["fin_lp"][a ^ 1].data_ptr())
        bs = L.kzv_beam_state(batch=B, num_beams=nb, max_len=max_len, vocab=vocab, eos_id=eos_id,
                              run_seq_in=st["run_seq"][a].data_ptr(), run_seq_out=st["run_seq"][a ^ 1].data_ptr(),
                              fin_seq_in=st["fin_seq"][a].data_ptr(), fin_seq_out=st["fin_seq"][a ^ 1].data_ptr(),
                              run_scores=st["run_sc"].data_ptr(), fin_scores=st["fin_sc"].data_ptr(), fin_done=st["fin_done"].data_ptr(),
                              fin_len=st["fin_len"].data_ptr(), unsatisfied=st["unsat"].data_ptr(), **lp_rows)
        if prefix_len is not None:
            L.check(lib.kzv_beam_update_prefix(C.byref(bs), lp.data_ptr(), ix.data_ptr(), cur, 1 if early_stopping is True else 0, float(length_penalty),
                                               div_tab.data_ptr(), prefix_len.data_ptr(), rows_buf.data_ptr(), flags_buf.data_ptr(),
                                               L.stream_handle()), "beam_update_prefix")
            return rows_buf, flags_buf
        L.check(lib.kzv_beam_update(C.byref(bs), lp.data_ptr(), ix.data_ptr(), cur, 1 if early_stopping is True else 0, float(length_penalty),
                                    rows_buf.data_ptr(), flags_buf.data_ptr(), L.stream_handle()), "beam_update")
        return rows_buf, flags_buf

    return topk, update


def make_greedy_hook(batch, vocab, pad_id, eos_id, device, max_len=4096):
    """``update`` for greedy() on the GPU (kzv_greedy_update through the C ABI, current stream)."""
    import torch
    from . import _lib as L
    lib = L.load()
    flags = torch.zeros(max(2, int(max_len)), dtype=torch.int32, device=device)     # sequences still running after step t

    def update(logits, ids, t, done8):
        L.check(lib.kzv_greedy_update(logits.data_ptr(), logits.stride(0), vocab, ids.data_ptr(), ids.stride(0), t, done8.data_ptr(), batch,
                                      pad_id, eos_id, flags.data_ptr(), L.stream_handle()), "greedy_update")
        return flags

    return update
