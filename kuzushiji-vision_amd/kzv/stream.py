"""Slot-refill greedy decoding of many images: the bookkeeping, stated in torch tensor arithmetic.

``generate`` decodes a batch in lockstep: a batch runs until its longest line has ended, and a row that emitted EOS keeps its
decoder row busy writing padding.  Here a fixed set of decoder SLOTS works through N images: a slot holds one image at its own
step index, and the step after its line has ended it holds the next image that has no slot yet, at BOS.  Greedy decoding is
prefix-consistent and every decoder step is local to a sequence, so per image the tokens are those of the lockstep greedy
generation -- in fewer steps.

``select_seat(logits, state)`` is what happens between two decoder steps; ``greedy_stream`` is the loop around it.  Both run on
whatever device the tensors live on.  On the GPU the same thing is two kernels (csrc/token_search.hip: stream_select_kernel,
stream_seat_kernel through kzv_stream_update) which tests/test_stream_gpu.py pins against this module state for state.

State (a dict of tensors; out_ids / out_logprob are written in place, the others replaced):
  slot_image int32 [slots]   the image a slot holds, -1 = idle
  slot_t     int32 [slots]   the step index of that image (0 = its BOS is the decoder input)
  tokens     int64 [slots]   the next step's input token
  posids     int32 [slots]   its RoBERTa position id (step + 1 + pad_id: a greedy prefix holds no padding)
  counters   int32 [3]       next image without a slot, lines ended, steps taken while a line was open
  out_ids    int64 [N, L]    BOS, the tokens, EOS if emitted, then padding
  out_logprob fp32 [N, L]    optional: log-probability of out_ids[i][j] at [i][j] (0 at BOS and padding)
  alt_ids    int32 [N, L, k] optional (``top_k``): the k best tokens at [i][j], best first (kzv_stream_topk); -1 in columns never scored
  alt_logprob fp32 [N, L, k] optional: their log-probabilities; 0 in columns never scored
"""
from __future__ import annotations


def topk_rows(logits, k: int):
    """The k best columns of every row of ``logits`` [R, V] and their log-softmax values, best first: descending logit, ties by
    ascending column (a stable sort), so entry 0 is select_seat's token; where V < k the surplus entries are -1 / -inf
    (kzv_token_topk).  Returns (int32 [R, k], fp32 [R, k])."""
    import torch
    x = logits.float()
    R, V = x.shape
    order = torch.sort(x, dim=-1, descending=True, stable=True)[1][:, :k]
    lp = torch.log_softmax(x, dim=-1).gather(1, order)
    lp = torch.where(x.gather(1, order) == float("-inf"), torch.full_like(lp, float("-inf")), lp)      # (an all -inf row: not NaN)
    ids = order.to(torch.int32)
    if V < k:
        ids = torch.cat((ids, torch.full((R, k - V), -1, dtype=torch.int32, device=x.device)), dim=1)
        lp = torch.cat((lp, torch.full((R, k - V), float("-inf"), dtype=lp.dtype, device=x.device)), dim=1)
    return ids, lp


def new_state(n_images: int, slots: int, max_len: int, pad_id: int, bos_id: int, device, want_logprobs: bool = False, top_k: int = 0):
    """The state with the first min(slots, n_images) images seated in slot order (kzv_stream_seat_first).  ``top_k`` in 1..8 adds the
    alternatives (alt_ids / alt_logprob, -1 / 0 throughout)."""
    import torch
    if not 0 <= int(top_k) <= 8:
        raise ValueError("top_k must be in 0..8")
    s = torch.arange(slots, dtype=torch.int32, device=device)
    out_ids = torch.full((n_images, max_len), pad_id, dtype=torch.int64, device=device)
    out_ids[:, 0] = bos_id
    st = {
        "slot_image": torch.where(s < n_images, s, torch.full_like(s, -1)),
        "slot_t": torch.zeros(slots, dtype=torch.int32, device=device),
        "tokens": torch.full((slots,), bos_id, dtype=torch.int64, device=device),
        "posids": torch.full((slots,), pad_id + 1, dtype=torch.int32, device=device),
        "counters": torch.tensor([min(slots, n_images), 0, 0], dtype=torch.int32, device=device),
        "out_ids": out_ids,
        "out_logprob": torch.zeros(n_images, max_len, dtype=torch.float32, device=device) if want_logprobs else None,
    }
    if top_k:                                    # (the keys exist only when asked for)
        st["alt_ids"] = torch.full((n_images, max_len, int(top_k)), -1, dtype=torch.int32, device=device)
        st["alt_logprob"] = torch.zeros(n_images, max_len, int(top_k), dtype=torch.float32, device=device)
    return st


def _slot_prefix(prefix, i64, device):
    """``prefix`` = (ids [N, P], lengths [N]) per image -> the tables of the images the slots hold: (ids [S, P], lengths int64 [S])."""
    pfx, plen = prefix
    return pfx.to(device).long()[i64], plen.to(device).long().reshape(-1)[i64]


def select_seat(logits, st, *, n_images: int, max_len: int, pad_id: int, bos_id: int, eos_id: int, limit=None, process=None, prefix=None):
    """One step's selection and seating.  ``logits`` [slots, V] are the next-token logits of every slot (rows of idle slots are
    ignored).  Per live slot holding image i at step t: token = the FIRST arg-max column; out_ids[i][t + 1] = token;
    out_logprob[i][t + 1] = max - logsumexp; the line has ended when token == eos_id, t + 2 >= limit[i] or t + 2 >= max_len.
    Then the slots whose lines ended take the images counters[0], counters[0] + 1, ... in ascending slot order (an exclusive prefix
    sum over the ended flags) at step 0 / BOS, or go idle when no image is left; the others advance.  ``limit``: optional int32
    [n_images], the most tokens, BOS included, an image may get.  Where the state holds alternatives (new_state's ``top_k``),
    alt_ids / alt_logprob[i][t + 1] = topk_rows of the slot's row.
    ``process(logits, hist [slots, L], lens [slots], live [slots]) -> logits`` (optional; kzv/controls.py: GenerationControls.rows_hook):
    generation controls on the raw logits, slot s with the history out_ids[slot_image[s]][:slot_t[s] + 1]; token, log-probability and
    alternatives are then those of the processed row.  None: what this computed before.
    ``prefix`` = (ids [n_images, P], lengths [n_images]) (optional; kzv/prefix.py): forced prefixes per IMAGE.  A live slot whose chosen
    index slot_t + 1 lies inside its image's prefix gets force_reference's row after ``process``; a reseated slot reads its new image's
    prefix from step 0.  Returns ``st``."""
    import torch
    dev = logits.device
    img, t = st["slot_image"], st["slot_t"]
    live = img >= 0
    x = logits.float()
    if process is not None:
        x = process(x, st["out_ids"][img.clamp(min=0).long()], t.long() + 1, live)
    if prefix is not None:
        from . import prefix as PF
        pfx_s, plen_s = _slot_prefix(prefix, img.clamp(min=0).long(), dev)
        x = PF.force_reference(x, t.long() + 1, pfx_s, torch.where(live, plen_s, torch.zeros_like(plen_s)))
    mx = x.max(dim=-1, keepdim=True)[0]
    V = x.shape[-1]
    cols = torch.arange(V, device=dev).expand_as(x)
    tok = torch.where(x == mx, cols, torch.full_like(cols, V)).min(dim=-1)[0]          # first maximum, on every device
    lp = mx[:, 0] - torch.logsumexp(x, dim=-1)
    i64 = img.clamp(min=0).long()
    lim = torch.full_like(t, max_len) if limit is None else limit.to(dev, dtype=torch.int32)[i64].clamp(max=max_len)
    ended = live & ((tok == eos_id) | (t + 2 >= lim))
    rows, colsw = i64[live], t[live].long() + 1
    st["out_ids"][rows, colsw] = tok[live]
    if st.get("out_logprob") is not None:
        st["out_logprob"][rows, colsw] = lp[live]
    if st.get("alt_ids") is not None:
        a_ids, a_lp = topk_rows(x[live], st["alt_ids"].shape[-1])
        st["alt_ids"][rows, colsw] = a_ids
        st["alt_logprob"][rows, colsw] = a_lp
    e32 = ended.to(torch.int32)
    n_ended = e32.sum().to(torch.int32)
    nxt = st["counters"][0]
    cand = nxt + torch.cumsum(e32, 0).to(torch.int32) - e32                                # the image an ended slot would take
    seated = torch.where(cand < n_images, cand, torch.full_like(cand, -1))
    go_on = live & ~ended
    st["slot_image"] = torch.where(ended, seated, img)
    st["slot_t"] = torch.where(ended, torch.zeros_like(t), torch.where(go_on, t + 1, t))
    st["tokens"] = torch.where(ended, torch.full_like(tok, bos_id), torch.where(go_on, tok, st["tokens"]))
    st["posids"] = torch.where(ended, torch.full_like(t, pad_id + 1), torch.where(go_on, t + 2 + pad_id, st["posids"]))
    c = st["counters"]
    # steps count the steps that had a line to work on: what the host issues past the end (it looks only every few steps) changes nothing
    st["counters"] = torch.stack((torch.clamp(c[0] + n_ended, max=n_images), c[1] + n_ended, c[2] + (c[1] < n_images))).to(torch.int32)
    return st


def step_bound(n_images: int, slots: int, max_len: int) -> int:
    """The most steps a wave can take: a line takes at most max_len - 1 steps and a slot is never idle while an image waits, so
    (list scheduling) the last line ends within ceil(N / slots) * (max_len - 1) steps of work per slot plus one line."""
    return (-(-n_images // slots) + 1) * (max_len - 1)


def greedy_stream(step_fn, n_images: int, slots: int, max_len: int, pad_id: int, bos_id: int, eos_id: int, device, limits=None,
                  return_logprobs: bool = False, poll: int = 8, return_state: bool = False, top_k: int = 0, process=None, prefix=None):
    """Greedy decoding of ``n_images`` images over ``slots`` decoder slots.  ``step_fn(state) -> logits [slots, V]`` runs one decoder
    step for every slot: slot b feeds state["tokens"][b] at step state["slot_t"][b] for image state["slot_image"][b] (idle slots may
    return anything).  The counters are looked at every ``poll``-th step; RuntimeError once the steps exceed ``step_bound``.
    Returns out_ids [N, max_len] (and out_logprob with ``return_logprobs``; and the final state with ``return_state``, which holds
    the alternatives asked for with ``top_k``).  ``process`` / ``prefix``: select_seat's optional hook and forced prefixes."""
    import torch
    st = new_state(n_images, slots, max_len, pad_id, bos_id, device, return_logprobs, top_k)
    lim = None if limits is None else torch.as_tensor(limits, dtype=torch.int32, device=device)
    bound = step_bound(n_images, slots, max_len)
    steps = 0
    while True:
        st = select_seat(step_fn(st), st, n_images=n_images, max_len=max_len, pad_id=pad_id, bos_id=bos_id, eos_id=eos_id, limit=lim,
                         process=process, prefix=prefix)
        steps += 1
        if steps % poll == 0 or steps >= bound:
            if int(st["counters"][1]) >= n_images:
                break
            if steps >= bound:
                raise RuntimeError(f"greedy_stream: {steps} steps for {n_images} images over {slots} slots exceed the bound {bound}")
    out = (st["out_ids"], st["out_logprob"]) if return_logprobs else st["out_ids"]
    return (out, st) if return_state else out


# ---- beam search on device-refilled slots ------------------------------------------------------------------------------------------------
# A slot holds an image's whole beam GROUP (nb decoder rows slot * nb .. slot * nb + nb - 1) at its own step index; the step after the
# image's search has ended the slot holds the next image that has no slot yet.  Beam search is independent per image, so per image the
# result is that of beam.beam_search run on it alone.  ``beam_select_seat`` is what happens between two decoder steps once the 2 * nb
# best continuations of every slot are ranked (kzv_beam_topk); ``beam_stream`` is the loop around it.  On the GPU the same thing is
# csrc/token_search.hip: stream_beam_update_kernel, stream_beam_seat_kernel (kzv_stream_beam_update), pinned against this state for state.
#
# State, beyond slot_image / slot_t [slots] as above:
#   tokens int64, posids int32 [slots * nb]    the next step's input of every beam row
#   run_seq, fin_seq int64 [slots, nb, L]      running / finished token rows; columns past a slot's step hold an EARLIER image's tokens
#                                              after a reseat and are never read (never cleared either)
#   run_sc, fin_sc fp32 [slots, nb]; fin_done u8, fin_len int64 [slots, nb]; unsat u8 [slots]       as in beam.beam_search
#   counters int32 [4]    next image without a slot, searches ended, steps taken while a search was open, running continuations that
#                         took pad_id (a prefix with padding breaks "position = step + 1 + pad_id, every cached key usable")
#   out_ids int64 [N, L]  BOS, the best finished hypothesis, then padding;  out_score fp32 [N]: its score (HF sequences_scores)
#   rowtab int32 [slots * nb, ld] (optional): the beam row table the step kernel reads; re-parented in place
#   run_lp, fin_lp fp32 [slots, nb, L] (optional, ``want_logprobs``): the per-token log-probabilities of the token rows, the fp32 difference
#                         top_lp[k] - run_sc[src[k]] at cur, moved through exactly the gathers of run_seq / fin_seq (beam.beam_search)
#   nbest_ids int64 [N * n, L], nbest_score fp32 [N * n], nbest_len int32 [N * n], nbest_logprob fp32 [N * n, L] (optional, ``n_best`` = n):
#                         rows 0 .. n - 1 of an image's finished list when its search ends, image-major, best first; only the row's
#                         length is written over BOS + padding / zeros; an entry that is not done: nothing, score -1e9, length 0
NEG = -1.0e9


def divisor_table(max_len: int, length_penalty: float, device="cpu"):
    """fp32 [max_len + 1]: entry n = float(n ** length_penalty) computed in double, rounded once (what beam_search divides by at
    generated length n); entry 0 is 1 and never used."""
    import torch
    return torch.tensor([1.0] + [float(n ** length_penalty) for n in range(1, max_len + 1)], dtype=torch.float64).to(torch.float32).to(device)


def new_beam_state(n_images: int, slots: int, num_beams: int, max_len: int, pad_id: int, bos_id: int, device, want_scores: bool = True,
                   rowtab_ld: int = 0, n_best: int = 0, want_logprobs: bool = False):
    """The state with the first min(slots, n_images) images seated in slot order (kzv_stream_beam_seat_first).  ``n_best`` in
    1..num_beams adds the n-best outputs, ``want_logprobs`` (needs n_best) the log-probability rows and their output; the keys exist
    only when asked for."""
    import torch
    nb = num_beams
    n_best = int(n_best)
    if not 0 <= n_best <= nb:
        raise ValueError(f"n_best must be in 1..num_beams = {nb} (got {n_best})")
    if want_logprobs and not n_best:
        raise ValueError("want_logprobs needs n_best >= 1 (the log-probability rows leave through the n-best outputs)")
    s = torch.arange(slots, dtype=torch.int32, device=device)
    out_ids = torch.full((n_images, max_len), pad_id, dtype=torch.int64, device=device)
    out_ids[:, 0] = bos_id
    run_seq = torch.full((slots, nb, max_len), pad_id, dtype=torch.int64, device=device)
    run_seq[:, :, 0] = bos_id
    run_sc = torch.zeros(slots, nb, device=device)
    run_sc[:, 1:] = NEG
    extra = {}
    if n_best:
        nbest_ids = torch.full((n_images * n_best, max_len), pad_id, dtype=torch.int64, device=device)
        nbest_ids[:, 0] = bos_id
        extra = {"nbest_ids": nbest_ids, "nbest_score": torch.zeros(n_images * n_best, dtype=torch.float32, device=device),
                 "nbest_len": torch.zeros(n_images * n_best, dtype=torch.int32, device=device)}
        if want_logprobs:
            extra["run_lp"] = torch.zeros(slots, nb, max_len, dtype=torch.float32, device=device)
            extra["fin_lp"] = torch.zeros(slots, nb, max_len, dtype=torch.float32, device=device)
            extra["nbest_logprob"] = torch.zeros(n_images * n_best, max_len, dtype=torch.float32, device=device)
    return {
        **extra,
        "slot_image": torch.where(s < n_images, s, torch.full_like(s, -1)),
        "slot_t": torch.zeros(slots, dtype=torch.int32, device=device),
        "tokens": torch.full((slots * nb,), bos_id, dtype=torch.int64, device=device),
        "posids": torch.full((slots * nb,), pad_id + 1, dtype=torch.int32, device=device),
        "run_seq": run_seq, "fin_seq": run_seq.clone(),
        "run_sc": run_sc, "fin_sc": torch.full((slots, nb), NEG, device=device),
        "fin_done": torch.zeros(slots, nb, dtype=torch.uint8, device=device),
        "fin_len": torch.ones(slots, nb, dtype=torch.int64, device=device),
        "unsat": torch.ones(slots, dtype=torch.uint8, device=device),
        "counters": torch.tensor([min(slots, n_images), 0, 0, 0], dtype=torch.int32, device=device),
        "out_ids": out_ids,
        "out_score": torch.zeros(n_images, dtype=torch.float32, device=device) if want_scores else None,
        "rowtab": torch.zeros(slots * nb, rowtab_ld, dtype=torch.int32, device=device) if rowtab_ld else None,
    }


def beam_select_seat(top_lp, top_ix, st, *, n_images: int, num_beams: int, max_len: int, vocab: int, pad_id: int, bos_id: int, eos_id: int,
                     early_stopping=True, length_penalty: float = 1.0, limit=None, divisors=None, prefix_len=None):
    """One step's beam bookkeeping and seating.  ``top_lp`` / ``top_ix`` [slots, 2 nb]: the ranked continuations of every slot (flat
    index beam * vocab + token; rows of idle slots are ignored).  A live slot holding image i at cur = slot_t + 1 does the body of
    beam.beam_search's loop for B = 1 with max_len = min(limit[i], max_len); equal scores rank by the smaller index (a stable sort:
    what the kernel's scalar ranking does).  The search has ended when beam_search's ``go_on`` is false for that image: then
    out_ids[i] = fin_seq[0][:fin_len[0]] and out_score[i] = fin_sc[0], and the slot is seated as in select_seat, its beam state back
    at the start.
    ``prefix_len`` [n_images] (optional): the images carry forced prefixes (the ranking was taken on forced rows), so the divisor of a
    slot holding image i is that of its own generated length max(cur - prefix_len[i], 1) -- beam.beam_search's rule, clamp included.
    Returns ``st``."""
    import torch
    dev = top_lp.device
    nb, K, L, V = num_beams, 2 * num_beams, max_len, vocab
    S = st["slot_image"].numel()
    img, t = st["slot_image"], st["slot_t"]
    live = img >= 0
    i64 = img.clamp(min=0).long()
    cur = (t.long() + 1).clamp(max=L - 1)                                                  # [S]
    lim = torch.full_like(t, L) if limit is None else limit.to(dev, dtype=torch.int32)[i64].clamp(max=L)
    div = divisor_table(L, length_penalty, dev) if divisors is None else divisors
    gen = cur if prefix_len is None else (cur - prefix_len.to(dev).long().reshape(-1)[i64]).clamp(min=1)
    d = div[gen].view(S, 1)                                                                # (cur + 1 - prompt) ** length_penalty, as fp32
    run_seq, fin_seq, run_sc, fin_sc = st["run_seq"], st["fin_seq"], st["run_sc"], st["fin_sc"]
    fin_done, fin_len, unsat = st["fin_done"].bool(), st["fin_len"], st["unsat"].bool().view(S, 1)
    top_lp = top_lp.float()
    src, tok = top_ix // V, top_ix % V
    cand = run_seq.gather(1, src.unsqueeze(-1).expand(S, K, L)).clone()
    cand.scatter_(2, cur.view(S, 1, 1).expand(S, K, 1), tok.unsqueeze(-1))
    hits = (tok == eos_id) | (cur + 1 >= lim.long()).view(S, 1)
    # running beams of the next step: the best nb continuations that did not stop
    s2 = top_lp + hits.float() * NEG
    nxt_ix = torch.sort(s2, dim=1, descending=True, stable=True)[1][:, :nb]
    n_run_seq = cand.gather(1, nxt_ix.unsqueeze(-1).expand(S, nb, L))
    run_lp, fin_lp = st.get("run_lp"), st.get("fin_lp")
    if run_lp is not None:                                                                 # the token's own log-probability, from the OLD running scores
        cand_lp = run_lp.gather(1, src.unsqueeze(-1).expand(S, K, L)).clone()
        cand_lp.scatter_(2, cur.view(S, 1, 1).expand(S, K, 1), (top_lp - run_sc.gather(1, src)).unsqueeze(-1))
        n_run_lp = cand_lp.gather(1, nxt_ix.unsqueeze(-1).expand(S, nb, L))
    n_run_sc = s2.gather(1, nxt_ix)
    parent = src.gather(1, nxt_ix)                                                         # [S, nb]: the beam of the slot each one continues
    n_tok = tok.gather(1, nxt_ix)
    took_pad = (n_tok == pad_id) & ~hits.gather(1, nxt_ix)
    # finished list: stopped continuations of rank < nb, normalised by the generated length
    top_mask = (torch.arange(K, device=dev) < nb).view(1, K)
    just = hits & top_mask
    full = fin_done.all(dim=1, keepdim=True) & (early_stopping is True)
    fsc = top_lp / d
    fsc = fsc + full.float() * NEG + (~unsat).float() * NEG + (~just).float() * NEG
    m_sc = torch.cat((fin_sc, fsc), dim=1)
    m_ix = torch.sort(m_sc, dim=1, descending=True, stable=True)[1][:, :nb]
    n_fin_seq = torch.cat((fin_seq, cand), dim=1).gather(1, m_ix.unsqueeze(-1).expand(S, nb, L))
    if run_lp is not None:
        n_fin_lp = torch.cat((fin_lp, cand_lp), dim=1).gather(1, m_ix.unsqueeze(-1).expand(S, nb, L))
    n_fin_sc = m_sc.gather(1, m_ix)
    n_fin_done = torch.cat((fin_done, just), dim=1).gather(1, m_ix)
    n_fin_len = torch.cat((fin_len, (cur + 1).view(S, 1).expand(S, K)), dim=1).gather(1, m_ix)
    best_open = n_run_sc[:, :1] / d
    worst_fin = torch.where(n_fin_done, n_fin_sc.min(dim=1, keepdim=True)[0], torch.full_like(n_fin_sc, NEG))
    n_unsat = unsat & (best_open > worst_fin).any(dim=-1, keepdim=True)
    go_on = n_unsat[:, 0] & ~(n_fin_done.all(dim=1) & (early_stopping is True)) & ~hits.all(dim=1)
    ended = live & ~go_on
    go_on = live & go_on
    # the ended searches' results: only fin_len[0] tokens are written (what lies behind them in fin_seq may be another image's)
    rows = i64[ended]
    if rows.numel():
        col = torch.arange(L, device=dev).view(1, L)
        keep = col < n_fin_len[ended][:, :1]
        st["out_ids"][rows] = torch.where(keep, n_fin_seq[ended][:, 0], torch.full_like(n_fin_seq[ended][:, 0], pad_id))
        if st.get("out_score") is not None:
            st["out_score"][rows] = n_fin_sc[ended][:, 0]
        if st.get("nbest_ids") is not None:            # rows 0 .. n - 1 of the finished list, each over its own length only
            n = st["nbest_ids"].shape[0] // n_images
            e_done = n_fin_done[ended][:, :n]
            e_len = torch.where(e_done, n_fin_len[ended][:, :n], torch.zeros_like(n_fin_len[ended][:, :n]))              # [E, n]
            keep_n = (col.view(1, 1, L) < e_len.unsqueeze(-1)).reshape(-1, L)
            dst = (rows.view(-1, 1) * n + torch.arange(n, device=dev).view(1, n)).reshape(-1)
            st["nbest_ids"][dst] = torch.where(keep_n, n_fin_seq[ended][:, :n].reshape(-1, L), st["nbest_ids"][dst])
            st["nbest_score"][dst] = torch.where(e_done, n_fin_sc[ended][:, :n], torch.full_like(n_fin_sc[ended][:, :n], NEG)).reshape(-1)
            st["nbest_len"][dst] = e_len.reshape(-1).to(torch.int32)
            if st.get("nbest_logprob") is not None:
                st["nbest_logprob"][dst] = torch.where(keep_n, n_fin_lp[ended][:, :n].reshape(-1, L), st["nbest_logprob"][dst])
    # seats: the slots whose searches ended take the next images in ascending slot order
    e32 = ended.to(torch.int32)
    n_ended = e32.sum().to(torch.int32)
    c = st["counters"]
    cand_img = c[0] + torch.cumsum(e32, 0).to(torch.int32) - e32
    seated = torch.where(cand_img < n_images, cand_img, torch.full_like(cand_img, -1))
    g1, g2, g3 = go_on.view(S, 1), go_on.view(S, 1, 1), ended.view(S, 1)
    first = (torch.arange(nb, device=dev) == 0).view(1, nb)
    st["run_seq"] = torch.where(g2, n_run_seq, run_seq)
    st["fin_seq"] = torch.where(g2, n_fin_seq, fin_seq)
    if run_lp is not None:
        st["run_lp"] = torch.where(g2, n_run_lp, run_lp)
        st["fin_lp"] = torch.where(g2, n_fin_lp, fin_lp)
    st["run_sc"] = torch.where(g3, torch.where(first, torch.zeros_like(run_sc), torch.full_like(run_sc, NEG)), torch.where(g1, n_run_sc, run_sc))
    st["fin_sc"] = torch.where(g3, torch.full_like(fin_sc, NEG), torch.where(g1, n_fin_sc, fin_sc))
    st["fin_done"] = torch.where(g3, torch.zeros_like(fin_done), torch.where(g1, n_fin_done, fin_done)).to(torch.uint8)
    st["fin_len"] = torch.where(g3, torch.ones_like(fin_len), torch.where(g1, n_fin_len, fin_len))
    st["unsat"] = torch.where(ended, torch.ones_like(ended), torch.where(go_on, n_unsat[:, 0], unsat[:, 0])).to(torch.uint8)
    if st.get("rowtab") is not None:                       # new[i][j] = old[parent_i][j] for j <= slot_t (the step wrote old[b][slot_t] = b)
        rt = st["rowtab"]
        ld = rt.shape[1]
        old = rt.view(S, nb, ld)
        moved = old.gather(1, parent.unsqueeze(-1).expand(S, nb, ld))
        upto = (torch.arange(ld, device=dev).view(1, 1, ld) <= t.view(S, 1, 1)) & g2
        st["rowtab"] = torch.where(upto, moved, old).view(S * nb, ld).contiguous()
    tk, ps = st["tokens"].view(S, nb), st["posids"].view(S, nb)
    st["tokens"] = torch.where(g3, torch.full_like(tk, bos_id), torch.where(g1, n_tok, tk)).reshape(-1)
    st["posids"] = torch.where(g3, torch.full_like(ps, pad_id + 1), torch.where(g1, (cur + 1 + pad_id).to(torch.int32).view(S, 1).expand(S, nb), ps)).reshape(-1)
    st["slot_image"] = torch.where(ended, seated, img)
    st["slot_t"] = torch.where(ended, torch.zeros_like(t), torch.where(go_on, t + 1, t))
    n_pad = (took_pad & g1).sum().to(torch.int32)
    st["counters"] = torch.stack((torch.clamp(c[0] + n_ended, max=n_images), c[1] + n_ended, c[2] + (c[1] < n_images), c[3] + n_pad)).to(torch.int32)
    return st


def beam_stream(step_fn, n_images: int, slots: int, num_beams: int, max_len: int, vocab: int, pad_id: int, bos_id: int, eos_id: int, device,
                early_stopping=True, length_penalty: float = 1.0, limits=None, topk=None, poll: int = 8, return_state: bool = False,
                process=None, num_return_sequences: int = 1, return_logprobs: bool = False, prefix=None):
    """Beam search of ``n_images`` images over ``slots`` slots of ``num_beams`` decoder rows.  ``step_fn(state) -> logits [slots * nb, V]``
    runs one decoder step for every row: row slot * nb + i feeds state["tokens"][row] at step state["slot_t"][slot] for image
    state["slot_image"][slot], its prefix state["run_seq"][slot][i][:slot_t + 1] (idle slots may return anything finite).
    ``topk(logits, run_sc) -> (top_lp, top_ix)``: optional fused ranking as in beam.beam_search.  Returns (out_ids [N, max_len],
    out_score [N]) (and the final state with ``return_state``).
    ``process(logp, hist [slots * nb, L], lens [slots * nb], live [slots * nb]) -> logp`` (optional; GenerationControls.rows_hook):
    generation controls on ``log_softmax(logits)``, row slot * nb + i with the history run_seq[slot][i][:slot_t[slot] + 1], before the
    beam score is added and with no second normalisation.  It belongs to the torch ranking (not combined with ``topk``).  None: what
    this computed before.
    ``num_return_sequences`` n in 1..num_beams / ``return_logprobs``: with n > 1 or log-probabilities asked for, the result is
    beam.nbest_result's dict instead (ids [N * n, width], scores, lengths, logprobs: image-major, best first), read off the n-best
    outputs that every ended search wrote; per image it equals beam.beam_search's with the same two keywords.
    ``prefix`` = (ids [n_images, P], lengths [n_images]) (optional): forced prefixes per image, beam.beam_search's keyword; the torch
    ranking forces the rows after ``process`` (with ``topk`` the caller forces inside ``step_fn``), and the lengths go to
    beam_select_seat."""
    import torch
    if process is not None and topk is not None:
        raise ValueError("beam_stream: `process` belongs to the torch ranking")
    nb, K = num_beams, 2 * num_beams
    n_ret = int(num_return_sequences)
    if not 1 <= n_ret <= nb:
        raise ValueError(f"num_return_sequences must be in 1..num_beams = {nb} (got {n_ret})")
    n_best = n_ret if (n_ret > 1 or return_logprobs) else 0
    st = new_beam_state(n_images, slots, nb, max_len, pad_id, bos_id, device, n_best=n_best, want_logprobs=bool(return_logprobs))
    lim = None if limits is None else torch.as_tensor(limits, dtype=torch.int32, device=device)
    div = divisor_table(max_len, length_penalty, device)
    bound = step_bound(n_images, slots, max_len)
    steps = 0
    while True:
        raw = step_fn(st)
        if topk is not None:
            top_lp, top_ix = topk(raw, st["run_sc"])
        else:
            logp = torch.log_softmax(raw.float(), dim=-1)
            if process is not None:
                logp = process(logp, st["run_seq"].view(slots * nb, max_len), (st["slot_t"].long() + 1).repeat_interleave(nb),
                               (st["slot_image"] >= 0).repeat_interleave(nb))
            if prefix is not None:
                from . import prefix as PF
                live = st["slot_image"] >= 0
                pfx_s, plen_s = _slot_prefix(prefix, st["slot_image"].clamp(min=0).long(), logp.device)
                logp = PF.force_reference(logp, (st["slot_t"].long() + 1).repeat_interleave(nb), pfx_s.repeat_interleave(nb, dim=0),
                                          torch.where(live, plen_s, torch.zeros_like(plen_s)).repeat_interleave(nb))
            acc = logp.view(slots, nb, vocab) + st["run_sc"].unsqueeze(-1)
            top_lp, top_ix = acc.view(slots, nb * vocab).topk(K, dim=1)
        st = beam_select_seat(top_lp, top_ix, st, n_images=n_images, num_beams=nb, max_len=max_len, vocab=vocab, pad_id=pad_id, bos_id=bos_id,
                              eos_id=eos_id, early_stopping=early_stopping, length_penalty=length_penalty, limit=lim, divisors=div,
                              prefix_len=None if prefix is None else prefix[1])
        steps += 1
        if steps % poll == 0 or steps >= bound:
            if int(st["counters"][1]) >= n_images:
                break
            if steps >= bound:
                raise RuntimeError(f"beam_stream: {steps} steps for {n_images} images over {slots} slots exceed the bound {bound}")
    out = (st["out_ids"], st["out_score"])
    if n_best:
        out = nbest_outputs(st["nbest_ids"], st["nbest_score"], st["nbest_len"], st.get("nbest_logprob"))
    return (out, st) if return_state else out


def nbest_outputs(nbest_ids, nbest_score, nbest_len, nbest_logprob=None):
    """The n-best outputs of a wave as beam.nbest_result's dict: cropped to the longest row (at least 2 columns)."""
    width = max(2, int(nbest_len.max()))
    out = {"ids": nbest_ids[:, :width], "scores": nbest_score, "lengths": nbest_len.long()}
    if nbest_logprob is not None:
        out["logprobs"] = nbest_logprob[:, :width]
    return out
