"""Slot-refill greedy decoding of many images: the bookkeeping, stated in torch tensor arithmetic.

``generate`` decodes a batch in lockstep: a batch runs until its longest line has ended, and a row that emitted EOS keeps its
decoder row busy writing padding.  Here a fixed set of decoder SLOTS works through N images: a slot holds one image at its own
step index, and the step after its line has ended it holds the next image that has no slot yet, at BOS.  Greedy decoding is
prefix-consistent and every decoder step is local to a sequence, so per image the tokens are those of the lockstep greedy
generation -- in fewer steps.

``select_seat(logits, state)`` is what happens between two decoder steps; ``greedy_stream`` is the loop around it.  Both run on
whatever device the tensors live on.  On the GPU the same thing is two kernels (csrc/decode.hip: stream_select_kernel,
stream_seat_kernel through kzv_stream_update) which tests/test_stream_gpu.py pins against this module state for state.

State (a dict of tensors; out_ids / out_logprob are written in place, the others replaced):
  slot_image int32 [slots]   the image a slot holds, -1 = idle
  slot_t     int32 [slots]   the step index of that image (0 = its BOS is the decoder input)
  tokens     int64 [slots]   the next step's input token
  posids     int32 [slots]   its RoBERTa position id (step + 1 + pad_id: a greedy prefix holds no padding)
  counters   int32 [3]       next image without a slot, lines ended, steps taken while a line was open
  out_ids    int64 [N, L]    BOS, the tokens, EOS if emitted, then padding
  out_logprob fp32 [N, L]    optional: log-probability of out_ids[i][j] at [i][j] (0 at BOS and padding)
"""
from __future__ import annotations


def new_state(n_images: int, slots: int, max_len: int, pad_id: int, bos_id: int, device, want_logprobs: bool = False):
    """The state with the first min(slots, n_images) images seated in slot order (kzv_stream_seat_first)."""
    import torch
    s = torch.arange(slots, dtype=torch.int32, device=device)
    out_ids = torch.full((n_images, max_len), pad_id, dtype=torch.int64, device=device)
    out_ids[:, 0] = bos_id
    return {
        "slot_image": torch.where(s < n_images, s, torch.full_like(s, -1)),
        "slot_t": torch.zeros(slots, dtype=torch.int32, device=device),
        "tokens": torch.full((slots,), bos_id, dtype=torch.int64, device=device),
        "posids": torch.full((slots,), pad_id + 1, dtype=torch.int32, device=device),
        "counters": torch.tensor([min(slots, n_images), 0, 0], dtype=torch.int32, device=device),
        "out_ids": out_ids,
        "out_logprob": torch.zeros(n_images, max_len, dtype=torch.float32, device=device) if want_logprobs else None,
    }


def select_seat(logits, st, *, n_images: int, max_len: int, pad_id: int, bos_id: int, eos_id: int, limit=None):
    """One step's selection and seating.  ``logits`` [slots, V] are the next-token logits of every slot (rows of idle slots are
    ignored).  Per live slot holding image i at step t: token = the FIRST arg-max column; out_ids[i][t + 1] = token;
    out_logprob[i][t + 1] = max - logsumexp; the line has ended when token == eos_id, t + 2 >= limit[i] or t + 2 >= max_len.
    Then the slots whose lines ended take the images counters[0], counters[0] + 1, ... in ascending slot order (an exclusive prefix
    sum over the ended flags) at step 0 / BOS, or go idle when no image is left; the others advance.  ``limit``: optional int32
    [n_images], the most tokens, BOS included, an image may get.  Returns ``st``."""
    import torch
    dev = logits.device
    img, t = st["slot_image"], st["slot_t"]
    live = img >= 0
    x = logits.float()
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
                  return_logprobs: bool = False, poll: int = 8, return_state: bool = False):
    """Greedy decoding of ``n_images`` images over ``slots`` decoder slots.  ``step_fn(state) -> logits [slots, V]`` runs one decoder
    step for every slot: slot b feeds state["tokens"][b] at step state["slot_t"][b] for image state["slot_image"][b] (idle slots may
    return anything).  The counters are looked at every ``poll``-th step; RuntimeError once the steps exceed ``step_bound``.
    Returns out_ids [N, max_len] (and out_logprob with ``return_logprobs``; and the final state with ``return_state``)."""
    import torch
    st = new_state(n_images, slots, max_len, pad_id, bos_id, device, return_logprobs)
    lim = None if limits is None else torch.as_tensor(limits, dtype=torch.int32, device=device)
    bound = step_bound(n_images, slots, max_len)
    steps = 0
    while True:
        st = select_seat(step_fn(st), st, n_images=n_images, max_len=max_len, pad_id=pad_id, bos_id=bos_id, eos_id=eos_id, limit=lim)
        steps += 1
        if steps % poll == 0 or steps >= bound:
            if int(st["counters"][1]) >= n_images:
                break
            if steps >= bound:
                raise RuntimeError(f"greedy_stream: {steps} steps for {n_images} images over {slots} slots exceed the bound {bound}")
    out = (st["out_ids"], st["out_logprob"]) if return_logprobs else st["out_ids"]
    return (out, st) if return_state else out
