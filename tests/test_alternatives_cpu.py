"""Top-k character alternatives, the parts that need no GPU:

  * align.build_records(..., alternatives=(alt_ids, alt_logprob)) on hand-made arrays: a row ending in EOS, a row cut by PAD, a BOS
    past column 0 (scored, not reported), -1 entries dropped, margins = first minus second log-probability (inf with one candidate),
    and without the keyword the record of before, key for key;
  * stream.select_seat with alternatives (stream.new_state(top_k=...)) on a 3-slot, 7-image run over 11 columns with planted ties:
    alternative 0 is the emitted token at every written column with out_logprob's value, ranks follow (descending logit, ascending
    column), columns never scored keep -1 / 0, and every other state tensor equals the run without alternatives."""
import math

import numpy as np
import pytest
import torch

from kzv import align as A
from kzv import stream as ST

PAD, BOS, EOS = 1, 2, 3


def _arrays():
    # row 0 ends in EOS; row 1 is cut by PAD; row 2 holds a BOS past column 0 and runs to the last column
    ids = np.array([[BOS, 5, 6, EOS, PAD, PAD],
                    [BOS, 7, 8, PAD, PAD, PAD],
                    [BOS, 9, BOS, 10, 4, 6]], dtype=np.int64)
    B, L = ids.shape
    lp = -0.1 * (1 + np.arange(B * (L - 1), dtype=np.float64).reshape(B, L - 1))
    cent = np.arange(B * (L - 1) * 2, dtype=np.float64).reshape(B, L - 1, 2)
    peak = np.arange(B * (L - 1)).reshape(B, L - 1)
    k = 3
    alt_ids = np.full((B, L - 1, k), -1, dtype=np.int64)
    alt_lp = np.zeros((B, L - 1, k), dtype=np.float32)
    for b in range(B):
        for t in range(L - 1):
            alt_ids[b, t] = [ids[b, t + 1], 20 + t, 30 + t]
            alt_lp[b, t] = [lp[b, t], lp[b, t] - 0.5 - t, lp[b, t] - 2.0 - t]
    alt_ids[0, 1, 2] = -1                                    # two candidates
    alt_ids[1, 0, 1:] = -1                                   # a single candidate
    alt_lp[1, 0, 1:] = -np.inf
    alt_ids[2, 3] = [11, 4, -1]                              # the chosen token is second (a beam search's teacher-forced pass)
    return ids, lp, cent, peak, alt_ids, alt_lp


def test_build_records_with_alternatives():
    ids, lp, cent, peak, alt_ids, alt_lp = _arrays()
    strings = lambda toks: [f"<{t}>" for t in toks]
    base = A.build_records(ids, lp, cent, peak, pad_id=PAD, bos_id=BOS, eos_id=EOS, texts=["a", "b", "c"], to_strings=strings)
    recs = A.build_records(ids, lp, cent, peak, pad_id=PAD, bos_id=BOS, eos_id=EOS, texts=["a", "b", "c"], to_strings=strings,
                           alternatives=(alt_ids, alt_lp))
    assert [r["tokens"] for r in recs] == [[5, 6], [7, 8], [9, 10, 4, 6]]
    for r, b in zip(recs, base):                             # the keys of before hold what they held
        assert set(r) == set(b) | {"alternatives", "margins"}
        assert {k: r[k] for k in b} == b
        assert "alternatives" not in b and "margins" not in b
        assert len(r["alternatives"]) == len(r["margins"]) == len(r["tokens"])
    # row 0: EOS ends it (its own alternatives are not reported); position 1 has two candidates
    a0 = recs[0]["alternatives"]
    assert [[c["token"] for c in a] for a in a0] == [[5, 20, 30], [6, 21]]
    assert a0[0][1] == {"token": 20, "string": "<20>", "logprob": pytest.approx(float(alt_lp[0, 0, 1]))}
    assert recs[0]["margins"] == [pytest.approx(0.5), pytest.approx(1.5)]
    # row 1: cut by PAD; position 0 has one candidate
    assert [[c["token"] for c in a] for a in recs[1]["alternatives"]] == [[7], [8, 21, 31]]
    assert recs[1]["margins"][0] == math.inf and recs[1]["margins"][1] == pytest.approx(1.5)
    # row 2: the BOS at column 2 is skipped with its alternatives; the lists stay aligned with the tokens
    a2 = recs[2]["alternatives"]
    assert [a[0]["token"] for a in a2[:2]] == [9, 10] and [c["token"] for c in a2[2]] == [11, 4]
    assert [c["token"] for c in a2[3]] == [6, 24, 34]
    assert all(c["string"] == f"<{c['token']}>" for a in a2 for c in a)
    assert all(m >= 0 for r in recs for m in r["margins"])
    # rank order is kept as given, log-probabilities are python floats
    for r in recs:
        for a in r["alternatives"]:
            assert all(isinstance(c["logprob"], float) for c in a)
    # without a tokenizer the strings are None
    bare = A.build_records(ids, lp, cent, peak, pad_id=PAD, bos_id=BOS, eos_id=EOS, alternatives=(alt_ids, alt_lp))
    assert all(c["string"] is None for r in bare for a in r["alternatives"] for c in a)
    with pytest.raises(ValueError):
        A.build_records(ids, lp, cent, peak, pad_id=PAD, bos_id=BOS, eos_id=EOS, alternatives=(alt_ids[:, :-1], alt_lp[:, :-1]))


def test_select_seat_with_alternatives():
    slots, n, V, ML, K = 3, 7, 11, 9, 4
    g = torch.Generator().manual_seed(3)
    limits = torch.tensor([9, 4, 9, 2, 6, 9, 5], dtype=torch.int32)
    on = ST.new_state(n, slots, ML, PAD, BOS, "cpu", want_logprobs=True, top_k=K)
    off = ST.new_state(n, slots, ML, PAD, BOS, "cpu", want_logprobs=True)
    assert "alt_ids" not in off and "alt_logprob" not in off and set(on) == set(off) | {"alt_ids", "alt_logprob"}
    assert on["alt_ids"].shape == (n, ML, K) and on["alt_ids"].dtype == torch.int32 and bool((on["alt_ids"] == -1).all())
    assert bool((on["alt_logprob"] == 0).all())
    written = torch.zeros(n, ML, dtype=torch.bool)
    ties = 0
    for step in range(40):
        x = torch.randn(slots, V, generator=g)
        x[:, PAD] = -10.0
        for b in range(slots):
            r = int(torch.randint(0, 4, (1,), generator=g))
            if r == 0:                                       # the maximum tied across distant columns: the first one wins
                x[b, 9] = x[b, 4] = x[b].max() + 1.0
                ties += 1
            elif r == 1:                                     # ranks 2 and 3 tied
                x[b, 10] = x[b, 5] = x[b].max() - 0.25
                x[b, 7] = x[b].max() + 0.5
                ties += 1
        if step % 7 == 5:
            x[:, EOS] = 30.0
        live = on["slot_image"] >= 0
        for b in torch.nonzero(live).reshape(-1).tolist():
            written[int(on["slot_image"][b]), int(on["slot_t"][b]) + 1] = True
        rows = [(int(on["slot_image"][b]), int(on["slot_t"][b]) + 1, b) for b in torch.nonzero(live).reshape(-1).tolist()]
        on = ST.select_seat(x, on, n_images=n, max_len=ML, pad_id=PAD, bos_id=BOS, eos_id=EOS, limit=limits)
        off = ST.select_seat(x, off, n_images=n, max_len=ML, pad_id=PAD, bos_id=BOS, eos_id=EOS, limit=limits)
        ls = torch.log_softmax(x, -1)
        for i, col, b in rows:                               # this step's rows: the stable descending order of the slot's logits
            order = sorted(range(V), key=lambda v: (-float(x[b, v]), v))[:K]
            assert on["alt_ids"][i, col].tolist() == order
            assert torch.allclose(on["alt_logprob"][i, col], ls[b, order], rtol=0, atol=1e-6)
        if int(on["counters"][1]) >= n:
            break
    assert int(on["counters"][1]) == n and ties >= 5
    for k in ("slot_image", "slot_t", "tokens", "posids", "counters", "out_ids", "out_logprob"):
        assert torch.equal(on[k], off[k]), k
    assert bool(written[:, 0].sum() == 0) and int(written.sum()) > n
    assert torch.equal(on["alt_ids"][..., 0][written].long(), on["out_ids"][written])
    assert torch.allclose(on["alt_logprob"][..., 0][written], on["out_logprob"][written], rtol=0, atol=1e-6)
    assert bool((on["alt_ids"][~written] == -1).all()) and bool((on["alt_logprob"][~written] == 0).all())
    assert bool((on["alt_ids"][written] >= 0).all())
    d = on["alt_logprob"][written]
    assert bool((d[:, :-1] >= d[:, 1:]).all())              # rank order


def test_topk_rows_edges():
    x = torch.tensor([[0.5, float("-inf"), 0.5, 2.0], [float("-inf")] * 4])
    ids, lp = ST.topk_rows(x, 6)
    assert ids.tolist() == [[3, 0, 2, 1, -1, -1], [0, 1, 2, 3, -1, -1]]
    assert lp[0, 3] == float("-inf") and bool((lp[0, 4:] == float("-inf")).all()) and bool((lp[1] == float("-inf")).all())
    assert torch.allclose(lp[0, :3], torch.log_softmax(x[0], -1)[[3, 0, 2]])
    with pytest.raises(ValueError):
        ST.new_state(3, 2, 5, PAD, BOS, "cpu", top_k=9)
