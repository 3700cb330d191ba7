"""Forced prefixes (kzv/prefix.py, the ``prefix`` keywords of kzv/beam.py and kzv/stream.py, include/kzv.h: kzv_force_prefix,
kzv_stream_set_prefix, kzv_beam_update_prefix, kzv_stream_beam_update_prefix), the parts that need no GPU:

  1. the HF pin: beam.greedy and beam.beam_search with a prompt against transformers' own ``generate(input_ids=[BOS] + prefix,
     encoder_hidden_states=...)`` on the small RobertaForCausalLM of tests/test_host_cpu.py, every image run ALONE (HF needs equal-length
     prompts): prefix lengths 0, 1, 3 and max_length - 2; 1, 2 and 4 beams; length_penalty 1.0 and 2.0 (a wrong divisor shows);
     early_stopping True and False (the heuristic inside the prefix shows).  Sequences equal; ``sequences_scores`` within 1e-5, the bound
     tests/test_nbest_cpu.py holds the same statement to against the same model (tests/test_host_cpu.py itself compares no scores).  A
     batch of ragged prefixes equals the per-image runs;
  2. equivalences: force_reference on hand rows; stream.py's bookkeeping with prefixes equals lockstep per image with fewer slots than
     images (so slots are reseated inside other images' prefixes); an empty prefix equals no prefix;
  3. refusals: BOS / EOS / padding / ids outside the vocabulary, prefixes that reach max_length - 1 or the image's limit - 1, wrong
     counts -- before anything runs; the C entries refuse bad arguments before any launch; libkzv.so exports the new symbols.
"""
import ctypes as C
import os
import warnings
import zlib

import pytest
import torch

from kzv import _lib as L
from kzv import align as A
from kzv import beam as BM
from kzv import prefix as PF
from kzv import stream as ST
from kzv.config import tiny_config

PAD, BOS, EOS = 1, 2, 3
INF = float("inf")

# ---- 1. the statement against HF ---------------------------------------------------------------------------------------------------------
HV, HB, HH, HL = 41, 3, 32, 12
PLENS = (0, 1, 3, HL - 2)


@pytest.fixture(scope="module")
def hf():
    from transformers import RobertaConfig, RobertaForCausalLM
    warnings.filterwarnings("ignore")
    cfg = RobertaConfig(vocab_size=HV, hidden_size=HH, num_hidden_layers=2, num_attention_heads=2, intermediate_size=64,
                        max_position_embeddings=40, pad_token_id=PAD, bos_token_id=BOS, eos_token_id=EOS, is_decoder=True,
                        add_cross_attention=True, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    out = []
    for seed, eos_bias in ((1, 2.5), (2, 4.0)):
        torch.manual_seed(seed)
        m = RobertaForCausalLM(cfg).eval()
        with torch.no_grad():
            for p in m.parameters():
                p.mul_(3.0)
            m.lm_head.bias[EOS] += eos_bias
        enc = torch.randn(HB, 6, HH) * 8
        g = torch.Generator().manual_seed(100 + seed)
        prefixes = {n: torch.randint(4, HV, (HB, max(n, 1)), generator=g)[:, :n] for n in PLENS}      # no special ids
        out.append((m, enc, prefixes))
    return out


def _make_step(m, enc, nb):
    e = enc.repeat_interleave(nb, 0)

    def step(t, ids):
        x = ids[:, :t + 1]
        with torch.no_grad():
            return m(input_ids=x, encoder_hidden_states=e, attention_mask=torch.ones_like(x),
                     position_ids=torch.arange(t + 1)[None].expand_as(x)).logits[:, -1]
    return step


def _hf_generate(m, enc, prompt, nb, es, lpen):
    with torch.no_grad():
        return m.generate(prompt, encoder_hidden_states=enc, max_length=HL, num_beams=nb, early_stopping=es, length_penalty=lpen,
                          pad_token_id=PAD, eos_token_id=EOS, use_cache=False, do_sample=False, return_dict_in_generate=True,
                          output_scores=nb > 1)


def _pair(pfx_row):
    n = pfx_row.numel()
    return (pfx_row.view(1, n) if n else torch.full((1, 1), PAD, dtype=torch.int64)), torch.tensor([n], dtype=torch.int32)


def test_greedy_with_a_prompt_equals_hf_generate(hf):
    ended = 0
    for m, enc, prefixes in hf:
        for n in PLENS:
            for i in range(HB):
                p = prefixes[n][i]
                prompt = torch.cat((torch.tensor([BOS]), p)).view(1, -1)
                h = _hf_generate(m, enc[i:i + 1], prompt, 1, False, 1.0).sequences
                g = BM.greedy(_make_step(m, enc[i:i + 1], 1), 1, HL, PAD, BOS, EOS, "cpu", prefix=_pair(p))
                assert g.shape == h.shape and torch.equal(g, h), (n, i, g, h)
                assert torch.equal(g[0, :1 + n], prompt[0])
                ended += int((h == EOS).any())
    assert ended >= 4                            # lines that end in EOS after a prompt were among them


@pytest.mark.parametrize("nb", [2, 4])
@pytest.mark.parametrize("es", [True, False])
@pytest.mark.parametrize("lpen", [1.0, 2.0])
def test_beam_search_with_a_prompt_equals_hf_generate(hf, nb, es, lpen):
    worst = 0.0
    for m, enc, prefixes in hf:
        for n in PLENS:
            for i in range(HB):
                p = prefixes[n][i]
                prompt = torch.cat((torch.tensor([BOS]), p)).view(1, -1)
                h = _hf_generate(m, enc[i:i + 1], prompt, nb, es, lpen)
                got = BM.beam_search(_make_step(m, enc[i:i + 1], nb), lambda rows, t: None, 1, nb, HL, HV, PAD, BOS, EOS, "cpu", early_stopping=es,
                                     length_penalty=lpen, num_return_sequences=1, return_logprobs=True, prefix=_pair(p))
                assert got["ids"].shape == h.sequences.shape and torch.equal(got["ids"], h.sequences), (n, i, got["ids"], h.sequences)
                err = float((got["scores"] - h.sequences_scores).abs().max())
                worst = max(worst, err)
                assert err <= 1e-5, (n, i, err)
                # forced columns carry exactly 0: the score sums the generated tokens only
                assert bool((got["logprobs"][0, :1 + n] == 0).all())
    print(f"nb {nb} early_stopping {es} length_penalty {lpen}: sequences_scores within {worst:.2e}")


@pytest.mark.parametrize("nb", [1, 2, 4])
def test_a_batch_of_ragged_prefixes_equals_the_per_image_runs(hf, nb):
    m, enc, prefixes = hf[0]
    lens = [0, 3, HL - 2][:HB]
    lists = [prefixes[n][i].tolist() for i, n in enumerate(lens)]
    both = PF.normalise(lists, HB, vocab=HV, pad_id=PAD, bos_id=BOS, eos_id=EOS, max_length=HL)
    assert both[1].tolist() == lens and both[0].shape == (HB, HL - 2)
    if nb == 1:
        got = BM.greedy(_make_step(m, enc, 1), HB, HL, PAD, BOS, EOS, "cpu", prefix=both)
    else:
        got = BM.beam_search(_make_step(m, enc, nb), lambda rows, t: None, HB, nb, HL, HV, PAD, BOS, EOS, "cpu", early_stopping=False,
                             length_penalty=2.0, prefix=both)
    for i in range(HB):
        pair = _pair(torch.tensor(lists[i], dtype=torch.int64))
        if nb == 1:
            one = BM.greedy(_make_step(m, enc[i:i + 1], 1), 1, HL, PAD, BOS, EOS, "cpu", prefix=pair)
        else:
            one = BM.beam_search(_make_step(m, enc[i:i + 1], nb), lambda rows, t: None, 1, nb, HL, HV, PAD, BOS, EOS, "cpu",
                                 early_stopping=False, length_penalty=2.0, prefix=pair)
        row = torch.full((HL,), PAD, dtype=torch.int64)
        row[:one.shape[1]] = one[0]
        full = torch.full((HL,), PAD, dtype=torch.int64)
        full[:got.shape[1]] = got[i]
        assert torch.equal(full, row), (i, full, row)      # (a lockstep row that ended keeps writing padding: equal as padded rows)
        assert full[:1 + lens[i]].tolist() == [BOS] + lists[i]


# ---- 2. equivalences ---------------------------------------------------------------------------------------------------------------------
def test_force_reference_on_hand_rows():
    x = torch.tensor([[0.5, -1.0, 2.0, 0.25, 7.0],
                      [1.0, 2.0, 3.0, 4.0, 5.0],
                      [-INF, 0.0, 1.0, -2.0, 3.0],
                      [9.0, 8.0, 7.0, 6.0, 5.0]])
    pfx = torch.tensor([[4, 2], [3, 1], [0, 0], [2, 4]])
    plen = torch.tensor([2, 1, 0, 2], dtype=torch.int32)
    # cur = 1: rows 0, 1 and 3 are forced to their first token; row 2 has no prefix
    y = PF.force_reference(x, 1, pfx, plen)
    assert y[0].tolist() == [-INF, -INF, -INF, -INF, 0.0]
    assert y[1].tolist() == [-INF, -INF, -INF, 0.0, -INF]
    assert torch.equal(y[2], x[2]) and y[3].tolist() == [-INF, -INF, 0.0, -INF, -INF]
    # cur = 2: row 1 is past its prefix
    y = PF.force_reference(x, 2, pfx, plen)
    assert y[0].tolist() == [-INF, -INF, 0.0, -INF, -INF] and torch.equal(y[1], x[1]) and torch.equal(y[2], x[2])
    assert y[3].tolist() == [-INF, -INF, -INF, -INF, 0.0]
    # cur = 3 and cur = 0: nothing is forced; the input is never edited
    keep = x.clone()
    assert torch.equal(PF.force_reference(x, 3, pfx, plen), x) and torch.equal(PF.force_reference(x, 0, pfx, plen), x) and torch.equal(x, keep)
    # per-row history lengths
    y = PF.force_reference(x, torch.tensor([2, 1, 1, 3]), pfx, plen)
    assert y[0].tolist() == [-INF, -INF, 0.0, -INF, -INF] and y[1].tolist() == [-INF, -INF, -INF, 0.0, -INF]
    assert torch.equal(y[2], x[2]) and torch.equal(y[3], x[3])
    # arg-max takes the forced token at log-probability exactly 0
    y = PF.force_reference(x, 1, pfx, plen)
    assert y.argmax(-1).tolist()[:2] == [4, 3] and float((y.max(-1)[0] - torch.logsumexp(y, -1))[0]) == 0.0
    # the model's own opinion of the forced token
    val, forced = PF.forced_logprob_reference(x, 1, pfx, plen)
    assert forced.tolist() == [True, True, False, True]
    assert float(val[0]) == pytest.approx(float(torch.log_softmax(x[0], -1)[4]))
    val, _ = PF.forced_logprob_reference(x, 1, pfx, plen, normalised=True)
    assert float(val[1]) == 4.0


V, LMAX, N = 11, 14, 17


def _logits(image: int, prefix) -> torch.Tensor:
    g = torch.Generator().manual_seed(zlib.crc32(repr((int(image), [int(x) for x in prefix])).encode()))
    x = torch.randn(V, generator=g)
    x[PAD] = -10.0
    return x


def _ragged(n=N, longest=5, seed=3):
    g = torch.Generator().manual_seed(seed)
    lens = [int(x) for x in torch.randint(0, longest + 1, (n,), generator=g)]
    lens[0], lens[1], lens[2] = 0, longest, 1
    lists = [[int(x) for x in torch.randint(4, V, (k,), generator=g)] for k in lens]
    return lists, PF.normalise(lists, n, vocab=V, pad_id=PAD, bos_id=BOS, eos_id=EOS, max_length=LMAX)


def _one(lst):
    return PF.normalise([lst], 1, vocab=V, pad_id=PAD, bos_id=BOS, eos_id=EOS, max_length=LMAX)


def test_greedy_stream_with_prefixes_equals_lockstep_per_image():
    lists, both = _ragged()
    slots = 4

    def step(st):
        out = torch.zeros(slots, V)
        for s, (i, t) in enumerate(zip(st["slot_image"].tolist(), st["slot_t"].tolist())):
            if i >= 0:
                out[s] = _logits(i, st["out_ids"][i, :t + 1])
        return out
    (ids, lp), st = ST.greedy_stream(step, N, slots, LMAX, PAD, BOS, EOS, "cpu", return_logprobs=True, return_state=True, prefix=both)
    for i in range(N):
        one = BM.greedy(lambda t, h, i=i: torch.stack([_logits(i, h[0, :t + 1])]), 1, LMAX, PAD, BOS, EOS, "cpu", prefix=_one(lists[i]))
        row = torch.full((LMAX,), PAD, dtype=torch.int64)
        row[:one.shape[1]] = one[0]
        assert torch.equal(ids[i], row), i
        assert ids[i, :1 + len(lists[i])].tolist() == [BOS] + lists[i]
        assert bool((lp[i, :1 + len(lists[i])] == 0).all())          # forced columns: exactly 0
        free = lp[i, 1 + len(lists[i]):int((row != PAD).sum())]
        assert bool((free < 0).all())
    assert st["counters"].tolist()[:2] == [N, N]
    # a stream without prefixes differs (the prefixes were not the model's own choice everywhere)
    plain = ST.greedy_stream(step, N, slots, LMAX, PAD, BOS, EOS, "cpu")
    assert not torch.equal(plain, ids)


@pytest.mark.parametrize("nb,early,lpen", [(2, True, 1.0), (2, False, 2.0), (4, True, 2.0), (4, False, 1.0)])
def test_beam_stream_with_prefixes_equals_lockstep_per_image(nb, early, lpen):
    lists, both = _ragged()
    slots = 3

    def step(st):
        out = torch.zeros(slots * nb, V)
        for s, (i, t) in enumerate(zip(st["slot_image"].tolist(), st["slot_t"].tolist())):
            if i >= 0:
                for k in range(nb):
                    out[s * nb + k] = _logits(i, st["run_seq"][s, k, :t + 1])
        return out
    (ids, score), st = ST.beam_stream(step, N, slots, nb, LMAX, V, PAD, BOS, EOS, "cpu", early_stopping=early, length_penalty=lpen,
                                      return_state=True, prefix=both)
    for i in range(N):
        one = BM.beam_search(lambda t, h, i=i: torch.stack([_logits(i, h[r, :t + 1]) for r in range(nb)]), lambda rows, t: None, 1, nb, LMAX, V,
                             PAD, BOS, EOS, "cpu", early_stopping=early, length_penalty=lpen, num_return_sequences=1, return_logprobs=True,
                             prefix=_one(lists[i]) if lists[i] else None)
        row = torch.full((LMAX,), PAD, dtype=torch.int64)
        row[:one["ids"].shape[1]] = one["ids"][0]
        assert torch.equal(ids[i], row), (i, ids[i], row)
        assert torch.equal(score[i], one["scores"][0]), (i, score[i], one["scores"])
        assert ids[i, :1 + len(lists[i])].tolist() == [BOS] + lists[i]
    assert st["counters"].tolist()[:2] == [N, N]


def test_an_empty_prefix_equals_no_prefix():
    assert PF.normalise(None, 3, vocab=V, pad_id=PAD, bos_id=BOS, eos_id=EOS, max_length=LMAX) is None
    assert PF.normalise([[], None, ()], 3, vocab=V, pad_id=PAD, bos_id=BOS, eos_id=EOS, max_length=LMAX) is None
    assert PF.normalise(torch.full((3, 4), PAD), 3, vocab=V, pad_id=PAD, bos_id=BOS, eos_id=EOS, max_length=LMAX) is None
    # a padded tensor and the ragged lists are the same request
    a = PF.normalise(torch.tensor([[5, 6, PAD], [PAD, PAD, PAD], [7, 8, 9]]), 3, vocab=V, pad_id=PAD, bos_id=BOS, eos_id=EOS, max_length=LMAX)
    b = PF.normalise([[5, 6], [], [7, 8, 9]], 3, vocab=V, pad_id=PAD, bos_id=BOS, eos_id=EOS, max_length=LMAX)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[1].dtype == torch.int32 and a[0].dtype == torch.int64
    # zero lengths through the bookkeeping: the plain result
    zero = (torch.full((2, 1), PAD, dtype=torch.int64), torch.zeros(2, dtype=torch.int32))
    step1 = lambda t, h: torch.stack([_logits(r, h[r, :t + 1]) for r in range(2)])      # noqa: E731
    assert torch.equal(BM.greedy(step1, 2, LMAX, PAD, BOS, EOS, "cpu", prefix=zero), BM.greedy(step1, 2, LMAX, PAD, BOS, EOS, "cpu"))
    for nb in (2, 4):
        stepb = lambda t, h, nb=nb: torch.stack([_logits(r // nb, h[r, :t + 1]) for r in range(2 * nb)])      # noqa: E731
        a = BM.beam_search(stepb, lambda rows, t: None, 2, nb, LMAX, V, PAD, BOS, EOS, "cpu", length_penalty=2.0, num_return_sequences=1,
                           return_logprobs=True, prefix=zero)
        b = BM.beam_search(stepb, lambda rows, t: None, 2, nb, LMAX, V, PAD, BOS, EOS, "cpu", length_penalty=2.0, num_return_sequences=1,
                           return_logprobs=True)
        assert torch.equal(a["ids"], b["ids"]) and torch.equal(a["logprobs"], b["logprobs"])
        assert float((a["scores"] - b["scores"]).abs().max()) <= 1e-6      # (a tensor divisor against a Python scalar's)


def test_records_with_forced_tokens():
    ids = [[BOS, 5, 6, 7, EOS, PAD]]
    lp = [[-0.0, -0.0, -0.5, -1.5, 0.0]]
    alts = ([[[5, 4], [6, 4], [7, 8], [EOS, 4], [-1, -1]]], [[[0.0, -INF], [0.0, -INF], [-0.5, -1.0], [-1.5, -2.0], [0.0, 0.0]]])
    import numpy as np
    kw = dict(pad_id=PAD, bos_id=BOS, eos_id=EOS)
    r = A.build_records(ids, lp, np.zeros((1, 5, 2)), np.zeros((1, 5), dtype=np.int64), alternatives=alts, forced=[2],
                        prefix_logprobs=[[0.0, -3.0, -4.0]], **kw)[0]
    assert r["forced"] == 2 and r["tokens"] == [5, 6, 7] and r["prefix_logprobs"] == [-3.0, -4.0]
    assert r["confidence"] == pytest.approx(float(np.exp((-0.5 - 1.5) / 2)))          # the free tokens only, EOS included
    assert r["alternatives"][0] == [] and r["alternatives"][1] == [] and len(r["alternatives"][2]) == 2
    plain = A.build_records(ids, lp, np.zeros((1, 5, 2)), np.zeros((1, 5), dtype=np.int64), **kw)[0]
    assert "forced" not in plain and plain["confidence"] == pytest.approx(float(np.exp((-0.5 - 1.5) / 4)))


# ---- 3. refusals -------------------------------------------------------------------------------------------------------------------------
def test_prefixes_are_refused_before_anything_runs():
    kw = dict(vocab=V, pad_id=PAD, bos_id=BOS, eos_id=EOS, max_length=LMAX)
    for bad in ([[5, BOS]], [[EOS]], [[5, PAD, 6]], [[V]], [[-1]]):
        with pytest.raises(ValueError, match="prefix_ids"):
            PF.normalise(bad, 1, **kw)
    with pytest.raises(ValueError, match="leave no room"):
        PF.normalise([[5] * (LMAX - 1)], 1, **kw)                                 # 1 + len = max_length: nothing to generate
    assert PF.normalise([[5] * (LMAX - 2)], 1, **kw)[1].tolist() == [LMAX - 2]    # the longest prefix that is served
    with pytest.raises(ValueError, match="leave no room"):
        PF.normalise([[5], [5, 6, 7]], 2, limits=[LMAX, 4], **kw)                 # against the image's own limit
    assert PF.normalise([[5], [5, 6]], 2, limits=[LMAX, 4], **kw) is not None
    with pytest.raises(ValueError, match="2 prefixes for 3 images"):
        PF.normalise([[5], [6]], 3, **kw)
    with pytest.raises(ValueError, match="integer tensor"):
        PF.normalise(torch.zeros(2, 3), 2, **kw)
    with pytest.raises(ValueError, match="batch"):
        BM.beam_search(lambda t, h: None, lambda r, t: None, 2, 2, LMAX, V, PAD, BOS, EOS, "cpu",
                       prefix=(torch.zeros(3, 1, dtype=torch.int64), torch.zeros(3, dtype=torch.int32)))

    class _NoTok:
        pass
    with pytest.raises(ValueError, match="tokenizer"):
        PF.texts_to_ids(None, ["a"])
    with pytest.raises(ValueError, match="one-character"):
        PF.texts_to_ids(_NoTok(), ["a"])


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load()


def test_abi_exports_and_refuses_bad_arguments_without_a_launch(lib):
    for name in ("kzv_force_prefix", "kzv_test_force_prefix_calls", "kzv_stream_set_prefix", "kzv_beam_update_prefix", "kzv_stream_beam_update_prefix"):
        assert hasattr(lib, name), name
    out = 4096                                                   # never dereferenced: only its presence is checked
    calls = lib.kzv_test_force_prefix_calls()
    good = dict(logits=out, ld=45, rows=8, vocab=41, t=0, group=2, slot_image=None, slot_t=None, by_image=0, n_images=4, prefix=out, ld_prefix=3,
                prefix_len=out, normalised=0, reserved=0, forced_logprob=None, ld_forced_logprob=0)
    bad = [dict(logits=None), dict(prefix=None), dict(prefix_len=None), dict(rows=0), dict(vocab=0), dict(vocab=16385, ld=16400), dict(ld=40),
           dict(ld_prefix=0), dict(group=0), dict(group=3), dict(t=-1), dict(slot_image=out), dict(slot_t=out), dict(slot_image=out, slot_t=out, n_images=0),
           dict(forced_logprob=out, ld_forced_logprob=3)]
    for extra in bad:
        a = L.kzv_force_prefix_args(**dict(good, **extra))
        assert lib.kzv_force_prefix(C.byref(a), None) == -1 and b"force_prefix" in lib.kzv_last_error(), extra
    assert lib.kzv_force_prefix(None, None) == -1
    assert lib.kzv_test_force_prefix_calls() == calls                # nothing reached a launch
    # the struct layouts the existing callers rely on did not move: the length tables are arguments of the *_prefix entries
    assert [f[0] for f in L.kzv_beam_state._fields_][-1] == "fin_lp_out" and [f[0] for f in L.kzv_stream_beam_state._fields_][-1] == "ld_nbest_logprob"
    bs = L.kzv_beam_state(batch=2, num_beams=4, max_len=16, vocab=V, eos_id=EOS, run_seq_in=out, run_seq_out=out + 8, fin_seq_in=out, fin_seq_out=out + 8,
                          run_scores=out, fin_scores=out, fin_done=out, fin_len=out, unsatisfied=out)
    assert lib.kzv_beam_update_prefix(C.byref(bs), out, out, 1, 1, 1.0, None, out, out, out, None) == -1 and b"divisor" in lib.kzv_last_error()
    assert lib.kzv_beam_update_prefix(C.byref(bs), out, out, 0, 1, 1.0, out, out, out, out, None) == -1
    st = L.kzv_stream_beam_state(slots=4, n_images=8, num_beams=3, max_len=16, vocab=V, bos_id=BOS, eos_id=EOS, pad_id=PAD, early_stopping=1,
                                 slot_image=out, slot_t=out, tokens=out, posids=out, run_seq=out, fin_seq=out, run_scores=out, fin_scores=out,
                                 fin_done=out, fin_len=out, unsatisfied=out, counters=out, scratch=out, out_ids=out, ld_ids=16, divisors=out)
    assert lib.kzv_stream_beam_update_prefix(C.byref(st), out, out, out, None) == -1 and b"stream_beam_update_prefix" in lib.kzv_last_error()
    # the handle entry: a state error before a wave has begun
    cfg = tiny_config()
    c = L.kzv_config(image_h=cfg.image_h, image_w=cfg.image_w, patch_h=cfg.patch_h, patch_w=cfg.patch_w, channels=cfg.channels,
                     enc_hidden=cfg.enc_hidden, enc_layers=cfg.enc_layers, enc_heads=cfg.enc_heads, enc_ffn=cfg.enc_ffn,
                     dec_hidden=cfg.dec_hidden, dec_layers=cfg.dec_layers, dec_heads=cfg.dec_heads, dec_ffn=cfg.dec_ffn,
                     vocab=cfg.vocab, max_pos=cfg.max_pos, type_vocab=cfg.type_vocab, pad_id=cfg.pad_id, ln_eps=1e-12)
    h = C.c_void_p()
    L.check(lib.kzv_model_create(C.byref(c), C.byref(h)), "create")
    try:
        assert lib.kzv_stream_set_prefix(h, out, 3, out, None, 0, None) == -3 and b"stream_set_prefix" in lib.kzv_last_error()
        assert lib.kzv_stream_set_prefix(None, out, 3, out, None, 0, None) == -3
    finally:
        lib.kzv_model_destroy(h)
