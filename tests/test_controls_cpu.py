"""Generation controls (kzv/controls.py; include/kzv.h: kzv_logits_process, kzv_stream_set_controls), the parts that need no GPU:

  1. ``process_reference`` against transformers' own logits processors (RepetitionPenalty, NoRepeatNGram, MinLength, SuppressTokens), each
     alone and all together, ``torch.equal`` on seeded scores of both signs, over histories that cover n + 1 < g, n = 1 (BOS only), g = 1,
     duplicates, a tail that occurs three times, and n = L - 1 / n = L;
  2. the hooked statements of kzv/beam.py (``greedy`` / ``beam_search`` with ``process``) against HF ``generate(**controls)`` on the small
     RobertaForCausalLM of tests/test_host_cpu.py::test_beam_and_greedy_bookkeeping_equal_hf_generate (its three (seed, eos_bias) pairs,
     its step function), max_length 24, greedy and 4 beams, every control alone and the combination (3, 1.2, min_length 4, suppress [1, 9]);
  3. the condition that comparison needs, asserted on HF's own outputs: every control changes at least one of the 12 greedy sequences and
     at least one of the 12 beam-4 sequences, and the n-gram ban removes every repeated 2-gram.  Observed here (rows of 12 changed, greedy
     / 4 beams): no_repeat_ngram_size=2 3 / 3, repetition_penalty=1.3 3 / 3, min_length=6 8 / 8, suppress [5, 7, 11, 1] 2 / 4, the
     combination 11 / 10; 3 of the 12 base decodes hold a repeated 2-gram (greedy and 4 beams alike), none with the ban;
  4. the slot statements of kzv/stream.py (``greedy_stream`` / ``beam_stream`` with ``process``) equal the lockstep statements with the
     hook on each image alone, over a seeded fake decoder;
  5. GenerationControls' validation and mask bits, the CLI flags' defaults, and the C entry points' argument refusals (they come before
     any launch, so they run on a machine without a GPU).
"""
import ctypes as C
import warnings
import zlib

import pytest
import torch

from kzv import _lib as L
from kzv import beam as BM
from kzv import controls as CT
from kzv import stream as ST

NEG_INF = float("-inf")


# ---- 1. process_reference == transformers' processors ---------------------------------------------------------------------------------
V1, EOS1 = 23, 3
HISTORIES = {
    "bos_only": [[2], [2]],
    "shorter_than_g": [[2, 5], [2, 6]],                                  # n + 1 < g for g = 4
    "duplicates": [[2, 5, 5, 5, 7, 5], [2, 9, 8, 9, 8, 9]],
    "tail_three_times": [[2, 4, 6, 10, 4, 6, 11, 4, 6, 12, 4, 6], [2, 7, 7, 13, 7, 7, 14, 7, 7, 15, 7, 7]],
    "eos_inside": [[2, 3, 1, 1, 1], [2, 8, 3, 1, 1]],
}


def _scores(rows, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, V1, generator=g) * 3.0                         # both signs
    assert (x > 0).any() and (x < 0).any()
    return x


def _hf(scores, ids, *, g=0, p=1.0, ml=0, sup=None):
    from transformers.generation.logits_process import (MinLengthLogitsProcessor, NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor,
                                                        SuppressTokensLogitsProcessor)
    x = scores.clone()
    if p != 1.0:
        x = RepetitionPenaltyLogitsProcessor(p)(ids, x)
    if g:
        x = NoRepeatNGramLogitsProcessor(g)(ids, x)
    if ml:
        x = MinLengthLogitsProcessor(ml, EOS1, device="cpu")(ids, x)
    if sup:
        x = SuppressTokensLogitsProcessor(sup, device="cpu")(ids, x)
    return x


@pytest.mark.parametrize("name", sorted(HISTORIES))
def test_process_reference_equals_transformers_processors(name):
    ids = torch.tensor(HISTORIES[name], dtype=torch.int64)
    n = ids.shape[1]
    x = _scores(ids.shape[0], seed=zlib.crc32(name.encode()))
    cases = [dict(p=1.3), dict(p=0.7), dict(ml=n), dict(ml=n + 1), dict(sup=[1, 9, 22]), dict(g=3, p=1.2, ml=n + 1, sup=[1, 9])]
    cases += [dict(g=g) for g in range(1, 9)]
    for kw in cases:
        want = _hf(x, ids, **kw)
        ctl = CT.GenerationControls(kw.get("g", 0), kw.get("p", 1.0), kw.get("ml", 0), kw.get("sup"))
        got = CT.process_reference(x, ids, ctl, EOS1)
        assert torch.equal(got, want), (name, kw)
        rows = CT.process_rows_reference(x, torch.nn.functional.pad(ids, (0, 3), value=1), torch.full((ids.shape[0],), n), ctl, EOS1)
        assert torch.equal(rows, want), (name, kw)
    # what the histories are for
    if name == "shorter_than_g":
        assert torch.equal(CT.process_reference(x, ids, CT.GenerationControls(4), EOS1), x)
    if name == "tail_three_times":
        assert CT.banned_ngram_tokens(HISTORIES[name][0], 3) == [10, 11, 12] and CT.banned_ngram_tokens(HISTORIES[name][1], 3) == [13, 14, 15]
    if name == "bos_only":
        assert CT.banned_ngram_tokens([2], 1) == [2] and CT.banned_ngram_tokens([2], 2) == []


# ---- 2. / 3. the hooked statements == HF generate(**controls) ---------------------------------------------------------------------------
LMAX2 = 24
CONTROLS = {
    "ngram2": dict(no_repeat_ngram_size=2),
    "penalty": dict(repetition_penalty=1.3),
    "min_length": dict(min_length=6),
    "suppress": dict(suppress_tokens=[5, 7, 11, 1]),
    "all": dict(no_repeat_ngram_size=3, repetition_penalty=1.2, min_length=4, suppress_tokens=[1, 9]),
}


@pytest.fixture(scope="module")
def hf_runs():
    """{(control name | None, num_beams): [sequences of seed 0, 1, 2]} from transformers' generate, the model and step function per seed."""
    from transformers import RobertaConfig, RobertaForCausalLM
    warnings.filterwarnings("ignore")
    V, B, H = 41, 4, 32
    cfg = RobertaConfig(vocab_size=V, hidden_size=H, num_hidden_layers=2, num_attention_heads=2, intermediate_size=64,
                        max_position_embeddings=40, pad_token_id=1, bos_token_id=2, eos_token_id=3, is_decoder=True,
                        add_cross_attention=True, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    models, runs = [], {}
    for seed, eos_bias in ((0, 0.0), (1, 2.5), (2, 4.0)):
        torch.manual_seed(seed)
        m = RobertaForCausalLM(cfg).eval()
        with torch.no_grad():
            for p in m.parameters():
                p.mul_(3.0)
            m.lm_head.bias[3] += eos_bias
        enc = torch.randn(B, 6, H) * 8
        models.append((m, enc))
        for name in [None] + list(CONTROLS):
            for nb in (1, 4):
                with torch.no_grad():
                    seq = m.generate(torch.full((B, 1), 2, dtype=torch.long), encoder_hidden_states=enc, max_length=LMAX2, num_beams=nb,
                                     early_stopping=True, length_penalty=1.0, pad_token_id=1, eos_token_id=3, use_cache=False, do_sample=False,
                                     return_dict_in_generate=True, **(CONTROLS[name] if name else {})).sequences
                runs.setdefault((name, nb), []).append(seq)
    return {"V": V, "B": B, "models": models, "runs": runs}


def _make_step(m, enc, nb):
    e = enc.repeat_interleave(nb, 0)

    def step(t, ids):
        x = ids[:, :t + 1]
        with torch.no_grad():
            return m(input_ids=x, encoder_hidden_states=e, attention_mask=torch.ones_like(x),
                     position_ids=torch.arange(t + 1)[None].expand_as(x)).logits[:, -1]
    return step


def _rows(seqs):
    """the 12 sequences as token lists without padding"""
    return [[t for t in r if t != 1] for s in seqs for r in s.tolist()]


@pytest.mark.parametrize("nb", [1, 4])
@pytest.mark.parametrize("name", list(CONTROLS))
def test_hooked_statements_equal_hf_generate(hf_runs, name, nb):
    V, B = hf_runs["V"], hf_runs["B"]
    base, want = hf_runs["runs"][(None, nb)], hf_runs["runs"][(name, nb)]
    # the condition first, on HF's own outputs: the control changes something
    changed = sum(a != b for a, b in zip(_rows(base), _rows(want)))
    print(f"{name}, {nb} beam(s): {changed} of 12 sequences changed")
    assert changed >= 1
    if name == "ngram2":
        n_rep = sum(CT.has_repeated_ngram(r, 2) for r in _rows(base))
        print(f"  base decodes with a repeated 2-gram: {n_rep} of 12")
        assert (nb != 1 or n_rep >= 1) and not any(CT.has_repeated_ngram(r, 2) for r in _rows(want))
    if name == "min_length":
        assert any(3 in r[:5] for r in _rows(base)) and not any(3 in r[:5] for r in _rows(want))
    ctl = CT.GenerationControls(**CONTROLS[name], eos_id=3)
    for (m, enc), h in zip(hf_runs["models"], want):
        if nb == 1:
            g = BM.greedy(_make_step(m, enc, 1), B, LMAX2, 1, 2, 3, "cpu", process=ctl.hook(3))
        else:
            g = BM.beam_search(_make_step(m, enc, nb), lambda rows, t: None, B, nb, LMAX2, V, 1, 2, 3, "cpu", early_stopping=True,
                               process=ctl.hook(3))
        assert g.shape == h.shape and torch.equal(g, h), (name, nb, g, h)


def test_no_hook_is_the_statement_as_it_was(hf_runs):
    m, enc = hf_runs["models"][1]
    assert torch.equal(BM.greedy(_make_step(m, enc, 1), 4, LMAX2, 1, 2, 3, "cpu"), hf_runs["runs"][(None, 1)][1])
    with pytest.raises(ValueError):
        BM.beam_search(None, None, 1, 2, 8, 11, 1, 2, 3, "cpu", topk=lambda a, b: None, process=lambda a, b, c: a)


# ---- 4. the slot statements with the hook == the lockstep statements with the hook, image by image -----------------------------------------
PAD, BOS, EOS, V4, LMAX4, N4 = 1, 2, 3, 11, 14, 13
CTL4 = CT.GenerationControls(no_repeat_ngram_size=2, repetition_penalty=1.2, min_length=5, suppress_tokens=[PAD, 9])


def _fake_logits(image, prefix):
    g = torch.Generator().manual_seed(zlib.crc32(repr((int(image), [int(x) for x in prefix])).encode()))
    x = torch.randn(V4, generator=g)
    x[EOS] += 0.5
    return x


def test_greedy_stream_with_hook_equals_lockstep_with_hook():
    def step_fn(st):
        out = torch.zeros(st["slot_image"].numel(), V4)
        for s, (i, t) in enumerate(zip(st["slot_image"].tolist(), st["slot_t"].tolist())):
            if i >= 0:
                out[s] = _fake_logits(i, st["out_ids"][i, :t + 1])
        return out
    (ids, lp), st = ST.greedy_stream(step_fn, N4, 4, LMAX4, PAD, BOS, EOS, "cpu", return_logprobs=True, return_state=True, top_k=3,
                                     process=CTL4.rows_hook(EOS))
    plain = ST.greedy_stream(step_fn, N4, 4, LMAX4, PAD, BOS, EOS, "cpu")
    differ = 0
    for i in range(N4):
        alone = BM.greedy(lambda t, x, i=i: torch.stack([_fake_logits(i, x[0, :t + 1])]), 1, LMAX4, PAD, BOS, EOS, "cpu", process=CTL4.hook(EOS))
        row = torch.full((LMAX4,), PAD, dtype=torch.int64)
        row[:alone.shape[1]] = alone[0]
        assert torch.equal(ids[i], row), i
        differ += int(not torch.equal(ids[i], plain[i]))
        toks = [t for t in row.tolist() if t != PAD]
        assert not CT.has_repeated_ngram(toks, 2) and 9 not in toks and EOS not in toks[:4]
        for j in range(1, len(toks)):                                  # entry 0 is the emitted token; nothing banned is an alternative above -inf
            assert int(st["alt_ids"][i, j, 0]) == toks[j]
            ban = set(CT.banned_ngram_tokens(toks[:j], 2)) | {PAD, 9}
            for k in range(3):
                assert int(st["alt_ids"][i, j, k]) not in ban or float(st["alt_logprob"][i, j, k]) == NEG_INF
    assert differ >= 1                                                 # the controls act on this fake decoder


@pytest.mark.parametrize("nb", [2, 4])
def test_beam_stream_with_hook_equals_lockstep_with_hook(nb):
    def step_fn(st):
        slots = st["slot_image"].numel()
        out = torch.zeros(slots * nb, V4)
        for s, (i, t) in enumerate(zip(st["slot_image"].tolist(), st["slot_t"].tolist())):
            if i >= 0:
                for k in range(nb):
                    out[s * nb + k] = _fake_logits(i, st["run_seq"][s, k, :t + 1])
        return out
    (ids, score), st = ST.beam_stream(step_fn, N4, 3, nb, LMAX4, V4, PAD, BOS, EOS, "cpu", return_state=True, process=CTL4.rows_hook(EOS))
    assert int(st["counters"][3]) == 0                                 # padding is suppressed: no running beam can take it
    for i in range(N4):
        alone = BM.beam_search(lambda t, x, i=i: torch.stack([_fake_logits(i, x[r, :t + 1]) for r in range(nb)]), lambda rows, t: None, 1, nb,
                               LMAX4, V4, PAD, BOS, EOS, "cpu", process=CTL4.hook(EOS))
        row = torch.full((LMAX4,), PAD, dtype=torch.int64)
        row[:alone.shape[1]] = alone[0]
        assert torch.equal(ids[i], row), i
        toks = [t for t in row.tolist() if t != PAD]
        assert not CT.has_repeated_ngram(toks, 2) and 9 not in toks and EOS not in toks[:4]


# ---- 5. validation, mask bits, CLI defaults, ABI refusals ------------------------------------------------------------------------------------
def test_generation_controls_validation_and_mask_bits():
    assert CT.GenerationControls().neutral and CT.from_kwargs(3) is None
    assert CT.GenerationControls(suppress_tokens=[]).neutral
    assert not CT.GenerationControls(allowed_tokens=[5]).neutral
    for bad in (dict(no_repeat_ngram_size=9), dict(no_repeat_ngram_size=-1), dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0),
                dict(min_length=-1), dict(suppress_tokens=[3], eos_id=3), dict(suppress_tokens=[1], allowed_tokens=[2]), dict(suppress_tokens=[-2])):
        with pytest.raises(ValueError):
            CT.GenerationControls(**bad)
    c = CT.GenerationControls(suppress_tokens=[0, 31, 32, 40, 40])
    mk = c.mask(41, eos_id=3)
    assert mk.dtype == torch.int32 and mk.tolist() == [1 - (1 << 31), 1 | (1 << 8)]          # bit 31 set: the int32 pattern of 0x80000001
    with pytest.raises(ValueError):
        c.mask(40, eos_id=3)                                           # id 40 outside a vocabulary of 40
    with pytest.raises(ValueError):
        CT.GenerationControls(suppress_tokens=[3]).mask(41, eos_id=3)
    assert CT.GenerationControls().mask(41, eos_id=3) is None
    a = CT.GenerationControls(allowed_tokens=[5, 6])
    assert a.suppressed(10, eos_id=3) == [0, 1, 2, 4, 7, 8, 9]         # EOS is always kept
    with pytest.raises(ValueError):
        a.suppressed(10)
    # what a decode cannot serve: a vocabulary beyond the kernel's bound; for beam search a mask that leaves fewer than 2 tokens
    only_eos = CT.GenerationControls(allowed_tokens=[])
    assert not only_eos.neutral and only_eos.suppressed(41, 3) == [v for v in range(41) if v != 3]
    only_eos.check(41, 3, num_beams=1)
    CT.GenerationControls(allowed_tokens=[5]).check(41, 3, num_beams=4)
    with pytest.raises(ValueError, match="at least 2"):
        only_eos.check(41, 3, num_beams=4)
    with pytest.raises(ValueError):
        CT.GenerationControls(no_repeat_ngram_size=2).check(16385, 3)


def test_train_cli_controls_default_to_off():
    from kzv.train import parse_args
    a = parse_args([])
    assert (a.no_repeat_ngram_size, a.repetition_penalty, a.min_length) == (0, 1.0, 0)
    b = parse_args(["--no_repeat_ngram_size", "3", "--repetition_penalty", "1.2", "--min_length", "4"])
    assert (b.no_repeat_ngram_size, b.repetition_penalty, b.min_length) == (3, 1.2, 4)


def _args(**kw):
    base = dict(logits=256, ld=48, rows=4, vocab=41, ids=256, ld_ids=16, t=3, group=1, slot_image=None, slot_t=None, by_image=0, n_images=0,
                no_repeat_ngram_size=2, min_length=0, eos_id=3, normalise=0, repetition_penalty=1.2, reserved=0, suppress_mask=None)
    base.update(kw)
    return L.kzv_logits_process_args(**base)


@pytest.mark.parametrize("kw,needle", [
    (dict(no_repeat_ngram_size=9), b"no_repeat_ngram_size"), (dict(no_repeat_ngram_size=-1), b"no_repeat_ngram_size"),
    (dict(repetition_penalty=0.0), b"repetition_penalty"), (dict(repetition_penalty=-2.0), b"repetition_penalty"),
    (dict(vocab=16385, ld=16388), b"vocab"), (dict(logits=None), b"null"), (dict(ids=None), b"null"), (dict(ld=40), b"ld"),
    (dict(rows=0), b"rows"), (dict(slot_image=256), b"slot_image"), (dict(slot_image=256, slot_t=256, group=3, n_images=5), b"multiple"),
    (dict(t=-1), b"step"), (dict(min_length=2, eos_id=41), b"EOS"),
])
def test_logits_process_refuses_bad_arguments_before_any_launch(kw, needle):
    import os
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = L.load()
    before = lib.kzv_test_logits_process_calls()
    assert lib.kzv_logits_process(C.byref(_args(**kw)), None) == -1
    assert needle in lib.kzv_last_error(), lib.kzv_last_error()
    assert lib.kzv_logits_process(None, None) == -1
    assert lib.kzv_test_logits_process_calls() == before
    assert lib.kzv_beam_rank_logprobs(None, 41, 256, 1, 2, 41, 4, 256, 256, None) == -1 and b"beam_rank_logprobs" in lib.kzv_last_error()
    assert lib.kzv_stream_set_controls(None, None, None) == -3         # KZV_E_STATE outside a begun wave
