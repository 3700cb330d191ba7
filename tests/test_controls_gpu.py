"""Generation controls on the GPU (csrc/logits_process.hip: kzv_logits_process; csrc/token_search.hip: kzv_beam_rank_logprobs;
kzv_stream_set_controls; TrOCRModel.generate / generate_stream with no_repeat_ngram_size, repetition_penalty, min_length, suppress_tokens):

  1. the kernel in raw mode against kzv/controls.py::process_reference, ``torch.equal`` including the -inf positions and the columns
     between vocab and ld: vocab 41 / 777 / 4300 with ld = vocab + 4; the three addressing cases -- lockstep (one history longer than
     256), greedy slots (histories by image), beam slots (7 slots x 2 / 4 rows, histories by row) -- with two idle slots whose rows must
     come back untouched and per-slot step indices 0, 1, g - 2, g - 1, 36; every call repeated with changed inputs;
  2. the normalising mode followed by kzv_beam_rank_logprobs against log_softmax -> process_reference -> + beam score -> topk: indices
     equal, scores within 2e-5 * max(1, max |ref|) (the bound of test_beam_topk_matches_log_softmax_plus_topk); planted exact ties go
     to the smaller flat index; with every control neutral the pair gives what kzv_beam_topk gives on the same logits (asserted
     within that bound; observed on MI355X: the scores differ by exactly 0 at all three vocabularies -- the two kernels reduce a row
     in the same order);
  3. argument refusals: nothing launched (kzv_test_logits_process_calls stands still), message set;
  4. whole lockstep decodes: generate(**controls) on the device kernel against the same generate with process_reference substituted on
     the engine's own step scores (TrOCRModel.controls_impl = "reference"), greedy and 4 beams, 8 patch keys, tokens ``torch.equal``;
  5. generate_stream(**controls, slots=6) == generate(**controls): tokens ``torch.equal`` and, for beams, the winners' scores
     ``torch.equal`` (both sum the same processed log-probabilities in the same order); greedy, 2 and 4 beams; 8 and 164 patch keys;
     bf16 and, for one case, e4m3; the combination (no_repeat_ngram_size=2, repetition_penalty=1.2, suppress [pad]) and min_length=12
     alone; no running beam took padding in any beam case (asserted: the wave was decoded by the slots, never again by generate); the
     same for allowed_tokens (a set of 12 tokens, greedy and 4 beams), whose decodes stay inside the set, and a mask that leaves beam
     search fewer than 2 tokens is refused by the Python layer and by kzv_stream_set_controls;
  6. the conditions those comparisons need, asserted on generate's own results before any stream runs: (a) without controls at least a
     quarter of the 40 decodes hold a repeated 2-gram, (b) with the ban none does, (c) with min_length=12 no EOS sits before index 11 and
     at least one decode without it had one;
  7. alternatives under controls: entry 0 of every position is the emitted token and no alternative is a token the n-gram rule bans for
     that prefix (recomputed in Python);
  8. neutral is absent: with every control at its default generate_stream returns the ids, log-probabilities and step count of a call
     that does not pass them, and kzv_test_logits_process_calls stands still across it (it moves for a call with a control on);
  9. the fitted fixture against the oracle: greedy with no_repeat_ngram_size=2 (and 1, which changes a fitted line) token for token
     against the oracle's step-wise forward + process_reference + kzv/beam.py on the CPU, leaving out lines on which the oracle's own
     margin (chosen minus runner-up processed score, at any step of the line) is below LOGIT_TOL = 3e-2 of tests/test_trained_gpu.py; at
     most 3 of the 12 lines may be left out.  With the oracle alone on the CPU: 0 of 12 are left out (smallest margins 0.27 for g = 2,
     0.27 for g = 1; g = 2 changes no line of the fixture, g = 1 cuts line 0 at its repeated character).

The model of cases 4 - 8 is the recipe of tests/test_stream_beam_gpu.py (decoder 256 / 4 heads / FFN 768 / 3 layers on the tiny encoder,
recipe seed 7, CROSS_GAIN, PAD_BIAS and the 8-key EOS bias as there), in a copy: Lh = 38, 40 crops, 6 slots.  The 164-key EOS bias is this
file's own: with that file's + 0.4 no greedy or beam-4 decode of the 40 crops holds EOS before index 11 (0 of 40, observed on MI355X), so
condition (c) had nothing to show; the switch is as sharp as that file describes -- at + 0.6 every greedy decode is BOS EOS -- and + 0.5
sits inside it.  Observed on MI355X, of 40 decodes, repeated 2-gram without controls / with the ban, EOS before index 11 without controls
/ with min_length=12:
  8 keys, + 0.3:   bf16 greedy 30 / 0, 10 / 0;  2 beams 34 / 0, 6 / 0;  4 beams 36 / 0, 5 / 0;  e4m3 4 beams 37 / 0, 5 / 0
  164 keys, + 0.5: bf16 greedy 20 / 0, 20 / 0;  4 beams 11 / 0, 20 / 0        (+ 0.4: 40 / 0 and 0 / 0 for both)
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from kzv import _lib as L
from kzv import beam as BM
from kzv import controls as CT
from kzv.config import tiny_config
from kzv.data import build_decoder_dir, synthetic_batch
from kzv.model import TrOCRModel

from _trained import load as load_trained

pytestmark = pytest.mark.gpu
DEV = "cuda"
LH = 38
CROSS_GAIN = 24.0
EOS_BIAS = {8: 0.3, 164: 0.5}
PAD_BIAS = -8.0
LOGIT_TOL = 3e-2
NEG_INF = float("-inf")


@pytest.fixture(autouse=True)
def _default_mode_afterwards():
    yield
    L.load().kzv_set_decode_one_launch(-1)


def _st():
    return L.stream_handle()


def _process(scores, ld, vocab, ids, ctl, eos, *, t=0, slot_image=None, slot_t=None, group=1, by_image=0, n_images=0, normalise=0, mask=None):
    a = L.kzv_logits_process_args(logits=scores.data_ptr(), ld=ld, rows=scores.shape[0], vocab=vocab, ids=ids.data_ptr(), ld_ids=ids.stride(0), t=t,
                                  group=group, slot_image=L.ptr(slot_image), slot_t=L.ptr(slot_t), by_image=by_image, n_images=n_images,
                                  no_repeat_ngram_size=ctl.no_repeat_ngram_size, min_length=ctl.min_length, eos_id=eos, normalise=normalise,
                                  repetition_penalty=ctl.repetition_penalty, reserved=0, suppress_mask=L.ptr(mask))
    L.check(L.load().kzv_logits_process(C.byref(a), _st()), "logits_process")


def _histories(rows, width, vocab, gen):
    """token rows with many repeats (a dozen distinct tokens), so that n-grams recur and the penalty has duplicates"""
    pool = torch.randint(0, vocab, (12,), generator=gen)
    return pool[torch.randint(0, 12, (rows, width), generator=gen)].to(torch.int64)


def _controls(vocab, which):
    if which == "all":
        return CT.GenerationControls(no_repeat_ngram_size=4, repetition_penalty=1.3, min_length=3, suppress_tokens=[0, 1, 31, 32, vocab - 1])
    return CT.GenerationControls(no_repeat_ngram_size=1, repetition_penalty=0.8)


# ---- 1. raw mode == process_reference --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["all", "g1"])
@pytest.mark.parametrize("vocab", [41, 777, 4300])
def test_raw_mode_equals_process_reference_in_every_addressing_case(vocab, which):
    eos, ld = 3, vocab + 4
    ctl = _controls(vocab, which)
    g = ctl.no_repeat_ngram_size
    mask = ctl.mask(vocab, eos)
    mask_d = None if mask is None else mask.to(DEV)
    gen = torch.Generator().manual_seed(vocab + len(which))
    for rnd in range(2):                                               # the call repeated with changed inputs
        # (a) lockstep: row r, history ids[r][:t + 1]
        for t, width in ((0, 40), (1, 40), (max(g - 2, 0), 40), (g - 1, 40), (36, 40), (299, 320)):
            ids = _histories(5, width, vocab, gen)
            x = torch.randn(5, ld, generator=gen) * 3
            xd, idd = x.to(DEV), ids.to(DEV)
            _process(xd, ld, vocab, idd, ctl, eos, t=t, mask=mask_d)
            want = x.clone()
            want[:, :vocab] = CT.process_reference(x[:, :vocab], ids[:, :t + 1], ctl, eos)
            assert torch.equal(xd.cpu(), want), ("lockstep", t, rnd)
        # (b) greedy slots and (c) beam slots: 7 slots, two idle, step indices 0, 1, g - 2, g - 1, 36
        slot_image = torch.tensor([4, -1, 0, 9, 2, -1, 7], dtype=torch.int32)
        slot_t = torch.tensor([0, 5, 1, max(g - 2, 0), g - 1, 3, 36], dtype=torch.int32)
        if rnd:
            slot_image, slot_t = slot_image.flip(0).contiguous(), slot_t.flip(0).contiguous()
        for group, by_image in ((1, 1), (1, 0), (2, 0), (4, 0)):
            R = 7 * group
            ids = _histories(10 if by_image else R, 40, vocab, gen)
            x = torch.randn(R, ld, generator=gen) * 3
            xd, idd = x.to(DEV), ids.to(DEV)
            _process(xd, ld, vocab, idd, ctl, eos, t=1234, slot_image=slot_image.to(DEV), slot_t=slot_t.to(DEV), group=group, by_image=by_image,
                     n_images=10, mask=mask_d)
            want = x.clone()
            for r in range(R):
                s = r // group
                if slot_image[s] >= 0:
                    h = ids[int(slot_image[s]) if by_image else r, :int(slot_t[s]) + 1]
                    want[r:r + 1, :vocab] = CT.process_reference(x[r:r + 1, :vocab], h[None], ctl, eos)
            assert torch.equal(xd.cpu(), want), ("slots", group, by_image, rnd)
            idle = [r for r in range(R) if slot_image[r // group] < 0]
            assert len(idle) == 2 * group and torch.equal(xd.cpu()[idle], x[idle])


# ---- 2. normalising mode + ranking over log-probabilities ----------------------------------------------------------------------------------
@pytest.mark.parametrize("B,nb,vocab", [(3, 4, 41), (5, 2, 777), (6, 4, 4300)])
def test_normalise_then_rank_equals_log_softmax_process_topk(B, nb, vocab):
    lib = L.load()
    eos, ld, K, R = 3, vocab + 4, 2 * nb, B * nb
    ctl = _controls(vocab, "all")
    mask_d = ctl.mask(vocab, eos).to(DEV)
    gen = torch.Generator().manual_seed(B * vocab + nb)
    t = 17
    ids = _histories(R, 24, vocab, gen).to(DEV)
    buf = (torch.randn(R, ld, generator=gen) * 3).to(DEV)
    sc = torch.randn(B, nb, generator=gen).to(DEV)
    sc[0, 1:] = -1.0e9
    out_lp, out_ix = torch.empty(B, K, device=DEV), torch.empty(B, K, dtype=torch.int64, device=DEV)

    def device(scores, controls, mask):
        work = scores.clone()
        _process(work, ld, vocab, ids, controls, eos, t=t, normalise=1, mask=mask)
        L.check(lib.kzv_beam_rank_logprobs(work.data_ptr(), ld, sc.data_ptr(), B, nb, vocab, K, out_lp.data_ptr(), out_ix.data_ptr(), _st()), "rank")
        torch.cuda.synchronize()
        assert torch.equal(work[:, vocab:], scores[:, vocab:])           # the columns past the vocabulary stay
        return out_lp.clone(), out_ix.clone(), work

    def reference(scores, controls):
        logp = CT.process_reference(torch.log_softmax(scores[:, :vocab].float(), dim=-1), ids[:, :t + 1], controls, eos)
        return (logp.view(B, nb, vocab) + sc.unsqueeze(-1)).view(B, nb * vocab).topk(K, dim=1), logp

    lp, ix, work = device(buf, ctl, mask_d)
    (ref_lp, ref_ix), logp = reference(buf, ctl)
    tol = 2e-5 * max(1.0, ref_lp[ref_lp > -1e8].abs().max().item())
    assert torch.equal(ix, ref_ix)
    assert (lp - ref_lp).abs().max().item() < tol
    assert torch.equal(work[:, :vocab] == NEG_INF, logp == NEG_INF) and bool((logp == NEG_INF).any())
    fin = logp > NEG_INF
    assert (work[:, :vocab][fin] - logp[fin]).abs().max().item() < tol
    # planted exact ties: identical rows, histories and scores -> the smaller flat index (beam * vocab + token) first
    buf2, sc0 = buf.clone(), sc.clone()
    buf2[:nb] = buf2[0]
    ids[:nb] = ids[0]
    sc[0] = 0.25
    lp, ix, _ = device(buf2, ctl, mask_d)
    (_, _), logp = reference(buf2, ctl)
    best = int(logp[0].argmax())
    assert ix[0, :nb].tolist() == [k * vocab + best for k in range(nb)] and float(lp[0, 0]) == float(lp[0, nb - 1])
    # every control neutral: what kzv_beam_topk gives on the same logits
    sc.copy_(sc0)
    lp, ix, _ = device(buf, CT.GenerationControls(), None)
    t_lp, t_ix = torch.empty_like(out_lp), torch.empty_like(out_ix)
    L.check(lib.kzv_beam_topk(buf.data_ptr(), ld, sc.data_ptr(), B, nb, vocab, K, t_lp.data_ptr(), t_ix.data_ptr(), _st()), "beam_topk")
    torch.cuda.synchronize()
    print(f"neutral normalise + rank against kzv_beam_topk, vocab {vocab}: max |score difference| {(lp - t_lp).abs().max().item():.3g}")
    assert torch.equal(ix, t_ix) and (lp - t_lp).abs().max().item() < tol


# ---- 3. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch():
    lib = L.load()
    x = torch.zeros(4, 48, device=DEV)
    ids = torch.zeros(4, 16, dtype=torch.int64, device=DEV)
    si = torch.zeros(4, dtype=torch.int32, device=DEV)
    base = dict(logits=x.data_ptr(), ld=48, rows=4, vocab=41, ids=ids.data_ptr(), ld_ids=16, t=3, group=1, slot_image=None, slot_t=None, by_image=0,
                n_images=0, no_repeat_ngram_size=2, min_length=0, eos_id=3, normalise=0, repetition_penalty=1.2, reserved=0, suppress_mask=None)
    before = lib.kzv_test_logits_process_calls()
    for kw, needle in ((dict(no_repeat_ngram_size=9), b"no_repeat_ngram_size"), (dict(repetition_penalty=0.0), b"repetition_penalty"),
                       (dict(vocab=16385, ld=16388), b"vocab"), (dict(logits=None), b"null"), (dict(ids=None), b"null"), (dict(ld=40), b"ld"),
                       (dict(slot_image=si.data_ptr()), b"slot_image"), (dict(slot_image=si.data_ptr(), slot_t=si.data_ptr(), group=3, n_images=4), b"multiple")):
        assert lib.kzv_logits_process(C.byref(L.kzv_logits_process_args(**dict(base, **kw))), _st()) == -1, kw
        assert needle in lib.kzv_last_error(), (kw, lib.kzv_last_error())
    assert lib.kzv_test_logits_process_calls() == before
    torch.cuda.synchronize()
    assert torch.equal(x, torch.zeros_like(x))
    assert lib.kzv_logits_process(C.byref(L.kzv_logits_process_args(**base)), _st()) == 0 and lib.kzv_test_logits_process_calls() == before + 1
    torch.cuda.synchronize()


# ---- the model of cases 4 - 8 ------------------------------------------------------------------------------------------------------------------
def _cfg(keys):
    w = {8: 64, 164: 1312}[keys]
    c = dataclasses.replace(tiny_config(), image_w=w, dec_hidden=256, dec_heads=4, dec_ffn=768, dec_layers=3)
    assert c.num_patches == keys
    return c


_models = {}
PAD = tiny_config().pad_id
COMBO = dict(no_repeat_ngram_size=2, repetition_penalty=1.2, suppress_tokens=[PAD])
MINLEN = dict(min_length=12)
NGRAM = dict(no_repeat_ngram_size=2)
CONTROLS = {"none": {}, "combo": COMBO, "minlen": MINLEN, "ngram": NGRAM}


@pytest.fixture(scope="module")
def decoder_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("dec"))


def _model(keys, decoder_dir):
    if keys not in _models:
        cfg = _cfg(keys)
        m = TrOCRModel(cfg.encoder_config_dict(), build_decoder_dir(decoder_dir + f"/{keys}", cfg), init_seed=7, load_tokenizer=False)
        views = m.state_dict_views()
        for k in [k for k in views if "crossattention.output.dense.weight" in k]:
            views[k] *= CROSS_GAIN
        views["decoder.lm_head.bias"][cfg.eos_id] += EOS_BIAS[keys]
        views["decoder.lm_head.bias"][cfg.pad_id] += PAD_BIAS
        m.eval()
        px = torch.from_numpy(synthetic_batch(cfg, 40, LH, seed=3)[0]).cuda()
        _models[keys] = (cfg, m, px, {})
    return _models[keys]


def _pad(ids, pad_id, width=LH):
    out = torch.full((ids.shape[0], width), pad_id, dtype=torch.int64, device=ids.device)
    out[:, :ids.shape[1]] = ids
    return out


def _tokens(row, cfg):
    return [t for t in row if t != cfg.pad_id]


def _lockstep(keys, fmt, nb, name, decoder_dir):
    """generate(num_beams=nb, **CONTROLS[name]) of the 40 crops, padded to LH, and the winners' scores (beams); computed once."""
    cfg, m, px, cache = _model(keys, decoder_dir)
    m.set_decode_weights(fmt)
    if (fmt, nb, name) not in cache:
        if nb == 1:
            ids, sc = m.generate(px, max_length=LH, **CONTROLS[name]), None
        else:
            ids, sc = m.generate(px, max_length=LH, num_beams=nb, return_scores=True, **CONTROLS[name])
        assert m.decode_step_impl == "one-launch" and m.decode_weights_impl == fmt
        cache[(fmt, nb, name)] = (_pad(ids, cfg.pad_id), sc)
    return cfg, m, px, cache[(fmt, nb, name)]


def _conditions(keys, fmt, nb, decoder_dir):
    """Case 6, on generate's own results: counts printed, then asserted."""
    cfg = _cfg(keys)
    base = _lockstep(keys, fmt, nb, "none", decoder_dir)[3][0].tolist()
    combo = _lockstep(keys, fmt, nb, "combo", decoder_dir)[3][0].tolist()
    minlen = _lockstep(keys, fmt, nb, "minlen", decoder_dir)[3][0].tolist()
    rep = sum(CT.has_repeated_ngram(_tokens(r, cfg), 2) for r in base)
    rep_on = sum(CT.has_repeated_ngram(_tokens(r, cfg), 2) for r in combo)
    early = sum(cfg.eos_id in r[:11] for r in base)
    early_on = sum(cfg.eos_id in r[:11] for r in minlen)
    print(f"{keys} keys, {fmt}, {nb} beam(s): repeated 2-gram in {rep} of 40 decodes, {rep_on} with the ban; EOS before index 11 in {early}, "
          f"{early_on} with min_length=12; padding inside a combo line: {sum(cfg.pad_id in r[:len(_tokens(r, cfg))] for r in combo)}")
    assert rep * 4 >= 40, rep                                          # (a)
    assert rep_on == 0                                                 # (b)
    assert early_on == 0 and early >= 1, (early, early_on)             # (c)


# ---- 4. device kernel == torch statement inside whole lockstep decodes ------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [1, 4])
def test_generate_on_the_kernel_equals_generate_on_process_reference(nb, decoder_dir):
    cfg, m, px, _ = _model(8, decoder_dir)
    m.set_decode_weights("bf16")
    kw = dict(no_repeat_ngram_size=2, repetition_penalty=1.2, min_length=6, suppress_tokens=[cfg.pad_id, 9])
    lib = L.load()
    before = lib.kzv_test_logits_process_calls()
    dev = m.generate(px, max_length=LH, num_beams=nb, **kw)
    launched = lib.kzv_test_logits_process_calls() - before
    assert launched == m.last_generate_steps                           # one launch per decoder step
    m.controls_impl = "reference"
    try:
        before = lib.kzv_test_logits_process_calls()
        ref = m.generate(px, max_length=LH, num_beams=nb, **kw)
        assert lib.kzv_test_logits_process_calls() == before             # the substitution launches no process kernel
    finally:
        m.controls_impl = "device"
    assert dev.shape == ref.shape and torch.equal(dev, ref)
    plain = _pad(m.generate(px, max_length=LH, num_beams=nb), cfg.pad_id)
    assert int((plain != _pad(dev, cfg.pad_id)).any(dim=1).sum()) >= 10      # the controls act on this model
    for r in dev.tolist():
        toks = _tokens(r, cfg)
        assert not CT.has_repeated_ngram(toks, 2) and 9 not in toks and cfg.eos_id not in toks[:6]


# ---- 5. / 6. stream == lockstep under controls ----------------------------------------------------------------------------------------------
CASES = [(8, "bf16", 1), (8, "bf16", 2), (8, "bf16", 4), (164, "bf16", 1), (164, "bf16", 4), (8, "e4m3", 4)]
# allowed_tokens on the GPU: a character set of 12 tokens (EOS is kept by the rule itself; BOS and padding are outside it)
CONTROLS["allowed"] = dict(allowed_tokens=[5, 9, 17, 20, 33, 48, 64, 77, 90, 101, 130, 155])


def _stream_case(keys, fmt, nb, name, decoder_dir):
    cfg, m, px, (want, want_sc) = _lockstep(keys, fmt, nb, name, decoder_dir)
    if nb == 1:
        got = m.generate_stream(px, max_length=LH, slots=6, **CONTROLS[name])
        assert m.stream_decode_impl == "slot-refill"
    else:
        got, sc = m.generate_stream(px, max_length=LH, slots=6, num_beams=nb, return_scores=True, **CONTROLS[name])
        assert m.stream_beam_impl == "slot-refill"
        # no running beam took padding (suppressed outright by combo / allowed; under min_length alone PAD_BIAS keeps it out of the
        # ranks, as in tests/test_stream_beam_gpu.py): the wave was decoded by the slots, not again by generate
        assert m.last_stream_pad_fallbacks == 0
        assert torch.equal(sc, want_sc)
    assert torch.equal(_pad(got, cfg.pad_id), want)
    assert m.last_stream_steps > 0
    return cfg, got


@pytest.mark.parametrize("name", ["combo", "minlen"])
@pytest.mark.parametrize("keys,fmt,nb", CASES)
def test_generate_stream_equals_generate_under_controls(keys, fmt, nb, name, decoder_dir):
    _conditions(keys, fmt, nb, decoder_dir)
    _stream_case(keys, fmt, nb, name, decoder_dir)


@pytest.mark.parametrize("nb", [1, 4])
def test_allowed_tokens_stream_equals_generate_and_stays_inside_the_set(nb, decoder_dir):
    cfg, got = _stream_case(8, "bf16", nb, "allowed", decoder_dir)
    keep = set(CONTROLS["allowed"]["allowed_tokens"]) | {cfg.eos_id, cfg.bos_id, cfg.pad_id}
    rows = got.tolist()
    assert all(set(r) <= keep for r in rows) and all(cfg.bos_id not in r[1:] for r in rows)
    base = _lockstep(8, "bf16", nb, "none", decoder_dir)[3][0].tolist()
    assert sum(not set(r) <= keep for r in base) >= 10                  # without the restriction the decodes leave the set
    # a mask that leaves beam search fewer than 2 tokens is refused before anything runs, by the Python layer and by the handle
    m, px = _model(8, decoder_dir)[1:3]
    if nb > 1:
        for call in (m.generate, lambda x, **kw: m.generate_stream(x, slots=6, **kw)):
            with pytest.raises(ValueError, match="at least 2"):
                call(px, max_length=LH, num_beams=nb, allowed_tokens=[])
        lib = L.load()
        only_eos = CT.GenerationControls(allowed_tokens=[]).mask(cfg.vocab, cfg.eos_id)
        cc = L.kzv_logits_controls(repetition_penalty=1.0, suppress_mask=only_eos.data_ptr())
        assert lib.kzv_stream_set_controls(m._h, C.byref(cc), _st()) == -1 and b"at least 2" in lib.kzv_last_error()      # (the last wave was a beam wave)
    else:
        assert m.generate(px[:2], max_length=LH, allowed_tokens=[]).tolist() == [[cfg.bos_id, cfg.eos_id]] * 2      # greedy: EOS at once


# ---- 7. alternatives under controls -----------------------------------------------------------------------------------------------------------
def test_alternatives_are_those_of_the_processed_row(decoder_dir):
    cfg, m, px, (want, _) = _lockstep(8, "bf16", 1, "ngram", decoder_dir)
    ids, lp, a_ids, a_lp = m.generate_stream(px, max_length=LH, slots=6, top_k=5, **NGRAM)
    assert torch.equal(_pad(ids, cfg.pad_id), want)
    rows, alts, alp, lps = ids.tolist(), a_ids.tolist(), a_lp.tolist(), lp.tolist()
    checked = banned_seen = 0
    for i, r in enumerate(rows):
        toks = _tokens(r, cfg)
        assert not CT.has_repeated_ngram(toks, 2)
        for j in range(1, len(toks)):
            assert alts[i][j][0] == toks[j] and abs(alp[i][j][0] - lps[i][j]) <= 1e-4      # (the bound of tests/test_alternatives_gpu.py)
            ban = set(CT.banned_ngram_tokens(toks[:j], 2))
            banned_seen += bool(ban)
            assert not ban & set(alts[i][j]), (i, j)
            assert all(v > NEG_INF for v in alp[i][j])
            checked += 1
    assert checked > 100 and banned_seen > 10


# ---- 8. neutral is absent -----------------------------------------------------------------------------------------------------------------------
def test_neutral_controls_launch_nothing_and_change_nothing(decoder_dir):
    cfg, m, px, _ = _model(8, decoder_dir)
    m.set_decode_weights("bf16")
    lib = L.load()
    ids0, lp0 = m.generate_stream(px, max_length=LH, slots=6, return_logprobs=True)
    steps0 = m.last_stream_steps
    before = lib.kzv_test_logits_process_calls()
    ids1, lp1 = m.generate_stream(px, max_length=LH, slots=6, return_logprobs=True, no_repeat_ngram_size=0, repetition_penalty=1.0, min_length=0,
                                  suppress_tokens=None, allowed_tokens=None)
    assert lib.kzv_test_logits_process_calls() == before
    assert torch.equal(ids0, ids1) and torch.equal(lp0, lp1) and m.last_stream_steps == steps0
    b0 = m.generate_stream(px, max_length=LH, slots=6, num_beams=4)
    b1 = m.generate_stream(px, max_length=LH, slots=6, num_beams=4, suppress_tokens=[], repetition_penalty=1.0)
    assert lib.kzv_test_logits_process_calls() == before and torch.equal(b0, b1)
    m.generate_stream(px, max_length=LH, slots=6, no_repeat_ngram_size=2)
    assert lib.kzv_test_logits_process_calls() > before                  # the counter does see a control that is on
    # the handle refuses what the Python layer would have refused first
    h = m._h
    for cc in (L.kzv_logits_controls(no_repeat_ngram_size=9, repetition_penalty=1.0), L.kzv_logits_controls(repetition_penalty=0.0),
               L.kzv_logits_controls(repetition_penalty=1.0, min_length=-1)):
        assert lib.kzv_stream_set_controls(h, C.byref(cc), _st()) == -1
    eos_mask = CT.GenerationControls(suppress_tokens=[cfg.eos_id]).mask(cfg.vocab)
    cc = L.kzv_logits_controls(repetition_penalty=1.0, suppress_mask=eos_mask.data_ptr())
    assert lib.kzv_stream_set_controls(h, C.byref(cc), _st()) == -1 and b"EOS" in lib.kzv_last_error()


# ---- 9. the fitted fixture against the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [2, 1])
def test_fitted_fixture_greedy_with_ngram_ban_equals_the_oracle(g, tmp_path):
    from oracle import trocr_oracle as O
    gold, cfg, sd, data = load_trained()
    Lh = int(gold["label_len"])
    px = np.concatenate([data["fit"][0], data["unseen"][0]])
    ctl = CT.GenerationControls(no_repeat_ngram_size=g)
    raw = O.stepwise_logits(cfg, O.leaf_state_dict(sd, requires_grad=False), px, repeat=1)
    margins = []

    def step(t, ids):
        y = CT.process_reference(torch.as_tensor(raw(t, ids)).float(), ids[:, :t + 1], ctl, cfg.eos_id)
        top = y.topk(2, dim=-1)[0]
        margins.append(top[:, 0] - top[:, 1])
        return y
    want = BM.greedy(step, px.shape[0], Lh, cfg.pad_id, cfg.bos_id, cfg.eos_id, "cpu").numpy()
    mg = torch.stack(margins, 1).numpy()                                # [12, steps]: step t chose column t + 1
    mins = []
    for b in range(12):
        row = want[b].tolist()
        n_live = row.index(cfg.eos_id) if cfg.eos_id in row else len(row) - 1      # steps taken while the line was open
        mins.append(float(mg[b, :n_live].min()))
    sure = np.array(mins) >= LOGIT_TOL
    print(f"g = {g}: {int((~sure).sum())} of 12 lines left out; smallest margin {min(mins):.3g}")
    assert (~sure).sum() <= 3
    plain = BM.greedy(lambda t, ids: torch.as_tensor(raw(t, ids)).float(), 12, Lh, cfg.pad_id, cfg.bos_id, cfg.eos_id, "cpu").numpy()
    if g == 1:                                                          # this control changes a fitted line
        w = max(plain.shape[1], want.shape[1])
        assert not np.array_equal(np.pad(plain, ((0, 0), (0, w - plain.shape[1])), constant_values=cfg.pad_id),
                                  np.pad(want, ((0, 0), (0, w - want.shape[1])), constant_values=cfg.pad_id))
    m = TrOCRModel(cfg.encoder_config_dict(), build_decoder_dir(str(tmp_path / "dec"), cfg), load_tokenizer=False)
    m.load_state_dict(sd, strict=True)
    m.eval()
    got = m.generate(torch.from_numpy(px), max_length=Lh, num_beams=1, no_repeat_ngram_size=g).cpu().numpy()
    w = max(got.shape[1], want.shape[1])
    got = np.pad(got, ((0, 0), (0, w - got.shape[1])), constant_values=cfg.pad_id)
    want = np.pad(want, ((0, 0), (0, w - want.shape[1])), constant_values=cfg.pad_id)
    assert np.array_equal(got[sure], want[sure])
