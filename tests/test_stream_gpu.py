"""Slot-refill greedy decoding on the GPU (TrOCRModel.generate_stream; include/kzv.h: kzv_stream_*; csrc/decode_fused.hip: the slot
instances of the one-launch step; csrc/token_search.hip: selection and seating):

  1. the selection and seating kernels alone against their torch statement (kzv/stream.py), state for state over 50 steps of seeded
     logits with planted ties, planted EOS and several lines ending in one step; log-probabilities against torch.log_softmax to 1e-5;
     7, 70 and 300 slots (one wave of slots, several, a second seating pass of 256) and 157 / 4,300 columns (one column sweep, two);
  2. generate_stream == generate(num_beams=1) cut at the limits, token for token: 8 and 164 patch keys (the one-pass and the chunked
     instances), bf16 and e4m3 weights, with and without limits;
  3. its log-probabilities against the teacher-forced pass (align) on the same ids, within 2e-2: twice the 1e-2 that
     tests/test_decode_fused_gpu.py allows between the cached step's logits and that pass -- a log-probability is a logit minus a
     log-sum-exp of logits;
  4. more slots than compute units and idle slots: 300 slots for 310 images, 1 image on 6 slots, as many images as slots;
  5. several waves in one call equal one wave;
  6. the fallback: a 64-wide decoder, or the one-launch mode off, runs generate() and says so;
  7. recognize_many on the fitted fixture against recognize(num_beams=1);
  8. a wave given every option at once (controls + mask, language model, prefixes, alternatives / n-best) is followed on the same handle
     by a wave given none, which equals a fresh handle's and launches no score node; the lockstep score nodes with group = 0.
The decoder is the one-launch tests' (hidden 256, 4 heads, FFN 768, 3 layers) on the tiny encoder: Lh = 38.
Observed on MI355X: kernel log-probabilities within 7.2e-7 of torch.log_softmax (1.4e-6 at 4,300 columns); with the EOS bias + 0.5 the engine's static decodes
stop by EOS at columns 11 / 14 / 24 / 32 (8 keys, bf16; fewer distinct stops with e4m3 or 164 keys), 27 of 40 lines ending by EOS before
their limit and 10 - 12 at it; 40 lines on 6 slots take 61 - 96 steps where lockstep batches of 6 take 70 - 135; stream
log-probabilities within 2.6e-3 (8 keys) and 2.1e-3 (164 keys) of the teacher-forced pass."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from kzv import _lib as L
from kzv import stream as ST
from kzv.config import tiny_config
from kzv.data import build_decoder_dir, synthetic_batch
from kzv.model import TrOCRModel

from _trained import load as load_trained

pytestmark = pytest.mark.gpu
LH = 38
EOS_BIAS = 0.5          # raised LM-head bias of EOS: an untrained model otherwise never stops (its top-2 gaps are ~1e-4)
LP_TOL = 2e-2


@pytest.fixture(autouse=True)
def _default_mode_afterwards():
    yield
    L.load().kzv_set_decode_one_launch(-1)


def _cfg(keys):
    w = {8: 64, 164: 1312}[keys]
    c = dataclasses.replace(tiny_config(), image_w=w, dec_hidden=256, dec_heads=4, dec_ffn=768, dec_layers=3)
    assert c.num_patches == keys
    return c


_models = {}


@pytest.fixture(scope="module")
def decoder_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("dec"))


def _model(keys, decoder_dir):
    """One model per crop width for the whole module (recipe seed 7, EOS bias raised), 40 crops, and its static decodes per format."""
    if keys not in _models:
        cfg = _cfg(keys)
        m = TrOCRModel(cfg.encoder_config_dict(), build_decoder_dir(decoder_dir + f"/{keys}", cfg), init_seed=7, load_tokenizer=False)
        m.state_dict_views()["decoder.lm_head.bias"][cfg.eos_id] += EOS_BIAS
        m.eval()
        px = torch.from_numpy(synthetic_batch(cfg, 40, LH, seed=3)[0]).cuda()
        _models[keys] = (cfg, m, px, {})
    return _models[keys]


def _static(keys, fmt, decoder_dir):
    cfg, m, px, cache = _model(keys, decoder_dir)
    m.set_decode_weights(fmt)
    if fmt not in cache:
        cache[fmt] = _pad(m.generate(px, max_length=LH, num_beams=1), cfg.pad_id)
        assert m.decode_step_impl == "one-launch" and m.decode_weights_impl == fmt
    return cfg, m, px, cache[fmt]


def _pad(ids, pad_id, width=LH):
    out = torch.full((ids.shape[0], width), pad_id, dtype=torch.int64, device=ids.device)
    out[:, :ids.shape[1]] = ids
    return out


def _cut(ids, limits, pad_id):
    out = ids.clone()
    for i, k in enumerate(limits.tolist()):
        out[i, k:] = pad_id
    return out


def _limits(n, seed):
    g = torch.Generator().manual_seed(seed)
    lim = torch.randint(2, LH + 1, (n,), generator=g, dtype=torch.int32)
    lim[0], lim[n - 1] = 2, LH                              # both ends
    return lim


# ---- 1. the kernels against the statement --------------------------------------------------------------------------------------------
# (7, 157, 30): one wave of slots, one seating pass, one column sweep.  (70, 157, 300): ended flags in two waves.  (300, 4300, 1500): a
# second seating pass of 256 slots with its carry, and a second column sweep beyond 8 x 256 = 2,048 columns.  Every live line ends at
# steps 4, 13, ..., 49 (six times), so N <= 5 slots images are all seated and ended by the last step.
@pytest.mark.parametrize("slots,V,N", [(7, 157, 30), (70, 157, 300), (300, 4300, 1500)])
def test_select_and_seat_kernels_equal_the_torch_statement(slots, V, N):
    lib = L.load()
    ML, pad, bos, eos = 12, 1, 2, 3
    g = torch.Generator().manual_seed(11)
    limits = torch.randint(2, ML + 1, (N,), generator=g, dtype=torch.int32)
    lim_d = limits.cuda()
    ref = ST.new_state(N, slots, ML, pad, bos, "cpu", want_logprobs=True)
    dev = {k: torch.zeros_like(v).cuda() for k, v in ref.items()}
    dev["out_ids"].copy_(ref["out_ids"])
    scratch = torch.zeros(2 * slots, dtype=torch.int32, device="cuda")
    st = L.kzv_stream_state(slots=slots, n_images=N, max_len=ML, vocab=V, bos_id=bos, eos_id=eos, pad_id=pad,
                            slot_image=dev["slot_image"].data_ptr(), slot_t=dev["slot_t"].data_ptr(), tokens=dev["tokens"].data_ptr(),
                            posids=dev["posids"].data_ptr(), counters=dev["counters"].data_ptr(), scratch=scratch.data_ptr(),
                            out_ids=dev["out_ids"].data_ptr(), ld_ids=ML, out_logprob=dev["out_logprob"].data_ptr(), ld_logprob=ML,
                            limit=lim_d.data_ptr())
    L.check(lib.kzv_stream_seat_first(C.byref(st), L.stream_handle()), "seat_first")
    for k in ref:
        assert torch.equal(dev[k].cpu(), ref[k]), ("start", k)
    worst_lp, seen_multi, seen_tie, seen_eos = 0.0, 0, 0, 0
    for step in range(50):
        x = torch.randn(slots, V, generator=g)
        x[:, pad] = -20.0
        for b in range(slots):
            r = int(torch.randint(0, 6, (1,), generator=g))
            if r == 0:                                      # an exact tie of the maximum: the first column wins
                cols = torch.randperm(V - 4, generator=g)[:3] + 4
                x[b, cols] = x[b].max() + 1.0
                seen_tie += 1
            elif r == 1:                                    # EOS as the maximum, tied with a later column
                x[b, eos] = x[b, 100] = x[b].max() + 0.5
                seen_eos += 1
        if step % 9 == 4:                                   # every live line ends in this step
            x[:, eos] = 50.0
        xd = x.cuda()
        before = ref["slot_image"].clone()
        L.check(lib.kzv_stream_update(C.byref(st), xd.data_ptr(), V, L.stream_handle()), "stream_update")
        ref = ST.select_seat(x, ref, n_images=N, max_len=ML, pad_id=pad, bos_id=bos, eos_id=eos, limit=limits)
        seen_multi += int(((ref["slot_image"] != before).sum() > 1))
        for k in ("slot_image", "slot_t", "tokens", "posids", "counters", "out_ids"):
            assert torch.equal(dev[k].cpu(), ref[k]), (step, k, dev[k].cpu(), ref[k])
        worst_lp = max(worst_lp, float((dev["out_logprob"].cpu() - ref["out_logprob"]).abs().max()))
    assert ref["counters"].tolist()[:2] == [N, N] and (ref["slot_image"] == -1).all()
    assert seen_multi >= 3 and seen_tie >= 5 and seen_eos >= 5
    print(f"log-probabilities: largest difference to torch.log_softmax {worst_lp:.2e}; {ref['counters'][2]} steps for {N} lines on {slots} slots")
    assert worst_lp <= 1e-5


# ---- 2. stream == static ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_limits", [True, False], ids=["limits", "nolimits"])
@pytest.mark.parametrize("fmt", ["bf16", "e4m3"])
@pytest.mark.parametrize("keys", [8, 164])
def test_stream_equals_static(decoder_dir, keys, fmt, with_limits):
    cfg, m, px, static = _static(keys, fmt, decoder_dir)
    n = px.shape[0]
    limits = _limits(n, 17)
    # the engine's own static result must exercise both ways a line ends
    length = (static != cfg.pad_id).sum(1).cpu()
    has_eos = (static == cfg.eos_id).any(1).cpu()
    by_eos = has_eos & (length < limits)
    by_limit = ~has_eos | (length > limits)
    print(f"{keys} keys, {fmt}: EOS stops at {sorted(set(length[has_eos].tolist()))}; {int(by_eos.sum())} lines end by EOS before their limit, "
          f"{int(by_limit.sum())} at their limit")
    assert int(by_eos.sum()) >= 1 and int(by_limit.sum()) >= 1
    got = m.generate_stream(px, max_length=LH, slots=6, limits=limits if with_limits else None)
    assert m.stream_decode_impl == "slot-refill" and m.decode_weights_impl == fmt
    want = _cut(static, limits, cfg.pad_id) if with_limits else static
    assert got.shape[1] == max(2, int((want != cfg.pad_id).sum(1).max()))
    assert torch.equal(_pad(got, cfg.pad_id), want)
    useful = int((want != cfg.pad_id).sum()) - n
    print(f"   {m.last_stream_steps} steps on 6 slots for {useful} tokens (lockstep batches of 6: {sum(int((want[a:a + 6] != cfg.pad_id).sum(1).max()) - 1 for a in range(0, n, 6))})")
    assert -(-useful // 6) <= m.last_stream_steps <= ST.step_bound(n, 6, LH)


# ---- 3. log-probabilities ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keys", [8, 164])
def test_stream_logprobs_against_the_teacher_forced_pass(decoder_dir, keys):
    cfg, m, px, _ = _static(keys, "bf16", decoder_dir)
    limits = _limits(px.shape[0], 23)
    ids, lp = m.generate_stream(px, max_length=LH, slots=6, limits=limits, return_logprobs=True)
    assert lp.shape == ids.shape
    sc = m.align(px, ids)
    live = sc["live"]
    assert int(live.sum()) > 40
    err = float((lp[:, 1:] - sc["logprob"])[live].abs().max())
    print(f"{keys} keys: largest |stream log-probability - teacher-forced| on {int(live.sum())} live positions: {err:.3e}")
    assert bool((lp[:, 1:][~live] == 0).all()) and bool((lp[:, 0] == 0).all())
    assert err <= LP_TOL


# ---- 4. more slots than compute units, idle slots -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,slots", [(310, 300), (1, 6), (6, 6)])
def test_many_slots_and_idle_slots(decoder_dir, n, slots):
    cfg, m, _, _ = _model(8, decoder_dir)
    m.set_decode_weights("bf16")
    px = torch.from_numpy(synthetic_batch(cfg, n, LH, seed=29)[0]).cuda()
    limits = _limits(n, 31) if n > 1 else None
    static = _pad(m.generate(px, max_length=LH, num_beams=1), cfg.pad_id)
    want = _cut(static, limits, cfg.pad_id) if limits is not None else static
    got = m.generate_stream(px, max_length=LH, slots=slots, limits=limits)
    assert m.stream_decode_impl == "slot-refill"
    assert torch.equal(_pad(got, cfg.pad_id), want)
    assert m.last_stream_steps <= ST.step_bound(n, slots, LH)
    print(f"{n} images on {slots} slots: {m.last_stream_steps} steps")


# ---- 5. waves ----------------------------------------------------------------------------------------------------------------------------
def test_three_waves_equal_one(decoder_dir):
    cfg, m, px, _ = _static(8, "bf16", decoder_dir)
    limits = _limits(px.shape[0], 37)
    one, lp1 = m.generate_stream(px, max_length=LH, slots=6, limits=limits, return_logprobs=True)
    steps_one = m.last_stream_steps
    per_image = cfg.dec_layers * 2 * cfg.num_patches * cfg.dec_hidden * 2
    seen = []
    orig = m._stream_wave
    m._stream_wave = lambda px_, *a: (seen.append(px_.shape[0]), orig(px_, *a))[1]
    try:
        # from an iterable of host batches of another size than the wave
        three, lp3 = m.generate_stream([px[:7].cpu(), px[7:29].cpu(), px[29:].cpu()], max_length=LH, slots=6, limits=limits, return_logprobs=True,
                                       pool_bytes=18 * per_image)
    finally:
        del m._stream_wave
    assert seen == [18, 18, 4]
    assert torch.equal(one, three) and torch.equal(lp1, lp3)
    assert m.last_stream_steps >= steps_one


# ---- 6. the fallback -----------------------------------------------------------------------------------------------------------------------
def test_fallback_is_static_generation(decoder_dir, tmp_path):
    lib = L.load()
    cfg = tiny_config()                                     # 64-wide decoder: no one-launch step
    m = TrOCRModel(cfg.encoder_config_dict(), build_decoder_dir(str(tmp_path / "dec"), cfg), init_seed=7, load_tokenizer=False)
    m.state_dict_views()["decoder.lm_head.bias"][cfg.eos_id] += EOS_BIAS
    m.eval()
    px = torch.from_numpy(synthetic_batch(cfg, 13, LH, seed=3)[0]).cuda()
    limits = _limits(13, 41)
    static = _pad(m.generate(px, max_length=LH, num_beams=1), cfg.pad_id)
    got = m.generate_stream(px, max_length=LH, slots=5, limits=limits)
    assert m.stream_decode_impl == "static"
    assert torch.equal(_pad(got, cfg.pad_id), _cut(static, limits, cfg.pad_id))
    assert torch.equal(_pad(m.generate_stream(px, max_length=LH, slots=5), cfg.pad_id), static)
    # the 256-wide model with the one-launch mode off
    cfg2, m2, px2, static2 = _static(8, "bf16", decoder_dir)
    L.check(lib.kzv_set_decode_one_launch(0), "mode")
    got2 = m2.generate_stream(px2, max_length=LH, slots=6)
    assert m2.stream_decode_impl == "static"
    mode0 = _pad(m2.generate(px2, max_length=LH, num_beams=1), cfg2.pad_id)
    assert torch.equal(_pad(got2, cfg2.pad_id), mode0)
    L.check(lib.kzv_set_decode_one_launch(-1), "mode")
    assert m2.stream_decode_impl == "slot-refill"


def test_begin_refuses_a_pool_smaller_than_the_slots(decoder_dir):
    lib = L.load()
    cfg, m, px, _ = _model(8, decoder_dir)
    m._check_inputs(px[:1])
    m._bind(6, LH)
    out = torch.full((4, LH), cfg.pad_id, dtype=torch.int64, device="cuda")
    assert lib.kzv_stream_begin(m._h, 4, 4, LH, cfg.bos_id, cfg.eos_id, out.data_ptr(), LH, None, 0, None, L.stream_handle()) == -1
    assert b"smaller than the 6 slots" in lib.kzv_last_error()
    assert lib.kzv_stream_begin(m._h, 6, 4, LH + 1, cfg.bos_id, cfg.eos_id, out.data_ptr(), LH + 1, None, 0, None, L.stream_handle()) == -1
    assert lib.kzv_stream_step(m._h, 0, L.stream_handle()) == -3          # a refused begin leaves no wave to step


# ---- 7. recognize_many -----------------------------------------------------------------------------------------------------------------
def test_recognize_many_on_the_fitted_fixture(tmp_path):
    g, cfg, sd, data = load_trained()
    m = TrOCRModel(cfg.encoder_config_dict(), build_decoder_dir(str(tmp_path / "dec"), cfg), load_tokenizer=True)
    m.load_state_dict(sd, strict=True)
    m.eval()
    px = torch.from_numpy(np.concatenate([data["fit"][0], data["unseen"][0]]))
    assert px.shape[0] == 12
    many = m.recognize_many(px, max_length=int(g["label_len"]), slots=5)
    assert m.stream_decode_impl == "static"
    one = m.recognize(px, num_beams=1, max_length=int(g["label_len"]))
    worst = 0.0
    for a, b in zip(many, one):
        assert a["text"] == b["text"] and a["tokens"] == b["tokens"] and a["token_strings"] == b["token_strings"]
        assert "centroids" not in a and "peak_patches" not in a
        assert len(a["logprobs"]) == len(b["logprobs"])
        worst = max(worst, abs(a["confidence"] - b["confidence"]))
    print(f"recognize_many against recognize(num_beams=1): largest confidence difference {worst:.3e}")
    assert worst <= LP_TOL


# ---- 8. a wave's options end with the wave; the lockstep score nodes never read `group` ------------------------------------------------------
def test_a_wave_with_every_option_leaves_nothing_to_the_next(decoder_dir):
    """Wave 1 sets everything a wave can be given at once -- controls with a suppress mask, a 2-gram language model, 2-token prefixes,
    and the top-2 alternatives (greedy) or the 2-best list (2 beams); wave 2 on the SAME handle sets nothing and must be the plain wave of
    a fresh handle, ids and log-probabilities / scores ``torch.equal``, with none of the three score nodes launched.  6 images on 4 slots,
    max_length 8: slots are reseated inside wave 1.  Then the lockstep kzv_logits_process / kzv_lm_fuse with group = 0 (never validated,
    never divided by in that case) against group = 1."""
    from kzv.lm import NGramLM
    lib = L.load()
    cfg = _cfg(8)

    dec = build_decoder_dir(decoder_dir + "/opts", cfg)

    def fresh():
        m = TrOCRModel(cfg.encoder_config_dict(), dec, init_seed=7, load_tokenizer=False)
        bias = m.state_dict_views()["decoder.lm_head.bias"]
        bias[cfg.eos_id] += EOS_BIAS
        bias[cfg.pad_id] -= 8.0                             # no running beam takes padding: the slots decode every beam wave themselves
        m.eval()
        return m
    used, plain = fresh(), fresh()
    px = torch.from_numpy(synthetic_batch(cfg, 6, LH, seed=3)[0]).cuda()
    lm = NGramLM.fit([[cfg.bos_id, 5, 6, 7, 5, 6, cfg.eos_id], [cfg.bos_id, 6, 5, 9, cfg.eos_id]], 2, cfg.vocab)
    everything = dict(no_repeat_ngram_size=2, repetition_penalty=1.2, suppress_tokens=[cfg.pad_id, 20, 40], lm=lm, lm_weight=1.5,
                      prefix_ids=[[5 + i, 6 + i] for i in range(6)])
    counters = (lib.kzv_test_logits_process_calls, lib.kzv_test_lm_fuse_calls, lib.kzv_test_force_prefix_calls)
    for kw1, kw2 in ((dict(top_k=2), dict(return_logprobs=True)),
                     (dict(num_beams=2, num_return_sequences=2, return_scores=True), dict(num_beams=2, return_scores=True))):
        before = [c() for c in counters]
        first = used.generate_stream(px, max_length=8, slots=4, **everything, **kw1)
        assert all(c() > b for c, b in zip(counters, before)), "wave 1 did not run the three score nodes"
        rows = first[0][0::2] if "num_beams" in kw1 else first[0]
        assert all(rows[i, 1:3].tolist() == [5 + i, 6 + i] for i in range(6))      # the options were on: every line starts with its prefix
        before = [c() for c in counters]
        ids, sc = used.generate_stream(px, max_length=8, slots=4, **kw2)
        assert [c() for c in counters] == before, "an option of wave 1 reached wave 2"
        want_ids, want_sc = plain.generate_stream(px, max_length=8, slots=4, **kw2)
        if "num_beams" in kw2:
            assert used.stream_beam_impl == "slot-refill" and used.last_stream_pad_fallbacks == 0 and plain.last_stream_pad_fallbacks == 0
        else:
            assert used.stream_decode_impl == "slot-refill"
        assert torch.equal(ids, want_ids) and torch.equal(sc, want_sc)
    # lockstep: rows of scores with their own histories, group = 0 against group = 1
    g = torch.Generator().manual_seed(5)
    V, ld, R, T = cfg.vocab, cfg.vocab + 3, 5, 6
    x = torch.randn(R, ld, generator=g).cuda()
    hist = torch.randint(4, 12, (R, T), generator=g).cuda()
    dlm = lm.to_device("cuda")
    st = L.stream_handle()
    out = {}
    for group in (1, 0):
        a, b = x.clone(), x.clone()
        pa = L.kzv_logits_process_args(logits=a.data_ptr(), ld=ld, rows=R, vocab=V, ids=hist.data_ptr(), ld_ids=T, t=T - 2, group=group, slot_image=None,
                                       slot_t=None, by_image=0, n_images=0, no_repeat_ngram_size=2, min_length=0, eos_id=cfg.eos_id, normalise=1,
                                       repetition_penalty=1.3, reserved=0, suppress_mask=None)
        fa = L.kzv_lm_fuse_args(logits=b.data_ptr(), ld=ld, rows=R, vocab=V, ids=hist.data_ptr(), ld_ids=T, t=T - 2, group=group, slot_image=None,
                                slot_t=None, by_image=0, n_images=0, weight=0.7, reserved=0, lm=C.pointer(dlm.struct))
        assert lib.kzv_logits_process(C.byref(pa), st) == 0, lib.kzv_last_error()
        assert lib.kzv_lm_fuse(C.byref(fa), st) == 0, lib.kzv_last_error()
        torch.cuda.synchronize()
        out[group] = (a, b)
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert not torch.equal(out[1][0], x) and not torch.equal(out[1][1], x)          # both nodes did edit the rows
