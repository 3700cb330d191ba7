"""Beam search on device-refilled slots on the GPU (TrOCRModel.generate_stream(num_beams=2 | 4); include/kzv.h: kzv_stream_begin_beams,
kzv_stream_beam_*; csrc/decode_fused.hip: the slot instances with 2 / 4 rows and the row table; csrc/token_search.hip: update and seating):

  1. the update and seating kernels alone against their torch statement (kzv/stream.py: beam_select_seat), state for state over 50 steps:
     rankings from kzv_beam_topk on seeded logits with planted ties, planted EOS, planted padding and several searches ending in one
     step; every integer array equal, every score torch.equal, the row table re-parented in place; 7, 70 and 300 slots (one wave of
     slots, several, and a second seating pass of 256 with its carry);
  2. generate_stream(num_beams=nb, slots=6) == generate(num_beams=nb), token for token: 8 and 164 patch keys (the one-pass and the
     chunked instances), bf16 and e4m3 weights, 2 and 4 beams; no running beam took padding;
  3. fewer steps than lockstep batches of 6 (generate's own last_generate_steps), and within the list-scheduling bound;
  4. six distinct limits: every group of images against generate(max_length=limit);
  5. more slots than compute units and idle slots: 70 slots (280 rows) for 75 images, 1 image on 6 slots, as many images as slots;
  6. two waves in one call equal one;
  7. the fallback: a 64-wide decoder, or the one-launch mode off, runs generate() and says so;
  8. return_scores against the mean teacher-forced log-probability of the returned ids (align), within 2e-2: LP_TOL of
     tests/test_stream_gpu.py for one log-probability -- a mean cannot be further off than its worst term;
  9. on the fitted fixture the strings of generate(num_beams=4).
The decoder is the one-launch tests' (hidden 256, 4 heads, FFN 768, 3 layers) on the tiny encoder: Lh = 38, 40 crops.

Cases 2 and 3 need searches that end at different steps.  The condition is asserted on generate's own results before the stream runs
(every image decoded alone; a search that issues fewer than Lh - 1 steps ended before the cap): at least a quarter of the 40 searches end
before step Lh - 1 and at least one reaches the cap.
CROSS_GAIN / EOS_BIAS / PAD_BIAS of the file's model and the end steps observed with them on MI355X: see the constants below.
Also observed there: 40 crops on 6 slots take 197 / 201 / 202 steps (8 keys: bf16 with 2 and 4 beams, e4m3 with 4) and 225 / 228 / 238
(164 keys) where lockstep batches of 6 issue 259 at 8 keys and the bound is 296; 75 images on 70 slots 41 steps; no running beam took
padding; sequence scores within 7.1e-4 (8 keys) and 3.4e-4 (164 keys) of the teacher-forced mean; the per-op case 23 steps for 30
searches on 7 slots with 4 - 7 planted padding continuations counted (31 - 73 at 70 slots, 319 at 300)."""
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
# The file's own model.  Under beam search the untrained recipe model ends every search at nearly the same step whatever the image: with
# the EOS bias + 0.5 of tests/test_stream_gpu.py all 40 searches end within 4 steps, up to + 0.2 all run to the cap, and between the
# two the switch takes 0.01 of bias and sits elsewhere for every (keys, weights, beams).  So the image is given more say -- the
# cross-attention output projections are scaled by CROSS_GAIN -- and the EOS bias is set per crop width inside the band where the
# searches then spread (a lower value than + 0.5, not a higher one).  Observed on MI355X, every image decoded alone, searches ending
# before step 37 / at the cap, (bf16, e4m3) x (2, 4) beams: 8 keys, + 0.3: 22 / 18, 22 / 18, 25 / 15, 24 / 16, the shortest within 4
# to 8 steps; 164 keys, + 0.4: 33 / 7, 32 / 8, 24 / 16, 27 / 13, the shortest within 24 (one step of 0.1 to either side: 5..7 / 33..35
# and 36..38 / 2..4 at 8 keys, 2..12 / 28..38 and 40 / 0 at 164).
# The bias of padding is lowered: a fitted model never emits padding inside a line, an untrained one ranks it like any other token, and
# a running beam that takes it sends the wave to the lockstep search (case 2 asserts that none did).
CROSS_GAIN = 24.0
EOS_BIAS = {8: 0.3, 164: 0.4}
PAD_BIAS = -8.0
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


def _bias(m, cfg, eos_bias, gain=1.0):
    views = m.state_dict_views()
    for k in [k for k in views if "crossattention.output.dense.weight" in k]:
        views[k] *= gain
    views["decoder.lm_head.bias"][cfg.eos_id] += eos_bias
    views["decoder.lm_head.bias"][cfg.pad_id] += PAD_BIAS


def _model(keys, decoder_dir):
    """One model per crop width for the whole module (recipe seed 7, gain and biases as above), 40 crops, and a cache of its lockstep decodes."""
    if keys not in _models:
        cfg = _cfg(keys)
        m = TrOCRModel(cfg.encoder_config_dict(), build_decoder_dir(decoder_dir + f"/{keys}", cfg), init_seed=7, load_tokenizer=False)
        _bias(m, cfg, EOS_BIAS[keys], CROSS_GAIN)
        m.eval()
        px = torch.from_numpy(synthetic_batch(cfg, 40, LH, seed=3)[0]).cuda()
        _models[keys] = (cfg, m, px, {})
    return _models[keys]


def _pad(ids, pad_id, width=LH):
    out = torch.full((ids.shape[0], width), pad_id, dtype=torch.int64, device=ids.device)
    out[:, :ids.shape[1]] = ids
    return out


def _static(keys, fmt, nb, decoder_dir):
    """generate(num_beams=nb) of the 40 crops (computed once), after the condition on its searches, each image alone."""
    cfg, m, px, cache = _model(keys, decoder_dir)
    m.set_decode_weights(fmt)
    if (fmt, nb) not in cache:
        ends = []
        for i in range(px.shape[0]):
            m.generate(px[i:i + 1], max_length=LH, num_beams=nb)
            ends.append(m.last_generate_steps)
        early, cap = sum(e < LH - 1 for e in ends), sum(e == LH - 1 for e in ends)
        print(f"{keys} keys, {fmt}, {nb} beams: {early} searches end before step {LH - 1}, {cap} at the cap; steps issued alone: {sorted(set(ends))}")
        assert early * 4 >= len(ends) and cap >= 1, ends
        cache[(fmt, nb)] = _pad(m.generate(px, max_length=LH, num_beams=nb), cfg.pad_id)
        assert m.decode_step_impl == "one-launch" and m.decode_weights_impl == fmt
    return cfg, m, px, cache[(fmt, nb)]


# ---- 1. the kernels against the statement --------------------------------------------------------------------------------------------
# 7 slots: one wave of slots, one seating pass.  70 slots: ended flags in two waves.  300 slots: a second seating pass of 256 slots with
# its carry (one beam setting: the statement is a Python loop over the slots).  Every live search ends at steps 4, 13, ..., 49 (six
# times), so N <= 5 slots images are all seated and ended by the last step.
@pytest.mark.parametrize("nb,early,lpen,slots,N", [
    pytest.param(2, True, 1.0, 7, 30, id="2-True-1.0"), pytest.param(4, True, 1.0, 7, 30, id="4-True-1.0"), pytest.param(4, False, 0.6, 7, 30, id="4-False-0.6"),
    (2, True, 1.0, 70, 300), (4, True, 1.0, 70, 300), (4, False, 0.6, 70, 300), (4, True, 1.0, 300, 1500)])
def test_update_and_seat_kernels_equal_the_torch_statement(nb, early, lpen, slots, N):
    lib = L.load()
    V, ML, pad, bos, eos = 157, 12, 1, 2, 3
    K, R = 2 * nb, slots * nb
    g = torch.Generator().manual_seed(13 + nb)
    limits = torch.randint(2, ML + 1, (N,), generator=g, dtype=torch.int32)
    lim_d = limits.cuda()
    div = ST.divisor_table(ML, lpen)
    div_d = div.cuda()
    ref = ST.new_beam_state(N, slots, nb, ML, pad, bos, "cpu", rowtab_ld=ML)
    ref["rowtab"] = torch.randint(0, R, (R, ML), generator=g, dtype=torch.int32)        # what an earlier wave left: never read before it is rewritten
    dev = {k: torch.randint(0, 3, v.shape, generator=g).to(v.dtype).cuda() for k, v in ref.items()}   # seat_first must not rely on clean memory
    dev["out_ids"].copy_(ref["out_ids"]); dev["out_score"].zero_(); dev["rowtab"].copy_(ref["rowtab"])
    scratch = torch.zeros(2 * slots, dtype=torch.int32, device="cuda")
    top_lp = torch.empty(slots, K, dtype=torch.float32, device="cuda")
    top_ix = torch.empty(slots, K, dtype=torch.int64, device="cuda")
    st = L.kzv_stream_beam_state(slots=slots, n_images=N, num_beams=nb, max_len=ML, vocab=V, bos_id=bos, eos_id=eos, pad_id=pad, early_stopping=int(early),
                                 slot_image=dev["slot_image"].data_ptr(), slot_t=dev["slot_t"].data_ptr(), tokens=dev["tokens"].data_ptr(),
                                 posids=dev["posids"].data_ptr(), run_seq=dev["run_seq"].data_ptr(), fin_seq=dev["fin_seq"].data_ptr(),
                                 run_scores=dev["run_sc"].data_ptr(), fin_scores=dev["fin_sc"].data_ptr(), fin_done=dev["fin_done"].data_ptr(),
                                 fin_len=dev["fin_len"].data_ptr(), unsatisfied=dev["unsat"].data_ptr(), counters=dev["counters"].data_ptr(),
                                 scratch=scratch.data_ptr(), out_ids=dev["out_ids"].data_ptr(), ld_ids=ML, out_score=dev["out_score"].data_ptr(),
                                 limit=lim_d.data_ptr(), divisors=div_d.data_ptr(), rows=dev["rowtab"].data_ptr(), ld_rows=ML)
    L.check(lib.kzv_stream_beam_seat_first(C.byref(st), L.stream_handle()), "beam_seat_first")
    ints = ("slot_image", "slot_t", "tokens", "posids", "run_seq", "fin_seq", "fin_done", "fin_len", "unsat", "counters", "out_ids", "rowtab")
    for k in ints + ("run_sc", "fin_sc", "out_score"):
        assert torch.equal(dev[k].cpu(), ref[k]), ("start", k)
    rows = torch.arange(R)
    seen_multi = seen_tie = seen_eos = 0
    for step in range(50):
        x = torch.randn(R, V, generator=g)
        x[:, pad] = -20.0
        for b in range(R):
            r = int(torch.randint(0, 8, (1,), generator=g))
            if r == 0:                                      # exact ties of the maximum: the smaller flat index ranks first
                cols = torch.randperm(V - 4, generator=g)[:3] + 4
                x[b, cols] = x[b].max() + 1.0
                seen_tie += 1
            elif r == 1:                                    # EOS as the maximum, tied with a later column
                x[b, eos] = x[b, 100] = x[b].max() + 0.5
                seen_eos += 1
            elif r == 2 and step % 7 == 3:                  # padding as the maximum: a running beam takes it
                x[b, pad] = x[b].max() + 1.0
        if step % 9 == 4:                                   # every live search ends in this step
            x[:, eos] = 50.0
        # what the step kernel does to the row table before the update: row b wrote its own key at its slot's step
        live = (ref["slot_image"] >= 0).repeat_interleave(nb)
        at = ref["slot_t"].repeat_interleave(nb).long()
        ref["rowtab"][rows[live], at[live]] = rows[live].to(torch.int32)
        dev["rowtab"][rows[live].cuda(), at[live].cuda()] = rows[live].to(torch.int32).cuda()
        xd = x.cuda()
        L.check(lib.kzv_beam_topk(xd.data_ptr(), V, dev["run_sc"].data_ptr(), slots, nb, V, K, top_lp.data_ptr(), top_ix.data_ptr(), L.stream_handle()), "beam_topk")
        before = ref["slot_image"].clone()
        L.check(lib.kzv_stream_beam_update(C.byref(st), top_lp.data_ptr(), top_ix.data_ptr(), L.stream_handle()), "stream_beam_update")
        ref = ST.beam_select_seat(top_lp.cpu(), top_ix.cpu(), ref, n_images=N, num_beams=nb, max_len=ML, vocab=V, pad_id=pad, bos_id=bos, eos_id=eos,
                                  early_stopping=early, length_penalty=lpen, limit=limits, divisors=div)
        seen_multi += int(((ref["slot_image"] != before).sum() > 1))
        for k in ints:
            assert torch.equal(dev[k].cpu(), ref[k]), (step, k, dev[k].cpu(), ref[k])
        for k in ("run_sc", "fin_sc", "out_score"):
            assert torch.equal(dev[k].cpu(), ref[k]), (step, k, dev[k].cpu(), ref[k])
    c = ref["counters"].tolist()
    print(f"{nb} beams: {c[2]} steps for {N} searches on {slots} slots, {c[3]} running beams took padding; {seen_multi} steps reseated several slots")
    assert c[:2] == [N, N] and (ref["slot_image"] == -1).all() and c[3] >= 1
    assert c[2] <= ST.step_bound(N, slots, ML)
    assert seen_multi >= 3 and seen_tie >= 5 and seen_eos >= 5


# ---- 2. stream == lockstep ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [2, 4])
@pytest.mark.parametrize("fmt", ["bf16", "e4m3"])
@pytest.mark.parametrize("keys", [8, 164])
def test_beam_stream_equals_lockstep_beam_search(decoder_dir, keys, fmt, nb):
    cfg, m, px, want = _static(keys, fmt, nb, decoder_dir)
    got = m.generate_stream(px, max_length=LH, slots=6, num_beams=nb)
    assert m.stream_beam_impl == "slot-refill" and m.stream_beam_impl_for(nb) == "slot-refill"
    assert m.last_stream_pad_fallbacks == 0
    assert got.shape[1] == max(2, int((want != cfg.pad_id).sum(1).max()))
    assert torch.equal(_pad(got, cfg.pad_id), want)
    print(f"{keys} keys, {fmt}, {nb} beams: {m.last_stream_steps} steps on 6 slots (bound {ST.step_bound(px.shape[0], 6, LH)})")
    assert m.last_stream_steps <= ST.step_bound(px.shape[0], 6, LH)


# ---- 3. step counts ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [2, 4])
def test_fewer_steps_than_lockstep_batches(decoder_dir, nb):
    cfg, m, px, want = _static(8, "bf16", nb, decoder_dir)
    n = px.shape[0]
    lockstep = 0
    for a in range(0, n, 6):
        g = m.generate(px[a:a + 6], max_length=LH, num_beams=nb)
        assert torch.equal(_pad(g, cfg.pad_id), want[a:a + 6])
        lockstep += m.last_generate_steps
    m.generate_stream(px, max_length=LH, slots=6, num_beams=nb)
    print(f"{nb} beams: {m.last_stream_steps} steps on 6 slots, lockstep batches of 6 issue {lockstep}")
    assert m.last_stream_steps < lockstep
    assert m.last_stream_steps <= ST.step_bound(n, 6, LH)


# ---- 4. limits ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [2, 4])
def test_limits_are_each_image_at_its_own_max_length(decoder_dir, nb):
    cfg, m, px, _ = _model(8, decoder_dir)
    m.set_decode_weights("bf16")
    n = px.shape[0]
    values = [2, 5, 11, 20, 29, LH]
    limits = torch.tensor([values[i % 6] for i in range(n)], dtype=torch.int32)
    got = _pad(m.generate_stream(px, max_length=LH, slots=6, limits=limits, num_beams=nb), cfg.pad_id)
    assert m.last_stream_pad_fallbacks == 0
    for v in values:
        idx = (limits == v).nonzero().reshape(-1).cuda()
        want = _pad(m.generate(px[idx], max_length=v, num_beams=nb), cfg.pad_id)
        assert torch.equal(got[idx], want), v
        assert int((got[idx] != cfg.pad_id).sum(1).max()) <= v


# ---- 5. more slots than compute units, idle slots -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,slots", [(75, 70), (1, 6), (6, 6)])
def test_many_slots_and_idle_slots(decoder_dir, n, slots):
    cfg, m, _, _ = _model(8, decoder_dir)
    m.set_decode_weights("bf16")
    px = torch.from_numpy(synthetic_batch(cfg, n, LH, seed=29)[0]).cuda()
    want = _pad(m.generate(px, max_length=LH, num_beams=4), cfg.pad_id)
    got = m.generate_stream(px, max_length=LH, slots=slots, num_beams=4)
    assert m.stream_beam_impl == "slot-refill" and m.last_stream_pad_fallbacks == 0
    assert torch.equal(_pad(got, cfg.pad_id), want)
    assert m.last_stream_steps <= ST.step_bound(n, slots, LH)
    print(f"{n} images on {slots} slots of 4 beams: {m.last_stream_steps} steps")


# ---- 6. waves ----------------------------------------------------------------------------------------------------------------------------
def test_two_waves_equal_one(decoder_dir):
    cfg, m, px, _ = _model(8, decoder_dir)
    m.set_decode_weights("bf16")
    one, sc1 = m.generate_stream(px, max_length=LH, slots=6, num_beams=4, return_scores=True)
    steps_one = m.last_stream_steps
    per_image = cfg.dec_layers * 2 * cfg.num_patches * cfg.dec_hidden * 2
    seen = []
    orig = m._stream_wave
    m._stream_wave = lambda px_, *a: (seen.append(px_.shape[0]), orig(px_, *a))[1]
    try:
        two, sc2 = m.generate_stream([px[:7].cpu(), px[7:29].cpu(), px[29:].cpu()], max_length=LH, slots=6, num_beams=4, return_scores=True,
                                     pool_bytes=24 * per_image)
    finally:
        del m._stream_wave
    assert seen == [24, 16]
    assert torch.equal(one, two) and torch.equal(sc1, sc2)
    assert m.last_stream_steps >= steps_one


# ---- 7. the fallback -----------------------------------------------------------------------------------------------------------------------
def test_fallback_is_lockstep_beam_search(decoder_dir, tmp_path):
    lib = L.load()
    cfg = tiny_config()                                     # 64-wide decoder: no one-launch step
    m = TrOCRModel(cfg.encoder_config_dict(), build_decoder_dir(str(tmp_path / "dec"), cfg), init_seed=7, load_tokenizer=False)
    _bias(m, cfg, 0.5)
    m.eval()
    px = torch.from_numpy(synthetic_batch(cfg, 13, LH, seed=3)[0]).cuda()
    want = _pad(m.generate(px, max_length=LH, num_beams=4), cfg.pad_id)
    got = m.generate_stream(px, max_length=LH, slots=13, num_beams=4)
    assert m.stream_beam_impl == "static" and m.last_stream_steps == 0
    assert torch.equal(_pad(got, cfg.pad_id), want)
    # three beams: no slot instance, whatever the decoder
    cfg2, m2, px2, _ = _model(8, decoder_dir)
    m2.set_decode_weights("bf16")
    want3 = _pad(m2.generate(px2, max_length=LH, num_beams=3), cfg2.pad_id)
    got3 = m2.generate_stream(px2, max_length=LH, slots=40, num_beams=3)
    assert m2.stream_beam_impl == "static" and m2.last_stream_steps == 0
    assert torch.equal(_pad(got3, cfg2.pad_id), want3)
    # the 256-wide model with the one-launch mode off
    L.check(lib.kzv_set_decode_one_launch(0), "mode")
    want0 = _pad(m2.generate(px2, max_length=LH, num_beams=4), cfg2.pad_id)
    got0 = m2.generate_stream(px2, max_length=LH, slots=40, num_beams=4)
    assert m2.stream_beam_impl == "static" and m2.last_stream_steps == 0
    assert torch.equal(_pad(got0, cfg2.pad_id), want0)
    L.check(lib.kzv_set_decode_one_launch(-1), "mode")
    assert m2.stream_beam_impl == "slot-refill"
    with pytest.raises(ValueError):
        m2.generate_stream(px2[:2], max_length=LH, slots=2, num_beams=4, return_logprobs=True)


def test_begin_beams_refusals_on_a_bound_handle(decoder_dir):
    lib = L.load()
    cfg, m, px, _ = _model(8, decoder_dir)
    m._check_inputs(px[:1])
    m._bind(24, LH)
    out = torch.full((8, LH), cfg.pad_id, dtype=torch.int64, device="cuda")
    begin = lambda nb, pool, n, ml: lib.kzv_stream_begin_beams(m._h, nb, 1, 1.0, None, pool, n, ml, cfg.bos_id, cfg.eos_id, out.data_ptr(), LH + 1, None, 0,
                                                               None, L.stream_handle())
    assert lib.kzv_stream_beam_impl(m._h, 4) == 1 and lib.kzv_stream_beam_impl(m._h, 2) == 1 and lib.kzv_stream_beam_impl(m._h, 3) == 0
    assert begin(4, 4, 4, LH) == -1 and b"smaller than the 6 slots" in lib.kzv_last_error()
    assert begin(4, 8, 8, LH + 1) == -1
    assert lib.kzv_stream_step(m._h, 0, L.stream_handle()) == -3          # a refused begin leaves no wave to step
    m._bind(6, LH)
    assert lib.kzv_stream_beam_impl(m._h, 4) == 0                          # 6 rows are no multiple of 4 beams
    assert begin(4, 8, 8, LH) == -1 and b"multiple" in lib.kzv_last_error()


# ---- 8. scores ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keys", [8, 164])
def test_scores_against_the_teacher_forced_pass(decoder_dir, keys):
    cfg, m, px, _ = _model(keys, decoder_dir)
    m.set_decode_weights("bf16")
    ids, score = m.generate_stream(px, max_length=LH, slots=6, num_beams=4, return_scores=True)
    assert score.shape == (px.shape[0],) and m.last_stream_pad_fallbacks == 0
    sc = m.align(px, ids)
    live = sc["live"].float()
    assert int(live.sum()) > 40
    mean = (sc["logprob"] * live).sum(1) / live.sum(1)
    err = float((score - mean).abs().max())
    print(f"{keys} keys: largest |sequence score - mean teacher-forced log-probability| over {px.shape[0]} winners: {err:.3e}")
    assert err <= LP_TOL


# ---- 9. the fitted fixture -----------------------------------------------------------------------------------------------------------------
def test_strings_on_the_fitted_fixture(tmp_path):
    g, cfg, sd, data = load_trained()
    m = TrOCRModel(cfg.encoder_config_dict(), build_decoder_dir(str(tmp_path / "dec"), cfg), load_tokenizer=True)
    m.load_state_dict(sd, strict=True)
    m.eval()
    px = torch.from_numpy(np.concatenate([data["fit"][0], data["unseen"][0]]))
    assert px.shape[0] == 12
    Lh = int(g["label_len"])
    got = m.generate_stream(px, max_length=Lh, slots=5, num_beams=4)
    want = m.generate(px, max_length=Lh, num_beams=4)
    strings = lambda ids: m.tokenizer.batch_decode(ids, skip_special_tokens=True)
    assert strings(got) == strings(want) and len(set(strings(want))) > 1
    assert torch.equal(_pad(got, cfg.pad_id, Lh), _pad(want, cfg.pad_id, Lh))
