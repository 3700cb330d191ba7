"""Top-k character alternatives at model level (TrOCRModel.align / generate_stream / recognize / recognize_many with ``top_k``;
include/kzv.h: kzv_score_tokens_topk, kzv_stream_set_topk), on the models and crops of tests/test_stream_gpu.py (8 and 164 patch
keys, the 3-layer reference-geometry decoder, LH = 38, 6 slots), the wide geometry of tests/test_align_gpu.py and the fitted fixture.

Teacher-forced: entry 0 of align(top_k=5) is top1 / top1_logprob (1e-4); against log_softmax of forward(px, labels)["logits"] ids
exactly and log-probabilities to 1e-4 -- also after the one-launch head + CE at the wide geometry (the re-run vocabulary GEMM gives
the returned logits bit for bit there too); kzv_backward after the read-back gives the gradients of a run without it;
kzv_score_tokens' KZV_E_STATE cases.

Stream (bf16 and e4m3, with limits): top_k changes neither the ids nor the step count; entry 0 is the emitted token with the returned
log-probability (1e-4); -1 / 0 everywhere else.  Against the teacher-forced pass an untrained model's candidates sit 1e-4 apart, so
ranks cannot be compared; instead, at EVERY live position, with tf = log_softmax of the teacher-forced logits of the generated ids:
every listed candidate c has |alt_logprob - tf[c]| <= LP_TOL, and no unlisted column has tf > alt_logprob[k - 1] + 2 * LP_TOL
(LP_TOL = 2e-2, the bound tests/test_stream_gpu.py asserts between the two paths).  310 images on 300 slots and three waves equal
one, with top_k = 3; the static fallback equals align(top_k)'s ids; recognize_many / recognize on the fitted fixture.
Observed on MI355X: log-probabilities within 1.2e-6 of float64 log-softmax; entry 0 within 1.5e-6 of the stream's own log-probability;
stream alternatives within 3.2e-3 of the teacher-forced pass, the best unlisted column at most 1.1e-3 above the last listed one."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from kzv import _lib as L
from kzv import params as P
from kzv.config import tiny_config
from kzv.data import build_decoder_dir, synthetic_batch
from kzv.model import TrOCRModel

import test_stream_gpu as SG
from _trained import load as load_trained

pytestmark = pytest.mark.gpu
LH, LP_TOL = SG.LH, SG.LP_TOL


@pytest.fixture(autouse=True)
def _default_modes_afterwards():
    yield
    lib = L.load()
    lib.kzv_set_decode_one_launch(-1)
    lib.kzv_set_head_ce(-1)


@pytest.fixture(scope="module")
def decoder_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("dec_alt"))


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    g, cfg, sd, data = load_trained()
    m = TrOCRModel(cfg.encoder_config_dict(), build_decoder_dir(str(tmp_path_factory.mktemp("dec_fit")), cfg), load_tokenizer=True)
    m.load_state_dict(sd, strict=True)
    m.eval()
    return g, cfg, data, m


@pytest.fixture(scope="module")
def wide(tmp_path_factory):
    """tests/test_align_gpu.py's wide geometry (hidden 256, 4 heads, FFN 768, vocabulary 4,300: the one-launch head + CE), random init."""
    cfg = dataclasses.replace(tiny_config(), image_h=64, image_w=640, enc_hidden=128, enc_layers=1, enc_heads=2, enc_ffn=256,
                              dec_hidden=256, dec_heads=4, dec_ffn=768, dec_layers=2, vocab=4300, max_pos=128)
    sd = P.state_dict_from_flat(cfg, P.recipe_flat(cfg, 11))
    m = TrOCRModel(cfg.encoder_config_dict(), build_decoder_dir(str(tmp_path_factory.mktemp("dec_wide")), cfg), load_tokenizer=False)
    m.load_state_dict(sd, strict=True)
    m.eval()
    batches = {"trimmed": synthetic_batch(cfg, 3, 40, seed=21, min_chars=3, max_chars=17),
               "untrimmed": synthetic_batch(cfg, 3, 20, seed=22, min_chars=19, max_chars=19)}
    return cfg, m, batches


def _margin_check(tag, alt_ids, alt_lp, tf, live, tol):
    """alt_ids / alt_lp [B, T, k] against tf [B, T, V] (log-softmax) at every live position: every listed candidate within tol of its
    teacher-forced value, no unlisted column above the last listed one by more than 2 * tol.  Returns the two largest figures."""
    assert bool((alt_ids[live] >= 0).all()), tag
    listed = torch.gather(tf, 2, alt_ids.clamp(min=0))
    err = float((alt_lp.double() - listed)[live].abs().max())
    rest = tf.clone()
    rest.scatter_(2, alt_ids.clamp(min=0), float("-inf"))
    over = float((rest.max(-1).values - alt_lp[..., -1].double())[live].max())
    print(f"{tag}: {int(live.sum())} live positions; largest |alternative - teacher-forced| {err:.3e}, best unlisted column above the last listed by {over:.3e}")
    assert err <= tol and over <= 2 * tol, tag
    return err, over


def _check_against_logits(tag, out, logits, k):
    """align(top_k=k)'s result against the logits [B, L - 1, V] the same forward returned."""
    live = out["live"]
    T = logits.shape[1]
    ids, lp = out["alt_ids"], out["alt_logprob"]
    assert ids.shape == (logits.shape[0], T, k) and ids.dtype == torch.int64 and lp.shape == ids.shape and lp.dtype == torch.float32
    assert bool(torch.equal(ids[..., 0][live], out["top1"][live])), tag
    e0 = float((lp[..., 0] - out["top1_logprob"])[live].abs().max())
    ls = torch.log_softmax(logits.double(), -1)
    order = torch.sort(logits, dim=-1, descending=True, stable=True).indices[..., :k]
    same = bool(torch.equal(ids[live], order[live]))
    err = float((lp.double() - torch.gather(ls, 2, ids.clamp(min=0)))[live].abs().max())
    print(f"{tag}: entry 0 against top1_logprob {e0:.3g}; ids equal the stable sort of the returned logits: {same}; |logprob - log_softmax| {err:.3g}")
    assert e0 <= 1e-4 and err <= 1e-4, tag
    assert same, tag                                         # the re-run vocabulary GEMM gives the returned logits bit for bit
    d = lp[live]
    assert bool((d[:, :-1] >= d[:, 1:]).all()), tag


# ---- teacher-forced ---------------------------------------------------------------------------------------------------------------------
def test_align_top_k_of_the_fitted_model(trained):
    g, cfg, data, m = trained
    for tag, (px, lab) in data.items():
        pxt, labt = torch.from_numpy(px), torch.from_numpy(lab)
        logits = m(pxt, labt)["logits"]
        out = m.align(pxt, labt, top_k=5)
        plain = m.align(pxt, labt)
        torch.cuda.synchronize()
        assert set(out) == set(plain) | {"alt_ids", "alt_logprob"} and "alt_ids" not in plain
        for key in plain:
            assert bool(torch.equal(out[key], plain[key])), key
        _check_against_logits(tag, out, logits, 5)
        Ta = m.last_active_length                            # trimmed padding: -1 / 0
        assert bool((out["alt_ids"][:, Ta:] == -1).all()) and bool((out["alt_logprob"][:, Ta:] == 0).all())
    with pytest.raises(ValueError):
        m.align(pxt, labt, top_k=9)


def test_align_top_k_after_the_one_launch_head(wide):
    cfg, m, batches = wide
    lib = L.load()
    for tag, (px, lab) in batches.items():
        pxt, labt = torch.from_numpy(px), torch.from_numpy(lab)
        logits = m(pxt, labt)["logits"]
        L.check(lib.kzv_set_head_ce(1), "set_head_ce")
        out = m.align(pxt, labt, top_k=5)
        torch.cuda.synchronize()
        _check_against_logits(f"wide {tag}", out, logits, 5)
        Ta = m.last_active_length
        assert (Ta < lab.shape[1] - 1) == (tag == "trimmed")
        assert bool((out["alt_ids"][:, Ta:] == -1).all()) and bool((out["alt_logprob"][:, Ta:] == 0).all())


def test_top_k_state_rules_and_backward(trained):
    g, cfg, data, m = trained
    lib = L.load()
    px, lab = data["fit"]
    pxt, labt = torch.from_numpy(px), torch.from_numpy(lab)
    B, Lh = lab.shape
    ibuf = torch.empty(B * Lh * 8, dtype=torch.int32, device="cuda")
    fbuf = torch.empty(B * Lh * 8, dtype=torch.float32, device="cuda")

    def refuses(why):
        assert lib.kzv_score_tokens_topk(m._h, 5, ibuf.data_ptr(), fbuf.data_ptr(), L.stream_handle()) == -3, why
        assert b"score_tokens_topk" in lib.kzv_last_error()
        with pytest.raises(L.KzvError):
            m.align_last(top_k=5)

    m.align(pxt, labt)
    step_logits = torch.empty(B, cfg.vocab, dtype=torch.float32, device="cuda")
    L.check(lib.kzv_decode_logits(m._h, m._keep[1].data_ptr(), 0, step_logits.data_ptr(), L.stream_handle()), "decode_logits")
    refuses("after kzv_decode_logits")
    m.align(pxt, labt)
    m.generate(pxt, max_length=Lh, num_beams=1)
    refuses("after generate")
    m.align(pxt, labt)
    L.check(lib.kzv_set_active_length(m._h, 1), "set_active_length")
    refuses("after a change of the active length")
    m.align(pxt, labt)
    for k in (0, 9):
        assert lib.kzv_score_tokens_topk(m._h, k, ibuf.data_ptr(), fbuf.data_ptr(), L.stream_handle()) == -1, k
    assert lib.kzv_score_tokens_topk(m._h, 5, None, fbuf.data_ptr(), L.stream_handle()) == -1
    assert lib.kzv_score_tokens_topk(m._h, 5, ibuf.data_ptr(), None, L.stream_handle()) == -1
    # a training-mode forward: the read-back in between changes neither the loss nor the gradients (tests/test_align_gpu.py's bounds)
    m.train()
    try:
        m.zero_grad()
        loss_a, _ = m.forward_loss(pxt, labt, seed=5)
        m.backward()
        torch.cuda.synchronize()
        la, ga = float(loss_a), m.flat_grads.clone()
        loss_b, _ = m.forward_loss(pxt, labt, seed=5)
        lb = float(loss_b)
        out = m.align_last(top_k=8)
        assert bool(torch.isfinite(out["alt_logprob"]).all()) and bool((out["alt_ids"][out["live"]] >= 0).all())
        m.backward()
        torch.cuda.synchronize()
        gb = m.flat_grads.clone()
        assert float(m._loss) == lb
    finally:
        m.eval()
    assert abs(la - lb) <= 2e-6 * max(1.0, abs(la))
    sc = float(ga.abs().max())
    assert sc > 0 and float((ga - gb).abs().max()) <= 1e-5 * sc


# ---- the stream ---------------------------------------------------------------------------------------------------------------------------
def _check_stream_result(tag, cfg, ids, lp, alt_ids, alt_lp, k):
    assert alt_ids.shape == ids.shape + (k,) and alt_ids.dtype == torch.int64 and alt_lp.shape == alt_ids.shape and lp.shape == ids.shape
    emitted = ids != cfg.pad_id
    emitted[:, 0] = False
    assert bool(torch.equal(alt_ids[..., 0][emitted], ids[emitted])), tag
    e0 = float((alt_lp[..., 0] - lp)[emitted].abs().max())
    assert bool((alt_ids[~emitted] == -1).all()) and bool((alt_lp[~emitted] == 0).all()), tag
    assert bool((alt_ids[emitted] >= 0).all()) and bool((alt_ids < cfg.vocab).all()), tag
    d = alt_lp[emitted]
    assert bool((d[:, :-1] >= d[:, 1:]).all()), tag
    assert e0 <= 1e-4, (tag, e0)
    return e0


@pytest.mark.parametrize("fmt", ["bf16", "e4m3"])
@pytest.mark.parametrize("keys", [8, 164])
def test_stream_top_k_leaves_the_decode_alone(decoder_dir, keys, fmt):
    cfg, m, px, _ = SG._static(keys, fmt, decoder_dir)
    limits = SG._limits(px.shape[0], 17)
    want, want_lp = m.generate_stream(px, max_length=LH, slots=6, limits=limits, return_logprobs=True)
    steps = m.last_stream_steps
    ids, lp, alt_ids, alt_lp = m.generate_stream(px, max_length=LH, slots=6, limits=limits, top_k=5)
    assert m.stream_decode_impl == "slot-refill" and m.decode_weights_impl == fmt
    assert torch.equal(ids, want) and torch.equal(lp, want_lp) and m.last_stream_steps == steps
    assert torch.equal(ids, m.generate_stream(px, max_length=LH, slots=6, limits=limits))          # ... and the wave after it carries none
    e0 = _check_stream_result((keys, fmt), cfg, ids, lp, alt_ids, alt_lp, 5)
    print(f"{keys} keys, {fmt}: {steps} steps; entry 0 against the returned log-probabilities {e0:.2e}")
    with pytest.raises(ValueError):
        m.generate_stream(px, max_length=LH, slots=6, top_k=5, num_beams=4)
    with pytest.raises(ValueError):
        m.generate_stream(px, max_length=LH, slots=6, top_k=9)


@pytest.mark.parametrize("keys", [8, 164])
def test_stream_alternatives_against_the_teacher_forced_pass(decoder_dir, keys):
    cfg, m, px, _ = SG._static(keys, "bf16", decoder_dir)
    limits = SG._limits(px.shape[0], 23)
    ids, lp, alt_ids, alt_lp = m.generate_stream(px, max_length=LH, slots=6, limits=limits, top_k=5)
    live = (ids[:, :-1] != cfg.pad_id) & (ids[:, 1:] != cfg.pad_id)
    assert int(live.sum()) > 40
    tf = torch.log_softmax(m(px, ids)["logits"].double(), -1)
    _margin_check(f"{keys} keys", alt_ids[:, 1:], alt_lp[:, 1:], tf, live, LP_TOL)


def test_stream_top_k_on_more_slots_than_compute_units(decoder_dir):
    cfg, m, _, _ = SG._model(8, decoder_dir)
    m.set_decode_weights("bf16")
    n, slots = 310, 300
    px = torch.from_numpy(synthetic_batch(cfg, n, LH, seed=29)[0]).cuda()
    limits = SG._limits(n, 31)
    want, want_lp = m.generate_stream(px, max_length=LH, slots=slots, limits=limits, return_logprobs=True)
    ids, lp, alt_ids, alt_lp = m.generate_stream(px, max_length=LH, slots=slots, limits=limits, top_k=3)
    assert m.stream_decode_impl == "slot-refill"
    assert torch.equal(ids, want) and torch.equal(lp, want_lp)
    _check_stream_result("310 on 300", cfg, ids, lp, alt_ids, alt_lp, 3)


def test_three_waves_with_top_k_equal_one(decoder_dir):
    cfg, m, px, _ = SG._static(8, "bf16", decoder_dir)
    limits = SG._limits(px.shape[0], 37)
    one = m.generate_stream(px, max_length=LH, slots=6, limits=limits, top_k=3)
    per_image = cfg.dec_layers * 2 * cfg.num_patches * cfg.dec_hidden * 2
    seen = []
    orig = m._stream_wave
    m._stream_wave = lambda px_, *a: (seen.append(px_.shape[0]), orig(px_, *a))[1]
    try:
        three = m.generate_stream([px[:7].cpu(), px[7:29].cpu(), px[29:].cpu()], max_length=LH, slots=6, limits=limits, top_k=3,
                                  pool_bytes=18 * per_image)
    finally:
        del m._stream_wave
    assert seen == [18, 18, 4]
    for a, b in zip(one, three):
        assert torch.equal(a, b)
    _check_stream_result("three waves", cfg, *three, 3)


def test_static_fallback_takes_its_alternatives_from_align(decoder_dir):
    lib = L.load()
    cfg, m, px, _ = SG._static(8, "bf16", decoder_dir)
    px = px[:13]
    L.check(lib.kzv_set_decode_one_launch(0), "mode")
    ids, lp, alt_ids, alt_lp = m.generate_stream(px, max_length=LH, slots=6, top_k=3)
    assert m.stream_decode_impl == "static"
    assert torch.equal(ids, m.generate_stream(px, max_length=LH, slots=6))
    full = SG._pad(ids, cfg.pad_id)
    for a in range(0, 13, 6):                                # the same batches
        sc = m.align(px[a:a + 6], full[a:a + 6], top_k=3)
        W = ids.shape[1] - 1
        live = sc["live"][:, :W]
        assert bool(torch.equal(alt_ids[a:a + 6, 1:][live], sc["alt_ids"][:, :W][live]))
        assert bool(torch.equal(alt_lp[a:a + 6, 1:][live], sc["alt_logprob"][:, :W][live]))
        assert bool((alt_ids[a:a + 6, 1:][~live] == -1).all()) and bool((alt_lp[a:a + 6, 1:][~live] == 0).all())
    assert bool((alt_ids[:, 0] == -1).all())
    L.check(lib.kzv_set_decode_one_launch(-1), "mode")


def test_set_topk_refusals(decoder_dir):
    lib = L.load()
    cfg, m, px, _ = SG._model(8, decoder_dir)
    m.set_decode_weights("bf16")
    m._check_inputs(px[:1])
    m._bind(8, LH)
    st = L.stream_handle()
    out = torch.full((8, LH), cfg.pad_id, dtype=torch.int64, device="cuda")
    out[:, 0] = cfg.bos_id
    ai = torch.full((8, LH, 8), -1, dtype=torch.int32, device="cuda")
    al = torch.zeros(8, LH, 8, device="cuda")
    assert lib.kzv_stream_begin(m._h, 4, 4, LH, cfg.bos_id, cfg.eos_id, out.data_ptr(), LH, None, 0, None, st) == -1     # no wave begun
    assert lib.kzv_stream_set_topk(m._h, 5, ai.data_ptr(), al.data_ptr(), LH * 5, st) == -3
    assert b"stream_set_topk" in lib.kzv_last_error()
    L.check(lib.kzv_stream_begin(m._h, 8, 8, LH, cfg.bos_id, cfg.eos_id, out.data_ptr(), LH, None, 0, None, st), "stream_begin")
    assert lib.kzv_stream_set_topk(m._h, 9, ai.data_ptr(), al.data_ptr(), LH * 9, st) == -1
    assert lib.kzv_stream_set_topk(m._h, -1, ai.data_ptr(), al.data_ptr(), LH * 8, st) == -1
    assert lib.kzv_stream_set_topk(m._h, 5, None, al.data_ptr(), LH * 5, st) == -1
    assert lib.kzv_stream_set_topk(m._h, 5, ai.data_ptr(), None, LH * 5, st) == -1
    assert lib.kzv_stream_set_topk(m._h, 5, ai.data_ptr(), al.data_ptr(), LH * 5 - 1, st) == -1
    assert lib.kzv_stream_set_topk(m._h, 5, ai.data_ptr(), al.data_ptr(), LH * 5, st) == 0
    assert lib.kzv_stream_set_topk(m._h, 0, None, None, 0, st) == 0                          # off again
    L.check(lib.kzv_stream_begin_beams(m._h, 4, 1, 1.0, None, 2, 2, LH, cfg.bos_id, cfg.eos_id, out.data_ptr(), LH, None, 0, None, st), "stream_begin_beams")
    assert lib.kzv_stream_set_topk(m._h, 5, ai.data_ptr(), al.data_ptr(), LH * 5, st) == -3
    assert b"beam" in lib.kzv_last_error()
    torch.cuda.synchronize()


# ---- records --------------------------------------------------------------------------------------------------------------------------------
def test_recognize_with_alternatives_on_the_fitted_fixture(trained):
    g, cfg, data, m = trained
    px = torch.from_numpy(np.concatenate([data["fit"][0], data["unseen"][0]]))
    Lmax = int(g["label_len"])
    many = m.recognize_many(px, max_length=Lmax, slots=5, top_k=3)
    one = m.recognize(px, num_beams=1, max_length=Lmax, top_k=3)
    assert "alternatives" not in m.recognize_many(px, max_length=Lmax, slots=5)[0]
    worst = 0.0
    for a, b in zip(many, one):
        assert a["tokens"] == b["tokens"] and a["text"] == b["text"]
        for r in (a, b):
            assert len(r["alternatives"]) == len(r["margins"]) == len(r["tokens"])
            for tok, lp, alts, margin in zip(r["tokens"], r["logprobs"], r["alternatives"], r["margins"]):
                assert 1 <= len(alts) <= 3
                assert all(x["logprob"] >= y["logprob"] for x, y in zip(alts, alts[1:]))
                assert alts[0]["token"] == tok                # greedy: the token is the first alternative
                worst = max(worst, abs(alts[0]["logprob"] - lp))
                assert margin >= 0
                assert all(isinstance(x["string"], str) for x in alts)
    assert sum(len(r["tokens"]) for r in many) > 12
    print(f"greedy records: first alternative against the token's log-probability {worst:.2e}")
    assert worst <= 1e-4
    beam = m.recognize(px, num_beams=4, max_length=Lmax, top_k=3)
    found = 0
    for r in beam:
        for tok, lp, alts, margin in zip(r["tokens"], r["logprobs"], r["alternatives"], r["margins"]):
            assert 1 <= len(alts) <= 3 and margin >= 0
            assert all(x["logprob"] >= y["logprob"] for x, y in zip(alts, alts[1:]))
            for x in alts:
                if x["token"] == tok:                         # after a beam search the token need not be first, or listed
                    assert abs(x["logprob"] - lp) <= 1e-4
                    found += 1
    assert found > 12
