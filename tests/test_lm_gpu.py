"""Language-model fusion on the GPU (csrc/lm_fusion.hip: kzv_lm_fuse; kzv_stream_set_lm; TrOCRModel.generate / generate_stream with
``lm=`` / ``lm_weight=``), numbered as in the feature's description:

  6. the kernel against kzv/lm.py::fuse_reference, ``torch.equal`` including the -inf positions and the columns between vocab and
     ld = vocab + 4: vocab 41 / 777 / 4300 with orders 1 / 3 / 4; LMs fitted on random sequences over a small pool plus a tail of rare
     tokens (some contexts found, some not), at 777 / 4300 with a planted context of 300 successors (the strided loop wraps); lockstep
     (one history longer than 256), greedy slots and beam slots with two idle slots whose rows come back untouched, step indices
     0, 1, 2, 36; a row holding -inf; the hand-built table whose length-2 context lacks its suffix; every call repeated;
     a table of 71,289 two-token contexts (the wave-wide search takes several rounds; first, last, present and absent keys);
  7. normalising kzv_logits_process (neutral controls) -> kzv_lm_fuse -> kzv_beam_rank_logprobs against log_softmax -> fuse_reference
     -> + beam score -> topk: indices equal, scores within 2e-5 * max(1, max |ref|);
  8. refusals of kzv_lm_fuse and kzv_stream_set_lm: nothing launched, message set;
  9. whole lockstep decodes on the kernel against ``lm_impl = "reference"``, greedy and 4 beams, alone and on top of controls;
 10. generate_stream(slots=6, lm=...) == generate(lm=...): tokens and beam scores ``torch.equal``; the condition (the fused decode
     differs from the unfused one on at least a quarter of the 40 crops) asserted on generate's own results first;
 11. off is absent; 12. alternatives under fusion; 13. the fitted fixture against the oracle.

The model of cases 9 - 12 is the recipe of tests/test_controls_gpu.py cases 4 - 8 in a copy (Lh = 38, 40 crops, 6 slots).  The LM of
cases 9 - 12 is fitted, order 3, on the model's own unfused greedy decodes of the first 20 of the 40 crops; LM_WEIGHT below.
Observed on MI355X, of 40 decodes, lines on which the fused decode differs from the unfused one:
  8 keys:   bf16 greedy 40 (40 with the controls on top);  2 beams 40 (40);  4 beams 40 (40);  e4m3 4 beams 40 (40)
  164 keys: bf16 greedy 27 (23);  4 beams 26 (40)
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from kzv import _lib as L
from kzv import beam as BM
from kzv import controls as CT
from kzv import lm as LM
from kzv.config import tiny_config
from kzv.data import build_decoder_dir, synthetic_batch
from kzv.lm import NGramLM
from kzv.model import TrOCRModel

from _trained import load as load_trained

pytestmark = pytest.mark.gpu
DEV = "cuda"
LH = 38
CROSS_GAIN = 24.0
EOS_BIAS = {8: 0.3, 164: 0.5}
PAD_BIAS = -8.0
LOGIT_TOL = 3e-2
LM_WEIGHT = 3.0
NEG_INF = float("-inf")


@pytest.fixture(autouse=True)
def _default_mode_afterwards():
    yield
    L.load().kzv_set_decode_one_launch(-1)


def _st():
    return L.stream_handle()


def _fuse(scores, ld, vocab, ids, dlm, weight, *, t=0, slot_image=None, slot_t=None, group=1, by_image=0, n_images=0):
    a = L.kzv_lm_fuse_args(logits=scores.data_ptr(), ld=ld, rows=scores.shape[0], vocab=vocab, ids=ids.data_ptr(), ld_ids=ids.stride(0), t=t,
                           group=group, slot_image=L.ptr(slot_image), slot_t=L.ptr(slot_t), by_image=by_image, n_images=n_images,
                           weight=weight, reserved=0, lm=C.pointer(dlm.struct))
    L.check(L.load().kzv_lm_fuse(C.byref(a), _st()), "lm_fuse")


def _random_lm(vocab, order, gen, plant):
    """(lm, pool, planted): fitted on sequences over a 12-token pool plus rare tokens; ``plant``: the context (pool[0], pool[1]) gets 300
    distinct successors (and so does its suffix)."""
    pool = torch.randperm(vocab - 3, generator=gen)[:12] + 3
    seqs = []
    for _ in range(60):
        n = int(torch.randint(3, 20, (1,), generator=gen))
        body = pool[torch.randint(0, 12, (n,), generator=gen)].tolist()
        if torch.rand(1, generator=gen) < 0.3:
            body[int(torch.randint(0, n, (1,), generator=gen))] = int(torch.randint(3, vocab, (1,), generator=gen))      # a rare token
        seqs.append([0] + body + [2])
    planted = (int(pool[0]), int(pool[1]))
    if plant:
        for v in (torch.randperm(vocab - 3, generator=gen)[:300] + 3).tolist():
            seqs.append([0, planted[0], planted[1], v, 2])
    return NGramLM.fit(seqs, order, vocab), pool, planted


def _histories(rows, width, pool, planted, vocab, gen):
    """rows over the pool (contexts that are found), with stretches of arbitrary tokens (contexts that are not) and the planted pair"""
    h = pool[torch.randint(0, 12, (rows, width), generator=gen)].to(torch.int64)
    wild = torch.rand(rows, width, generator=gen) < 0.15
    h = torch.where(wild, torch.randint(0, vocab, (rows, width), generator=gen), h)
    for r in range(0, rows, 3):                  # every third row ends its histories of every length >= 2 ... at even positions
        h[r, 0::2], h[r, 1::2] = planted[0], planted[1]
    h[:, 0] = 0
    return h


def _want(x, vocab, hists, lm, w):
    want = x.clone()
    for r, h in enumerate(hists):
        if h is not None:
            want[r:r + 1, :vocab] = LM.fuse_reference(x[r:r + 1, :vocab], h[None], lm, w)
    return want


# ---- 6. kernel == fuse_reference ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vocab,order", [(41, 1), (777, 3), (4300, 4), (41, 4), (4300, 2)])
def test_kernel_equals_fuse_reference_in_every_addressing_case(vocab, order):
    ld, w = vocab + 4, 0.37
    gen = torch.Generator().manual_seed(vocab * 7 + order)
    lm, pool, planted = _random_lm(vocab, order, gen, plant=vocab > 41)
    if vocab > 41 and order > 1:
        j = lm._find(planted[-(order - 1):] if order == 2 else planted)
        assert j >= 0 and (lm.off[min(order - 1, 2) - 1][j + 1] - lm.off[min(order - 1, 2) - 1][j]) > 256
    dlm = lm.to_device(DEV)
    found = missed = 0
    unseen = next((v for v in range(3, vocab) if order > 1 and lm._find([v]) < 0), None)      # a token that is no context of any length
    for rnd in range(2):                                               # every call repeated with changed inputs
        for t, width in ((0, 40), (1, 40), (2, 40), (36, 40), (299, 320)):
            ids = _histories(6, width, pool, planted, vocab, gen)
            if unseen is not None and t >= 1:
                ids[4, t] = unseen                                     # row 4 backs off all the way to the unigrams
            x = torch.randn(6, ld, generator=gen) * 3
            x[1, torch.randint(0, vocab, (7,), generator=gen)] = NEG_INF
            x[0, planted[0]] = NEG_INF
            xd, idd = x.to(DEV), ids.to(DEV)
            _fuse(xd, ld, vocab, idd, dlm, w, t=t)
            assert torch.equal(xd.cpu(), _want(x, vocab, [ids[r, :t + 1] for r in range(6)], lm, w)), ("lockstep", t, rnd)
            if order > 1 and t >= 1:
                for r in range(6):
                    hit = lm._find(ids[r, t:t + 1].tolist()) >= 0
                    found, missed = found + hit, missed + (not hit)
        slot_image = torch.tensor([4, -1, 0, 9, 2, 10, 7], dtype=torch.int32)      # 10 >= n_images: idle as well
        slot_t = torch.tensor([0, 5, 1, 2, 36, 3, 35], dtype=torch.int32)
        if rnd:
            slot_image, slot_t = slot_image.flip(0).contiguous(), slot_t.flip(0).contiguous()
        for group, by_image in ((1, 1), (1, 0), (2, 0), (4, 0)):
            R = 7 * group
            ids = _histories(10 if by_image else R, 40, pool, planted, vocab, gen)
            x = torch.randn(R, ld, generator=gen) * 3
            x[0, :5] = NEG_INF
            xd, idd = x.to(DEV), ids.to(DEV)
            _fuse(xd, ld, vocab, idd, dlm, w, t=1234, slot_image=slot_image.to(DEV), slot_t=slot_t.to(DEV), group=group, by_image=by_image, n_images=10)
            hists = []
            for r in range(R):
                s = r // group
                live = 0 <= int(slot_image[s]) < 10
                hists.append(ids[int(slot_image[s]) if by_image else r, :int(slot_t[s]) + 1] if live else None)
            got = xd.cpu()
            assert torch.equal(got, _want(x, vocab, hists, lm, w)), ("slots", group, by_image, rnd)
            idle = [r for r in range(R) if hists[r] is None]
            assert len(idle) == 2 * group and torch.equal(got[idle], x[idle])
    if order > 1:
        assert unseen is not None and found >= 10 and missed >= 8, (found, missed)      # some contexts found, some not


def test_kernel_on_the_hand_built_table_whose_context_lacks_its_suffix():
    import math
    uni = np.log(np.array([0.05, 0.1, 0.1, 0.15, 0.2, 0.1, 0.25, 0.05]))
    lm = NGramLM.from_tables(3, 8, uni, {(1, 2): (math.log(0.4), {5: math.log(0.5), 7: math.log(0.1)}),
                                         (3,): (math.log(0.3), {5: math.log(0.6), 6: math.log(0.1)}),
                                         (4, 3): (math.log(0.2), {6: math.log(0.7)})})
    dlm = lm.to_device(DEV)
    ids = torch.tensor([[0, 1, 2], [0, 4, 3], [0, 7, 3], [0, 3, 5], [9, 1, 2]], dtype=torch.int64)
    for rnd in range(2):
        x = torch.randn(5, 12, generator=torch.Generator().manual_seed(rnd)) * 2
        x[3, 6] = NEG_INF
        xd = x.to(DEV)
        _fuse(xd, 12, 8, ids.to(DEV), dlm, -1.25, t=2)
        assert torch.equal(xd.cpu(), _want(x, 8, list(ids), lm, -1.25))


def test_kernel_searches_a_large_context_table():
    """71,289 contexts of two tokens (every pair over 267 tokens) and 267 of one: the wave-wide search takes several rounds; histories over
    300 tokens, so some pairs are found and some are not."""
    vocab, w = 777, 0.6
    gen = torch.Generator().manual_seed(5)
    toks = list(range(3, 270))
    lp = (torch.rand(len(toks), len(toks), generator=gen) * -6 - 0.1).tolist()
    ctx = {(a, b): (-0.5 - 0.001 * i, {3 + (i * 7 + j * 13) % 700: lp[i][j]}) for i, a in enumerate(toks) for j, b in enumerate(toks)}
    ctx.update({(a,): (-0.25 - 0.002 * i, {5 + i: -1.0 - 0.01 * i, 6 + i: -2.0}) for i, a in enumerate(toks)})
    lm = NGramLM.from_tables(3, vocab, np.log(np.full(vocab, 1.0 / vocab)) - np.arange(vocab) * 1e-3, ctx)
    assert lm.n_contexts() == [267, 267 * 267]
    dlm = lm.to_device(DEV)
    found = missed = 0
    for t in (1, 2, 17, 39):
        ids = torch.randint(3, 300, (24, 40), generator=gen)
        ids[0, :], ids[1, :], ids[2, t - 1:t + 1] = 3, 269, torch.tensor([269, 3])      # the table's first and last keys
        x = torch.randn(24, vocab + 4, generator=gen) * 3
        xd = x.to(DEV)
        _fuse(xd, vocab + 4, vocab, ids.to(DEV), dlm, w, t=t)
        assert torch.equal(xd.cpu(), _want(x, vocab, [ids[r, :t + 1] for r in range(24)], lm, w)), t
        for r in range(24):
            hit = lm._find(ids[r, t - 1:t + 1].tolist()) >= 0
            found, missed = found + hit, missed + (not hit)
    assert found > 40 and missed > 5, (found, missed)


# ---- 7. normalise -> fuse -> rank ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,nb,vocab", [(3, 4, 41), (5, 2, 777), (6, 4, 4300)])
def test_normalise_fuse_rank_equals_log_softmax_fuse_topk(B, nb, vocab):
    lib = L.load()
    ld, K, R, t, w = vocab + 4, 2 * nb, B * nb, 17, 0.8
    gen = torch.Generator().manual_seed(B * vocab + nb)
    lm, pool, planted = _random_lm(vocab, 3, gen, plant=vocab > 41)
    dlm = lm.to_device(DEV)
    ids = _histories(R, 24, pool, planted, vocab, gen)
    buf = torch.randn(R, ld, generator=gen) * 3
    sc = torch.randn(B, nb, generator=gen)
    sc[0, 1:] = -1.0e9
    work, idd, scd = buf.to(DEV), ids.to(DEV), sc.to(DEV)
    neutral = CT.GenerationControls()
    a = L.kzv_logits_process_args(logits=work.data_ptr(), ld=ld, rows=R, vocab=vocab, ids=idd.data_ptr(), ld_ids=24, t=t, group=1, slot_image=None,
                                  slot_t=None, by_image=0, n_images=0, no_repeat_ngram_size=0, min_length=0, eos_id=2, normalise=1,
                                  repetition_penalty=neutral.repetition_penalty, reserved=0, suppress_mask=None)
    L.check(lib.kzv_logits_process(C.byref(a), _st()), "logits_process")
    _fuse(work, ld, vocab, idd, dlm, w, t=t)
    out_lp, out_ix = torch.empty(B, K, device=DEV), torch.empty(B, K, dtype=torch.int64, device=DEV)
    L.check(lib.kzv_beam_rank_logprobs(work.data_ptr(), ld, scd.data_ptr(), B, nb, vocab, K, out_lp.data_ptr(), out_ix.data_ptr(), _st()), "rank")
    torch.cuda.synchronize()
    logp = LM.fuse_reference(torch.log_softmax(buf[:, :vocab], dim=-1), ids[:, :t + 1], lm, w)
    ref_lp, ref_ix = (logp.view(B, nb, vocab) + sc.unsqueeze(-1)).view(B, nb * vocab).topk(K, dim=1)
    tol = 2e-5 * max(1.0, ref_lp[ref_lp > -1e8].abs().max().item())
    print(f"vocab {vocab}: max |score difference| {(out_lp.cpu() - ref_lp).abs().max().item():.3g} (bound {tol:.3g})")
    assert torch.equal(out_ix.cpu(), ref_ix)
    assert (out_lp.cpu() - ref_lp).abs().max().item() < tol
    assert torch.equal(work.cpu()[:, vocab:], buf[:, vocab:])


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch():
    lib = L.load()
    lm = NGramLM.fit([[0, 5, 6, 7, 5, 6, 2], [0, 6, 5, 2]], 3, 41)
    dlm = lm.to_device(DEV)
    x = torch.zeros(4, 48, device=DEV)
    ids = torch.zeros(4, 16, dtype=torch.int64, device=DEV)
    si = torch.zeros(4, dtype=torch.int32, device=DEV)
    base = dict(logits=x.data_ptr(), ld=48, rows=4, vocab=41, ids=ids.data_ptr(), ld_ids=16, t=3, group=1, slot_image=None, slot_t=None, by_image=0,
                n_images=0, weight=0.5, reserved=0, lm=C.pointer(dlm.struct))

    def variant(**kw):
        s = L.kzv_ngram_lm()
        C.memmove(C.byref(s), C.byref(dlm.struct), C.sizeof(s))
        for k, v in kw.items():
            setattr(s, k, v)
        return s
    bad_order, bad_vocab, no_uni = variant(order=5), variant(vocab=40), variant(uni=None)
    no_keys = variant()
    no_keys.keys[0] = None
    before = lib.kzv_test_lm_fuse_calls()
    cases = [(dict(logits=None), b"null"), (dict(ids=None), b"null"), (dict(lm=None), b"null"), (dict(rows=0), b"rows"),
             (dict(vocab=16385, ld=16388), b"vocab"), (dict(vocab=0), b"vocab"), (dict(vocab=40), b"vocabulary"), (dict(ld=40), b"ld"),
             (dict(ld_ids=0), b"ld_ids"), (dict(lm=C.pointer(bad_order)), b"order"), (dict(lm=C.pointer(bad_vocab)), b"vocabulary"),
             (dict(lm=C.pointer(no_uni)), b"null"), (dict(lm=C.pointer(no_keys)), b"null"), (dict(weight=float("nan")), b"finite"),
             (dict(weight=float("inf")), b"finite"), (dict(slot_image=si.data_ptr()), b"slot_image"), (dict(slot_t=si.data_ptr()), b"slot_image"),
             (dict(slot_image=si.data_ptr(), slot_t=si.data_ptr(), group=3, n_images=4), b"multiple"), (dict(t=-1), b"negative")]
    for kw, needle in cases:
        assert lib.kzv_lm_fuse(C.byref(L.kzv_lm_fuse_args(**dict(base, **kw))), _st()) == -1, kw
        assert needle in lib.kzv_last_error(), (kw, lib.kzv_last_error())
    assert lib.kzv_lm_fuse(None, _st()) == -1 and b"null" in lib.kzv_last_error()
    assert lib.kzv_test_lm_fuse_calls() == before
    torch.cuda.synchronize()
    assert torch.equal(x, torch.zeros_like(x))
    assert lib.kzv_lm_fuse(C.byref(L.kzv_lm_fuse_args(**base)), _st()) == 0 and lib.kzv_test_lm_fuse_calls() == before + 1
    torch.cuda.synchronize()


# ---- the model of cases 9 - 12 -------------------------------------------------------------------------------------------------------------------
def _cfg(keys):
    w = {8: 64, 164: 1312}[keys]
    c = dataclasses.replace(tiny_config(), image_w=w, dec_hidden=256, dec_heads=4, dec_ffn=768, dec_layers=3)
    assert c.num_patches == keys
    return c


_models = {}
PAD = tiny_config().pad_id
COMBO = dict(no_repeat_ngram_size=2, repetition_penalty=1.2)


@pytest.fixture(scope="module")
def decoder_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("dec"))


def _pad(ids, pad_id, width=LH):
    out = torch.full((ids.shape[0], width), pad_id, dtype=torch.int64, device=ids.device)
    out[:, :ids.shape[1]] = ids
    return out


def _model(keys, decoder_dir):
    """(cfg, model, crops, cache, lm): the LM is fitted on the model's own unfused bf16 greedy decodes of the first 20 crops"""
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
        own = _pad(m.generate(px[:20], max_length=LH), cfg.pad_id).cpu().numpy()
        lm = NGramLM.fit(LM.sequences_from_labels(own, cfg.pad_id, cfg.eos_id), 3, cfg.vocab)
        _models[keys] = (cfg, m, px, {}, lm)
    return _models[keys]


def _lockstep(keys, fmt, nb, fused, combo, decoder_dir):
    cfg, m, px, cache, lm = _model(keys, decoder_dir)
    m.set_decode_weights(fmt)
    key = (fmt, nb, fused, combo)
    if key not in cache:
        kw = dict(COMBO if combo else {}, **(dict(lm=lm, lm_weight=LM_WEIGHT) if fused else {}))
        if nb == 1:
            ids, sc = m.generate(px, max_length=LH, **kw), None
        else:
            ids, sc = m.generate(px, max_length=LH, num_beams=nb, return_scores=True, **kw)
        assert m.decode_step_impl == "one-launch" and m.decode_weights_impl == fmt
        cache[key] = (_pad(ids, cfg.pad_id), sc)
    return cfg, m, px, lm, cache[key]


# ---- 9. device kernel == torch statement inside whole lockstep decodes ------------------------------------------------------------------------
@pytest.mark.parametrize("combo", [False, True])
@pytest.mark.parametrize("nb", [1, 4])
def test_generate_on_the_kernel_equals_generate_on_fuse_reference(nb, combo, decoder_dir):
    cfg, m, px, lm, (dev, _) = _lockstep(8, "bf16", nb, True, combo, decoder_dir)
    lib = L.load()
    kw = dict(COMBO if combo else {}, lm=lm, lm_weight=LM_WEIGHT)
    before = lib.kzv_test_lm_fuse_calls()
    again = m.generate(px, max_length=LH, num_beams=nb, **kw)
    assert lib.kzv_test_lm_fuse_calls() - before == m.last_generate_steps      # one launch per decoder step
    m.lm_impl = "reference"
    try:
        before = lib.kzv_test_lm_fuse_calls()
        ref = m.generate(px, max_length=LH, num_beams=nb, **kw)                # the controls stay on the device in both arms
        assert lib.kzv_test_lm_fuse_calls() == before
    finally:
        m.lm_impl = "device"
    assert torch.equal(_pad(again, cfg.pad_id), dev) and torch.equal(_pad(ref, cfg.pad_id), dev)


# ---- 10. stream == lockstep under fusion -----------------------------------------------------------------------------------------------------
CASES = [(8, "bf16", 1), (8, "bf16", 2), (8, "bf16", 4), (164, "bf16", 1), (164, "bf16", 4), (8, "e4m3", 4)]


@pytest.mark.parametrize("combo", [False, True])
@pytest.mark.parametrize("keys,fmt,nb", CASES)
def test_generate_stream_equals_generate_under_fusion(keys, fmt, nb, combo, decoder_dir):
    cfg, m, px, lm, (want, want_sc) = _lockstep(keys, fmt, nb, True, combo, decoder_dir)
    plain = _lockstep(keys, fmt, nb, False, combo, decoder_dir)[4][0]
    changed = int((plain != want).any(dim=1).sum())
    print(f"{keys} keys, {fmt}, {nb} beam(s), controls {'on' if combo else 'off'}: the fused decode differs on {changed} of 40 crops")
    assert changed * 4 >= 40, changed                                  # the condition, on generate's own results, before any stream runs
    kw = dict(COMBO if combo else {}, lm=lm, lm_weight=LM_WEIGHT)
    if nb == 1:
        got = m.generate_stream(px, max_length=LH, slots=6, **kw)
        assert m.stream_decode_impl == "slot-refill"
    else:
        got, sc = m.generate_stream(px, max_length=LH, slots=6, num_beams=nb, return_scores=True, **kw)
        assert m.stream_beam_impl == "slot-refill"
        assert m.last_stream_pad_fallbacks == 0                          # no running beam took padding: the slots decoded the wave
        assert torch.equal(sc, want_sc)
    assert torch.equal(_pad(got, cfg.pad_id), want)
    assert m.last_stream_steps > 0


# ---- 11. off is absent -----------------------------------------------------------------------------------------------------------------------
def test_off_launches_nothing_and_changes_nothing(decoder_dir):
    cfg, m, px, _, lm = _model(8, decoder_dir)
    m.set_decode_weights("bf16")
    lib = L.load()
    ids0, lp0 = m.generate_stream(px, max_length=LH, slots=6, return_logprobs=True)
    steps0 = m.last_stream_steps
    b0 = m.generate_stream(px, max_length=LH, slots=6, num_beams=4)
    fuse0, proc0 = lib.kzv_test_lm_fuse_calls(), lib.kzv_test_logits_process_calls()
    for kw in (dict(lm=None, lm_weight=0.7), dict(lm=lm, lm_weight=0.0), dict(lm=lm.to_device(DEV), lm_weight=0.0)):
        ids1, lp1 = m.generate_stream(px, max_length=LH, slots=6, return_logprobs=True, **kw)
        assert torch.equal(ids0, ids1) and torch.equal(lp0, lp1) and m.last_stream_steps == steps0
        assert torch.equal(b0, m.generate_stream(px, max_length=LH, slots=6, num_beams=4, **kw))
        assert torch.equal(_pad(ids0, cfg.pad_id), _pad(m.generate(px, max_length=LH, **kw), cfg.pad_id))
    assert lib.kzv_test_lm_fuse_calls() == fuse0 and lib.kzv_test_logits_process_calls() == proc0
    m.generate_stream(px, max_length=LH, slots=6, num_beams=4, lm=lm, lm_weight=LM_WEIGHT)
    assert lib.kzv_test_lm_fuse_calls() > fuse0 and lib.kzv_test_logits_process_calls() > proc0      # a beam wave normalises through the controls' node
    # the handle refuses what the Python layer would have refused first (the last wave is still begun), and launches nothing for it
    d = lm.to_device(DEV)
    fuse1 = lib.kzv_test_lm_fuse_calls()
    bad = L.kzv_ngram_lm()
    C.memmove(C.byref(bad), C.byref(d.struct), C.sizeof(bad))
    bad.order = 0
    other = NGramLM(2, cfg.vocab - 1).to_device(DEV)
    no_uni, no_off = L.kzv_ngram_lm(), L.kzv_ngram_lm()
    for s in (no_uni, no_off):
        C.memmove(C.byref(s), C.byref(d.struct), C.sizeof(s))
    no_uni.uni = None
    no_off.off[1] = None
    assert d.struct.n_ctx[1] > 0
    for args, needle in (((None, 0.5), b"null"), ((C.byref(bad), 0.5), b"order"), ((C.byref(other.struct), 0.5), b"vocabulary"),
                         ((C.byref(no_uni), 0.5), b"null"), ((C.byref(no_off), 0.5), b"null"),
                         ((C.byref(d.struct), float("nan")), b"finite"), ((C.byref(d.struct), float("-inf")), b"finite")):
        assert lib.kzv_stream_set_lm(m._h, args[0], args[1], _st()) == -1 and needle in lib.kzv_last_error(), lib.kzv_last_error()
    assert lib.kzv_stream_set_lm(m._h, C.byref(d.struct), 0.0, _st()) == 0        # fine, and off
    # KZV_E_STATE outside a begun wave: no handle, and a bound model that has begun none
    assert lib.kzv_stream_set_lm(None, C.byref(d.struct), 0.5, _st()) == -3
    fresh = TrOCRModel(cfg.encoder_config_dict(), build_decoder_dir(decoder_dir + "/fresh", cfg), init_seed=7, load_tokenizer=False)
    fresh._bind(6, LH)
    assert lib.kzv_stream_set_lm(fresh._h, C.byref(d.struct), 0.5, _st()) == -3 and b"stream_begin" in lib.kzv_last_error()
    assert lib.kzv_test_lm_fuse_calls() == fuse1


# ---- 12. alternatives under fusion -----------------------------------------------------------------------------------------------------------
def test_alternatives_and_logprobs_are_those_of_the_fused_row(decoder_dir, monkeypatch):
    cfg, m, px, _, lm = _model(8, decoder_dir)
    m.set_decode_weights("bf16")
    six = px[:6]
    ids, lp, a_ids, a_lp = m.generate_stream(six, max_length=LH, slots=6, top_k=5, lm=lm, lm_weight=LM_WEIGHT)      # one wave of 6 slots
    rows = []                                    # the fused rows of lockstep generate's own steps, taken off the torch statement
    real = LM.fuse_reference

    def recording(scores, hist, model, weight):
        y = real(scores, hist, model, weight)
        rows.append(y.clone())
        return y
    monkeypatch.setattr(LM, "fuse_reference", recording)
    m.lm_impl = "reference"
    try:
        ref = m.generate(six, max_length=LH, lm=lm, lm_weight=LM_WEIGHT)
    finally:
        m.lm_impl = "device"
    assert torch.equal(_pad(ids, cfg.pad_id), _pad(ref, cfg.pad_id))
    checked = 0
    for i, r in enumerate(ids.tolist()):
        n = len([t for t in r if t != cfg.pad_id])
        for j in range(1, n):
            logp = torch.log_softmax(rows[j - 1][i], dim=-1)
            top = logp.topk(5)
            assert int(a_ids[i, j, 0]) == r[j]
            assert (a_lp[i, j] - top.values).abs().max().item() < 1e-5 and abs(float(lp[i, j]) - float(logp[r[j]])) < 1e-5
            checked += 1
    assert checked > 30


# ---- 13. the fitted fixture against the oracle ---------------------------------------------------------------------------------------------------
def _edit(a, b):
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = cur
    return prev[-1]


def test_fitted_fixture_greedy_with_the_fitted_lm_equals_the_oracle(tmp_path):
    """With the oracle alone on the CPU: 0 of 12 lines left out, smallest margin 0.238; lines 9, 10, 11 differ from the unfused decode;
    edit errors of the four unseen lines 16 / 10 / 9 / 9 -> 16 / 7 / 4 / 7."""
    from oracle import trocr_oracle as O
    gold, cfg, sd, data = load_trained()
    Lh = int(gold["label_len"])
    px = np.concatenate([data["fit"][0], data["unseen"][0]])
    labs = np.concatenate([data["fit"][1], data["unseen"][1]])
    seqs = LM.sequences_from_labels(labs, cfg.pad_id, cfg.eos_id)
    lm = NGramLM.fit(seqs, 3, cfg.vocab, discount=0.75)
    weight = 8.0
    raw = O.stepwise_logits(cfg, O.leaf_state_dict(sd, requires_grad=False), px, repeat=1)
    margins = []

    def step(t, ids):
        y = LM.fuse_reference(torch.as_tensor(raw(t, ids)).float(), ids[:, :t + 1], lm, weight)
        top = y.topk(2, dim=-1)[0]
        margins.append(top[:, 0] - top[:, 1])
        return y
    want = BM.greedy(step, 12, Lh, cfg.pad_id, cfg.bos_id, cfg.eos_id, "cpu").numpy()
    mg = torch.stack(margins, 1).numpy()
    mins = []
    for b in range(12):
        row = want[b].tolist()
        n_live = row.index(cfg.eos_id) if cfg.eos_id in row else len(row) - 1
        mins.append(float(mg[b, :n_live].min()))
    sure = np.array(mins) >= LOGIT_TOL
    plain = BM.greedy(lambda t, ids: torch.as_tensor(raw(t, ids)).float(), 12, Lh, cfg.pad_id, cfg.bos_id, cfg.eos_id, "cpu").numpy()

    def toks(r):
        return [int(t) for t in r if t not in (cfg.pad_id, cfg.bos_id, cfg.eos_id)]
    differ = [b for b in range(12) if toks(plain[b]) != toks(want[b])]
    err0 = [_edit(toks(plain[b]), seqs[b][1:-1]) for b in range(8, 12)]
    err1 = [_edit(toks(want[b]), seqs[b][1:-1]) for b in range(8, 12)]
    print(f"{int((~sure).sum())} of 12 lines left out; smallest margin {min(mins):.3g}; lines {differ} differ; unseen edit errors {err0} -> {err1}")
    assert (~sure).sum() <= 3
    assert differ and sum(err1) <= sum(err0)
    m = TrOCRModel(cfg.encoder_config_dict(), build_decoder_dir(str(tmp_path / "dec"), cfg), load_tokenizer=False)
    m.load_state_dict(sd, strict=True)
    m.eval()
    got = m.generate(torch.from_numpy(px), max_length=Lh, num_beams=1, lm=lm, lm_weight=weight).cpu().numpy()
    w = max(got.shape[1], want.shape[1])
    got = np.pad(got, ((0, 0), (0, w - got.shape[1])), constant_values=cfg.pad_id)
    want = np.pad(want, ((0, 0), (0, w - want.shape[1])), constant_values=cfg.pad_id)
    assert np.array_equal(got[sure], want[sure])
