"""Forced prefixes on the GPU (csrc/force_prefix.hip: kzv_force_prefix; kzv_stream_set_prefix; kzv_beam_update_prefix /
kzv_stream_beam_update_prefix; TrOCRModel.generate / generate_stream with ``prefix_ids``):

  1. the kernel against kzv/prefix.py::force_reference with ``torch.equal``: vocab 41 / 777 / 4300 / 16,384 with ld = vocab + 4; the
     lockstep case (1 and 4 rows per image) at t = 0, 1, prefix_len - 1 (last forced) and prefix_len (first free); the slot cases with 7
     slots, two idle, (group, by_image) = (1, 1), (2, 0), (4, 0); mixed prefix lengths including 0; every call repeated with changed
     inputs; idle rows and the columns between vocab and ld bit-unchanged.  ``forced_logprob`` against the fp64 log_softmax of the same
     fp32 rows (randn * 3) within 1e-4 -- the bound tests/test_alternatives_gpu.py holds kzv_token_topk to on such rows -- equal to x[f]
     exactly when ``normalised``, untouched where nothing is forced;
  2. whole lockstep decodes on the kernel equal those on ``prefix_impl = "reference"``: 1 and 4 beams, plain and with controls + the
     language model on; kzv_test_force_prefix_calls rises by last_generate_steps on the device path, not at all on the reference path;
  3. greedy self-consistency: forcing the first k = 1, 4 tokens of the model's own greedy decode (k clipped to the tokens a line has before
     its first special token: a prefix holds none) returns that decode for all 40 crops; a first token different from the model's changes
     all 40; every output row starts with [BOS] + prefix;
  4. generate_stream(prefix_ids, slots=6) == generate(prefix_ids) per image, ids and beam scores ``torch.equal``, ragged prefixes of 0..5
     tokens over 40 images, so slots are reseated inside other images' prefixes; (keys, format, beams) = (8, bf16, 1), (8, bf16, 2),
     (8, bf16, 4), (164, bf16, 1), (164, bf16, 4), (8, e4m3, 4); no pad fallback; ``limits`` with prefixes against
     generate(max_length=limit); n-best rows and per-token log-probabilities with a prefix: forced columns exactly 0;
  5. off is absent: no ``prefix_ids``, or all empty: the counter stands still and ids / log-probabilities / step counts are those of the
     plain call, greedy and 4 beams; the handle refuses a null length table, a prefix that reaches max_len - 1 and a call outside a wave.

The model is that of tests/test_controls_gpu.py (in a copy): decoder 256 / 4 heads / FFN 768 / 3 layers on the tiny encoder, recipe seed 7,
CROSS_GAIN, PAD_BIAS and its EOS biases; Lh = 38, 40 crops, 6 slots.
"""
import ctypes as C
import dataclasses

import pytest
import torch

from kzv import _lib as L
from kzv import lm as LM
from kzv import prefix as PF
from kzv.config import tiny_config
from kzv.data import build_decoder_dir, synthetic_batch
from kzv.lm import NGramLM
from kzv.model import TrOCRModel

pytestmark = pytest.mark.gpu
DEV = "cuda"
LH = 38
CROSS_GAIN = 24.0
EOS_BIAS = {8: 0.3, 164: 0.5}
PAD_BIAS = -8.0
NEG_INF = float("-inf")
SENTINEL = 7.25


@pytest.fixture(autouse=True)
def _default_mode_afterwards():
    yield
    L.load().kzv_set_decode_one_launch(-1)


def _st():
    return L.stream_handle()


def _force(x, ld, vocab, pfx, plen, *, t=0, slot_image=None, slot_t=None, group=1, by_image=0, n_images=0, normalised=0, flp=None):
    a = L.kzv_force_prefix_args(logits=x.data_ptr(), ld=ld, rows=x.shape[0], vocab=vocab, t=t, group=group, slot_image=L.ptr(slot_image),
                                slot_t=L.ptr(slot_t), by_image=by_image, n_images=n_images, prefix=pfx.data_ptr(), ld_prefix=pfx.stride(0),
                                prefix_len=plen.data_ptr(), normalised=normalised, reserved=0, forced_logprob=L.ptr(flp),
                                ld_forced_logprob=0 if flp is None else flp.stride(0))
    L.check(L.load().kzv_force_prefix(C.byref(a), _st()), "force_prefix")


def _check_flp(flp_d, x, vocab, img_of_row, cur_of_row, live_row, group, pfx, plen, normalised):
    """forced_logprob after a call: the first row of every forced group wrote [image][cur]; everything else holds the sentinel."""
    got = flp_d.cpu()
    want_mask = torch.zeros_like(got, dtype=torch.bool)
    worst = 0.0
    for r in range(0, x.shape[0], group):
        if not live_row[r]:
            continue
        i, cur = img_of_row[r], cur_of_row[r]
        if 1 <= cur <= int(plen[i]):
            f = int(pfx[i, cur - 1])
            want_mask[i, cur] = True
            if normalised:
                assert float(got[i, cur]) == float(x[r, f]), (r, i, cur)
            else:
                ref = float(torch.log_softmax(x[r, :vocab].double(), -1)[f])
                worst = max(worst, abs(float(got[i, cur]) - ref))
    assert bool((got[~want_mask] == SENTINEL).all())                   # untouched where nothing is forced
    assert worst <= 1e-4, worst
    return int(want_mask.sum())


# ---- 1. the kernel == force_reference ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vocab", [41, 777, 4300, 16384])
def test_kernel_equals_force_reference_in_every_addressing_case(vocab):
    ld = vocab + 4
    gen = torch.Generator().manual_seed(vocab)
    P = 5
    written = 0
    for rnd in range(2):                                               # the call repeated with changed inputs
        # (a) lockstep: group rows per image, images 0 .. 5 with prefix lengths 0, 1, 3, 5, 5, 2
        plen = torch.tensor([0, 1, 3, 5, 5, 2], dtype=torch.int32)
        if rnd:
            plen = plen.flip(0).contiguous()
        pfx = torch.randint(0, vocab, (6, P), generator=gen)
        for group in (1, 4):
            for t in (0, 1, P - 1, P):                                 # P - 1: the last forced step of the longest; P: the first free step of all
                for normalised in (0, 1):
                    R = 6 * group
                    x = torch.randn(R, ld, generator=gen) * 3
                    xd = x.to(DEV)
                    flp = torch.full((6, P + 1), SENTINEL, device=DEV)
                    _force(xd, ld, vocab, pfx.to(DEV), plen.to(DEV), t=t, group=group, normalised=normalised, flp=flp)
                    want = x.clone()
                    want[:, :vocab] = PF.force_reference(x[:, :vocab], t + 1, pfx.repeat_interleave(group, 0), plen.repeat_interleave(group))
                    assert torch.equal(xd.cpu(), want), ("lockstep", group, t, rnd)
                    assert torch.equal(xd.cpu()[:, vocab:], x[:, vocab:])
                    n_forced = int((plen >= t + 1).sum())
                    assert int((want[:, :vocab] == 0).all(dim=1).sum()) == 0 and int((want[:, :vocab] == NEG_INF).sum()) == n_forced * group * (vocab - 1)
                    written += _check_flp(flp, x, vocab, [r // group for r in range(R)], [t + 1] * R, [True] * R, group, pfx, plen, normalised)
        # (b) greedy slots and (c) beam slots: 7 slots, two idle, 10 images
        slot_image = torch.tensor([4, -1, 0, 9, 2, -1, 7], dtype=torch.int32)
        slot_t = torch.tensor([0, 5, 1, 2, 4, 3, 36], dtype=torch.int32)
        if rnd:
            slot_image, slot_t = slot_image.flip(0).contiguous(), slot_t.flip(0).contiguous()
        plen = torch.tensor([2, 0, 5, 1, 3 if rnd else 1, 0, 4, 5, 0, 3], dtype=torch.int32)
        pfx = torch.randint(0, vocab, (10, P), generator=gen)
        for group, by_image in ((1, 1), (2, 0), (4, 0)):
            R = 7 * group
            x = torch.randn(R, ld, generator=gen) * 3
            xd = x.to(DEV)
            flp = torch.full((10, P + 1), SENTINEL, device=DEV)
            _force(xd, ld, vocab, pfx.to(DEV), plen.to(DEV), t=1234, slot_image=slot_image.to(DEV), slot_t=slot_t.to(DEV), group=group,
                   by_image=by_image, n_images=10, flp=flp)
            want = x.clone()
            live = [bool(slot_image[r // group] >= 0) for r in range(R)]
            imgs = [max(int(slot_image[r // group]), 0) for r in range(R)]
            curs = [int(slot_t[r // group]) + 1 for r in range(R)]
            rows_len = torch.tensor([int(plen[i]) if lv else 0 for i, lv in zip(imgs, live)])
            want[:, :vocab] = PF.force_reference(x[:, :vocab], torch.tensor(curs), pfx[torch.tensor(imgs)], rows_len)
            assert torch.equal(xd.cpu(), want), ("slots", group, by_image, rnd)
            idle = [r for r in range(R) if not live[r]]
            assert len(idle) == 2 * group and torch.equal(xd.cpu()[idle], x[idle])
            assert int((want != x).any(dim=1).sum()) >= group           # some slot is inside its prefix
            written += _check_flp(flp, x, vocab, imgs, curs, live, group, pfx, plen, 0)
    assert written >= 40
    torch.cuda.synchronize()


# ---- the model of cases 2 - 5 ------------------------------------------------------------------------------------------------------------
def _cfg(keys):
    w = {8: 64, 164: 1312}[keys]
    c = dataclasses.replace(tiny_config(), image_w=w, dec_hidden=256, dec_heads=4, dec_ffn=768, dec_layers=3)
    assert c.num_patches == keys
    return c


_models = {}
PAD = tiny_config().pad_id
COMBO = dict(no_repeat_ngram_size=2, repetition_penalty=1.2, suppress_tokens=[PAD])
LM_WEIGHT = 3.0


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


def _ragged(cfg, n=40, longest=5, seed=11):
    """n prefixes of 0 .. longest tokens, no special ids; the first three have lengths 0, longest, 1."""
    g = torch.Generator().manual_seed(seed)
    lens = [int(x) for x in torch.randint(0, longest + 1, (n,), generator=g)]
    lens[0], lens[1], lens[2] = 0, longest, 1
    return [[int(x) for x in torch.randint(5, cfg.vocab, (k,), generator=g)] for k in lens]


def _starts_with_prefix(rows, lists, cfg):
    for r, p in zip(rows.tolist(), lists):
        assert r[:1 + len(p)] == [cfg.bos_id] + p, (r, p)


def _lockstep(keys, fmt, nb, decoder_dir):
    """generate(num_beams=nb, prefix_ids=ragged) of the 40 crops, padded to LH, and the winners' scores (beams); computed once."""
    cfg, m, px, cache = _model(keys, decoder_dir)
    m.set_decode_weights(fmt)
    lists = _ragged(cfg)
    if (fmt, nb) not in cache:
        if nb == 1:
            ids, sc = m.generate(px, max_length=LH, prefix_ids=lists), None
        else:
            ids, sc = m.generate(px, max_length=LH, num_beams=nb, return_scores=True, prefix_ids=lists)
        assert m.decode_step_impl == "one-launch" and m.decode_weights_impl == fmt
        _starts_with_prefix(ids, lists, cfg)
        cache[(fmt, nb)] = (_pad(ids, cfg.pad_id), sc)
    return cfg, m, px, lists, cache[(fmt, nb)]


# ---- 2. device kernel == torch statement inside whole lockstep decodes -------------------------------------------------------------------
@pytest.mark.parametrize("extras", [False, True])
@pytest.mark.parametrize("nb", [1, 4])
def test_generate_on_the_kernel_equals_generate_on_force_reference(nb, extras, decoder_dir):
    cfg, m, px, _ = _model(8, decoder_dir)
    m.set_decode_weights("bf16")
    lists = _ragged(cfg)
    kw = {}
    if extras:                                   # controls + language model on: the prefix comes after both
        own = _pad(m.generate(px[:20], max_length=LH), cfg.pad_id).cpu().numpy()
        lm = NGramLM.fit(LM.sequences_from_labels(own, cfg.pad_id, cfg.eos_id), 3, cfg.vocab)
        kw = dict(COMBO, lm=lm, lm_weight=LM_WEIGHT)
    lib = L.load()
    before = lib.kzv_test_force_prefix_calls()
    dev = m.generate(px, max_length=LH, num_beams=nb, prefix_ids=lists, **kw)
    assert lib.kzv_test_force_prefix_calls() - before == m.last_generate_steps      # one launch per decoder step
    m.prefix_impl = "reference"
    try:
        before = lib.kzv_test_force_prefix_calls()
        ref = m.generate(px, max_length=LH, num_beams=nb, prefix_ids=lists, **kw)
        assert lib.kzv_test_force_prefix_calls() == before               # the substitution launches no force kernel
    finally:
        m.prefix_impl = "device"
    assert dev.shape == ref.shape and torch.equal(dev, ref)
    _starts_with_prefix(dev, lists, cfg)
    plain = _pad(m.generate(px, max_length=LH, num_beams=nb, **kw), cfg.pad_id)
    nonempty = sum(1 for p in lists if p)
    assert nonempty == 32                                                # (the recipe of _ragged)
    # the prefixes act on this model: a random first token is the model's own for 1 row in ~150
    assert int((plain != _pad(dev, cfg.pad_id)).any(dim=1).sum()) >= nonempty - 2


# ---- 3. greedy self-consistency ----------------------------------------------------------------------------------------------------------
def test_forcing_the_models_own_first_tokens_returns_its_own_decode(decoder_dir):
    cfg, m, px, _ = _model(8, decoder_dir)
    m.set_decode_weights("bf16")
    base = _pad(m.generate(px, max_length=LH), cfg.pad_id)
    rows = base.tolist()
    special = {cfg.pad_id, cfg.bos_id, cfg.eos_id}
    total = 0
    for k in (1, 4):
        lists = []
        for r in rows:
            p = []
            for tok in r[1:1 + k]:
                if tok in special:               # a prefix holds no special token: the line gives fewer than k
                    break
                p.append(tok)
            lists.append(p)
        total += sum(len(p) for p in lists)
        got = m.generate(px, max_length=LH, prefix_ids=lists)
        assert torch.equal(_pad(got, cfg.pad_id), base), k
        _starts_with_prefix(got, lists, cfg)
    assert total >= 40 * 3                       # most lines gave k tokens
    other = [[5 + (r[1] - 5 + 1) % (cfg.vocab - 5) if r[1] >= 5 else 5] for r in rows]
    assert all(p[0] != r[1] and p[0] >= 5 for p, r in zip(other, rows))
    got = _pad(m.generate(px, max_length=LH, prefix_ids=other), cfg.pad_id)
    _starts_with_prefix(got, other, cfg)
    assert int((got != base).any(dim=1).sum()) == 40


# ---- 4. stream == lockstep ---------------------------------------------------------------------------------------------------------------
CASES = [(8, "bf16", 1), (8, "bf16", 2), (8, "bf16", 4), (164, "bf16", 1), (164, "bf16", 4), (8, "e4m3", 4)]


@pytest.mark.parametrize("keys,fmt,nb", CASES)
def test_generate_stream_equals_generate_with_ragged_prefixes(keys, fmt, nb, decoder_dir):
    cfg, m, px, lists, (want, want_sc) = _lockstep(keys, fmt, nb, decoder_dir)
    lib = L.load()
    before = lib.kzv_test_force_prefix_calls()
    if nb == 1:
        got, lp = m.generate_stream(px, max_length=LH, slots=6, prefix_ids=lists, return_logprobs=True)
        assert m.stream_decode_impl == "slot-refill"
        for i, p in enumerate(lists):            # forced columns carry exactly 0; the first free token does not
            assert bool((lp[i, :1 + len(p)] == 0).all()) and float(lp[i, 1 + len(p)]) < 0
    else:
        got, sc = m.generate_stream(px, max_length=LH, slots=6, num_beams=nb, return_scores=True, prefix_ids=lists)
        assert m.stream_beam_impl == "slot-refill"
        assert m.last_stream_pad_fallbacks == 0
        assert torch.equal(sc, want_sc)
    assert lib.kzv_test_force_prefix_calls() == before + 1               # the wave's one captured step holds the node
    assert torch.equal(_pad(got, cfg.pad_id), want)
    _starts_with_prefix(got, lists, cfg)
    assert m.last_stream_steps > 0


@pytest.mark.parametrize("nb", [1, 4])
def test_limits_with_prefixes_equal_generate_at_that_max_length(nb, decoder_dir):
    cfg, m, px, _ = _model(8, decoder_dir)
    m.set_decode_weights("bf16")
    lists = _ragged(cfg)
    choices = (8, 17, LH)                        # every limit leaves room behind the longest prefix: 1 + 5 <= 8 - 1
    limits = torch.tensor([choices[i % 3] for i in range(40)], dtype=torch.int32)
    kw = {} if nb == 1 else dict(num_beams=nb)
    got = _pad(m.generate_stream(px, max_length=LH, slots=6, limits=limits, prefix_ids=lists, **kw), cfg.pad_id)
    if nb > 1:
        assert m.last_stream_pad_fallbacks == 0
    for v in choices:
        idx = (limits == v).nonzero().reshape(-1)
        ref = m.generate(px[idx.cuda()], max_length=v, prefix_ids=[lists[i] for i in idx.tolist()], **kw)
        assert torch.equal(got[idx.cuda()], _pad(ref, cfg.pad_id)), v
    # a prefix that reaches the image's limit - 1 is refused before any wave runs
    with pytest.raises(ValueError, match="leave no room"):
        m.generate_stream(px, max_length=LH, slots=6, limits=torch.full((40,), 6, dtype=torch.int32), prefix_ids=lists, **kw)
    with pytest.raises(ValueError, match="leave no room"):
        m.generate(px[:1], max_length=6, prefix_ids=[[5, 6, 7, 8, 9]], **kw)


def test_nbest_rows_and_token_logprobs_with_a_prefix(decoder_dir):
    cfg, m, px, _ = _model(8, decoder_dir)
    m.set_decode_weights("bf16")
    lists = _ragged(cfg)
    kw = dict(max_length=LH, num_beams=4, num_return_sequences=2, return_scores=True, return_logprobs=True, prefix_ids=lists)
    ids, sc, lp = m.generate_stream(px, slots=6, **kw)
    assert m.last_stream_pad_fallbacks == 0
    rids, rsc, rlp = m.generate(px, **kw)
    W = max(ids.shape[1], rids.shape[1])
    assert torch.equal(_pad(ids, cfg.pad_id, W), _pad(rids, cfg.pad_id, W)) and torch.equal(sc, rsc)
    assert torch.equal(torch.nn.functional.pad(lp, (0, W - lp.shape[1])), torch.nn.functional.pad(rlp, (0, W - rlp.shape[1])))
    for i, p in enumerate(lists):
        for r in (2 * i, 2 * i + 1):
            assert ids[r, :1 + len(p)].tolist() == [cfg.bos_id] + p
            assert bool((lp[r, :1 + len(p)] == 0).all()) and float(lp[r, 1 + len(p)]) < 0      # forced columns: exactly 0
    # the score sums the generated tokens only, over the generated length
    n_tok = (ids != cfg.pad_id).sum(1)
    gen_len = (n_tok - 1 - torch.tensor([len(p) for p in lists], device=ids.device).repeat_interleave(2)).clamp(min=1)
    assert float((lp.double().sum(1) / gen_len.double() - sc.double()).abs().max()) <= 1e-5


def test_prefix_logprobs_are_the_models_own_opinion(decoder_dir):
    cfg, m, px, _ = _model(8, decoder_dir)
    m.set_decode_weights("bf16")
    lists = _ragged(cfg)
    ids, lp, pl = m.generate_stream(px, max_length=LH, slots=6, prefix_ids=lists, return_logprobs=True, return_prefix_logprobs=True)
    assert pl.shape == ids.shape
    # a teacher-forced pass over the same rows scores the same tokens (the bf16 step against the bf16 pass: a loose bound, the exact
    # statement is case 1's)
    sc = m.align(px, _pad(ids, cfg.pad_id))["logprob"]
    for i, p in enumerate(lists):
        n = len(p)
        assert bool((pl[i, 1:1 + n] < 0).all()) and bool((pl[i, 1 + n:] == 0).all()) and float(pl[i, 0]) == 0
        if n:
            assert float((pl[i, 1:1 + n] - sc[i, :n]).abs().max()) <= 0.05 * max(1.0, float(sc[i, :n].abs().max()))
    recs = m.recognize_many(px, slots=6, max_length=LH, prefix_ids=lists, prefix_logprobs=True)
    for r, p in zip(recs, lists):
        assert r["forced"] == len(p) and r["tokens"][:len(p)] == p and len(r["prefix_logprobs"]) == len(p)
        assert all(v == 0 for v in r["logprobs"][:len(p)])


# ---- 5. off is absent ----------------------------------------------------------------------------------------------------------------------
def test_no_prefix_launches_nothing_and_changes_nothing(decoder_dir):
    cfg, m, px, _ = _model(8, decoder_dir)
    m.set_decode_weights("bf16")
    lib = L.load()
    ids0, lp0 = m.generate_stream(px, max_length=LH, slots=6, return_logprobs=True)
    steps0 = m.last_stream_steps
    g0 = m.generate(px, max_length=LH)
    gsteps0 = m.last_generate_steps
    before = lib.kzv_test_force_prefix_calls()
    for empty in (None, [[] for _ in range(40)], torch.full((40, 3), cfg.pad_id)):
        ids1, lp1 = m.generate_stream(px, max_length=LH, slots=6, return_logprobs=True, prefix_ids=empty)
        assert torch.equal(ids0, ids1) and torch.equal(lp0, lp1) and m.last_stream_steps == steps0
        assert torch.equal(m.generate(px, max_length=LH, prefix_ids=empty), g0) and m.last_generate_steps == gsteps0
    b0, s0 = m.generate_stream(px, max_length=LH, slots=6, num_beams=4, return_scores=True)
    bsteps0 = m.last_stream_steps
    b1, s1 = m.generate_stream(px, max_length=LH, slots=6, num_beams=4, return_scores=True, prefix_ids=[[] for _ in range(40)])
    assert torch.equal(b0, b1) and torch.equal(s0, s1) and m.last_stream_steps == bsteps0
    l0, ls0 = m.generate(px, max_length=LH, num_beams=4, return_scores=True)
    l1, ls1 = m.generate(px, max_length=LH, num_beams=4, return_scores=True, prefix_ids=[[] for _ in range(40)])
    assert torch.equal(l0, l1) and torch.equal(ls0, ls1)
    assert lib.kzv_test_force_prefix_calls() == before
    m.generate_stream(px, max_length=LH, slots=6, prefix_ids=[[7]] + [[] for _ in range(39)])
    assert lib.kzv_test_force_prefix_calls() > before                    # the counter does see a prefix that is on
    # the handle refuses what the Python layer would have refused first (the last wave is still the handle's)
    h = m._h
    tab = torch.full((40, LH), 7, dtype=torch.int64, device=DEV)
    ln = torch.ones(40, dtype=torch.int32, device=DEV)
    assert lib.kzv_stream_set_prefix(h, tab.data_ptr(), 3, None, None, 0, _st()) == -1 and b"prefix_len" in lib.kzv_last_error()
    assert lib.kzv_stream_set_prefix(h, None, 3, ln.data_ptr(), None, 0, _st()) == -1
    assert lib.kzv_stream_set_prefix(h, tab.data_ptr(), LH - 1, ln.data_ptr(), None, 0, _st()) == -1 and b"max_len - 1" in lib.kzv_last_error()
    assert lib.kzv_stream_set_prefix(h, tab.data_ptr(), LH - 2, ln.data_ptr(), None, 0, _st()) == 0       # the longest that is served
    flp = torch.zeros(40, 3, device=DEV)
    assert lib.kzv_stream_set_prefix(h, tab.data_ptr(), 3, ln.data_ptr(), flp.data_ptr(), 3, _st()) == -1
    assert lib.kzv_stream_set_prefix(h, tab.data_ptr(), 0, None, None, 0, _st()) == 0                    # every prefix empty: off
    assert lib.kzv_stream_set_prefix(None, tab.data_ptr(), 3, ln.data_ptr(), None, 0, _st()) == -3       # outside a begun wave
    fresh = TrOCRModel(cfg.encoder_config_dict(), build_decoder_dir(decoder_dir + "/fresh", cfg), init_seed=7, load_tokenizer=False)
    assert lib.kzv_stream_set_prefix(fresh._h, tab.data_ptr(), 3, ln.data_ptr(), None, 0, _st()) == -3 and b"stream_set_prefix" in lib.kzv_last_error()
    torch.cuda.synchronize()
