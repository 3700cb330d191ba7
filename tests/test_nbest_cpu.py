"""N-best lists and per-token log-probabilities of the beam search (kzv/beam.py, kzv/stream.py, kzv/nbest.py; include/kzv.h:
kzv_stream_set_nbest and the appended fields of kzv_beam_state / kzv_stream_beam_state), the parts that need no GPU:

  1. the torch statement against transformers' own ``generate(num_return_sequences=n, output_scores=True)`` and
     ``compute_transition_scores`` on the small RobertaForCausalLM, seeds and 15 (seed, setting) cases of
     tests/test_host_cpu.py::test_beam_and_greedy_bookkeeping_equal_hf_generate, n in {2, num_beams}: sequences equal, sequence
     scores within 1e-5, per-token log-probabilities within ONE fp32 ulp of the largest accumulated score of the case.  The bound
     is derived, not observed: a token's value is fl(fl(a + lp) - a), a the parent's accumulated score; the sum is rounded once
     (<= half an ulp of the accumulated score) and the subtraction of two neighbours adds no larger error (its result is a
     multiple of the smaller operand's ulp and at most half an ulp of itself off).  The test asserts of its own inputs that every
     finished entry is done and that no ordering rests on a tie (smallest gap between adjacent finished scores > 0);
  2. the default return of beam_search is what it was: a tensor, equal to HF's ``sequences``;
  3. the slot statement (beam_stream) equals the lockstep statement per image, log-probability rows bit for bit, with limits too;
  4. the oracle CER keys on a hand-made 3 x 3 table against metrics.edit_stats_reference, a tie going to the lower rank;
  5. the refusals: n out of range, n > 1 with greedy, --test_n_best without stream-beam, --model ocr, and the ABI's argument errors
     before any launch."""
import ctypes as C
import os
import warnings
import zlib

import numpy as np
import pytest
import torch

from kzv import _lib as L
from kzv import beam as BM
from kzv import metrics as M
from kzv import nbest as NB
from kzv import stream as ST
from kzv.config import tiny_config

# ---- 1, 2. the statement against HF -----------------------------------------------------------------------------------------------------
SETTINGS = ((4, 16, True, 1.0), (4, 16, False, 1.0), (3, 7, True, 1.0), (2, 12, False, 2.0), (4, 12, True, 0.0))
SEEDS = ((0, 0.0), (1, 2.5), (2, 4.0))


@pytest.fixture(scope="module")
def hf_models():
    from transformers import RobertaConfig, RobertaForCausalLM
    warnings.filterwarnings("ignore")
    V, B, H = 41, 4, 32
    cfg = RobertaConfig(vocab_size=V, hidden_size=H, num_hidden_layers=2, num_attention_heads=2, intermediate_size=64,
                        max_position_embeddings=40, pad_token_id=1, bos_token_id=2, eos_token_id=3, is_decoder=True,
                        add_cross_attention=True, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    out = []
    for seed, eos_bias in SEEDS:
        torch.manual_seed(seed)
        m = RobertaForCausalLM(cfg).eval()
        with torch.no_grad():
            for p in m.parameters():
                p.mul_(3.0)
            m.lm_head.bias[3] += eos_bias
        out.append((m, torch.randn(B, 6, H) * 8))
    return V, B, out


def _make_step(m, enc, nb):
    e = enc.repeat_interleave(nb, 0)

    def step(t, ids):
        x = ids[:, :t + 1]
        with torch.no_grad():
            return m(input_ids=x, encoder_hidden_states=e, attention_mask=torch.ones_like(x),
                     position_ids=torch.arange(t + 1)[None].expand_as(x)).logits[:, -1]
    return step


def test_nbest_and_token_logprobs_equal_hf_generate(hf_models):
    V, B, models = hf_models
    cases, gap, worst_lp, worst_sc, worst_sum = 0, float("inf"), 0.0, 0.0, 0.0
    for m, enc in models:
        for nb, Lmax, es, lpen in SETTINGS:
            for n in sorted({2, nb}):
                with torch.no_grad():
                    h = m.generate(torch.full((B, 1), 2, dtype=torch.long), encoder_hidden_states=enc, max_length=Lmax, num_beams=nb,
                                   early_stopping=es, length_penalty=lpen, pad_token_id=1, eos_token_id=3, use_cache=False, do_sample=False,
                                   num_return_sequences=n, output_scores=True, return_dict_in_generate=True)
                    trans = m.compute_transition_scores(h.sequences, h.scores, h.beam_indices, normalize_logits=False)
                got = BM.beam_search(_make_step(m, enc, nb), lambda rows, t: None, B, nb, Lmax, V, 1, 2, 3, "cpu", early_stopping=es,
                                     length_penalty=lpen, num_return_sequences=n, return_logprobs=True)
                assert set(got) == {"ids", "scores", "lengths", "logprobs"}
                assert got["ids"].shape == h.sequences.shape and torch.equal(got["ids"], h.sequences), (nb, Lmax, es, lpen, n)
                sc_err = float((got["scores"] - h.sequences_scores).abs().max())
                assert sc_err <= 1e-5, (nb, Lmax, es, lpen, n, sc_err)
                # lengths: BOS included, the row's tokens up to its last one that is no padding
                W = got["ids"].shape[1]
                want_len = W - (got["ids"].flip(1) != 1).int().argmax(dim=1)
                assert torch.equal(got["lengths"], want_len)
                assert int(got["lengths"].min()) >= 2                                   # every returned finished entry is done
                # column t of logprobs scores the token in column t; HF's column t - 1 does; 0 in column 0 and from the length on
                lp = got["logprobs"]
                assert lp.dtype == torch.float32 and lp.shape == got["ids"].shape
                col = torch.arange(W).view(1, W)
                dead = (col == 0) | (col >= got["lengths"].view(-1, 1))
                assert bool((lp[dead] == 0).all())
                k = min(W - 1, trans.shape[1])
                assert k == W - 1 and bool((trans[:, k:] == 0).all())
                acc = float(trans.double().cumsum(1).abs().max())                         # the largest accumulated score of the case
                tol = float(np.spacing(np.float32(acc)))
                err = float((lp[:, 1:] - trans[:, :k]).abs().max())
                assert err <= tol, (nb, Lmax, es, lpen, n, err, tol)
                # the sum over the row / generated length ** length_penalty is the hypothesis score
                gen_len = (got["lengths"] - 1).double()
                s_err = float((lp.double().sum(1) / gen_len.pow(lpen) - got["scores"].double()).abs().max())
                worst_lp, worst_sc, worst_sum = max(worst_lp, err), max(worst_sc, sc_err), max(worst_sum, s_err)
                if n == nb:                                                             # the whole finished list: done, and no tie decides an order
                    sc = got["scores"].view(B, nb)
                    gap = min(gap, float((sc[:, :-1] - sc[:, 1:]).min()))
                cases += 1
    print(f"{cases} cases: log-probabilities within {worst_lp:.2e} of compute_transition_scores, scores within {worst_sc:.2e}, "
          f"sum / length ** penalty within {worst_sum:.2e} of the score; smallest gap between adjacent finished scores {gap:.2e}")
    assert cases == 27                       # 15 (seed, setting) cases, n = 2 and n = num_beams (the 2-beam setting has one n)
    assert gap > 0
    assert worst_sum <= 1e-5


def test_default_return_is_unchanged(hf_models):
    V, B, models = hf_models
    m, enc = models[1]
    for nb, Lmax, es, lpen in SETTINGS[:3]:
        with torch.no_grad():
            h = m.generate(torch.full((B, 1), 2, dtype=torch.long), encoder_hidden_states=enc, max_length=Lmax, num_beams=nb, early_stopping=es,
                           length_penalty=lpen, pad_token_id=1, eos_token_id=3, use_cache=False, do_sample=False, return_dict_in_generate=True).sequences
        plain = BM.beam_search(_make_step(m, enc, nb), lambda rows, t: None, B, nb, Lmax, V, 1, 2, 3, "cpu", early_stopping=es, length_penalty=lpen)
        stated = BM.beam_search(_make_step(m, enc, nb), lambda rows, t: None, B, nb, Lmax, V, 1, 2, 3, "cpu", early_stopping=es, length_penalty=lpen,
                                num_return_sequences=1, return_logprobs=False)
        assert type(plain) is torch.Tensor and type(stated) is torch.Tensor
        assert plain.dtype == torch.int64 and torch.equal(plain, h) and torch.equal(stated, h)
        # the winner is row 0 of every image's n-best list
        best = BM.beam_search(_make_step(m, enc, nb), lambda rows, t: None, B, nb, Lmax, V, 1, 2, 3, "cpu", early_stopping=es, length_penalty=lpen,
                              num_return_sequences=nb)
        assert set(best) == {"ids", "scores", "lengths"}
        assert torch.equal(best["ids"][0::nb][:, :plain.shape[1]], plain) and bool((best["ids"][0::nb][:, plain.shape[1]:] == 1).all())


# ---- 3. slot statement == lockstep statement ----------------------------------------------------------------------------------------------
PAD, BOS, EOS, V11, LMAX, N = 1, 2, 3, 11, 14, 23
GRID = [(nb, early, lp) for nb in (2, 4) for early in (True, False) for lp in (1.0, 0.6)]


def _logits(image: int, prefix) -> torch.Tensor:
    """[V] logits of (image, prefix): the fake decoder of tests/test_stream_beam_cpu.py, seed for seed."""
    g = torch.Generator().manual_seed(zlib.crc32(repr((int(image), [int(x) for x in prefix])).encode()))
    x = torch.randn(V11, generator=g)
    x[PAD] = -10.0
    return x


def _step_fn(nb):
    def step(st):
        slots = st["slot_image"].numel()
        out = torch.zeros(slots * nb, V11)
        for s, (i, t) in enumerate(zip(st["slot_image"].tolist(), st["slot_t"].tolist())):
            if i >= 0:
                for k in range(nb):
                    out[s * nb + k] = _logits(i, st["run_seq"][s, k, :t + 1])
        return out
    return step


def _topk(nb):
    def topk(raw, run_sc):
        acc = torch.log_softmax(raw.float(), dim=-1).view(-1, nb, V11) + run_sc.unsqueeze(-1)
        return acc.view(-1, nb * V11).topk(2 * nb, dim=1)
    return topk


_ALONE = {}


def _alone(image, nb, early, lp, n, max_len=LMAX):
    key = (image, nb, early, lp, n, max_len)
    if key not in _ALONE:
        step = lambda t, ids: torch.stack([_logits(image, ids[r, :t + 1]) for r in range(nb)])      # noqa: E731
        _ALONE[key] = BM.beam_search(step, lambda rows, t: None, 1, nb, max_len, V11, PAD, BOS, EOS, "cpu", early_stopping=early, length_penalty=lp,
                                     topk=_topk(nb), num_return_sequences=n, return_logprobs=True)
    return _ALONE[key]


def _wide(x, fill):
    out = torch.full((x.shape[0], LMAX), fill, dtype=x.dtype)
    out[:, :x.shape[1]] = x
    return out


def _check_against_alone(got, nb, early, lp, n, n_images, limits=None):
    assert got["ids"].shape[0] == n_images * n and got["ids"].shape[1] == max(2, int(got["lengths"].max()))
    ids, lps = _wide(got["ids"], PAD), _wide(got["logprobs"], 0.0)
    for i in range(n_images):
        want = _alone(i, nb, early, lp, n, LMAX if limits is None else int(limits[i]))
        rows = slice(i * n, (i + 1) * n)
        assert torch.equal(ids[rows], _wide(want["ids"], PAD)), i
        assert torch.equal(got["scores"][rows], want["scores"]), i                        # bit for bit: the same divisions
        assert torch.equal(got["lengths"][rows], want["lengths"]), i
        assert torch.equal(lps[rows], _wide(want["logprobs"], 0.0)), i                    # bit for bit: the same subtraction
    assert int(got["lengths"].min()) >= 2


@pytest.mark.parametrize("nb,early,lp", GRID)
def test_slot_statement_equals_lockstep_statement(nb, early, lp):
    n = nb if early else 2
    got, st = ST.beam_stream(_step_fn(nb), N, 4, nb, LMAX, V11, PAD, BOS, EOS, "cpu", early_stopping=early, length_penalty=lp, topk=_topk(nb),
                             return_state=True, num_return_sequences=n, return_logprobs=True)
    _check_against_alone(got, nb, early, lp, n, N)
    # row 0 is what out_ids / out_score get, which keep being written
    assert torch.equal(st["out_ids"], _wide(got["ids"], PAD)[0::n]) and torch.equal(st["out_score"], got["scores"][0::n])
    assert st["counters"].tolist()[:2] == [N, N]
    # without the keywords: the pair it returned before, and no new key in the state
    (out, score), st0 = ST.beam_stream(_step_fn(nb), N, 4, nb, LMAX, V11, PAD, BOS, EOS, "cpu", early_stopping=early, length_penalty=lp,
                                       topk=_topk(nb), return_state=True)
    assert torch.equal(out, st["out_ids"]) and torch.equal(score, st["out_score"])
    assert not any(k in st0 for k in ("run_lp", "fin_lp", "nbest_ids", "nbest_score", "nbest_len", "nbest_logprob"))
    for k in st0:
        if st0[k] is not None:
            assert torch.equal(st0[k], st[k]), k


def test_slot_statement_with_limits_and_without_logprobs():
    nb, n = 4, 3
    g = torch.Generator().manual_seed(5)
    limits = torch.randint(2, LMAX + 1, (N,), generator=g)
    limits[0], limits[1] = 2, LMAX
    got = ST.beam_stream(_step_fn(nb), N, 4, nb, LMAX, V11, PAD, BOS, EOS, "cpu", limits=limits, topk=_topk(nb), num_return_sequences=n,
                         return_logprobs=True)
    _check_against_alone(got, nb, True, 1.0, n, N, limits)
    assert int(got["lengths"].max()) <= LMAX and bool((got["lengths"].view(N, n) <= limits.view(N, 1)).all())
    plain = ST.beam_stream(_step_fn(nb), N, 4, nb, LMAX, V11, PAD, BOS, EOS, "cpu", limits=limits, topk=_topk(nb), num_return_sequences=n)
    assert set(plain) == {"ids", "scores", "lengths"}
    assert torch.equal(plain["ids"], got["ids"]) and torch.equal(plain["scores"], got["scores"]) and torch.equal(plain["lengths"], got["lengths"])


# ---- 4. the oracle keys ------------------------------------------------------------------------------------------------------------------
def test_oracle_keys_on_a_hand_made_table():
    special, vocab = [PAD, BOS, EOS], 20
    row = lambda *t: [BOS] + list(t) + [EOS] + [PAD] * (6 - len(t))                               # noqa: E731
    labels = torch.tensor([row(5, 6, 7, 8), row(9, 10), row(11, 12, 13)])
    hyps = torch.tensor([
        row(5, 6, 7, 9), row(5, 6, 7, 8), row(5, 6),                   # line 0: the 2nd reading is exact (distances 1, 0, 2)
        row(9, 11), row(10, 10), row(9, 10, 10),                       # line 1: distances 1, 1, 1 -- a three-way tie: rank 0
        row(4, 4, 4, 4), row(11, 12), row(11, 13),                     # line 2: distances 4, 1, 1 -- ranks 1 and 2 tie: rank 1
    ])
    n = 3
    ref = M.edit_stats_reference(hyps, labels.repeat_interleave(n, dim=0), special, vocab, ops=False)
    dist, ref_len, pred_len = (ref[k].reshape(3, n) for k in ("dist", "ref_len", "pred_len"))
    assert dist.tolist() == [[1, 0, 2], [1, 1, 1], [4, 1, 1]] and ref_len[:, 0].tolist() == [4, 2, 3]
    o = NB.oracle_stats(dist, ref_len[:, 0], pred_len)
    assert o["oracle_rank"] == [1, 2, 0]
    assert o["cer_oracle_lines"] == [0.0, 1 / 2, 1 / 3]
    assert o["cer_oracle"] == (0.0 + 1 / 2 + 1 / 3) / 3
    assert o["cer_oracle_corpus"] == (0 + 1 + 1) / 9
    assert np.array_equal(o["dist_nbest"], dist)
    # the winner's own CER is never better than the oracle's
    win = M.cer_values(dist[:, 0], ref_len[:, 0], pred_len[:, 0])
    assert o["cer_oracle"] <= sum(win) / 3 and all(a <= b for a, b in zip(o["cer_oracle_lines"], win))
    # one hypothesis per line: the oracle is the winner
    o1 = NB.oracle_stats(dist[:, :1], ref_len[:, 0], pred_len[:, :1])
    assert o1["oracle_rank"] == [3] and o1["cer_oracle"] == sum(win) / 3
    # an empty label: CER 1.0 for a non-empty reading, 0.0 for an empty one (calculate_cer's rule) -- the empty reading wins
    o2 = NB.oracle_stats(np.array([[2, 0]]), np.array([0]), np.array([[2, 0]]))
    assert o2["oracle_rank"] == [0, 1] and o2["cer_oracle"] == 0.0 and o2["cer_oracle_corpus"] == 0.0
    with pytest.raises(ValueError):
        NB.oracle_stats(dist, ref_len[:2, 0], pred_len)


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_requests_out_of_range_are_refused():
    assert NB.check_request(4, 1) == 1 and NB.check_request(4, 4, True) == 4 and NB.check_request(1, 1) == 1
    for nb, n in ((4, 0), (4, 5), (2, 3), (4, -1)):
        with pytest.raises(ValueError, match="1..num_beams"):
            NB.check_request(nb, n)
    with pytest.raises(ValueError, match="needs a beam search"):
        NB.check_request(1, 2)                                                     # n > 1 with greedy
    step = lambda t, ids: torch.zeros(ids.shape[0], V11)                             # noqa: E731
    for n in (0, 3):
        with pytest.raises(ValueError):
            BM.beam_search(step, lambda rows, t: None, 1, 2, 6, V11, PAD, BOS, EOS, "cpu", num_return_sequences=n)
        with pytest.raises(ValueError):
            BM.beam_search_fused(step, lambda rows, t: None, 1, 2, 6, V11, PAD, BOS, EOS, "cpu", True, 1.0, None, None, num_return_sequences=n)
        with pytest.raises(ValueError):
            ST.beam_stream(_step_fn(2), 3, 2, 2, 6, V11, PAD, BOS, EOS, "cpu", num_return_sequences=n)
    with pytest.raises(ValueError):
        ST.new_beam_state(3, 2, 2, 6, PAD, BOS, "cpu", n_best=3)
    with pytest.raises(ValueError):
        ST.new_beam_state(3, 2, 2, 6, PAD, BOS, "cpu", want_logprobs=True)
    with pytest.raises(RuntimeError, match="never received"):
        NB.check_done(torch.tensor([3, 0, 2]))


def test_cli_flag_and_trainer_refusals(capsys):
    from kzv import trainer
    from kzv.train import parse_args
    assert parse_args([]).test_n_best == 0
    assert parse_args(["--test_decode", "stream-beam", "--test_n_best", "4"]).test_n_best == 4
    for argv in (["--test_n_best", "2"], ["--test_decode", "stream", "--test_n_best", "2"], ["--test_decode", "stream-beam", "--test_n_best", "5"],
                 ["--model", "ocr", "--test_decode", "stream-beam", "--test_n_best", "2"], ["--test_decode", "stream-beam", "--test_n_best", "-1"]):
        with pytest.raises(SystemExit):
            parse_args(argv)
        assert "--test_n_best" in capsys.readouterr().err
    for mode in (False, True):
        with pytest.raises(ValueError, match="stream-beam"):
            trainer.test(None, [], n_best=2, stream_decode=mode)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load()


def test_abi_refuses_bad_arguments_without_a_launch(lib):
    out = 4096                                                   # never dereferenced: only its presence is checked
    assert [f[0] for f in L.kzv_stream_beam_state._fields_][9] == "n_best"
    assert [f[0] for f in L.kzv_stream_beam_state._fields_][-8:] == ["run_lp", "fin_lp", "nbest_ids", "ld_nbest", "nbest_scores", "nbest_len",
                                                                      "nbest_logprob", "ld_nbest_logprob"]
    assert [f[0] for f in L.kzv_beam_state._fields_][-4:] == ["run_lp_in", "run_lp_out", "fin_lp_in", "fin_lp_out"]
    base = dict(slots=4, n_images=8, num_beams=4, max_len=16, vocab=V11, bos_id=BOS, eos_id=EOS, pad_id=PAD, early_stopping=1,
                slot_image=out, slot_t=out, tokens=out, posids=out, run_seq=out, fin_seq=out, run_scores=out, fin_scores=out,
                fin_done=out, fin_len=out, unsatisfied=out, counters=out, scratch=out, out_ids=out, ld_ids=16, divisors=out)
    nbest = dict(n_best=4, nbest_ids=out, ld_nbest=16, nbest_scores=out, nbest_len=out)
    bad = [dict(nbest, n_best=5), dict(nbest, n_best=-1), dict(nbest, nbest_ids=None), dict(nbest, nbest_scores=None), dict(nbest, nbest_len=None),
           dict(nbest, ld_nbest=15), dict(nbest, run_lp=out), dict(nbest, fin_lp=out), dict(nbest, nbest_logprob=out, ld_nbest_logprob=16),
           dict(nbest, run_lp=out, fin_lp=out, nbest_logprob=out, ld_nbest_logprob=15), dict(nbest, n_best=0), dict(run_lp=out, fin_lp=out)]
    for extra in bad:
        st = L.kzv_stream_beam_state(**base, **extra)
        assert lib.kzv_stream_beam_update(C.byref(st), out, out, None) == -1, extra
        assert lib.kzv_stream_beam_seat_first(C.byref(st), None) == -1, extra
    # the lockstep update: the four log-probability row arrays come together, in != out
    bs = dict(batch=2, num_beams=4, max_len=16, vocab=V11, eos_id=EOS, run_seq_in=out, run_seq_out=out + 8, fin_seq_in=out, fin_seq_out=out + 8,
              run_scores=out, fin_scores=out, fin_done=out, fin_len=out, unsatisfied=out)
    for extra in (dict(run_lp_in=out), dict(run_lp_in=out, run_lp_out=out + 8, fin_lp_in=out), dict(run_lp_in=out, run_lp_out=out, fin_lp_in=out, fin_lp_out=out + 8)):
        st = L.kzv_beam_state(**bs, **extra)
        assert lib.kzv_beam_update(C.byref(st), out, out, 1, 1, 1.0, out, out, None) == -1 and b"log-probability" in lib.kzv_last_error(), extra
    # the handle entry: a state error before a wave has begun
    cfg = tiny_config()
    c = L.kzv_config(image_h=cfg.image_h, image_w=cfg.image_w, patch_h=cfg.patch_h, patch_w=cfg.patch_w, channels=cfg.channels,
                     enc_hidden=cfg.enc_hidden, enc_layers=cfg.enc_layers, enc_heads=cfg.enc_heads, enc_ffn=cfg.enc_ffn,
                     dec_hidden=cfg.dec_hidden, dec_layers=cfg.dec_layers, dec_heads=cfg.dec_heads, dec_ffn=cfg.dec_ffn,
                     vocab=cfg.vocab, max_pos=cfg.max_pos, type_vocab=cfg.type_vocab, pad_id=cfg.pad_id, ln_eps=1e-12)
    h = C.c_void_p()
    L.check(lib.kzv_model_create(C.byref(c), C.byref(h)), "create")
    try:
        assert lib.kzv_stream_set_nbest(h, 4, out, 16, out, out, None, 0, None) == -3 and b"stream_set_nbest" in lib.kzv_last_error()
        assert lib.kzv_stream_set_nbest(None, 4, out, 16, out, out, None, 0, None) == -3
    finally:
        lib.kzv_model_destroy(h)
