"""N-best lists and per-token log-probabilities of the device beam search on the GPU (csrc/token_search.hip: the LP instance of
beam_update_kernel, the NBEST / LP instances of stream_beam_update_kernel; include/kzv.h: kzv_stream_set_nbest; kzv/nbest.py):

  6. the two bookkeeping kernels with the new fields against their torch statement: the slot kernel state for state over 50 steps on
     random rankings with limits and reseated slots (token rows and lengths equal, scores and log-probability rows bit for bit), in
     all three instances at once -- with log-probabilities, n-best only, and the fields null, whose every output must equal the
     statement's too; the lockstep kernel through beam_search_fused against beam_search's torch bookkeeping on the same device ranking;
  7. generate_stream(num_beams=nb, num_return_sequences=nb, return_logprobs=True, return_scores=True) == generate(...) with the same
     keywords on the model of tests/test_stream_beam_gpu.py (8 and 164 patch keys, bf16 and e4m3 weights, 2 and 4 beams, 29 crops on 6
     slots): ids equal, scores and log-probabilities within LP_TOL (that file's bound for ONE log-probability: a score is a mean of
     them); rows 0::n equal generate_stream(num_beams=nb); one case under no_repeat_ngram_size=3, one that takes the padding fallback;
  8. the log-probabilities are the model's: per hypothesis within LP_TOL of align's teacher-forced values on the live columns, and their
     sum / length ** length_penalty equals the returned score within generated_length ulps of the sum (each difference of two
     accumulated scores is off by at most half an ulp of the larger one);
  9. records and oracle on the fitted fixture."""
import ctypes as C

import numpy as np
import pytest
import torch

from kzv import _lib as L
from kzv import beam as BM
from kzv import stream as ST
from kzv.data import build_decoder_dir
from kzv.model import TrOCRModel

import test_stream_beam_gpu as SB
from _trained import load as load_trained

pytestmark = pytest.mark.gpu
LH, LP_TOL, N_IMG, SLOTS = SB.LH, SB.LP_TOL, 29, 6


@pytest.fixture(autouse=True)
def _default_mode_afterwards():
    yield
    L.load().kzv_set_decode_one_launch(-1)


@pytest.fixture(scope="module")
def decoder_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("dec_nbest"))


# ---- 6. the kernels against the statement ------------------------------------------------------------------------------------------------
def _beam_state_struct(dev, scratch, slots, N, nb, ML, V, bos, eos, pad, early, lim_d, div_d, n_best):
    extra = {}
    if n_best:
        extra = dict(n_best=n_best, nbest_ids=dev["nbest_ids"].data_ptr(), ld_nbest=ML, nbest_scores=dev["nbest_score"].data_ptr(),
                     nbest_len=dev["nbest_len"].data_ptr())
        if "run_lp" in dev:
            extra.update(run_lp=dev["run_lp"].data_ptr(), fin_lp=dev["fin_lp"].data_ptr(), nbest_logprob=dev["nbest_logprob"].data_ptr(),
                         ld_nbest_logprob=ML)
    return L.kzv_stream_beam_state(slots=slots, n_images=N, num_beams=nb, max_len=ML, vocab=V, bos_id=bos, eos_id=eos, pad_id=pad, early_stopping=int(early),
                                   slot_image=dev["slot_image"].data_ptr(), slot_t=dev["slot_t"].data_ptr(), tokens=dev["tokens"].data_ptr(),
                                   posids=dev["posids"].data_ptr(), run_seq=dev["run_seq"].data_ptr(), fin_seq=dev["fin_seq"].data_ptr(),
                                   run_scores=dev["run_sc"].data_ptr(), fin_scores=dev["fin_sc"].data_ptr(), fin_done=dev["fin_done"].data_ptr(),
                                   fin_len=dev["fin_len"].data_ptr(), unsatisfied=dev["unsat"].data_ptr(), counters=dev["counters"].data_ptr(),
                                   scratch=scratch.data_ptr(), out_ids=dev["out_ids"].data_ptr(), ld_ids=ML, out_score=dev["out_score"].data_ptr(),
                                   limit=lim_d.data_ptr(), divisors=div_d.data_ptr(), rows=dev["rowtab"].data_ptr(), ld_rows=ML, **extra)


@pytest.mark.parametrize("nb,early,lpen,n", [(2, True, 1.0, 2), (4, True, 1.0, 4), (4, False, 0.6, 2), (4, True, 1.0, 1)])
def test_slot_update_kernel_equals_the_torch_statement(nb, early, lpen, n):
    """tests/test_stream_beam_gpu.py::test_update_and_seat_kernels_equal_the_torch_statement's drive (7 slots, 30 images: every slot
    is reseated several times; a limit per image), three device states side by side on the same logits: "lp" (n-best with
    log-probabilities), "nbest" (n-best only) and "off" (the new fields null).  Each is compared with the statement state for state."""
    lib = L.load()
    slots, N, V, ML, pad, bos, eos = 7, 30, 157, 12, 1, 2, 3
    K, R = 2 * nb, slots * nb
    g = torch.Generator().manual_seed(29 + nb + n)
    limits = torch.randint(2, ML + 1, (N,), generator=g, dtype=torch.int32)
    lim_d, div = limits.cuda(), ST.divisor_table(ML, lpen)
    div_d = div.cuda()
    ref = ST.new_beam_state(N, slots, nb, ML, pad, bos, "cpu", rowtab_ld=ML, n_best=n, want_logprobs=True)
    ref["rowtab"] = torch.randint(0, R, (R, ML), generator=g, dtype=torch.int32)
    lp_keys, nbest_keys = ("run_lp", "fin_lp", "nbest_logprob"), ("nbest_ids", "nbest_score", "nbest_len")
    base_keys = [k for k in ref if k not in lp_keys + nbest_keys]
    variants = {"lp": base_keys + list(lp_keys + nbest_keys), "nbest": base_keys + list(nbest_keys), "off": base_keys}
    devs, structs, keepalive = {}, {}, []
    for name, keys in variants.items():
        dev = {k: torch.randint(0, 3, ref[k].shape, generator=g).to(ref[k].dtype).cuda() for k in keys}     # seat_first must not rely on clean memory
        for k in ("out_ids", "rowtab") + tuple(k for k in nbest_keys + ("nbest_logprob",) if k in dev):      # what the caller fills
            dev[k].copy_(ref[k])
        dev["out_score"].zero_()
        scratch = torch.zeros(2 * slots, dtype=torch.int32, device="cuda")
        keepalive.append(scratch)
        devs[name] = dev
        structs[name] = _beam_state_struct(dev, scratch, slots, N, nb, ML, V, bos, eos, pad, early, lim_d, div_d, 0 if name == "off" else n)
        L.check(lib.kzv_stream_beam_seat_first(C.byref(structs[name]), L.stream_handle()), "beam_seat_first")
        for k in keys:
            assert torch.equal(dev[k].cpu(), ref[k]), ("start", name, k)
    top_lp = torch.empty(slots, K, dtype=torch.float32, device="cuda")
    top_ix = torch.empty(slots, K, dtype=torch.int64, device="cuda")
    rows = torch.arange(R)
    ended_with_rows = 0
    for step in range(50):
        x = torch.randn(R, V, generator=g)
        x[:, pad] = -20.0
        for b in range(R):
            r = int(torch.randint(0, 8, (1,), generator=g))
            if r == 0:                                      # exact ties of the maximum: the smaller flat index ranks first
                cols = torch.randperm(V - 4, generator=g)[:3] + 4
                x[b, cols] = x[b].max() + 1.0
            elif r == 1:                                    # EOS as the maximum, tied with a later column
                x[b, eos] = x[b, 100] = x[b].max() + 0.5
        if step % 9 == 4:                                   # every live search ends in this step
            x[:, eos] = 50.0
        live = (ref["slot_image"] >= 0).repeat_interleave(nb)
        at = ref["slot_t"].repeat_interleave(nb).long()
        ref["rowtab"][rows[live], at[live]] = rows[live].to(torch.int32)
        xd = x.cuda()
        for name, dev in devs.items():
            dev["rowtab"][rows[live].cuda(), at[live].cuda()] = rows[live].to(torch.int32).cuda()
            L.check(lib.kzv_beam_topk(xd.data_ptr(), V, dev["run_sc"].data_ptr(), slots, nb, V, K, top_lp.data_ptr(), top_ix.data_ptr(), L.stream_handle()), "beam_topk")
            L.check(lib.kzv_stream_beam_update(C.byref(structs[name]), top_lp.data_ptr(), top_ix.data_ptr(), L.stream_handle()), "stream_beam_update")
            if name == "lp":
                lp_cpu, ix_cpu = top_lp.cpu(), top_ix.cpu()
        before = int(ref["counters"][1])
        ref = ST.beam_select_seat(lp_cpu, ix_cpu, ref, n_images=N, num_beams=nb, max_len=ML, vocab=V, pad_id=pad, bos_id=bos, eos_id=eos,
                                  early_stopping=early, length_penalty=lpen, limit=limits, divisors=div)
        ended_with_rows += int(ref["counters"][1]) - before
        for name, keys in variants.items():
            for k in keys:                                  # integers equal; fp32 scores and log-probability rows bit for bit (torch.equal)
                assert torch.equal(devs[name][k].cpu(), ref[k]), (step, name, k, devs[name][k].cpu(), ref[k])
    c = ref["counters"].tolist()
    assert c[:2] == [N, N] and ended_with_rows == N and (ref["slot_image"] == -1).all()
    # the outputs mean something: every row done, row 0 is out_ids / out_score, log-probabilities sum to the score
    ln = ref["nbest_len"].view(N, n)
    assert int(ln[:, 0].min()) >= 2
    assert torch.equal(ref["nbest_ids"].view(N, n, ML)[:, 0], ref["out_ids"]) and torch.equal(ref["nbest_score"].view(N, n)[:, 0], ref["out_score"])
    done = ln > 0
    sums = ref["nbest_logprob"].double().sum(1).view(N, n)
    want = ref["nbest_score"].view(N, n).double() * div.double()[(ln - 1).clamp(min=0).long()]
    assert float((sums - want)[done].abs().max()) <= 1e-4
    print(f"{nb} beams, n = {n}: {c[2]} steps for {N} searches on {slots} slots; {int(done.sum())} of {N * n} rows done")


def _synthetic_step(V, T, seed, eos_bias):
    g = torch.Generator().manual_seed(seed)
    W = (torch.randn(T, V, V, generator=g) * 2.0).cuda()
    W[:, :, 2] += eos_bias
    W[:, :, 1] = -30.0
    W[:, :, 0] = -30.0
    return lambda t, ids: W[t][ids[:, t].cuda()].contiguous()


@pytest.mark.parametrize("B,nb,V,T,eos_bias,early,lp", [(7, 4, 157, 14, 1.5, True, 1.0), (5, 4, 41, 12, 3.0, False, 1.0), (9, 3, 300, 10, 2.0, True, 0.75),
                                                        (4, 2, 64, 20, 0.5, False, 1.25), (3, 8, 97, 9, 2.5, True, 1.0)])
def test_lockstep_update_kernel_equals_the_torch_statement(B, nb, V, T, eos_bias, early, lp):
    """tests/test_beam_gpu.py's synthetic step functions (PAD 1, BOS 0, EOS 2).  Both sides rank with kzv_beam_topk; the bookkeeping is
    beam_search's torch statement on one side and kzv_beam_update with the log-probability rows on the other.  The statement's
    bookkeeping runs on CPU tensors, where it is pinned against HF: torch divides a CUDA tensor by a Python scalar as a multiplication
    by its reciprocal, which is not the kernel's (nor the CPU's) division.  The length penalties are values fp32 holds exactly: kzv_beam_update
    takes the penalty as a C float, the statement as a Python double, and a value like 1.3 gives the two different divisors."""
    PAD, BOS, EOS = 1, 0, 2
    nothing = lambda rows, t: None                              # noqa: E731
    topk, update = BM.make_device_hooks(B, nb, T, V, EOS, early, lp, "cuda")

    def topk_cpu(raw, run_sc):
        top_lp, top_ix = topk(raw, run_sc.cuda())
        return top_lp.cpu(), top_ix.cpu()

    for n in sorted({2, nb}):
        want = BM.beam_search(_synthetic_step(V, T, B + V, eos_bias), nothing, B, nb, T, V, PAD, BOS, EOS, "cpu", early_stopping=early, length_penalty=lp,
                              topk=topk_cpu, num_return_sequences=n, return_logprobs=True)
        got, st = BM.beam_search_fused(_synthetic_step(V, T, B + V, eos_bias), nothing, B, nb, T, V, PAD, BOS, EOS, "cuda", early, lp, topk, update,
                                       return_state=True, num_return_sequences=n, return_logprobs=True)
        torch.cuda.synchronize()
        assert set(got) == {"ids", "scores", "lengths", "logprobs"} and "run_lp" in st
        for k in ("ids", "lengths", "scores", "logprobs"):      # scores and log-probabilities bit for bit
            assert torch.equal(got[k].cpu(), want[k]), (n, k, got[k].cpu(), want[k])
        assert int(got["lengths"].min()) >= 2
        # n-best without log-probabilities: the plain instance of the kernel, the same rows
        plain_n, st_n = BM.beam_search_fused(_synthetic_step(V, T, B + V, eos_bias), nothing, B, nb, T, V, PAD, BOS, EOS, "cuda", early, lp, topk, update,
                                             return_state=True, num_return_sequences=n)
        assert set(plain_n) == {"ids", "scores", "lengths"} and "run_lp" not in st_n
        for k in plain_n:
            assert torch.equal(plain_n[k].cpu(), want[k]), (n, k)
    # with the new fields null every existing output equals the call with them
    plain, st0 = BM.beam_search_fused(_synthetic_step(V, T, B + V, eos_bias), nothing, B, nb, T, V, PAD, BOS, EOS, "cuda", early, lp, topk, update, return_state=True)
    torch.cuda.synchronize()
    assert type(plain) is torch.Tensor
    w = plain.shape[1]
    first = got["ids"][0::n]
    assert torch.equal(first[:, :w], plain) and bool((first[:, w:] == PAD).all())
    for k in ("run_sc", "fin_sc", "fin_done", "fin_len", "unsat"):
        assert torch.equal(st0[k], st[k]), k
    assert torch.equal(st0["fin_seq"][st0["cur_buf"]], st["fin_seq"][st["cur_buf"]]) and torch.equal(st0["run_seq"][st0["cur_buf"]], st["run_seq"][st["cur_buf"]])


# ---- 7, 8. on the model ----------------------------------------------------------------------------------------------------------------------
_runs = {}


def _pad(x, fill, width=LH):
    out = torch.full((x.shape[0], width), fill, dtype=x.dtype, device=x.device)
    out[:, :x.shape[1]] = x
    return out


def _both(keys, fmt, nb, decoder_dir, **kw):
    """(cfg, m, px, stream results, lockstep results) of the 29 crops, n = nb, computed once per case."""
    key = (keys, fmt, nb, tuple(sorted(kw.items())))
    cfg, m, px, _ = SB._model(keys, decoder_dir)
    px = px[:N_IMG]
    m.set_decode_weights(fmt)
    if key not in _runs:
        stream = m.generate_stream(px, max_length=LH, slots=SLOTS, num_beams=nb, num_return_sequences=nb, return_logprobs=True, return_scores=True, **kw)
        info = (m.stream_beam_impl_for(nb), m.last_stream_pad_fallbacks, m.last_stream_steps)
        lock = m.generate(px, max_length=LH, num_beams=nb, num_return_sequences=nb, return_logprobs=True, return_scores=True, **kw)
        _runs[key] = (stream, lock, info)
    return (cfg, m, px) + _runs[key]


def _assert_same_rows(cfg, nb, stream, lock):
    (s_ids, s_sc, s_lp), (l_ids, l_sc, l_lp) = stream, lock
    assert s_ids.shape == (N_IMG * nb, s_lp.shape[1]) and s_sc.shape == (N_IMG * nb,) and s_lp.dtype == torch.float32
    assert s_ids.shape == l_ids.shape and torch.equal(s_ids, l_ids)
    sc_err, lp_err = float((s_sc - l_sc).abs().max()), float((s_lp - l_lp).abs().max())
    print(f"stream against lockstep over {N_IMG * nb} hypotheses: scores within {sc_err:.3e}, per-token log-probabilities within {lp_err:.3e}")
    assert sc_err <= LP_TOL and lp_err <= LP_TOL
    # best first; column 0 and the columns from a row's length on hold 0
    assert bool((s_sc.view(N_IMG, nb)[:, :-1] >= s_sc.view(N_IMG, nb)[:, 1:]).all())
    length = s_ids.shape[1] - (s_ids.flip(1) != cfg.pad_id).int().argmax(dim=1)
    col = torch.arange(s_ids.shape[1], device=s_ids.device).view(1, -1)
    for lp in (s_lp, l_lp):
        assert bool((lp[(col == 0) | (col >= length.view(-1, 1))] == 0).all())


@pytest.mark.parametrize("keys,fmt,nb", [(8, "bf16", 4), (8, "e4m3", 2), (164, "bf16", 2), (164, "e4m3", 4)])
def test_stream_nbest_equals_lockstep_nbest(decoder_dir, keys, fmt, nb):
    cfg, m, px, stream, lock, info = _both(keys, fmt, nb, decoder_dir)
    assert info[0] == "slot-refill" and info[1] == 0 and 0 < info[2] <= ST.step_bound(N_IMG, SLOTS, LH)
    _assert_same_rows(cfg, nb, stream, lock)
    # rows 0::n are what the call without the keywords returns
    plain, plain_sc = m.generate_stream(px, max_length=LH, slots=SLOTS, num_beams=nb, return_scores=True)
    assert torch.equal(_pad(stream[0][0::nb], cfg.pad_id), _pad(plain, cfg.pad_id)) and torch.equal(stream[1][0::nb], plain_sc)
    # fewer rows: a prefix of every image's list; a winner with its log-probabilities
    two = m.generate_stream(px, max_length=LH, slots=SLOTS, num_beams=nb, num_return_sequences=2)
    rows2 = _pad(stream[0], cfg.pad_id).view(N_IMG, nb, LH)[:, :2].reshape(-1, LH)
    assert torch.is_tensor(two) and torch.equal(_pad(two, cfg.pad_id), rows2)
    one, one_lp = m.generate_stream(px, max_length=LH, slots=SLOTS, num_beams=nb, num_return_sequences=1, return_logprobs=True)
    assert torch.equal(_pad(one, cfg.pad_id), _pad(plain, cfg.pad_id)) and torch.equal(_pad(one_lp, 0.0), _pad(stream[2], 0.0)[0::nb])


def test_stream_nbest_under_an_ngram_ban(decoder_dir):
    cfg, m, px, stream, lock, info = _both(8, "bf16", 4, decoder_dir, no_repeat_ngram_size=3)
    assert info[0] == "slot-refill" and info[1] == 0
    _assert_same_rows(cfg, 4, stream, lock)
    ids = stream[0].cpu().tolist()
    for row in ids:                                             # the ban held in every hypothesis
        toks = [t for t in row if t != cfg.pad_id]
        grams = [tuple(toks[i:i + 3]) for i in range(len(toks) - 2)]
        assert len(grams) == len(set(grams))


def test_stream_nbest_after_the_padding_fallback(decoder_dir):
    """A running beam that takes padding sends the wave to lockstep ``generate`` with the same keywords: the same rows.  Padding is made
    likely for this case alone (the file's model lowers its bias by 8) and the model is put back afterwards."""
    cfg, m, px, _ = SB._model(8, decoder_dir)
    px = px[:13]
    m.set_decode_weights("bf16")
    bias = m.state_dict_views()["decoder.lm_head.bias"]
    bias[cfg.pad_id] += 11.0
    m.sync_weights()
    try:
        kw = dict(max_length=LH, num_beams=4, num_return_sequences=4, return_logprobs=True, return_scores=True)
        s_ids, s_sc, s_lp = m.generate_stream(px, slots=SLOTS, **kw)
        assert m.last_stream_pad_fallbacks > 0, "no running beam took padding: the case does not reach the fallback"
        l_ids, l_sc, l_lp = m.generate(px, **kw)
    finally:
        bias[cfg.pad_id] -= 11.0
        m.sync_weights()
    assert torch.equal(_pad(s_ids, cfg.pad_id), _pad(l_ids, cfg.pad_id))
    assert float((s_sc - l_sc).abs().max()) <= LP_TOL and float((_pad(s_lp, 0.0) - _pad(l_lp, 0.0)).abs().max()) <= LP_TOL


@pytest.mark.parametrize("keys", [8, 164])
def test_logprobs_are_the_models(decoder_dir, keys):
    nb = {8: 4, 164: 2}[keys]
    cfg, m, px, stream, lock, info = _both(keys, "bf16", nb, decoder_dir)
    for name, (ids, score, lp) in (("stream", stream), ("lockstep", lock)):
        sc = m.align(px.repeat_interleave(nb, dim=0), ids)
        live = sc["live"]
        assert int(live.sum()) > 4 * N_IMG
        err = float((lp[:, 1:] - sc["logprob"])[live].abs().max())
        print(f"{keys} keys, {name}: per-token log-probabilities within {err:.3e} of the teacher-forced pass over {int(live.sum())} tokens")
        assert err <= LP_TOL
        # sum / length ** length_penalty (1.0) is the score: within generated_length ulps of the sum
        gen_len = (ids.shape[1] - (ids.flip(1) != cfg.pad_id).int().argmax(dim=1) - 1).double()
        total = lp.double().sum(1)
        ulp = torch.from_numpy(np.spacing(total.abs().float().cpu().numpy())).to(total.device).double()
        off = (total - score.double() * gen_len).abs()
        assert bool((off <= gen_len * ulp).all()), float((off / (gen_len * ulp)).max())


# ---- 9. the fitted fixture --------------------------------------------------------------------------------------------------------------
def test_records_and_oracle_on_the_fitted_fixture(tmp_path):
    g, cfg, sd, data = load_trained()
    m = TrOCRModel(cfg.encoder_config_dict(), build_decoder_dir(str(tmp_path / "dec"), cfg), load_tokenizer=True)
    m.load_state_dict(sd, strict=True)
    m.eval()
    px = torch.from_numpy(np.concatenate([data["fit"][0], data["unseen"][0]]))
    labels = torch.from_numpy(np.concatenate([np.asarray(data["fit"][1]), np.asarray(data["unseen"][1])])).long()
    Lh = int(g["label_len"])
    recs = m.recognize_many(px, num_beams=4, n_best=4, max_length=Lh, slots=5)
    assert len(recs) == 12
    for r in recs:
        assert len(r["hypotheses"]) == 4 and "hypotheses" not in r["hypotheses"][0]
        for k in ("text", "tokens", "token_strings", "logprobs", "confidence", "score"):
            assert r["hypotheses"][0][k] == r[k], k
        scores = [h["score"] for h in r["hypotheses"]]
        assert scores == sorted(scores, reverse=True) and len({tuple(h["tokens"]) for h in r["hypotheses"]}) == 4
        assert "centroids" not in r and 0.0 < r["confidence"] <= 1.0
        assert abs(np.log(r["confidence"]) - r["score"]) <= 1e-4          # length_penalty 1: the score is the mean log-probability
    want = m.recognize(px, num_beams=4, max_length=Lh)
    assert [r["text"] for r in recs] == [w["text"] for w in want] and len({r["text"] for r in recs}) > 1
    assert [r["tokens"] for r in recs] == [w["tokens"] for w in want]
    both = m.recognize(px, num_beams=4, max_length=Lh, n_best=2)
    assert [b["text"] for b in both] == [w["text"] for w in want] and all(len(b["hypotheses"]) == 2 and "centroids" in b for b in both)
    assert [[h["tokens"] for h in b["hypotheses"]] for b in both] == [[h["tokens"] for h in r["hypotheses"][:2]] for r in recs]
    with pytest.raises(ValueError):
        m.recognize_many(px, n_best=2, max_length=Lh, slots=5)                     # n > 1 with greedy
    with pytest.raises(ValueError):
        m.generate(px, max_length=Lh, num_beams=4, num_return_sequences=5)
    with pytest.raises(ValueError):
        m.generate(px, max_length=Lh, num_beams=1, num_return_sequences=2)
    # the oracle
    ev = m.evaluate_many(px, labels, num_beams=4, n_best=4, max_length=Lh, slots=5)
    base = m.evaluate_many(px, labels, num_beams=4, max_length=Lh, slots=5)
    assert ev["cer_oracle"] <= ev["cer"] and ev["cer_oracle_corpus"] <= ev["cer_corpus"]
    assert np.array_equal(ev["per_line"]["dist_nbest"][:, 0], ev["per_line"]["dist"]) and ev["per_line"]["dist_nbest"].shape == (12, 4)
    assert sum(ev["oracle_rank"]) == 12 and len(ev["oracle_rank"]) == 4
    for k in ("cer", "cer_corpus", "exact", "substitutions", "deletions", "insertions", "ref_chars"):      # the winner's keys, unchanged
        assert ev[k] == base[k], k
    assert torch.equal(ev["ids"], base["ids"]) and np.array_equal(ev["per_line"]["dist"], base["per_line"]["dist"])
    assert not any(k in base for k in ("cer_oracle", "cer_oracle_corpus", "oracle_rank")) and "dist_nbest" not in base["per_line"]
    print(f"fitted fixture: CER {ev['cer']:.4f}, oracle CER over 4 readings {ev['cer_oracle']:.4f}, best reading at rank {ev['oracle_rank']}")
    with pytest.raises(ValueError):
        m.evaluate_many(px, labels, num_beams=1, n_best=2, max_length=Lh, slots=5)
    # trainer.test(n_best=4): the same two means, from the ids on the device and from the decoded strings
    from kzv import metrics as M
    from kzv import trainer as T
    loader = [{"pixel_values": px[:6], "labels": labels[:6]}, {"pixel_values": px[6:], "labels": labels[6:]}]
    ev128 = m.evaluate_many(px, labels, num_beams=4, n_best=4)                       # trainer.test decodes at generate_stream's default max_length
    outs = []
    for one_char in (True, False):
        m._one_char = None
        orig = M.is_one_char_tokenizer
        if not one_char:
            M.is_one_char_tokenizer = lambda tok: False
        try:
            lines = []
            outs.append(T.test(m, loader, log=lines.append, stream_decode="stream-beam", n_best=4))
        finally:
            M.is_one_char_tokenizer = orig
            m._one_char = None
        assert list(outs[-1]) == ["test_loss", "test_cer", "test_cer_stream_beam", "test_cer_oracle"]
        assert "best reading at rank (0 = the winner): " + " ".join(f"{k}:{c}" for k, c in enumerate(ev128["oracle_rank"])) in lines[-1]
        assert outs[-1]["test_cer_stream_beam"] == ev128["cer"] and outs[-1]["test_cer_oracle"] == ev128["cer_oracle"]
        assert len(m.logged["test_cer_oracle"]) == 12
