"""The KV-cached generation step against the fp64 oracle on a model with PEAKED attention (tests/_peaked.py).

Every other test of the step runs on recipe weights, whose attention is uniform, and compares one engine path with another: a wrong
softmax scale, a wrong online-softmax correction, a key read from the wrong ancestor's cache row or a stale key of a slot's former
occupant move those logits by less than the 1e-2 they allow.  On the sharpened model (largest probability of a row about 0.5 in both
attentions; halving either softmax scale moves the logits by at least 6 x err_ref, asserted by the helper on every case's own batch)
they do not pass.

Protocol of tests/test_decode_fused_gpu.py::_lockstep: teacher-forced ids with ragged row ends through kzv_decode_step (or
kzv_decode_step_graph), step by step; with 2 or 4 rows per image a re-parenting inside each image's group every 3 steps
(kzv_decode_reorder).  At every step the reference is oracle/trocr_oracle.py's decoder_forward in fp64 over the current prefix, on the
once-computed fp64 encoder output; ``err_ref`` is the same oracle with state dict, pixels and arithmetic in bf16, measured at every step
on the same ids and rows.  On live rows (newest token not padding) the engine must stay within 2 x err_ref, the margin of
tests/test_align_gpu.py on the same ground: the engine's rounding points are not the all-bf16 oracle's.  The e4m3 cases take as reference
the fp64 oracle on kzv.quant.dequantised_decoder_weights of the sharpened state dict.  Every case asserts kzv_decode_step_impl and
kzv_decode_weights_impl before its first step.

Slot refill (generate_stream) on the same kind of model with an EOS bias: the log-probability of every emitted token against the fp64
oracle's log_softmax on the returned ids, within 2 x (2 x err_ref) -- a log-probability is a logit minus a log-sum-exp of logits, the
rule of LP_TOL in tests/test_stream_gpu.py; with 4 beams the returned score against the oracle's log-probabilities under the same length
penalty.  At least 20 of the 40 lines must end by EOS before their limit.

Measured on an MI355X: engine error / err_ref 0.42 .. 0.58 over the 23 lockstep cases (err_ref 0.013 .. 0.028); stream log-probabilities
within 0.006 and beam scores within 0.003 of the oracle's at err_ref 0.039; 28 .. 35 of 40 lines ending by EOS before their limit.  Per
case: DESIGN.md section 7, "The generation step on peaked attention"."""
import numpy as np
import pytest
import torch

import _peaked as PK
from kzv import _lib as L
from kzv import quant as Q
from kzv.data import build_decoder_dir, synthetic_batch
from kzv.model import TrOCRModel
from test_stream_beam_gpu import PAD_BIAS
from test_stream_gpu import LH as STREAM_LH, _limits

pytestmark = pytest.mark.gpu
IMAGES, LH, REPARENT_EVERY = 5, 30, 3
SEED = 21                                # recipe seed of every sharpened model here
MARGIN = 2.0
# crops by their number of patch keys (16 x 16 patches); beyond 287 keys the model is created with long_sequences; 512 and 516 keys: 2 decoder layers
CROPS = {160: dict(image_h=64, image_w=640), 164: dict(image_h=32, image_w=1312), 320: dict(image_h=64, image_w=1280),
         512: dict(image_h=2048, image_w=64, dec_layers=2), 516: dict(image_h=2064, image_w=64, dec_layers=2)}
# The slot-refill model.  With test_stream_gpu.py's + 0.5 the sharpened model (logits up to 1.5 instead of 0.1) never emits EOS, so
# the bias is raised.  The fp32 oracle's greedy decode of the 40 crops, lines ending by EOS before their limit (of _limits(40, 23)):
# + 0.7: 3 / 1 (164 / 320 keys), + 0.8: 9 / 15, + 0.85: 17 / 24, + 0.9: 31 / 32 at 7 / 4 distinct lengths between 3 and 33, + 1.0: 36
# but all within 8 tokens, + 2.0: every line ends after its first token.
EOS_BIAS = 0.9


@pytest.fixture(autouse=True)
def _default_mode_afterwards():
    yield
    L.load().kzv_set_decode_one_launch(-1)


@pytest.fixture(scope="module")
def decoder_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("dec"))


_engines = {}


def _engine(keys, decoder_dir):
    """One engine model per crop for the whole module; every case loads its own sharpened weights into it."""
    if keys not in _engines:
        cfg = PK.geometry(**CROPS[keys])
        assert cfg.num_patches == keys
        m = TrOCRModel(cfg.encoder_config_dict(), build_decoder_dir(decoder_dir + f"/{keys}", cfg), init_seed=SEED, load_tokenizer=False,
                       long_sequences=keys > 287)        # kzv_model_create itself refuses more than 287 patches
        m.eval()
        _engines[keys] = (cfg, m)
    return _engines[keys]


def _oracles(cfg, sd, px16):
    """[(state dict, encoder output)] of the oracle in fp64 and in bf16."""
    return [PK.encode(cfg, sd, px16, dt) for dt in (torch.float64, torch.bfloat16)]


def _lockstep(keys, decoder_dir, rows, one_launch, fmt="bf16", graph=False):
    """-> (largest |engine - fp64 oracle|, largest |bf16 oracle - fp64 oracle|) over the live rows of every step."""
    lib = L.load()
    cfg, m = _engine(keys, decoder_dir)
    BB = IMAGES * rows
    px, lab = PK.batch(cfg, IMAGES, rows, LH, seed=21 + rows)
    sd, px16, info = PK.peaked(cfg, SEED, px, lab)
    print(f"\n{keys} keys, {rows} rows per image: " + PK.describe(info))
    m.load_state_dict(sd, strict=True)
    m.set_decode_weights(fmt)
    ref_sd = sd if fmt == "bf16" else {k: v.numpy() for k, v in Q.dequantised_decoder_weights(sd).items()}
    (sd64, enc64), (sd16, enc16) = _oracles(cfg, ref_sd, px16)
    ids_h = torch.from_numpy(lab).clone()
    ids = ids_h.cuda()
    pxt = torch.from_numpy(px16).cuda()
    stream = torch.cuda.Stream() if graph else torch.cuda.current_stream()
    err = err_ref = 0.0
    compared = 0
    try:
        with torch.cuda.stream(stream):
            L.check(lib.kzv_set_decode_one_launch(one_launch), "mode")
            m._bind(BB, LH)
            L.check(lib.kzv_encode_images(m._h, pxt.data_ptr(), IMAGES, L.stream_handle()), "encode_images")
            L.check(lib.kzv_set_active_length(m._h, 1), "set_active_length")
            L.check(lib.kzv_decode_begin(m._h, L.stream_handle()), "decode_begin")
            impl = (m.decode_step_impl, m.decode_weights_impl)
            assert impl == ("one-launch" if one_launch else "per-operation", fmt), impl
            out = torch.empty(BB, cfg.vocab, device="cuda")
            valid = torch.zeros(BB, LH, dtype=torch.uint8, device="cuda")        # fixed buffers: the replayed graph holds their addresses
            posids = torch.empty(BB, dtype=torch.int32, device="cuda")
            tok = torch.empty(BB, dtype=torch.int64, device="cuda")
            rng = np.random.default_rng(SEED + rows)
            for t in range(LH - 1):
                if rows > 1 and t > 0 and t % REPARENT_EVERY == 0:
                    # row r continues from a row of ITS image's group (forks, die-outs, permutations), as beam search does
                    par = torch.from_numpy(np.concatenate([g * rows + rng.integers(0, rows, size=rows) for g in range(IMAGES)]))
                    perm = par.cuda()
                    ids_h = ids_h[par].contiguous(); ids = ids[perm].contiguous()
                    valid.copy_(valid[perm])
                    L.check(lib.kzv_decode_reorder(m._h, perm.data_ptr(), t, L.stream_handle()), "reorder")
                tok.copy_(ids[:, t])
                live = tok != cfg.pad_id
                valid[:, t] = live.to(torch.uint8)
                posids.copy_(torch.where(live, torch.full_like(tok, t + 1 + cfg.pad_id), torch.full_like(tok, cfg.pad_id)).to(torch.int32))
                out.fill_(float("nan"))
                if graph:
                    L.check(lib.kzv_decode_step_graph(m._h, tok.data_ptr(), posids.data_ptr(), valid.data_ptr(), LH, out.data_ptr(), L.stream_handle()), "graph step")
                else:
                    L.check(lib.kzv_decode_step(m._h, tok.data_ptr(), posids.data_ptr(), t, valid.data_ptr(), LH, out.data_ptr(), L.stream_handle()), "step")
                # the reference meanwhile, on the host: the prefix as it stands after the re-parenting
                prefix = ids_h[:, :t + 1].contiguous()
                rows_live = prefix[:, t] != cfg.pad_id                       # rows whose newest token is padding have no defined output
                want = PK.decode(cfg, sd64, prefix, enc64)[:, t]
                want16 = PK.decode(cfg, sd16, prefix, enc16)[:, t].double()
                torch.cuda.synchronize()
                if bool(rows_live.any()):
                    got = out.cpu().double()[rows_live]
                    assert bool(torch.isfinite(got).all()), t
                    err = max(err, float((got - want[rows_live]).abs().max()))
                    err_ref = max(err_ref, float((want16 - want)[rows_live].abs().max()))
                    compared += int(rows_live.sum())
    finally:
        torch.cuda.synchronize()
    assert compared > BB                                                     # the comparison was not vacuous
    print(f"   {impl[0]}{' (graph)' if graph else ''}, {fmt}: engine error {err:.4g}, err_ref {err_ref:.4g}, ratio {err / err_ref:.2f} "
          f"(sens_self {info['sens_self']:.3g}, sens_cross {info['sens_cross']:.3g})")
    return err, err_ref


def _check(err, err_ref):
    assert err <= MARGIN * err_ref, (err, err_ref, err / err_ref)


# ---- the one-launch kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 2, 4])
def test_one_launch_step_one_pass(decoder_dir, rows):
    """160 patch keys, the limit of the pass that holds every score in registers."""
    _check(*_lockstep(160, decoder_dir, rows, 1))


@pytest.mark.parametrize("rows", [1, 2, 4])
@pytest.mark.parametrize("keys", [164, 320])
def test_one_launch_step_chunked(decoder_dir, keys, rows):
    """The instances with the online softmax: 164 keys (4 keys in the second chunk) and 320 (their limit)."""
    _check(*_lockstep(keys, decoder_dir, rows, 1))


# ---- one launch per operation -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 2, 4])
@pytest.mark.parametrize("keys", [160, 320])
def test_launch_per_operation_step(decoder_dir, keys, rows):
    """attn_decode_kernel<24, G> (160 keys) and <40, G> (320 keys) for the cross-attention, G = the rows per image; <24, 1> with the row
    table for the self-attention."""
    _check(*_lockstep(keys, decoder_dir, rows, 0))


@pytest.mark.parametrize("one_launch", [0, 1])
def test_graph_replayed_step(decoder_dir, one_launch):
    """kzv_decode_step_graph: the step index is read on the device (nkeys = t + 1, append_at = t)."""
    _check(*_lockstep(160, decoder_dir, 1, one_launch, graph=True))


@pytest.mark.parametrize("rows", [1, 4])
@pytest.mark.parametrize("keys", [512, 516])
def test_long_sequence_step(decoder_dir, keys, rows):
    """long_sequences=True, 2 decoder layers, attn_decode_long_kernel<G>: 2048 x 64 pixels (513 encoder tokens, 512 patch keys: eight
    whole chunks of 64) and 2064 x 64 (516 keys: eight chunks and a ninth of 4 keys, whose clamped rows are masked)."""
    _check(*_lockstep(keys, decoder_dir, rows, 0))


# ---- e4m3 weights -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keys,rows", [(160, 4), (320, 1)])
def test_e4m3_step(decoder_dir, keys, rows):
    """The header documents the e4m3 step as bit-equal to the bf16 step on the dequantised weights: the reference is the oracle on those."""
    _check(*_lockstep(keys, decoder_dir, rows, 1, fmt="e4m3"))


# ---- slot refill ------------------------------------------------------------------------------------------------------------------------
_stream_models = {}


def _stream_model(keys, decoder_dir):
    """peaked() on the crop's _lockstep batch, EOS bias raised and padding's lowered (a running beam that takes padding sends the wave
    to the lockstep search: tests/test_stream_beam_gpu.py); 40 crops; the oracle in fp64 and bf16."""
    if keys not in _stream_models:
        cfg, m = _engine(keys, decoder_dir)
        px, lab = PK.batch(cfg, IMAGES, 1, LH, seed=22)
        sd, _, info = PK.peaked(cfg, SEED, px, lab)
        print(f"\n{keys} keys, slot refill: " + PK.describe(info))
        bias = sd["decoder.lm_head.bias"].copy()
        bias[cfg.eos_id] += EOS_BIAS
        bias[cfg.pad_id] += PAD_BIAS
        for k in ("decoder.lm_head.bias", "decoder.lm_head.decoder.bias"):   # one tensor under two names: load_state_dict copies both
            assert k in sd
            sd[k] = PK.bf16_exact(bias)
        px16 = PK.bf16_exact(synthetic_batch(cfg, 40, STREAM_LH, seed=3)[0])
        _stream_models[keys] = (cfg, m, sd, px16, _oracles(cfg, sd, px16))
    cfg, m, sd, px16, oracles = _stream_models[keys]
    m.load_state_dict(sd, strict=True)
    m.set_decode_weights("bf16")
    L.check(L.load().kzv_set_decode_one_launch(1), "mode")
    return cfg, m, torch.from_numpy(px16).cuda(), oracles


def _oracle_logprobs(cfg, oracles, ids):
    """ids [N, W] as returned -> (fp64 log-probability of every emitted token [N, W - 1], emitted [N, W - 1], err_ref of the logits on
    the rows whose newest token is not padding)."""
    ids = ids.cpu()
    inp, tgt = ids[:, :-1].contiguous(), ids[:, 1:]
    (sd64, enc64), (sd16, enc16) = oracles
    want = PK.decode(cfg, sd64, inp, enc64)
    live = inp != cfg.pad_id
    err_ref = float((PK.decode(cfg, sd16, inp, enc16).double() - want)[live].abs().max())
    lp = torch.gather(torch.log_softmax(want, -1), 2, tgt[:, :, None]).squeeze(-1)
    return lp, live & (tgt != cfg.pad_id), err_ref


def _ended_early(cfg, ids, limits):
    ids = ids.cpu()
    length = (ids != cfg.pad_id).sum(1)
    by_eos = (ids == cfg.eos_id).any(1) & (length < limits)
    return int(by_eos.sum()), sorted(set(length[by_eos].tolist()))


@pytest.mark.parametrize("keys", [164, 320])
def test_slot_refill_logprobs_against_the_oracle(decoder_dir, keys):
    """40 crops on 6 slots, greedy: a stale key of a slot's former occupant, or a wrong number of keys after a refill, moves these
    log-probabilities by the order of sens_self."""
    cfg, m, px, oracles = _stream_model(keys, decoder_dir)
    limits = _limits(40, 23)
    ids, lp = m.generate_stream(px, max_length=STREAM_LH, slots=6, limits=limits, return_logprobs=True)
    assert m.stream_decode_impl == "slot-refill" and m.decode_step_impl == "one-launch" and m.decode_weights_impl == "bf16"
    early, ends = _ended_early(cfg, ids, limits)
    want, emitted, err_ref = _oracle_logprobs(cfg, oracles, ids)
    err = float((lp.cpu().double()[:, 1:] - want)[emitted].abs().max())
    bound = 2 * MARGIN * err_ref
    print(f"\n{keys} keys, greedy: {early} of 40 lines end by EOS before their limit, at lengths {ends}; {m.last_stream_steps} steps on 6 slots; "
          f"|log-probability - oracle| {err:.4g} on {int(emitted.sum())} tokens, err_ref {err_ref:.4g}, ratio to the bound {err / bound:.2f}")
    assert early >= 20 and len(ends) >= 4
    assert int(emitted.sum()) > 40
    assert err <= bound, (err, err_ref)


@pytest.mark.parametrize("keys", [164, 320])
def test_slot_refill_beam_scores_against_the_oracle(decoder_dir, keys):
    """The same with 4 beams: the returned score of each returned sequence against the sum of the oracle's log-probabilities divided by
    length ** length_penalty; the per-token bound times the number of tokens, divided by the same length term."""
    cfg, m, px, oracles = _stream_model(keys, decoder_dir)
    limits = _limits(40, 23)
    lpen = 1.0
    ids, score = m.generate_stream(px, max_length=STREAM_LH, slots=6, limits=limits, num_beams=4, length_penalty=lpen, return_scores=True)
    assert m.stream_beam_impl == "slot-refill" and m.last_stream_pad_fallbacks == 0
    assert m.decode_step_impl == "one-launch" and m.decode_weights_impl == "bf16"
    early, ends = _ended_early(cfg, ids, limits)
    want, emitted, err_ref = _oracle_logprobs(cfg, oracles, ids)
    n = emitted.sum(1).double()
    assert bool((n >= 1).all())
    want_score = (want * emitted).sum(1) / n.pow(lpen)
    bound = 2 * MARGIN * err_ref * n / n.pow(lpen)
    rel = ((score.cpu().double() - want_score).abs() / bound)
    print(f"\n{keys} keys, 4 beams: {early} of 40 searches return a line that ends by EOS before its limit, at lengths {ends}; {m.last_stream_steps} steps on "
          f"6 slots; |score - oracle| up to {float((score.cpu().double() - want_score).abs().max()):.4g}, err_ref {err_ref:.4g}, "
          f"largest ratio to the bound {float(rel.max()):.2f}")
    assert early >= 20 and len(ends) >= 4
    assert float(rel.max()) <= 1.0, (float(rel.max()), err_ref)
