"""The one-launch decoder step (csrc/decode_fused.hip: embeddings, every decoder layer and the LM head's dense layer of a generation
token in one launch, a workgroup per image) against the launch-per-operation step it replaces (HF RobertaLayer with use_cache,
modeling_roberta.py:186-326, 421-464, as driven by src/models/trocr_model.py:306-316 with num_beams = 4):

  * step by step through the C ABI on the same ids -- 1, 2 and 4 rows per image, rows that have ended (padding keys), beam
    re-parenting inside an image's group (the cache rows never move: the attention follows the row table) -- the logits of the two
    paths agree to 1e-2 with each other and each with the teacher-forced pass over the whole prefix (the two cached paths round to
    bf16 at the same places and differ in fp32 summation order only; observed 3e-3 .. 5e-3);
  * at the benchmark geometry (160 patch keys, 127 cached keys, 12 decoder layers = the kernel's limits) for beam 4 and greedy;
  * generate() end to end in both modes.
The cached step itself is pinned against the teacher-forced pass and the reference's step-wise decode in test_model_gpu.py /
test_trained_gpu.py (their 256-wide case takes the one-launch path by default).
These are recipe weights, whose attention is uniform: the comparisons here pin layout, launch geometry and the agreement of the paths;
the arithmetic of the attention (softmax scale, online-softmax correction, ancestor rows) is pinned in test_decode_peaked_gpu.py."""
import dataclasses

import numpy as np
import pytest
import torch

from kzv import _lib as L
from kzv.config import small_config, tiny_config
from kzv.data import build_decoder_dir, synthetic_batch
from kzv.model import TrOCRModel

pytestmark = pytest.mark.gpu
TOL = 1e-2          # observed 3e-3 (3 layers) .. 5e-3 (12 layers) at logits up to ~1.3; a bf16-accumulating dot product in the scores
                    # (v_dot2c_f32_bf16, tried) reads 1.3e-2 .. 3e-2 here


@pytest.fixture(autouse=True)
def _default_mode_afterwards():
    yield
    L.load().kzv_set_decode_one_launch(-1)


def _pair(cfg, tmp_path, seed, n=2):
    d = build_decoder_dir(str(tmp_path / "dec"), cfg)
    return [TrOCRModel(cfg.encoder_config_dict(), d, init_seed=seed, load_tokenizer=False) for _ in range(n)]


def _lockstep(cfg, tmp_path, images, beams, Lh, reparent_every, seed):
    """Teacher-forced ids through kzv_decode_step on two identical models, one per mode; returns the largest logit difference."""
    lib = L.load()
    cfg = dataclasses.replace(cfg, enc_hidden_dropout=0.0, enc_attn_dropout=0.0, dec_hidden_dropout=0.0, dec_attn_dropout=0.0)
    *models, recompute = _pair(cfg, tmp_path, seed, 3)
    BB = images * beams
    px, lab = synthetic_batch(cfg, BB, Lh, seed=seed, min_chars=2, max_chars=Lh - 2)
    ids = torch.from_numpy(lab).cuda()
    ids[:, 0] = cfg.bos_id
    pxt = torch.from_numpy(px[::beams].copy()).cuda()               # one crop per image
    for m in models:
        m.eval()
        m._bind(BB, Lh)
        L.check(lib.kzv_encode_images(m._h, pxt.data_ptr(), images, L.stream_handle()), "encode_images")
        L.check(lib.kzv_set_active_length(m._h, 1), "set_active_length")
        L.check(lib.kzv_decode_begin(m._h, L.stream_handle()), "decode_begin")
    # the reference of both: the teacher-forced pass over the whole prefix (kzv_decode_logits), every row with its own copy of the image
    recompute.eval()
    recompute.forward_loss(pxt.repeat_interleave(beams, dim=0), ids, want_logits=False, seed=0)
    out = [torch.empty(BB, cfg.vocab, device="cuda") for _ in range(2)]
    valid = torch.zeros(BB, Lh, dtype=torch.uint8, device="cuda")
    posids = torch.empty(BB, dtype=torch.int32, device="cuda")
    rng = np.random.default_rng(seed)
    worst = 0.0
    ref = torch.empty(BB, cfg.vocab, device="cuda")
    to_ref = [0.0, 0.0]                                             # each path against the teacher-forced pass over the whole prefix
    for t in range(Lh - 1):
        if beams > 1 and t > 0 and t % reparent_every == 0:
            # row r continues from a row of ITS image's group (forks, die-outs, permutations), as beam search does
            par = np.concatenate([g * beams + rng.integers(0, beams, size=beams) for g in range(images)])
            perm = torch.from_numpy(par).cuda()
            ids = ids[perm].contiguous(); valid = valid[perm].contiguous()
            for m in models:
                L.check(lib.kzv_decode_reorder(m._h, perm.data_ptr(), t, L.stream_handle()), "reorder")
        tok = ids[:, t].contiguous()
        live = tok != cfg.pad_id
        valid[:, t] = live.to(torch.uint8)
        posids.copy_(torch.where(live, torch.full_like(tok, t + 1 + cfg.pad_id), torch.full_like(tok, cfg.pad_id)).to(torch.int32))
        for mode, (m, o) in enumerate(zip(models, out)):
            L.check(lib.kzv_set_decode_one_launch(mode), "mode")
            L.check(lib.kzv_decode_step(m._h, tok.data_ptr(), posids.data_ptr(), t, valid.data_ptr(), Lh, o.data_ptr(), L.stream_handle()), "step")
        L.check(lib.kzv_set_active_length(recompute._h, t + 1), "len")
        L.check(lib.kzv_decode_logits(recompute._h, ids.data_ptr(), t, ref.data_ptr(), L.stream_handle()), "logits")
        torch.cuda.synchronize()
        rows = live.cpu().numpy()                                   # rows whose newest token is padding have no defined output
        if rows.any():
            d = np.abs((out[0] - out[1]).cpu().numpy()[rows])
            assert np.isfinite(d).all(), t
            worst = max(worst, float(d.max()))
            for k in range(2):
                to_ref[k] = max(to_ref[k], float(np.abs((out[k] - ref).cpu().numpy()[rows]).max()))
    return worst, float(out[0].abs().max()), to_ref


@pytest.mark.parametrize("beams", [1, 2, 4])
def test_one_launch_step_equals_the_launch_per_operation_step(tmp_path, beams):
    cfg = dataclasses.replace(tiny_config(), dec_hidden=256, dec_heads=4, dec_ffn=768, dec_layers=3)
    worst, scale, to_ref = _lockstep(cfg, tmp_path, images=5, beams=beams, Lh=30, reparent_every=3, seed=21 + beams)
    print(f"{beams} rows per image: largest logit difference {worst:.2e} (logits up to {scale:.2f}); against the prefix recompute: "
          f"per-operation {to_ref[0]:.2e}, one launch {to_ref[1]:.2e}")
    assert worst < TOL and to_ref[1] < TOL


@pytest.mark.parametrize("beams", [4, 1])
def test_one_launch_step_at_the_benchmark_geometry(tmp_path, beams):
    """160 patch keys, 127 cached keys, 12 decoder layers: every key iteration of the kernel and its layer-table limit."""
    cfg = small_config()
    worst, scale, to_ref = _lockstep(cfg, tmp_path, images=3, beams=beams, Lh=cfg.max_pos - cfg.pad_id - 1, reparent_every=5, seed=5)
    print(f"{beams} rows per image, 160 / 127 keys, 12 layers: largest logit difference {worst:.2e} (logits up to {scale:.2f}); against the "
          f"prefix recompute: per-operation {to_ref[0]:.2e}, one launch {to_ref[1]:.2e}")
    assert worst < TOL and to_ref[1] < TOL


def test_generate_in_both_modes(tmp_path):
    lib = L.load()
    cfg = dataclasses.replace(tiny_config(), dec_hidden=256, dec_heads=4, dec_ffn=768)
    m = _pair(cfg, tmp_path, 3)[0]
    m.eval()
    px = torch.from_numpy(synthetic_batch(cfg, 6, 20, seed=8)[0]).cuda()
    for beams in (1, 2, 4, 3):                                       # 3 rows per image: not instantiated, both modes take the old path
        got = []
        for mode in (0, 1):
            L.check(lib.kzv_set_decode_one_launch(mode), "mode")
            got.append(m.generate(px, max_length=20, num_beams=beams, early_stopping=False).cpu())
        w = min(got[0].shape[1], got[1].shape[1])
        agree = float((got[0][:, :w] == got[1][:, :w]).float().mean())
        print(f"beams {beams}: token agreement {agree:.3f}")
        assert agree > 0.9                                          # untrained, nearly flat logits: rare argmax ties may flip


def test_generation_with_more_images_than_compute_units(tmp_path):
    """600 images in ONE generate call (one workgroup per image in decode_fused.hip: 600 workgroups on 256 CUs, two rounds and slower loads)
    against the same images in batches of 100, greedy and beam-4: token for token.  (Added with the decoder-chain fix of round 4: a wait that
    hipcc sized too leniently only showed once a launch had more workgroups than CUs; tests/test_decoder_chain_gpu.py.)"""
    import dataclasses

    import torch

    from kzv.config import tiny_config
    from kzv.data import build_decoder_dir, synthetic_batch
    from kzv.model import TrOCRModel
    cfg = dataclasses.replace(tiny_config(), dec_hidden=256, dec_heads=4, dec_ffn=768, dec_layers=6)
    m = TrOCRModel(cfg.encoder_config_dict(), build_decoder_dir(str(tmp_path / "dec"), cfg), init_seed=4, load_tokenizer=False)
    m.eval()
    px, _ = synthetic_batch(cfg, 600, 20, seed=3)
    px = torch.from_numpy(px).cuda()
    for beams in (1, 4):
        whole = m.generate(px, max_length=24, num_beams=beams)
        parts = torch.cat([m.generate(px[i:i + 100], max_length=24, num_beams=beams) for i in range(0, 600, 100)])
        assert whole.shape == parts.shape and torch.equal(whole, parts), f"beams {beams}: {int((whole != parts).any(1).sum())} sequences differ"
