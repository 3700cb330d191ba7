"""Long encoder sequences through the whole model (TrOCRModel(long_sequences=True) -> kzv_model_create_ex(KZV_MODEL_LONG_SEQ)):
tiny-depth models with head_dim 64 and 96 at 2048 x 64 (513 tokens), 64 x 1280 (321) and 1024 x 64 with 8 x 8 patches (1,025),
whose encoder self-attention and decoder cross-attention run on the K/V-streaming kernels.  Logits against the fp32 oracle,
training gradients against the oracle with the step's own dropout masks replayed, trimmed == untrimmed, generation with and
without the cache over 513 and 1,025 patch keys (the chunked decode instance beyond 320 keys), and the CLI end to end.
These are recipe weights, whose attention is uniform: the generation comparisons here pin layout, launch geometry and the agreement of
the paths; the arithmetic of the decode attention (its online-softmax correction) is pinned in test_decode_peaked_gpu.py."""
import dataclasses
import gc
import os
import subprocess
import sys

import pytest
import torch

from kzv import params as P
from kzv.config import tiny_config
from kzv.data import build_decoder_dir, synthetic_batch
from kzv.model import TrOCRModel
from oracle import trocr_oracle as O
from _replay import step_masks
from test_bench_geometry_gpu import _check_grads, _grad_errors

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
SEED = 2024
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GEOMS = {"2048x64": dict(image_h=2048, image_w=64), "64x1280": dict(image_h=64, image_w=1280),
         "1024x64p8": dict(image_h=1024, image_w=64, patch_h=8, patch_w=8)}
SEQ = {"2048x64": 513, "64x1280": 321, "1024x64p8": 1025}


def _cfg(hd, geom, dropout=True):
    c = dataclasses.replace(tiny_config(), enc_hidden=2 * hd, enc_heads=2, enc_ffn=256, enc_layers=1, dec_layers=1, **GEOMS[geom])
    if not dropout:
        c = dataclasses.replace(c, enc_hidden_dropout=0.0, enc_attn_dropout=0.0, dec_hidden_dropout=0.0, dec_attn_dropout=0.0)
    assert c.enc_seq == SEQ[geom]
    return c


def _make(cfg, tmp_path, seed):
    m = TrOCRModel(cfg.encoder_config_dict(), build_decoder_dir(str(tmp_path / "dec"), cfg), init_seed=seed, load_tokenizer=False,
                   device=DEV, long_sequences=True)
    assert m.encoder_attention_impl == ("stream96" if cfg.enc_hidden // cfg.enc_heads == 96 else "stream64")
    return m


@pytest.fixture(autouse=True)
def _free():
    yield
    gc.collect()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("geom", list(GEOMS))
@pytest.mark.parametrize("hd", [64, 96])
def test_long_encoder_logits_and_gradients(tmp_path, hd, geom):
    """Eval: logits within 3e-2 of the fp32 oracle, loss within 5e-3.  Training with dropout 0.1 everywhere: the step's masks
    (tests/_replay.step_masks) replayed through the oracle, every gradient tensor within 0.05 of its largest entry, median <= 0.02
    (the bounds of test_bench_geometry_gpu.py); flat_grads NaN-filled first."""
    cfg = _cfg(hd, geom)
    m = _make(cfg, tmp_path, 7)
    sd = P.state_dict_from_flat(cfg, P.recipe_flat(cfg, 7))
    B = 4
    px, lab = synthetic_batch(cfg, B, 24, seed=3, min_chars=3, max_chars=23)
    m.eval()
    loss, logits = m.forward_loss(torch.from_numpy(px), torch.from_numpy(lab), want_logits=True, seed=SEED)
    torch.cuda.synchronize()
    r = O.forward_backward(cfg, sd, px, lab, device=DEV)
    err = float((logits.float().cpu() - torch.from_numpy(r["logits"])).abs().max())
    print(f"d{hd} {geom}: {cfg.enc_seq} tokens, eval max|dlogit| {err:.4g}")
    assert err < 3e-2 and abs(float(loss.item()) - r["loss"]) < 5e-3
    m.train()
    m.flat_grads.fill_(NAN)
    loss, _ = m.forward_loss(torch.from_numpy(px), torch.from_numpy(lab), seed=SEED)
    m.backward()
    torch.cuda.synchronize()
    T = m.last_active_length
    masks = step_masks(cfg, SEED, B, T, device=DEV)
    r = O.forward_backward(cfg, sd, px, lab[:, :T + 1], masks=masks, device=DEV)
    assert abs(float(loss.item()) - r["loss"]) < 5e-3
    _check_grads(f"d{hd} {geom} dropout replay", _grad_errors(cfg, m.flat_grads, r["grads"]), 0.05, 0.02)


@pytest.mark.parametrize("hd", [64, 96])
def test_long_encoder_trim_does_not_change_the_step(tmp_path, hd):
    """513 tokens, dropout off: the decoder on the trimmed prefix gives the loss and gradients of the full length (float-atomic
    summation order only, as test_model_gpu.py bounds it)."""
    cfg = _cfg(hd, "2048x64", dropout=False)
    m = _make(cfg, tmp_path, 13)
    px, lab = synthetic_batch(cfg, 4, 36, seed=2, min_chars=2, max_chars=11)
    batch = (torch.from_numpy(px), torch.from_numpy(lab))
    m.train()
    res = {}
    for trim in (False, True):
        m.trim_padding = trim
        loss, _ = m.forward_loss(*batch)
        m.backward()
        torch.cuda.synchronize()
        res[trim] = (float(loss.item()), m.flat_grads.clone())
    assert abs(res[True][0] - res[False][0]) < 1e-5
    d = (res[True][1] - res[False][1]).abs().max().item()
    assert d < 2e-4 * res[False][1].abs().max().item() + 1e-7, d


@pytest.mark.parametrize("geom", ["2048x64", "1024x64p8"])
@pytest.mark.parametrize("hd", [64, 96])
def test_long_encoder_generation_cache_matches_recompute(tmp_path, hd, geom):
    """Greedy and beam-4 generation over 512 / 1,024 patch keys: the cached step (cross-attention by the chunked decode instance
    beyond 320 keys; launch-per-operation step bodies and the graph-replayed step) and use_cache=False (the full decoder forward
    per token: cross-attention by the streaming kernels) give the same tokens."""
    cfg = _cfg(hd, geom)
    m = _make(cfg, tmp_path, 21)
    m.eval()
    px, _ = synthetic_batch(cfg, 3, 16, seed=5)
    pxt = torch.from_numpy(px)
    for beams in (1, 4):
        g1 = m.generate(pxt, max_length=10, num_beams=beams, early_stopping=False, use_cache=True).cpu()
        g0 = m.generate(pxt, max_length=10, num_beams=beams, early_stopping=False, use_cache=False).cpu()
        assert g1.shape == g0.shape and torch.equal(g1, g0), (beams, g1, g0)


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("geom", ["2048x64", "1024x64p8"])
@pytest.mark.parametrize("hd", [64, 96])
def test_long_encoder_cached_step_logits_equal_the_prefix_recompute(tmp_path, hd, geom, wide):
    """kzv_decode_step (one token against the cache; cross-attention over 512 / 1,024 patch keys by the chunked decode instance)
    against kzv_decode_logits (the teacher-forced pass over the whole prefix; cross-attention by the streaming kernels) on the same
    ids, every step: logits within 2e-2, test_model_gpu.py's bound for the same comparison at <= 320 keys.  wide: decoder hidden
    256, whose step takes the LayerNorm-folded body (decode_step_body_fused); otherwise the plain launch-per-operation body."""
    import ctypes as C
    from kzv import _lib as L
    cfg = _cfg(hd, geom, dropout=False)
    if wide:
        cfg = dataclasses.replace(cfg, dec_hidden=256, dec_heads=4, dec_ffn=768)
    m = _make(cfg, tmp_path, 9)
    m.eval()
    B, Lh = 4, 12
    px, lab = synthetic_batch(cfg, B, Lh, seed=4, min_chars=2, max_chars=10)
    ids = torch.from_numpy(lab).cuda()
    ids[:, 0] = cfg.bos_id
    lib = L.load()
    m.forward_loss(torch.from_numpy(px).cuda(), ids, want_logits=False, seed=0)
    a = torch.empty(B, cfg.vocab, device=DEV)
    b = torch.empty(B, cfg.vocab, device=DEV)
    valid = torch.zeros(B, Lh, dtype=torch.uint8, device=DEV)
    posids = torch.empty(B, dtype=torch.int32, device=DEV)
    worst = 0.0
    for t in range(Lh - 1):
        tok = ids[:, t].contiguous()
        live = tok != cfg.pad_id
        valid[:, t] = live.to(torch.uint8)
        posids.copy_(torch.where(live, torch.full_like(tok, t + 1 + cfg.pad_id), torch.full_like(tok, cfg.pad_id)).to(torch.int32))
        a.fill_(NAN)
        b.fill_(NAN)
        L.check(lib.kzv_decode_step(m._h, tok.data_ptr(), posids.data_ptr(), t, valid.data_ptr(), Lh, a.data_ptr(), L.stream_handle()), "step")
        L.check(lib.kzv_set_active_length(m._h, t + 1), "len")
        L.check(lib.kzv_decode_logits(m._h, ids.data_ptr(), t, b.data_ptr(), L.stream_handle()), "logits")
        torch.cuda.synchronize()
        rows = live.cpu()                                         # rows whose newest token is padding have no defined output
        if rows.any():
            err = float((a - b).abs()[rows.cuda()].max())
            worst = max(worst, err)
            assert err < 2e-2, (t, err)
    print(f"d{hd} {geom} wide={wide}: cached step vs prefix recompute, max |dlogit| {worst:.3g}")


def test_cli_trains_validates_and_tests_at_2048x64(tmp_path):
    """python -m kzv.train --synthetic at 2048 x 64 with a small head_dim-64 encoder: training, beam-4 validation, checkpoint and
    test run, and the printed attention implementation is a streaming one."""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "kuzushiji-vision_amd")]))
    cmd = [sys.executable, "-m", "kzv.train", "--synthetic", "24", "--num_workers", "0", "--image_size", "2048", "64", "--encoder_hidden_size", "128",
           "--encoder_num_layers", "1", "--encoder_num_heads", "2", "--batch_size", "4", "--max_epochs", "1", "--max_length", "16",
           "--output_dir", str(tmp_path / "out")]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "encoder attention: stream64" in out, out[-4000:]
