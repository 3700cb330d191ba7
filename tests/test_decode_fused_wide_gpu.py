"""The one-launch decoder step beyond 160 patch keys (csrc/decode_fused.hip, the chunked instances: 161 .. 320 keys go through the
attention waves' registers in chunks, with an online softmax carried from chunk to chunk) at the smallest shapes where that code can
go wrong -- one real key in the second 160, one full 8-key iteration of it, the reference CLI's 256 patches in both orientations, 287
(the largest without long_sequences) and 320 (the limit):

  * lock-step against the launch-per-operation step and the teacher-forced recompute of the whole prefix, to the 1e-2 of
    test_decode_fused_gpu.py (the chunked softmax changes fp32 summation order only), with kzv_decode_step_impl checked on the very
    handles right before the loop.  Observed on MI355X, 3 layers / Lh 30, logits up to 1.15: between the modes 1.3e-3 .. 3.1e-3, one
    launch against the recompute 2.7e-3 .. 3.8e-3 (per-operation: 2.7e-3 .. 4.0e-3); 12 layers / 125 cached keys at 256 patches: 4.7e-3
    and 5.0e-3 (per-operation 4.7e-3);
  * generate() over a width-bucket switch across the 160-key boundary on the graph-replayed step, in both modes;
  * more images than compute units at 256 patches;
  * 321 patches and 3 rows per image stay on the launch-per-operation path and say so.
These are recipe weights, whose attention is uniform (the online softmax's correction is about 1): the comparisons here pin layout,
launch geometry and the agreement of the paths; the arithmetic of the attention is pinned in test_decode_peaked_gpu.py."""
import dataclasses

import numpy as np
import pytest
import torch

import test_decode_fused_gpu as base
from test_decode_fused_gpu import TOL, _lockstep, _pair
from kzv import _lib as L
from kzv.config import tiny_config
from kzv.data import build_decoder_dir, synthetic_batch
from kzv.model import TrOCRModel

pytestmark = pytest.mark.gpu

# patches -> image (16 x 16 patches)
SHAPES = {"161": (16, 2576, 161), "168": (16, 2688, 168), "256-wide": (64, 1024, 256), "256-tall": (1024, 64, 256),
          "287": (16, 4592, 287), "320": (64, 1280, 320)}


@pytest.fixture(autouse=True)
def _default_mode_afterwards():
    yield
    L.load().kzv_set_decode_one_launch(-1)


def _cfg(shape, dec_layers=3):
    h, w, patches = SHAPES[shape]
    # tiny encoder (128 hidden, 2 heads of 64, 1 layer), the reference decoder's widths
    c = dataclasses.replace(tiny_config(), image_h=h, image_w=w, enc_layers=1, dec_hidden=256, dec_heads=4, dec_ffn=768, dec_layers=dec_layers)
    assert c.num_patches == patches and c.enc_hidden // c.enc_heads == 64
    return c


def _pair_long(cfg, tmp_path, seed, n=2):
    """_pair for encoders beyond 288 tokens (kzv_model_create_ex with KZV_MODEL_LONG_SEQ)."""
    d = build_decoder_dir(str(tmp_path / "dec"), cfg)
    return [TrOCRModel(cfg.encoder_config_dict(), d, init_seed=seed, load_tokenizer=False, long_sequences=True) for _ in range(n)]


def _lockstep_checked(monkeypatch, cfg, tmp_path, **kw):
    """_lockstep, with kzv_decode_step_impl asked on each of its two stepping handles right after their kzv_decode_begin, i.e. bound,
    encoded and just before the loop: 0 in mode 0, 1 in mode 1."""
    lib = L.load()
    begin = lib.kzv_decode_begin
    seen = []

    def begin_and_ask(h, stream):
        rc = begin(h, stream)
        for mode in (0, 1):
            L.check(lib.kzv_set_decode_one_launch(mode), "mode")
            seen.append((mode, lib.kzv_decode_step_impl(h)))
        return rc
    monkeypatch.setattr(lib, "kzv_decode_begin", begin_and_ask)
    if cfg.enc_seq > 288:
        monkeypatch.setattr(base, "_pair", _pair_long)
    else:
        assert base._pair is _pair
    out = _lockstep(cfg, tmp_path, **kw)
    assert seen == [(0, 0), (1, 1)] * 2, seen
    return out


@pytest.mark.parametrize("beams", [1, 2, 4])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_chunked_one_launch_step_equals_the_launch_per_operation_step(tmp_path, monkeypatch, shape, beams):
    """1, 2 and 4 rows per image, rows that have ended (synthetic labels of 2 .. 28 characters in 30 columns), re-parenting every 3 steps."""
    cfg = _cfg(shape)
    worst, scale, to_ref = _lockstep_checked(monkeypatch, cfg, tmp_path, images=5, beams=beams, Lh=30, reparent_every=3, seed=31 + beams)
    print(f"{cfg.num_patches} patch keys ({cfg.image_h} x {cfg.image_w}), {beams} rows per image: largest logit difference {worst:.2e} "
          f"(logits up to {scale:.2f}); against the prefix recompute: per-operation {to_ref[0]:.2e}, one launch {to_ref[1]:.2e}")
    assert worst < TOL and to_ref[1] < TOL


def test_chunked_one_launch_step_at_the_layer_and_cache_limits(tmp_path, monkeypatch):
    """256 patch keys, 12 decoder layers, Lh = max_pos - pad_id - 1 = 126 (125 cached keys at the last step): the layer table's and
    the cached-key limits of test_one_launch_step_at_the_benchmark_geometry."""
    cfg = _cfg("256-wide", dec_layers=12)
    cfg = dataclasses.replace(cfg, vocab=4300, max_pos=128)
    worst, scale, to_ref = _lockstep_checked(monkeypatch, cfg, tmp_path, images=3, beams=4, Lh=cfg.max_pos - cfg.pad_id - 1, reparent_every=5, seed=5)
    print(f"256 patch keys, 12 layers, {cfg.max_pos - cfg.pad_id - 2} cached keys, 4 rows per image: largest logit difference {worst:.2e} "
          f"(logits up to {scale:.2f}); against the prefix recompute: per-operation {to_ref[0]:.2e}, one launch {to_ref[1]:.2e}")
    assert worst < TOL and to_ref[1] < TOL


def _bucket_rows(cfg, w):
    gh, gw, gmax = cfg.grid_h, w // cfg.patch_w, cfg.grid_w
    return np.array([0] + [1 + h * gmax + x for h in range(gh) for x in range(gw)])


def test_bucket_switch_across_the_160_key_boundary(tmp_path):
    """One model at 64 x 1024 with the width buckets 640 (160 keys: the one-pass instances) and 1024 (256 keys: the chunked ones),
    generating on the graph-replayed step at 640, 1024, 640, 1024: every switch re-captures the step's graph."""
    lib = L.load()
    cfg = _cfg("256-wide", dec_layers=2)
    m = TrOCRModel(cfg.encoder_config_dict(), build_decoder_dir(str(tmp_path / "dec"), cfg), init_seed=3, load_tokenizer=False, width_buckets=(640, 1024))
    m.eval()
    narrow_cfg = dataclasses.replace(cfg, image_w=640)
    px = {640: torch.from_numpy(synthetic_batch(narrow_cfg, 6, 20, seed=8)[0]).cuda(), 1024: torch.from_numpy(synthetic_batch(cfg, 6, 20, seed=9)[0]).cuda()}
    got = {}
    for mode in (0, 1):
        L.check(lib.kzv_set_decode_one_launch(mode), "mode")
        for rep in range(2):
            for w in (640, 1024):
                for beams in (1, 4):
                    ids = m.generate(px[w], max_length=20, num_beams=beams, early_stopping=False).cpu()
                    assert m.decode_step_impl == ("one-launch" if mode else "per-operation"), (mode, w, beams)
                    if rep:
                        assert torch.equal(ids, got[mode, w, beams]), f"mode {mode}, width {w}, beams {beams}: the second visit differs"
                    got[mode, w, beams] = ids
    for w in (640, 1024):
        for beams in (1, 4):
            a, b = got[0, w, beams], got[1, w, beams]
            n = min(a.shape[1], b.shape[1])
            agree = float((a[:, :n] == b[:, :n]).float().mean())
            print(f"width {w}, beams {beams}: token agreement between the modes {agree:.3f}")
            assert agree > 0.9                                          # untrained, nearly flat logits: rare argmax ties may flip
    # the 640 bucket IS the 64 x 640 model: same weights, the position rows of the same grid cells (tests/test_buckets_gpu.py)
    narrow = TrOCRModel(narrow_cfg.encoder_config_dict(), build_decoder_dir(str(tmp_path / "dec640"), narrow_cfg), init_seed=3, load_tokenizer=False)
    sd = m.state_dict()
    sd["encoder.position_embeddings"] = sd["encoder.position_embeddings"][:, torch.from_numpy(_bucket_rows(cfg, 640)).to(sd["encoder.position_embeddings"].device)]
    narrow.load_state_dict(sd)
    narrow.eval()
    L.check(lib.kzv_set_decode_one_launch(1), "mode")
    for beams in (1, 4):
        ids = narrow.generate(px[640], max_length=20, num_beams=beams, early_stopping=False).cpu()
        assert narrow.decode_step_impl == "one-launch"
        assert torch.equal(ids, got[1, 640, beams]), f"beams {beams}: the 640 bucket differs from the 64 x 640 model"


def test_more_images_than_compute_units_at_256_patches(tmp_path):
    """300 images in ONE generate call (a workgroup per image: more workgroups than the 256 CUs, each holding its rows through two chunks
    per layer) against the same images in batches of 100, greedy and beam-4: token for token."""
    cfg = _cfg("256-wide", dec_layers=6)
    m = TrOCRModel(cfg.encoder_config_dict(), build_decoder_dir(str(tmp_path / "dec"), cfg), init_seed=4, load_tokenizer=False)
    m.eval()
    px = torch.from_numpy(synthetic_batch(cfg, 300, 20, seed=3)[0]).cuda()
    for beams in (1, 4):
        whole = m.generate(px, max_length=24, num_beams=beams)
        assert m.decode_step_impl == "one-launch"
        parts = torch.cat([m.generate(px[i:i + 100], max_length=24, num_beams=beams) for i in range(0, 300, 100)])
        assert whole.shape == parts.shape and torch.equal(whole, parts), f"beams {beams}: {int((whole != parts).any(1).sum())} sequences differ"


def test_geometry_limits_keep_the_launch_per_operation_step(tmp_path):
    """321 patch keys, and 3 rows per image at 256: not instantiated -- mode 1 reports "per-operation" and generates all the same."""
    lib = L.load()
    L.check(lib.kzv_set_decode_one_launch(1), "mode")
    c321 = dataclasses.replace(_cfg("161", dec_layers=2), image_w=16 * 321)
    assert c321.num_patches == 321
    m = _pair_long(c321, tmp_path, 6, 1)[0]
    m.eval()
    px = torch.from_numpy(synthetic_batch(c321, 3, 12, seed=1)[0]).cuda()
    for beams in (1, 4):
        ids = m.generate(px, max_length=12, num_beams=beams, early_stopping=False)
        assert m.decode_step_impl == "per-operation"
        assert ids.shape[0] == 3 and int(ids.min()) >= 0 and int(ids.max()) < c321.vocab
    c256 = _cfg("256-wide", dec_layers=2)
    m = TrOCRModel(c256.encoder_config_dict(), build_decoder_dir(str(tmp_path / "dec256"), c256), init_seed=6, load_tokenizer=False)
    m.eval()
    px = torch.from_numpy(synthetic_batch(c256, 3, 12, seed=1)[0]).cuda()
    ids = m.generate(px, max_length=12, num_beams=3, early_stopping=False)
    assert m.decode_step_impl == "per-operation"
    assert ids.shape[0] == 3 and int(ids.min()) >= 0 and int(ids.max()) < c256.vocab
    ids = m.generate(px, max_length=12, num_beams=4, early_stopping=False)
    assert m.decode_step_impl == "one-launch"
