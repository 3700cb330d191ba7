"""Generation from e4m3 decoder weights on the GPU (csrc/decode_fused.hip: decode_fused_kernel<G, NC, true>, quant_pack8_kernel).

Model A runs in e4m3 mode.  Model B is the same seed with load_state_dict(dequantised_decoder_weights(A.state_dict())) in the bf16
one-launch mode: the weights A's kernel multiplies with are q * 2^e, B's bf16 copies hold exactly those numbers, both kernels run the
same MFMAs in the same order and a power-of-two row scale commutes with every fp32 rounding -- so the logits are EQUAL, bit for bit,
and every comparison below is torch.equal.  If one fails, the accumulation order or a scale is wrong; a tolerance would hide that.
How far B is from the unquantised model is the recipe's business and is measured on the CPU (test_decode_e4m3_cpu.py)."""
import dataclasses

import numpy as np
import pytest
import torch

from _e4m3 import special_rows
from kzv import _lib as L
from kzv import quant as Q
from kzv.config import small_config, tiny_config
from kzv.data import build_decoder_dir, synthetic_batch
from kzv.model import TrOCRModel

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _default_mode_afterwards():
    yield
    L.load().kzv_set_decode_one_launch(-1)


def _wide(**kw):
    return dataclasses.replace(tiny_config(), dec_hidden=256, dec_heads=4, dec_ffn=768, **kw)


def _model(cfg, tmp_path, seed, **kw):
    d = build_decoder_dir(str(tmp_path / f"dec{cfg.dec_hidden}x{cfg.dec_layers}"), cfg)
    m = TrOCRModel(cfg.encoder_config_dict(), d, init_seed=seed, load_tokenizer=False, **kw)
    m.eval()
    return m


def _ab(cfg, tmp_path, seed):
    """A in e4m3 mode; B in bf16 mode on the weights A's mode is arithmetically equal to."""
    a = _model(cfg, tmp_path, seed, decode_weights="e4m3")
    b = _model(cfg, tmp_path, seed)
    b.load_state_dict(Q.dequantised_decoder_weights(a.state_dict()))
    assert a.decode_weights == "e4m3" and b.decode_weights == "bf16"
    return a, b


@pytest.mark.parametrize("N,K", [(768, 256), (256, 256), (256, 768)])
def test_quantiser_equals_the_recipe(N, K):
    lib = L.load()
    gen = torch.Generator().manual_seed(N + K)
    sp = special_rows(K, gen)
    w = torch.randn(N, K, generator=gen) * 10 ** torch.empty(N, 1).uniform_(-4, 2, generator=gen)
    w[5:5 + sp.shape[0]] = sp
    w16 = w.to(torch.bfloat16)
    q_ref, s_ref = Q.row_pow2_e4m3(w16)
    wd = w16.cuda()
    q = torch.full((N, K), 0x55, dtype=torch.uint8, device="cuda")
    s = torch.full((N,), -1.0, device="cuda")
    L.check(lib.kzv_quant_pack_e4m3(wd.data_ptr(), N, K, q.data_ptr(), s.data_ptr(), L.stream_handle()), "quant_pack_e4m3")
    torch.cuda.synchronize()
    assert torch.equal(s.cpu(), s_ref)
    bad = (q.cpu() != q_ref.view(torch.uint8)).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} bytes differ, first at {bad[0].tolist()}"
    assert lib.kzv_quant_pack_e4m3(wd.data_ptr(), N + 8, K, q.data_ptr(), s.data_ptr(), L.stream_handle()) < 0      # N % 16
    assert lib.kzv_quant_pack_e4m3(wd.data_ptr(), N, 32, q.data_ptr(), s.data_ptr(), L.stream_handle()) < 0         # K % 64


def _lockstep_equal(cfg, tmp_path, images, beams, Lh, reparent_every, seed):
    """Teacher-forced ids through kzv_decode_step on A and B (tests/test_decode_fused_gpu.py::_lockstep's schedule: rows that have
    ended, beam re-parenting inside an image's group); the live rows' logits must be equal at every step."""
    lib = L.load()
    cfg = dataclasses.replace(cfg, enc_hidden_dropout=0.0, enc_attn_dropout=0.0, dec_hidden_dropout=0.0, dec_attn_dropout=0.0)
    models = _ab(cfg, tmp_path, seed)
    BB = images * beams
    px, lab = synthetic_batch(cfg, BB, Lh, seed=seed, min_chars=2, max_chars=Lh - 2)
    ids = torch.from_numpy(lab).cuda()
    ids[:, 0] = cfg.bos_id
    pxt = torch.from_numpy(px[::beams].copy()).cuda()               # one crop per image
    L.check(lib.kzv_set_decode_one_launch(1), "mode")
    for m, want in zip(models, ("e4m3", "bf16")):
        m._bind(BB, Lh)
        L.check(lib.kzv_encode_images(m._h, pxt.data_ptr(), images, L.stream_handle()), "encode_images")
        L.check(lib.kzv_set_active_length(m._h, 1), "set_active_length")
        L.check(lib.kzv_decode_begin(m._h, L.stream_handle()), "decode_begin")
        assert m.decode_step_impl == "one-launch" and m.decode_weights_impl == want
    out = [torch.empty(BB, cfg.vocab, device="cuda") for _ in range(2)]
    valid = torch.zeros(BB, Lh, dtype=torch.uint8, device="cuda")
    posids = torch.empty(BB, dtype=torch.int32, device="cuda")
    rng = np.random.default_rng(seed)
    compared = 0
    for t in range(Lh - 1):
        if beams > 1 and t > 0 and t % reparent_every == 0:
            par = np.concatenate([g * beams + rng.integers(0, beams, size=beams) for g in range(images)])
            perm = torch.from_numpy(par).cuda()
            ids = ids[perm].contiguous(); valid = valid[perm].contiguous()
            for m in models:
                L.check(lib.kzv_decode_reorder(m._h, perm.data_ptr(), t, L.stream_handle()), "reorder")
        tok = ids[:, t].contiguous()
        live = tok != cfg.pad_id
        valid[:, t] = live.to(torch.uint8)
        posids.copy_(torch.where(live, torch.full_like(tok, t + 1 + cfg.pad_id), torch.full_like(tok, cfg.pad_id)).to(torch.int32))
        for m, o in zip(models, out):
            L.check(lib.kzv_decode_step(m._h, tok.data_ptr(), posids.data_ptr(), t, valid.data_ptr(), Lh, o.data_ptr(), L.stream_handle()), "step")
        torch.cuda.synchronize()
        if bool(live.any()):                                        # rows whose newest token is padding have no defined output
            a, b = out[0][live], out[1][live]
            assert bool(torch.isfinite(a).all()), t
            assert torch.equal(a, b), f"step {t}: {int((a != b).any(1).sum())} of {a.shape[0]} live rows differ, by up to {float((a - b).abs().max()):.3e}"
            compared += int(live.sum())
    assert compared > BB                                            # the comparison was not vacuous
    return compared


@pytest.mark.parametrize("beams", [1, 2, 4])
def test_e4m3_step_equals_the_bf16_step_on_the_dequantised_weights(tmp_path, beams):
    """3 layers: the window wraps across layer boundaries; 5 images x 4 rows: every G and the padding-row path."""
    _lockstep_equal(_wide(dec_layers=3), tmp_path, images=5, beams=beams, Lh=30, reparent_every=3, seed=21 + beams)


@pytest.mark.parametrize("beams", [4, 1])
def test_e4m3_step_at_the_kernels_limits(tmp_path, beams):
    """12 layers (the layer table's limit and the longest stream), 160 patch keys, 127 cached keys."""
    cfg = small_config()
    _lockstep_equal(cfg, tmp_path, images=3, beams=beams, Lh=cfg.max_pos - cfg.pad_id - 1, reparent_every=5, seed=5)


@pytest.mark.parametrize("beams", [4, 1])
def test_e4m3_step_in_the_chunked_instances(tmp_path, beams):
    """256 patch keys (64 x 1024 pixels in 16 x 16 patches): the instances with the online softmax, whose LDS the row scales add to."""
    cfg = _wide(image_h=64, image_w=1024, enc_layers=1, dec_layers=2)
    assert cfg.num_patches == 256
    _lockstep_equal(cfg, tmp_path, images=3, beams=beams, Lh=20, reparent_every=3, seed=9)


def test_generate_end_to_end_and_format_switches(tmp_path):
    """generate with the default graph replay: A equals B token for token, greedy and beam-4; bf16 -> e4m3 -> bf16 on one model
    returns to the first result (a graph captured in one format is not replayed in the other); after load_state_dict the e4m3
    copies are refreshed."""
    cfg = _wide()
    a, b = _ab(cfg, tmp_path, 3)
    px = torch.from_numpy(synthetic_batch(cfg, 6, 20, seed=8)[0]).cuda()
    for beams in (1, 4):
        kw = dict(max_length=20, num_beams=beams, early_stopping=False)
        got_a = a.generate(px, **kw)
        assert a.decode_step_impl == "one-launch" and a.decode_weights_impl == "e4m3"
        got_b = b.generate(px, **kw)
        assert b.decode_weights_impl == "bf16"
        assert torch.equal(got_a, got_b), beams
        a.set_decode_weights("bf16")
        plain = a.generate(px, **kw)
        assert a.decode_weights_impl == "bf16"
        a.set_decode_weights("e4m3")
        assert torch.equal(a.generate(px, **kw), got_a)
        a.set_decode_weights("bf16")
        assert torch.equal(a.generate(px, **kw), plain)
        a.set_decode_weights("e4m3")
    # other weights: A's copies must follow them
    other = _model(cfg, tmp_path, 11)
    a.load_state_dict(other.state_dict())
    b2 = _model(cfg, tmp_path, 11)
    b2.load_state_dict(Q.dequantised_decoder_weights(other.state_dict()))
    for beams in (1, 4):
        kw = dict(max_length=20, num_beams=beams, early_stopping=False)
        assert torch.equal(a.generate(px, **kw), b2.generate(px, **kw)), beams
    assert a.decode_weights_impl == "e4m3"


def test_e4m3_generation_with_more_images_than_compute_units(tmp_path):
    """600 images in one call (600 workgroups, two rounds, slower loads) against six calls of 100: token for token.  The guard
    tests/test_decode_fused_gpu.py has for the bf16 stream's refills, on the e4m3 stream's."""
    cfg = _wide(dec_layers=6)
    m = _model(cfg, tmp_path, 4, decode_weights="e4m3")
    px = torch.from_numpy(synthetic_batch(cfg, 600, 20, seed=3)[0]).cuda()
    for beams in (1, 4):
        whole = m.generate(px, max_length=24, num_beams=beams)
        assert m.decode_weights_impl == "e4m3"
        parts = torch.cat([m.generate(px[i:i + 100], max_length=24, num_beams=beams) for i in range(0, 600, 100)])
        assert whole.shape == parts.shape and torch.equal(whole, parts), f"beams {beams}: {int((whole != parts).any(1).sum())} sequences differ"


def test_geometries_without_an_e4m3_path_keep_bf16(tmp_path):
    """The stock 64-wide decoder, and 3 rows per image at 256-wide: e4m3 asked for, bf16 read, results equal to the bf16 mode's."""
    for cfg, beams in ((tiny_config(), 1), (tiny_config(), 4), (_wide(), 3)):
        m = _model(cfg, tmp_path, 3)
        px = torch.from_numpy(synthetic_batch(cfg, 6, 20, seed=8)[0]).cuda()
        kw = dict(max_length=20, num_beams=beams, early_stopping=False)
        plain = m.generate(px, **kw)
        m.set_decode_weights("e4m3")
        got = m.generate(px, **kw)
        assert m.decode_weights == "e4m3" and m.decode_weights_impl == "bf16" and m.decode_step_impl == "per-operation"
        assert torch.equal(got, plain), (cfg.dec_hidden, beams)
