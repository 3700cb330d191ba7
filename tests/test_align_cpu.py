"""CPU side of per-character confidence and position: the four new symbols of include/kzv.h are exported and bound, the two
handle calls refuse an unbound handle without touching a GPU, and kzv/align.py turns padded per-position arrays + ids into
records (the shift by one, EOS in the confidence but not in the text, PAD rows dropped, patch -> pixel, empty generations)."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from kzv import _lib as L
from kzv import align as A
from kzv.config import tiny_config

PAD, BOS, EOS = 1, 0, 2


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load()


def test_the_four_symbols_are_exported_and_bound(lib):
    for name in ("kzv_attn_probs", "kzv_token_scores", "kzv_cross_attention", "kzv_score_tokens"):
        assert name in L.SYMBOLS, name
        assert getattr(lib, name).restype is C.c_int
    # the argument block of kzv_attn_probs: the header's fields in the header's order
    assert [f[0] for f in L.kzv_attn_probs_args._fields_] == ["Q", "K", "ldq", "ldk", "LSE", "map", "ld_map", "pos", "peak",
                                                             "B", "heads", "Sq", "Sk", "grid_w", "head_dim", "mode"]
    assert C.sizeof(L.kzv_attn_probs_args) == 9 * 8 + 7 * 4 + 4          # nine 8-byte fields, seven int32, tail padding


def test_handle_calls_refuse_an_unbound_handle_with_a_message(lib):
    cfg = tiny_config()
    c = L.kzv_config(image_h=cfg.image_h, image_w=cfg.image_w, patch_h=cfg.patch_h, patch_w=cfg.patch_w, channels=cfg.channels,
                     enc_hidden=cfg.enc_hidden, enc_layers=cfg.enc_layers, enc_heads=cfg.enc_heads, enc_ffn=cfg.enc_ffn,
                     dec_hidden=cfg.dec_hidden, dec_layers=cfg.dec_layers, dec_heads=cfg.dec_heads, dec_ffn=cfg.dec_ffn,
                     vocab=cfg.vocab, max_pos=cfg.max_pos, type_vocab=cfg.type_vocab, pad_id=cfg.pad_id, ln_eps=1e-12)
    h = C.c_void_p()
    L.check(lib.kzv_model_create(C.byref(c), C.byref(h)), "create")
    try:
        assert lib.kzv_cross_attention(h, -1, None, 0, None, None, None) == -3          # KZV_E_STATE
        assert b"cross_attention" in lib.kzv_last_error()
        assert lib.kzv_score_tokens(h, None, None, None, None) == -3
        assert b"score_tokens" in lib.kzv_last_error()
        with pytest.raises(L.KzvError, match="score_tokens"):
            L.check(lib.kzv_score_tokens(h, None, None, None, None), "kzv_score_tokens")
    finally:
        lib.kzv_model_destroy(h)


def test_per_op_entry_points_refuse_bad_arguments_before_any_launch(lib):
    a = L.kzv_attn_probs_args()
    assert lib.kzv_attn_probs(C.byref(a), None) == -1 and b"null operand" in lib.kzv_last_error()
    a.Q = a.K = a.LSE = 4096          # never dereferenced: every refusal below comes before the launch
    a.ldq = a.ldk = 64
    a.B, a.heads, a.Sq, a.Sk, a.grid_w = 1, 1, 16, 16, 4
    for field, value, msg in (("mode", 1, b"mode 0"), ("head_dim", 96, b"head_dim"), ("Sq", 289, b"1..288"), ("Sk", 4098, b"1..4097"),
                              ("heads", 0, b"positive"), ("ldk", 60, b"multiples of 8")):
        old = getattr(a, field)
        setattr(a, field, value)
        assert lib.kzv_attn_probs(C.byref(a), None) == -1, field
        assert msg in lib.kzv_last_error(), (field, lib.kzv_last_error())
        setattr(a, field, old)
    assert lib.kzv_token_scores(None, 8, None, 2, 1, 1, 8, 1, None, None, None, None) == -1


def _arrays(ids, lp=None):
    ids = np.asarray(ids)
    B, Lh = ids.shape
    lp = np.full((B, Lh - 1), -0.25) if lp is None else np.asarray(lp, dtype=np.float64)
    t = np.arange(Lh - 1, dtype=np.float64)
    cen = np.broadcast_to(np.stack((100.0 + t, 200.0 + t), axis=-1), (B, Lh - 1, 2)).copy()
    peak = np.broadcast_to(10 + np.arange(Lh - 1), (B, Lh - 1)).copy()
    return ids, lp, cen, peak


def test_row_t_belongs_to_token_t_plus_one():
    ids, lp, cen, peak = _arrays([[BOS, 7, 8, 9, EOS, PAD]], [[-0.1, -0.2, -0.3, -0.4, -9.0]])
    (r,) = A.build_records(ids, lp, cen, peak, pad_id=PAD, bos_id=BOS, eos_id=EOS)
    assert r["tokens"] == [7, 8, 9]
    assert r["logprobs"] == [-0.1, -0.2, -0.3]                       # row 0 scores token 1 (the first after BOS), ...
    assert r["centroids"] == [(100.0, 200.0), (101.0, 201.0), (102.0, 202.0)]
    assert r["peak_patches"] == [10, 11, 12]


def test_eos_counts_in_the_confidence_but_not_in_the_text_and_pad_rows_are_dropped():
    ids, lp, cen, peak = _arrays([[BOS, 7, 8, EOS, PAD, PAD], [BOS, 5, EOS, PAD, PAD, PAD]],
                                 [[-0.1, -0.2, -0.6, -50.0, -50.0], [-1.0, -2.0, -50.0, -50.0, -50.0]])
    texts = ["ab", "c"]
    rec = A.build_records(ids, lp, cen, peak, pad_id=PAD, bos_id=BOS, eos_id=EOS, texts=texts, to_strings=lambda t: [f"<{i}>" for i in t])
    assert [r["text"] for r in rec] == texts
    assert rec[0]["tokens"] == [7, 8] and rec[0]["token_strings"] == ["<7>", "<8>"] and EOS not in rec[0]["tokens"]
    assert rec[0]["logprobs"] == [-0.1, -0.2]                                         # the EOS row is not a character ...
    assert rec[0]["confidence"] == pytest.approx(math.exp((-0.1 - 0.2 - 0.6) / 3))    # ... but it is in the confidence; -50 rows are not
    assert rec[1]["tokens"] == [5] and rec[1]["confidence"] == pytest.approx(math.exp(-1.5))
    assert all(len(r["tokens"]) == len(r["centroids"]) == len(r["peak_patches"]) == len(r["logprobs"]) for r in rec)
    # a sequence that ran into the length limit has no EOS: the mean is over its tokens alone
    ids2, lp2, cen2, peak2 = _arrays([[BOS, 7, 8, 9]], [[-0.3, -0.3, -0.9]])
    (r,) = A.build_records(ids2, lp2, cen2, peak2, pad_id=PAD, bos_id=BOS, eos_id=EOS)
    assert r["tokens"] == [7, 8, 9] and r["confidence"] == pytest.approx(math.exp(-0.5))


def test_an_empty_generation_gives_empty_lists():
    ids, lp, cen, peak = _arrays([[BOS, EOS, PAD, PAD], [BOS, PAD, PAD, PAD]], [[-0.7, -50.0, -50.0], [-50.0, -50.0, -50.0]])
    rec = A.build_records(ids, lp, cen, peak, pad_id=PAD, bos_id=BOS, eos_id=EOS, texts=["", ""], to_strings=lambda t: [str(i) for i in t])
    for r in rec:
        assert r["tokens"] == [] and r["token_strings"] == [] and r["logprobs"] == [] and r["centroids"] == [] and r["peak_patches"] == []
        assert r["text"] == ""
    assert rec[0]["confidence"] == pytest.approx(math.exp(-0.7))          # BOS, EOS: the EOS's own probability
    assert rec[1]["confidence"] == 0.0                                    # nothing was scored
    with pytest.raises(ValueError):
        A.build_records(ids, lp[:, :2], cen, peak, pad_id=PAD, bos_id=BOS, eos_id=EOS)


@pytest.mark.parametrize("ph,pw", [(16, 16), (8, 8)])
def test_patch_to_pixel_gives_patch_centres(ph, pw):
    rc = np.array([[0.0, 0.0], [1.0, 3.0], [0.5, 2.25]])
    want = np.array([[0.5 * ph, 0.5 * pw], [1.5 * ph, 3.5 * pw], [1.0 * ph, 2.75 * pw]])
    assert np.array_equal(A.patch_to_pixel(rc, ph, pw), want)
    assert np.array_equal(A.patch_to_pixel(torch.from_numpy(rc), ph, pw).numpy(), want)
    grid_w = 40
    assert A.peak_to_pixel(0, grid_w, ph, pw) == (0.5 * ph, 0.5 * pw)
    assert A.peak_to_pixel(grid_w + 3, grid_w, ph, pw) == (1.5 * ph, 3.5 * pw)      # second patch row, fourth column


def test_live_mask_stats_and_padding_helpers():
    ids = torch.tensor([[BOS, 7, EOS, PAD], [BOS, 7, 8, EOS]])
    assert A.live_mask(ids, PAD).tolist() == [[True, True, False], [True, True, True]]
    assert A.live_mask(ids.numpy(), PAD).tolist() == [[True, True, False], [True, True, True]]
    amap = torch.zeros(1, 2, 8)
    amap[0, 0, 5] = 0.75; amap[0, 0, 2] = 0.25                    # grid 2 x 4: patch 5 = (1, 1), patch 2 = (0, 2)
    amap[0, 1, 3] = 0.5; amap[0, 1, 6] = 0.5                      # a tie: the FIRST maximum wins
    pos, peak = A.stats_from_map(amap, 4)
    assert peak.tolist() == [[5, 3]] and peak.dtype == torch.int32
    assert torch.allclose(pos[0, 0], torch.tensor([0.75, 0.75 * 1 + 0.25 * 2, 0.75, 1.0]))
    assert torch.allclose(pos[0, 1], torch.tensor([0.5, 0.5 * 3 + 0.5 * 2, 0.5, 1.0]))
    x = torch.ones(2, 3, 2)
    y = A.pad_rows(x, 5, 7)
    assert y.shape == (2, 5, 2) and bool((y[:, :3] == 1).all()) and bool((y[:, 3:] == 7).all()) and A.pad_rows(x, 3) is x
