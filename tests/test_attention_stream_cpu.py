"""Long sequences on the CPU: the dispatch table of kzv_attn_impl_ex (which kernels a KZV_MODEL_LONG_SEQ model runs), the geometry
checks of kzv_model_create_ex, and a workspace that does not grow with S^2.  Nothing is launched."""
import ctypes as C
import dataclasses
import os

import pytest

from kzv import _lib as L
from kzv.config import ModelConfig, reference_cli_config, tiny_config, vit_b_config
from kzv.model import encoder_attention_impl


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load()


def _args(head_dim, Sq, Sk, mode=0, heads=8):
    a = L.kzv_attn_args()
    a.Q = a.K = a.V = a.O = a.LSE = a.dO = a.dQ = a.dK = a.dV = 16
    width = heads * (head_dim or 64)
    a.ldq = a.ldk = a.ldv = 3 * width
    a.ldo = width
    a.ids = 16
    a.ld_ids = Sk
    a.B, a.heads, a.Sq, a.Sk, a.mode, a.head_dim = 2, heads, Sq, Sk, mode, head_dim
    return a


def _impl(lib, a, bwd):
    rc = lib.kzv_attn_impl(C.byref(a), int(bwd))
    return rc, (lib.kzv_last_error().decode() if rc < 0 else "")


def _impl_ex(lib, a, bwd, flags=L.MODEL_LONG_SEQ):
    rc = lib.kzv_attn_impl_ex(C.byref(a), int(bwd), flags)
    return rc, (lib.kzv_last_error().decode() if rc < 0 else "")


LONG = [289, 385, 513, 1025, 4097]


@pytest.mark.parametrize("bwd", [0, 1])
@pytest.mark.parametrize("head_dim", [0, 64, 96])
@pytest.mark.parametrize("sk", LONG)
def test_long_keys_take_the_stream_kernels(lib, head_dim, sk, bwd):
    want = L.ATTN_STREAM96 if head_dim == 96 else L.ATTN_STREAM64
    assert _impl_ex(lib, _args(head_dim, sk, sk), bwd) == (want, "")
    assert _impl_ex(lib, _args(head_dim, 100, sk), bwd) == (want, "")      # cross-attention shape: few queries, many keys
    assert _impl_ex(lib, _args(head_dim, sk, 40), bwd) == (want, "")       # and the other way round


@pytest.mark.parametrize("bwd", [0, 1])
@pytest.mark.parametrize("head_dim", [0, 64, 96, 32, 128])
@pytest.mark.parametrize("sq,sk,mode", [(1, 1, 0), (37, 37, 0), (257, 257, 0), (288, 288, 0), (60, 257, 0), (100, 100, 1),
                                         (192, 192, 1), (300, 300, 1)])
def test_short_or_masked_calls_get_the_old_answer(lib, head_dim, sq, sk, mode, bwd):
    assert _impl_ex(lib, _args(head_dim, sq, sk, mode=mode), bwd) == _impl(lib, _args(head_dim, sq, sk, mode=mode), bwd)


@pytest.mark.parametrize("bwd", [0, 1])
@pytest.mark.parametrize("head_dim", [0, 64, 96])
def test_beyond_4097_is_refused(lib, head_dim, bwd):
    for sq, sk in [(4098, 4098), (100, 4098), (4098, 100)]:
        rc, msg = _impl_ex(lib, _args(head_dim, sq, sk), bwd)
        assert rc == -1 and "Sq/Sk must be in 1..4097" in msg


@pytest.mark.parametrize("bwd", [0, 1])
def test_other_head_dims_keep_their_limits(lib, bwd):
    rc, msg = _impl_ex(lib, _args(128, 50, 513), bwd)
    assert rc == -1 and "Sk must be in 1..512" in msg
    assert _impl_ex(lib, _args(32, 385, 385), bwd) == _impl(lib, _args(32, 385, 385), bwd)


@pytest.mark.parametrize("bwd", [0, 1])
@pytest.mark.parametrize("head_dim", [0, 64, 96, 32, 128])
@pytest.mark.parametrize("sq,sk", [(s, s) for s in LONG] + [(4098, 4098), (127, 1024), (513, 40)])
def test_without_the_flag_nothing_changes(lib, head_dim, sq, sk, bwd):
    assert _impl_ex(lib, _args(head_dim, sq, sk), bwd, flags=0) == _impl(lib, _args(head_dim, sq, sk), bwd)


def test_stream_entry_points_refuse_what_they_cannot_run(lib):
    a = _args(128, 513, 513)
    assert lib.kzv_attn_stream_fwd(C.byref(a), None) == -1 and "head_dim must be 64 or 96" in lib.kzv_last_error().decode()
    a = _args(64, 100, 100, mode=1)
    assert lib.kzv_attn_stream_fwd(C.byref(a), None) == -1 and "only mode 0" in lib.kzv_last_error().decode()
    a = _args(96, 100, 4098)
    assert lib.kzv_attn_stream_bwd(C.byref(a), None) == -1 and "1..4097" in lib.kzv_last_error().decode()
    a = _args(64, 1025, 1025)
    a.dK = None
    assert lib.kzv_attn_stream_bwd(C.byref(a), None) == -1 and "null gradient operand" in lib.kzv_last_error().decode()


def test_python_reports_the_stream_names(lib):
    assert L.attention_impl(96, 385, 385, heads=8, long_sequences=True) == "stream96"
    assert L.attention_impl(64, 1025, 1025, heads=12, bwd=True, long_sequences=True) == "stream64"
    assert L.attention_impl(96, 385, 385, heads=8) == "valu"
    # the benchmark geometry is untouched by the flag
    assert encoder_attention_impl(vit_b_config(), long_sequences=True) == "mfma64"
    assert encoder_attention_impl(reference_cli_config(), long_sequences=True) == "mfma96"
    long96 = dataclasses.replace(reference_cli_config(), image_h=2048)
    assert encoder_attention_impl(long96, long_sequences=True) == "stream96"
    with pytest.raises(L.KzvError, match="Sk must be in 1..512"):
        encoder_attention_impl(long96)


def _ccfg(c: ModelConfig):
    return L.kzv_config(image_h=c.image_h, image_w=c.image_w, patch_h=c.patch_h, patch_w=c.patch_w, channels=c.channels,
                        enc_hidden=c.enc_hidden, enc_layers=c.enc_layers, enc_heads=c.enc_heads, enc_ffn=c.enc_ffn,
                        dec_hidden=c.dec_hidden, dec_layers=c.dec_layers, dec_heads=c.dec_heads, dec_ffn=c.dec_ffn,
                        vocab=c.vocab, max_pos=c.max_pos, type_vocab=c.type_vocab, pad_id=c.pad_id,
                        enc_hidden_dropout=c.enc_hidden_dropout, enc_attn_dropout=c.enc_attn_dropout,
                        dec_hidden_dropout=c.dec_hidden_dropout, dec_attn_dropout=c.dec_attn_dropout, ln_eps=c.ln_eps)


def _create(lib, c: ModelConfig, flags):
    h = C.c_void_p()
    rc = lib.kzv_model_create_ex(C.byref(_ccfg(c)), flags, C.byref(h))
    return rc, h, (lib.kzv_last_error().decode() if rc else "")


def _long(hd, h=2048, w=64, **kw):
    return dataclasses.replace(reference_cli_config(), image_h=h, image_w=w, enc_hidden=8 * hd, enc_layers=1, dec_layers=1, **kw)


@pytest.mark.parametrize("hd", [64, 96])
def test_model_create_ex_accepts_long_columns(lib, hd):
    c = _long(hd)
    assert c.enc_seq == 513
    rc, h, msg = _create(lib, c, L.MODEL_LONG_SEQ)
    assert rc == 0, msg
    assert lib.kzv_workspace_bytes(h, 4, 16) > 0
    lib.kzv_model_destroy(h)
    c.validate(long_sequences=True)
    # the same geometry without the flag: today's refusal
    rc, h, msg = _create(lib, c, 0)
    assert rc == -1 and "288-token" in msg
    h = C.c_void_p()
    assert lib.kzv_model_create(C.byref(_ccfg(c)), C.byref(h)) == -1
    assert "exceed the 288-token attention kernels" in lib.kzv_last_error().decode()


def test_model_create_ex_tiny_and_refusals(lib):
    tiny = dataclasses.replace(tiny_config(), image_h=1024, image_w=80)
    assert tiny.enc_seq == 321
    rc, h, msg = _create(lib, tiny, L.MODEL_LONG_SEQ)
    assert rc == 0, msg
    lib.kzv_model_destroy(h)
    hd32 = dataclasses.replace(tiny, enc_heads=4)         # head_dim 32 at 321 tokens: no streaming kernel
    rc, h, msg = _create(lib, hd32, L.MODEL_LONG_SEQ)
    assert rc == -1 and "288-token" in msg and "64 and 96 only" in msg
    with pytest.raises(ValueError, match="64 and 96 only"):
        hd32.validate(long_sequences=True)
    hd32.validate()                                        # the default keeps today's checks
    big = _long(64, h=4096, w=80, patch_h=8, patch_w=8)   # 5,120 patches
    rc, h, msg = _create(lib, big, L.MODEL_LONG_SEQ)
    assert rc == -1 and "4,097-token" in msg
    rc, h, msg = _create(lib, tiny_config(), 2)
    assert rc == -1 and "unknown flags" in msg


def test_bind_refuses_more_dropout_blocks_than_the_32_bit_block_word(lib):
    """kzv_model_bind of a long-sequence model refuses a batch whose attention-dropout block index B * heads * ceil(S / 4)^2 would
    pass 2^32 (the masks would repeat); the check runs before any device work, so fake 256-byte-aligned pointers reach it.  At
    1,025 tokens and 16 heads: 257^2 * 16 * 4,000 < 2^32 < 257^2 * 16 * 8,000."""
    c = _long(64, h=1024, w=64, patch_h=8, patch_w=8)
    c = dataclasses.replace(c, enc_hidden=1024, enc_heads=16, enc_ffn=64)
    assert c.enc_seq == 1025
    rc, h, msg = _create(lib, c, L.MODEL_LONG_SEQ)
    assert rc == 0, msg
    fake = C.c_void_p(1 << 20)
    try:
        assert lib.kzv_model_bind(h, fake, fake, fake, C.c_int64(1 << 40), 8000, 16) == -1
        assert "2^32 attention-dropout blocks" in lib.kzv_last_error().decode()
        # half the batch passes that check and stops at the next one (no workspace of that size was given)
        assert lib.kzv_model_bind(h, fake, fake, fake, C.c_int64(256), 4000, 16) == -1
        assert "workspace" in lib.kzv_last_error().decode()
    finally:
        lib.kzv_model_destroy(h)


def test_workspace_has_no_s_squared_term(lib):
    """Workspace bytes at 513, 1,025 and 1,537 tokens: every buffer is linear in the token count, so the step from 513 to 1,025
    tokens equals the step from 1,025 to 1,537 (an S^2 buffer would make the second 1.5 times the first) up to the 256-byte
    alignment of each buffer."""
    def ws(h_img):
        c = _long(64, h=h_img, w=64, patch_h=8, patch_w=8)   # (h / 8) * 8 patches + CLS
        rc, h, msg = _create(lib, c, L.MODEL_LONG_SEQ)
        assert rc == 0, msg
        n = lib.kzv_workspace_bytes(h, 8, 32)
        lib.kzv_model_destroy(h)
        return c.enc_seq, n
    s1, w1 = ws(512)
    s2, w2 = ws(1024)
    s3, w3 = ws(1536)
    assert (s1, s2, s3) == (513, 1025, 1537)
    d1, d2 = w2 - w1, w3 - w2
    assert d1 > 0 and abs(d2 - d1) <= 64 * 1024, (w1, w2, w3)
    assert w2 < 2.1 * w1
