"""kzv_decode_step_impl without a GPU: the query launches nothing, and before kzv_model_bind it is a state error, not an answer."""
import ctypes as C
import os

from kzv import _lib as L
from kzv.config import tiny_config


def test_decode_step_impl_before_bind_is_an_error():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = L.load()
    cfg = tiny_config()
    c = L.kzv_config(image_h=cfg.image_h, image_w=cfg.image_w, patch_h=cfg.patch_h, patch_w=cfg.patch_w, channels=cfg.channels,
                     enc_hidden=cfg.enc_hidden, enc_layers=cfg.enc_layers, enc_heads=cfg.enc_heads, enc_ffn=cfg.enc_ffn,
                     dec_hidden=cfg.dec_hidden, dec_layers=cfg.dec_layers, dec_heads=cfg.dec_heads, dec_ffn=cfg.dec_ffn,
                     vocab=cfg.vocab, max_pos=cfg.max_pos, type_vocab=cfg.type_vocab, pad_id=cfg.pad_id, ln_eps=1e-12)
    h = C.c_void_p()
    L.check(lib.kzv_model_create(C.byref(c), C.byref(h)), "create")
    try:
        assert lib.kzv_decode_step_impl(h) < 0
        assert b"decode_step_impl" in lib.kzv_last_error()
        assert lib.kzv_decode_step_impl(None) < 0
    finally:
        lib.kzv_model_destroy(h)
