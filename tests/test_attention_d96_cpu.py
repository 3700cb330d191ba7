"""Which attention kernels serve a call (kzv_attn_impl), checked on the CPU: the dispatch table of kzv_attn_fwd / kzv_attn_bwd,
its refusals with the launch's messages, and the encoder report of the Python surface.  Nothing is launched."""
import ctypes as C
import os

import pytest

from kzv import _lib as L
from kzv.config import ModelConfig, reference_cli_config, vit_b_config
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
    return lib.kzv_attn_impl(C.byref(a), int(bwd))


@pytest.mark.parametrize("bwd", [0, 1])
@pytest.mark.parametrize("sq,sk", [(1, 1), (16, 16), (37, 37), (257, 257), (288, 288), (60, 257), (257, 40)])
def test_head_dim_96_unmasked_takes_the_mfma96_kernels(lib, sq, sk, bwd):
    assert _impl(lib, _args(96, sq, sk), bwd) == L.ATTN_MFMA96


@pytest.mark.parametrize("bwd", [0, 1])
@pytest.mark.parametrize("head_dim", [0, 64])
@pytest.mark.parametrize("mode", [0, 1])
def test_head_dim_64_keeps_the_mfma64_kernels(lib, head_dim, mode, bwd):
    assert _impl(lib, _args(head_dim, 100, 100, mode=mode, heads=4), bwd) == L.ATTN_MFMA64


@pytest.mark.parametrize("bwd", [0, 1])
@pytest.mark.parametrize("head_dim,sq,sk", [(8, 40, 40), (32, 257, 257), (128, 257, 257), (96, 289, 289), (96, 40, 289),
                                             (96, 384, 384), (96, 300, 200)])
def test_other_geometries_stay_on_the_valu_kernel(lib, head_dim, sq, sk, bwd):
    assert _impl(lib, _args(head_dim, sq, sk), bwd) == L.ATTN_VALU


@pytest.mark.parametrize("bwd", [0, 1])
@pytest.mark.parametrize("head_dim,sk,mode,text", [
    (96, 100, 1, "causal / key-padding mode exists for head_dim 64 only"),
    (4, 100, 0, "head_dim must be a multiple of 8 in 8..128"),
    (96, 513, 0, "Sk must be in 1..512"),
    # the VALU kernel stages K and V of the head in LDS: 512 keys of 96 do not fit, as before
    (96, 512, 0, "do not fit the 160 KiB LDS"),
])
def test_refused_arguments_report_the_launch_error(lib, head_dim, sk, mode, text, bwd):
    rc = _impl(lib, _args(head_dim, 50, sk, mode=mode), bwd)
    assert rc == -1                                          # KZV_E_ARG
    assert text in lib.kzv_last_error().decode()


def test_null_operands_and_strides_are_refused(lib):
    a = _args(96, 257, 257)
    a.dQ = None
    assert _impl(lib, a, 0) == L.ATTN_MFMA96                 # the forward does not need it
    assert _impl(lib, a, 1) < 0 and "attn_bwd: null operand" in lib.kzv_last_error().decode()
    a = _args(96, 257, 257)
    a.ldo = 770
    assert _impl(lib, a, 0) < 0 and "row strides must be multiples of 8" in lib.kzv_last_error().decode()
    a = _args(0, 257, 257, heads=4)
    a.Q = None
    assert _impl(lib, a, 0) < 0 and "attn: null operand" in lib.kzv_last_error().decode()


def test_python_report_of_the_encoder(lib):
    ref = reference_cli_config()
    assert (ref.enc_hidden, ref.enc_heads, ref.image_h, ref.image_w, ref.enc_seq) == (768, 8, 1024, 64, 257)
    assert encoder_attention_impl(ref) == "mfma96"
    assert encoder_attention_impl(vit_b_config()) == "mfma64"
    assert encoder_attention_impl(ModelConfig(enc_hidden=768, enc_heads=6)) == "valu"      # head_dim 128
    assert L.attention_impl(96, 257, 257, heads=8, bwd=True) == "mfma96"
    with pytest.raises(L.KzvError, match="Sk must be in 1..512"):
        L.attention_impl(96, 600, 600, heads=8)
