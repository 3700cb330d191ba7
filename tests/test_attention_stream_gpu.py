"""The K/V-streaming attention kernels (csrc/attention_stream.hip) against float64 references at the op level, against the
whole-head kernels at <= 288 tokens, at the model's strides at scale (B = 64 x 8 heads x 513 tokens), and run to run.  Cases
beyond 288 tokens assert that kzv_attn_impl_ex sends them to the streaming kernels; shorter ones call kzv_attn_stream_fwd / _bwd,
which run nothing else.  The unit checkers and their bounds are those of test_bench_geometry_gpu.py."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from kzv import _lib as L
from test_bench_geometry_gpu import _assert_flags, _attn_compare, _check_all

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    return L.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _args(v, g, drop, key, O=None, LSE=None):
    return L.kzv_attn_args(Q=v["Q"].data_ptr(), K=v["K"].data_ptr(), V=v["V"].data_ptr(), O=(O if O is not None else v["O"]).data_ptr(),
                           LSE=(LSE if LSE is not None else v["LSE"]).data_ptr(),
                           dO=v["dO"].data_ptr(), dQ=v["dQ"].data_ptr(), dK=v["dK"].data_ptr(), dV=v["dV"].data_ptr(),
                           ldq=v["ldq"], ldk=v["ldk"], ldv=v["ldk"], ldo=v["ldo"], B=g.B, heads=g.heads, Sq=g.Sq, Sk=g.Sk, mode=0,
                           drop_p=drop, drop_key=key, head_dim=g.D)


def _operands(D, B, heads, Sq, Sk, gen, packed, scale=1.0):
    """packed: Q, K, V as column blocks of one [B * S, 3 * heads * D] buffer (model.cpp's encoder layout, Sq == Sk); otherwise
    separate buffers with padded row strides.  Returns (views, buffers to NaN-fill, geometry)."""
    H = heads * D
    rnd = lambda *s: (torch.randn(*s, device=DEV, generator=gen) * scale).bfloat16()
    if packed:
        qkv = rnd(B * Sq, 3 * H)
        dqkv = torch.empty_like(qkv)
        v = dict(Q=qkv[:, :H], K=qkv[:, H:2 * H], V=qkv[:, 2 * H:], dQ=dqkv[:, :H], dK=dqkv[:, H:2 * H], dV=dqkv[:, 2 * H:],
                 ldq=3 * H, ldk=3 * H, ldo=H)
        owned = [dqkv]
    else:
        q, kv = rnd(B * Sq, H + 8), rnd(B * Sk, 2 * H + 16)
        dq, dkv = torch.empty_like(q), torch.empty_like(kv)
        v = dict(Q=q[:, :H], K=kv[:, :H], V=kv[:, H + 8:2 * H + 8], dQ=dq[:, :H], dK=dkv[:, :H], dV=dkv[:, H + 8:2 * H + 8],
                 ldq=H + 8, ldk=2 * H + 16, ldo=H + 8)
        owned = [dq, dkv]
    v["O"] = torch.empty(B * Sq, v["ldo"], dtype=torch.bfloat16, device=DEV)
    v["dO"] = torch.randn(B * Sq, v["ldo"], device=DEV, generator=gen).bfloat16()
    v["LSE"] = torch.empty(B, heads, Sq, device=DEV)
    owned += [v["O"], v["LSE"]]
    return v, owned, types.SimpleNamespace(B=B, heads=heads, Sq=Sq, Sk=Sk, H=H, D=D)


def _heads(t, g, S):
    return t[:, :g.H].reshape(g.B, S, g.heads, g.D).transpose(1, 2)       # [B, heads, S, D]: unit = (b, h)


def _outputs(v, g):
    return {"O": _heads(v["O"], g, g.Sq).clone(), "LSE": v["LSE"].clone(), "dQ": _heads(v["dQ"], g, g.Sq).clone(),
            "dK": _heads(v["dK"], g, g.Sk).clone(), "dV": _heads(v["dV"], g, g.Sk).clone()}


def _run_stream(lib, v, owned, g, drop, key):
    for t in owned:
        t.fill_(NAN)
    a = _args(v, g, drop, key)
    if max(g.Sq, g.Sk) > 288:
        want = L.ATTN_STREAM96 if g.D == 96 else L.ATTN_STREAM64
        assert lib.kzv_attn_impl_ex(C.byref(a), 0, L.MODEL_LONG_SEQ) == want
        assert lib.kzv_attn_impl_ex(C.byref(a), 1, L.MODEL_LONG_SEQ) == want
    L.check(lib.kzv_attn_stream_fwd(C.byref(a), _st()), "attn_stream_fwd")
    L.check(lib.kzv_attn_stream_bwd(C.byref(a), _st()), "attn_stream_bwd")
    torch.cuda.synchronize()
    return _outputs(v, g)


def _mask(lib, g, drop, key):
    m = torch.empty(g.B * g.heads * g.Sq, g.Sk, device=DEV)
    L.check(lib.kzv_debug_attn_dropout_mask(key, drop, g.B * g.heads, g.Sq, g.Sk, m.data_ptr(), _st()), "mask")
    return m.view(g.B, g.heads, g.Sq, g.Sk)


def _ref(lib, v, g, drop, key):
    """float64 softmax(q k^T D^-0.5) [x the dropout multipliers kzv_debug_attn_dropout_mask reports] v and its gradients."""
    qh, kh, vh = (_heads(v[k], g, S).double().requires_grad_(True) for k, S in (("Q", g.Sq), ("K", g.Sk), ("V", g.Sk)))
    s = qh @ kh.transpose(2, 3) * (1.0 / np.sqrt(g.D))
    p = torch.softmax(s, -1)
    if drop > 0:
        p = p * _mask(lib, g, drop, key).double()
    o = p @ vh
    dq, dk, dv = torch.autograd.grad(o, (qh, kh, vh), _heads(v["dO"], g, g.Sq).double())
    return {"O": o.detach(), "LSE": torch.logsumexp(s.detach(), -1), "dQ": dq, "dK": dk, "dV": dv}


# ------------------------------------------------------------------------------------------------ 1. op level
OP_CASES = [(3, 2, 1, 1), (3, 2, 37, 37), (2, 2, 257, 257), (2, 2, 289, 289), (2, 2, 385, 385), (2, 2, 513, 513),
            (1, 2, 1025, 1025), (1, 1, 2049, 2049), (1, 1, 4097, 4097), (2, 2, 127, 1024), (2, 2, 60, 513), (2, 2, 513, 40)]


@pytest.mark.parametrize("drop", [0.0, 0.1, 0.25])
@pytest.mark.parametrize("B,heads,Sq,Sk", OP_CASES)
@pytest.mark.parametrize("D", [64, 96])
def test_attention_stream_fwd_bwd(lib, D, B, heads, Sq, Sk, drop):
    """One key, partial key blocks, one to 65 blocks of 64 keys (4,097 = the upper bound: the dK / dV kernel's largest LDS, its
    LSE / delta rows of every query), Sq != Sk both ways (cross-attention: 127 queries over 1,024
    keys), padded row strides, dropout off / 0.1 / 0.25 on the masks kzv_debug_attn_dropout_mask reports.  The bounds of
    _attn_compare are kept as they stand at every length: the bf16 roundings of P and of the outputs are relative (2^-8) and
    the softmax weights sum to 1 whatever the key count, so the error of O stays a fraction of the unit's largest |V|."""
    gen = torch.Generator(device=DEV)
    gen.manual_seed(31 * Sq + Sk + D)
    v, owned, g = _operands(D, B, heads, Sq, Sk, gen, packed=False)
    key = 777 + Sq + 3 * Sk
    ref = _ref(lib, v, g, drop, key)
    _check_all(f"stream d{D} B={B} h={heads} Sq={Sq} Sk={Sk} p={drop}", _attn_compare(_run_stream(lib, v, owned, g, drop, key), ref))


# ------------------------------------------------------------------------------------------------ 2. against the whole-head kernels
def _whole(lib, v, g, drop, key, LSE=None, fwd=True):
    a = _args(v, g, drop, key, LSE=LSE)
    assert lib.kzv_attn_impl(C.byref(a), 0) == (L.ATTN_MFMA96 if g.D == 96 else L.ATTN_MFMA64)
    if fwd:
        L.check(lib.kzv_attn_fwd(C.byref(a), _st()), "attn_fwd")
    L.check(lib.kzv_attn_bwd(C.byref(a), _st()), "attn_bwd")
    torch.cuda.synchronize()


@pytest.mark.parametrize("D,Sq,Sk", [(64, 100, 60), (64, 257, 64), (96, 257, 96), (96, 37, 80)])
def test_dropout_zeros_match_the_whole_head_kernels(lib, D, Sq, Sk):
    """V = one-hot rows (key k -> column k; Sk <= head_dim), so O[q, k] = P(q, k) * keep(q, k) / P(keep): the zeros of O are the
    dropped probabilities.  Streaming and whole-head forwards drop exactly the same elements, and those are the zeros of
    kzv_debug_attn_dropout_mask (small scores: no probability rounds to zero)."""
    gen = torch.Generator(device=DEV)
    gen.manual_seed(Sq + Sk)
    v, owned, g = _operands(D, 2, 3, Sq, Sk, gen, packed=False, scale=0.3)
    vh = _heads(v["V"], g, Sk)
    vh.zero_()
    for k in range(Sk):
        vh[:, :, k, k] = 1.0
    drop, key = 0.25, 4242 + Sq
    a = _args(v, g, drop, key)
    v["O"].fill_(NAN)
    L.check(lib.kzv_attn_stream_fwd(C.byref(a), _st()), "attn_stream_fwd")
    torch.cuda.synchronize()
    o_stream = _heads(v["O"], g, Sq)[..., :Sk].clone()
    v["O"].fill_(NAN)
    L.check(lib.kzv_attn_fwd(C.byref(a), _st()), "attn_fwd")
    torch.cuda.synchronize()
    o_whole = _heads(v["O"], g, Sq)[..., :Sk].clone()
    keep = _mask(lib, g, drop, key) != 0
    assert torch.isfinite(o_stream).all() and torch.isfinite(o_whole).all()
    assert torch.equal(o_stream != 0, keep)
    assert torch.equal(o_whole != 0, keep)
    assert 0.2 < 1.0 - keep.float().mean().item() < 0.3


@pytest.mark.parametrize("drop", [0.0, 0.1])
@pytest.mark.parametrize("D,Sq,Sk", [(64, 257, 257), (64, 160, 161), (96, 257, 257), (96, 60, 288)])
def test_stream_agrees_with_the_whole_head_kernels(lib, D, Sq, Sk, drop):
    """At <= 288 tokens: streaming O within bf16 rounding of the whole-head O (2^-7 of the unit's largest |O|: both round P to bf16
    against a different max, then O to bf16); LSE within 1e-4; the whole-head backward fed the streaming forward's LSE
    reproduces its own gradients (within 2^-7 of the unit's largest entry: the two LSEs differ in the last fp32 bits)."""
    gen = torch.Generator(device=DEV)
    gen.manual_seed(3 * Sq + Sk + D)
    v, owned, g = _operands(D, 4, 3, Sq, Sk, gen, packed=False)
    key = 99 + Sq
    for t in owned:
        t.fill_(NAN)
    _whole(lib, v, g, drop, key)
    whole = _outputs(v, g)
    o_s, lse_s = torch.full_like(v["O"], NAN), torch.full_like(v["LSE"], NAN)
    L.check(lib.kzv_attn_stream_fwd(C.byref(_args(v, g, drop, key, O=o_s, LSE=lse_s)), _st()), "attn_stream_fwd")
    torch.cuda.synchronize()
    o_stream = _heads(o_s, g, Sq).float()
    scale = whole["O"].float().abs().amax(dim=(2, 3), keepdim=True).clamp(min=1e-3)
    assert ((o_stream - whole["O"].float()).abs() <= scale * 2 ** -7).all()
    assert ((lse_s - whole["LSE"]).abs() <= 1e-4).all()
    for k in ("dQ", "dK", "dV"):
        v[k].fill_(NAN)
    _whole(lib, v, g, drop, key, LSE=lse_s, fwd=False)
    fed = _outputs(v, g)
    for k in ("dQ", "dK", "dV"):
        want = whole[k].float()
        tol = want.abs().amax(dim=(2, 3), keepdim=True).clamp(min=1e-3) * 2 ** -7
        assert ((fed[k].float() - want).abs() <= tol).all(), k


# ------------------------------------------------------------------------------------------------ 3. the model's strides at scale
def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


@pytest.mark.parametrize("D", [64, 96])
def test_attention_stream_at_scale(lib, D):
    """B = 64, 8 heads, 513 tokens in the packed QKV buffer [64 * 513, 3 * 8 * D], dropout 0.1.  Inputs A, B, A through the same
    NaN-filled buffers, each (batch, head) judged alone; the checker flags one planted stale (batch, head) tile.  Then forward and
    backward once more on input A: bitwise equal to the first run (no atomics)."""
    B, heads, S, drop = 64, 8, 513, 0.1
    gen = torch.Generator(device=DEV)
    gen.manual_seed(50 + D)
    va, owned, g = _operands(D, B, heads, S, S, gen, packed=True)
    gen.manual_seed(60 + D)
    vb, _, _ = _operands(D, B, heads, S, S, gen, packed=True)
    keys = {"A": 501, "B": 502}
    saved = {k: va[k].clone() for k in ("Q", "K", "V", "dO")}
    refs = {"A": _ref(lib, va, g, drop, keys["A"]), "B": _ref(lib, vb, g, drop, keys["B"])}
    runs = []
    for which in ("A", "B", "A"):
        src = vb if which == "B" else saved
        for k in ("Q", "K", "V", "dO"):
            va[k].copy_(src[k])
        got = _run_stream(lib, va, owned, g, drop, keys[which])
        _check_all(f"stream d{D} at scale input {which}", _attn_compare(got, refs[which]))
        runs.append(got)
    b, h, r = B - 3, heads - 1, 16
    for name in ("O", "LSE", "dQ", "dK", "dV"):
        planted = {k: t.clone() for k, t in runs[2].items()}
        planted[name][b, h, r:r + 16] = runs[1][name][b, h, r:r + 16]
        _assert_flags(_attn_compare(planted, refs["A"]), name, (b, h))
    again = _run_stream(lib, va, owned, g, drop, keys["A"])
    for k in runs[2]:
        assert torch.equal(_bits(again[k]), _bits(runs[2][k])), k
