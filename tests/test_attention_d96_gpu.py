"""The head_dim-96 MFMA attention kernels (csrc/attention_d96.hip) against float64 references, at the op level, at the reference
CLI's geometry with the model's strides (B = 64 x 8 heads = 512 workgroups, more than the CUs), and inside the whole reference-
default model against the fp32 oracle.  Every case asserts that kzv_attn_impl sends it to the new kernels, so nothing here can
pass on the VALU fallback.  The unit checkers, the oracle driver and their bounds are those of test_bench_geometry_gpu.py."""
import ctypes as C
import gc
import types

import numpy as np
import pytest
import torch

from kzv import _lib as L
from kzv import params as P
from kzv.config import reference_cli_config
from kzv.data import build_decoder_dir, synthetic_batch
from kzv.model import TrOCRModel
from _replay import step_masks
from test_bench_geometry_gpu import (_assert_flags, _attn_compare, _check_all, _check_grads, _grad_errors, _logit_compare,
                                     _no_dropout, _oracle)

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
D = 96
SEED = 4242


@pytest.fixture(scope="module")
def lib():
    return L.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _args(v, g, drop, key):
    return L.kzv_attn_args(Q=v["Q"].data_ptr(), K=v["K"].data_ptr(), V=v["V"].data_ptr(), O=v["O"].data_ptr(), LSE=v["LSE"].data_ptr(),
                           dO=v["dO"].data_ptr(), dQ=v["dQ"].data_ptr(), dK=v["dK"].data_ptr(), dV=v["dV"].data_ptr(),
                           ldq=v["ldq"], ldk=v["ldk"], ldv=v["ldk"], ldo=v["ldo"], B=g.B, heads=g.heads, Sq=g.Sq, Sk=g.Sk, mode=0,
                           drop_p=drop, drop_key=key, head_dim=D)


def _operands(B, heads, Sq, Sk, gen, packed):
    """packed: Q, K, V as column blocks of one [B * S, 3 * heads * 96] buffer (model.cpp's encoder layout, Sq == Sk); otherwise
    separate buffers with padded row strides.  Returns (views, buffers to NaN-fill, geometry)."""
    H = heads * D
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=gen).bfloat16()
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
    v["dO"] = rnd(B * Sq, v["ldo"])
    v["LSE"] = torch.empty(B, heads, Sq, device=DEV)
    owned += [v["O"], v["LSE"]]
    return v, owned, types.SimpleNamespace(B=B, heads=heads, Sq=Sq, Sk=Sk, H=H)


def _heads(t, g, S):
    return t[:, :g.H].reshape(g.B, S, g.heads, D).transpose(1, 2)       # [B, heads, S, 96]: unit = (b, h)


def _run(lib, v, owned, g, drop, key):
    for t in owned:
        t.fill_(NAN)
    a = _args(v, g, drop, key)
    assert lib.kzv_attn_impl(C.byref(a), 0) == L.ATTN_MFMA96 and lib.kzv_attn_impl(C.byref(a), 1) == L.ATTN_MFMA96
    L.check(lib.kzv_attn_fwd(C.byref(a), _st()), "attn_fwd")
    L.check(lib.kzv_attn_bwd(C.byref(a), _st()), "attn_bwd")
    torch.cuda.synchronize()
    return {"O": _heads(v["O"], g, g.Sq).clone(), "LSE": v["LSE"].clone(), "dQ": _heads(v["dQ"], g, g.Sq).clone(),
            "dK": _heads(v["dK"], g, g.Sk).clone(), "dV": _heads(v["dV"], g, g.Sk).clone()}


def _ref(lib, v, g, drop, key):
    """float64 softmax(q k^T 96^-0.5) [x the dropout multipliers kzv_debug_attn_dropout_mask reports] v and its gradients."""
    qh, kh, vh = (_heads(v[k], g, S).double().requires_grad_(True) for k, S in (("Q", g.Sq), ("K", g.Sk), ("V", g.Sk)))
    s = qh @ kh.transpose(2, 3) * (1.0 / np.sqrt(D))
    p = torch.softmax(s, -1)
    if drop > 0:
        m = torch.empty(g.B * g.heads * g.Sq, g.Sk, device=DEV)
        L.check(lib.kzv_debug_attn_dropout_mask(key, drop, g.B * g.heads, g.Sq, g.Sk, m.data_ptr(), _st()), "mask")
        p = p * m.view(g.B, g.heads, g.Sq, g.Sk).double()
    o = p @ vh
    dq, dk, dv = torch.autograd.grad(o, (qh, kh, vh), _heads(v["dO"], g, g.Sq).double())
    return {"O": o.detach(), "LSE": torch.logsumexp(s.detach(), -1), "dQ": dq, "dK": dk, "dV": dv}


# ------------------------------------------------------------------------------------------------ 1. op level
OP_CASES = [(3, 2, 1, 1), (2, 3, 16, 16), (3, 2, 37, 37), (2, 2, 97, 97), (2, 3, 161, 161), (2, 2, 257, 257), (2, 2, 288, 288),
            (2, 2, 60, 257), (2, 2, 257, 40)]


@pytest.mark.parametrize("drop", [0.0, 0.1, 0.25])
@pytest.mark.parametrize("B,heads,Sq,Sk", OP_CASES)
def test_attention_d96_fwd_bwd(lib, B, heads, Sq, Sk, drop):
    """Every token count the tile loops treat differently (one key, one tile, partial tiles, odd tile counts, the 257 of the
    reference geometry, the 288 maximum, Sq != Sk both ways), padded row strides, dropout off / 0.1 / 0.25 on the masks
    kzv_debug_attn_dropout_mask reports."""
    gen = torch.Generator(device=DEV)
    gen.manual_seed(17 * Sq + Sk)
    v, owned, g = _operands(B, heads, Sq, Sk, gen, packed=False)
    key = 1234 + Sq
    _check_all(f"d96 B={B} h={heads} Sq={Sq} Sk={Sk} p={drop}", _attn_compare(_run(lib, v, owned, g, drop, key), _ref(lib, v, g, drop, key)))


# ------------------------------------------------------------------------------------------------ 2. the model's strides
@pytest.mark.parametrize("drop", [0.0, 0.1])
def test_attention_d96_at_the_reference_geometry(lib, drop):
    """B = 64, 8 heads, 257 tokens in the packed QKV buffer [64 * 257, 2304], ldo 768: 512 workgroups on 256 CUs.  Inputs A, B, A
    through the same NaN-filled buffers, each (batch, head) judged alone; the checker flags one planted stale (batch, head) tile."""
    B, heads, S = 64, 8, 257
    gen = torch.Generator(device=DEV)
    gen.manual_seed(5)
    va, owned, g = _operands(B, heads, S, S, gen, packed=True)
    gen.manual_seed(6)
    vb, _, _ = _operands(B, heads, S, S, gen, packed=True)
    keys = {"A": 301, "B": 302}
    refs = {"A": _ref(lib, va, g, drop, keys["A"]), "B": _ref(lib, vb, g, drop, keys["B"])}
    saved = {k: va[k].clone() for k in ("Q", "K", "V", "dO")}
    runs = []
    for which in ("A", "B", "A"):
        src = vb if which == "B" else saved
        for k in ("Q", "K", "V", "dO"):
            va[k].copy_(src[k])
        got = _run(lib, va, owned, g, drop, keys[which])
        _check_all(f"d96 reference geometry p={drop} input {which}", _attn_compare(got, refs[which]))
        runs.append(got)
    b, h, r = B - 3, heads - 1, 16
    for name in ("O", "LSE", "dQ", "dK", "dV"):
        planted = {k: t.clone() for k, t in runs[2].items()}
        planted[name][b, h, r:r + 16] = runs[1][name][b, h, r:r + 16]
        _assert_flags(_attn_compare(planted, refs["A"]), name, (b, h))


# ------------------------------------------------------------------------------------------------ 3. the whole model
@pytest.fixture(scope="module")
def refcli():
    cfg = reference_cli_config()
    ns = types.SimpleNamespace(cfg=cfg, sd=P.state_dict_from_flat(cfg, P.recipe_flat(cfg, 42)), refs={})
    ns.inputs = {"A": synthetic_batch(cfg, 64, 128, seed=11), "B": synthetic_batch(cfg, 64, 128, seed=12)}

    def ref(which):
        if which not in ns.refs:
            ns.refs[which] = _oracle(cfg, ns.sd, *ns.inputs[which])
        return ns.refs[which]
    ns.ref = ref
    return ns


def _engine(cfg, tmp_path):
    m = TrOCRModel(cfg.encoder_config_dict(), build_decoder_dir(str(tmp_path / "dec"), cfg), init_seed=42, load_tokenizer=False)
    assert m.encoder_attention_impl == "mfma96"
    yield m
    del m
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture
def drop_engine(refcli, tmp_path):
    yield from _engine(refcli.cfg, tmp_path)


@pytest.fixture
def nodrop_engine(refcli, tmp_path):
    yield from _engine(_no_dropout(refcli.cfg), tmp_path)


def test_reference_default_model_logits(refcli, drop_engine):
    """Eval mode, the reference CLI's model (ViT 768 / 12 layers / 8 heads / FFN 3072 on 1024 x 64, the reference decoder) at its
    default batch 64 with labels of length 128: logits per image within 3e-2 of the fp32 oracle, loss within 5e-3; inputs A, B, A;
    a swapped image is flagged."""
    m = drop_engine
    m.eval()
    runs = []
    for which in ("A", "B", "A"):
        px, lab = refcli.inputs[which]
        r = refcli.ref(which)
        loss, logits = m.forward_loss(torch.from_numpy(px), torch.from_numpy(lab), want_logits=True, seed=SEED)
        torch.cuda.synchronize()
        _check_all(f"reference-default logits input {which}", _logit_compare(logits, torch.from_numpy(r["logits"]).to(DEV)))
        assert abs(float(loss.item()) - r["loss"]) < 5e-3
        runs.append(logits.clone())
    planted = runs[2].clone()
    planted[37] = runs[1][37]
    _assert_flags(_logit_compare(planted, torch.from_numpy(refcli.ref("A")["logits"]).to(DEV)), "logits", (37,))


def test_reference_default_model_gradients(refcli, nodrop_engine):
    """Dropout off, batch 64: loss within 5e-3, every gradient tensor within 0.05 of its largest entry, median <= 0.02; inputs
    A, B, A with flat_grads NaN-filled; a tensor swapped for the other input's is flagged."""
    m, cfg = nodrop_engine, refcli.cfg
    m.train()
    got = {}
    for which in ("A", "B", "A"):
        px, lab = refcli.inputs[which]
        r = refcli.ref(which)
        m.flat_grads.fill_(NAN)
        loss, _ = m.forward_loss(torch.from_numpy(px), torch.from_numpy(lab), seed=SEED)
        m.backward()
        torch.cuda.synchronize()
        assert abs(float(loss.item()) - r["loss"]) < 5e-3
        _check_grads(f"reference-default grads input {which}", _grad_errors(cfg, m.flat_grads, r["grads"]), 0.05, 0.02)
        got[which] = m.flat_grads.clone()
    name = "encoder.encoder.layer.0.attention.attention.query.weight"
    planted = got["A"].clone()
    P.state_dict_from_flat(cfg, planted)[name].copy_(P.state_dict_from_flat(cfg, got["B"])[name])
    worst = _grad_errors(cfg, planted, refcli.ref("A")["grads"])
    assert worst[name] > 0.05 and sum(e > 0.05 for e in worst.values()) == 1, worst[name]


def test_reference_default_model_with_dropout_replayed(refcli, drop_engine):
    """Dropout on (0.1 everywhere, the CLI's), batch 64: the step's masks (tests/_replay.step_masks) replayed through the fp32
    oracle: loss within 5e-3, every gradient tensor within 0.05 of its largest entry, median <= 0.02."""
    m, cfg = drop_engine, refcli.cfg
    px, lab = refcli.inputs["A"]
    m.train()
    m.flat_grads.fill_(NAN)
    loss, _ = m.forward_loss(torch.from_numpy(px), torch.from_numpy(lab), seed=SEED)
    m.backward()
    torch.cuda.synchronize()
    T = m.last_active_length
    masks = step_masks(cfg, SEED, 64, T, device=DEV)
    r = _oracle(cfg, refcli.sd, px, lab[:, :T + 1], masks=masks)
    del masks
    assert abs(float(loss.item()) - r["loss"]) < 5e-3
    _check_grads("reference-default dropout replay", _grad_errors(cfg, m.flat_grads, r["grads"]), 0.05, 0.02)
