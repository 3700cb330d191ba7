"""The training attention kernels (csrc/attention.hip, attention_d96.hip, attention_stream.hip, attention_generic.hip), forward and
backward, on PEAKED softmax, held to the bound of tests/_attn_emul.py: per (batch, head) unit and output
MARGIN (2) x max(err_ref, half a bf16 ulp of the unit's largest entry), err_ref = the distance of an fp32 emulation that rounds
where the kernel family rounds from the float64 reference on the same bf16 operands.  No constant floor: a unit with small
gradients is judged against its own size.  tests/test_attention_emul_cpu.py shows what this bound flags.

Inputs (``_attn_emul.operands``): flat (randn, as the older tests), sharp (Q and K of unit u x (0.5, 1, 2, 3)[u % 4]: row maxima from
1 / Sk to 1.000 in one launch), rise / fall (a score ramp of 9 along the keys: every ``alpha`` of the streaming kernels far from 1 /
later blocks underflow).  B x heads = 2 x 4, dropout 0 and 0.1 on the masks kzv_debug_attn_dropout_mask reports, padded row strides,
outputs NaN-filled before the launch.  The shapes are the smallest that reach each kernel instance (``_attn_emul.CASES``); the
dispatch is asserted through kzv_attn_impl.  Every case prints its worst error / err_ref and error / bound per output.

MEASURED ON AN MI355X, engine error / err_ref over every unit, kind and dropout of a family (smallest .. largest of the cases'
worst units; the bound is at 2.0).  O / dQ / dK / dV: whole-head d64 mode 0 1.00 .. 1.13 (dK; the others 1.00), mode 1 1.00;
whole-head d96 1.00 .. 1.10 (O); streaming d64 1.00 .. 1.04 (dQ); streaming d96 1.00 .. 1.18 (dK); generic d32 1.00, d128 1.00 .. 1.43
(dK).  1.00 means the engine's worst element IS the emulation's: the two round the same fp32 value to the same bf16.  err_ref itself
is 0.3 .. 3 % of the unit's largest entry.  LSE: error / err_ref 0.97 .. 2.41, but its err_ref (1e-7 relative) is below the fp32 floor
of the bound, 2^-21 max(1, |LSE|); error / bound 0.09 .. 0.26 over all families, i.e. at most 0.52 of that floor.  No unit of any
kernel exceeded the margin.  The whole module takes about 15 s.

The first causal query row (one key, dS = 0 exactly) has its own test: test_causal_first_query_row_has_zero_dq."""
import ctypes as C
import functools
import types

import pytest
import torch

import _attn_emul as E
from kzv import _lib as L
from test_bench_geometry_gpu import _assert_flags, _check_all, _unit_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
B, HEADS = 2, 4
DROPS = (0.0, 0.1)
IMPL = {("whole", 64): L.ATTN_MFMA64, ("whole", 96): L.ATTN_MFMA96, ("generic", 32): L.ATTN_VALU, ("generic", 128): L.ATTN_VALU}


@pytest.fixture(scope="module")
def lib():
    return L.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ids(c):
    return f"{c[0]}-d{c[1]}-m{c[2]}-{c[3]}x{c[4]}"


def _rows(t):
    """heads view [B, heads, S, D] -> rows [B * S, heads * D]."""
    b, h, s, d = t.shape
    return t.transpose(1, 2).reshape(b * s, h * d)


def _heads(t, S, D):
    return t[:, :HEADS * D].reshape(B, S, HEADS, D).transpose(1, 2)


def _engine(lib, fam, D, mode, q, k, v, do, ids, drop, key):
    """One forward and one backward of the family's kernels on the heads-view operands; separate buffers with padded row strides
    (tests/test_attention_stream_gpu.py::_operands), every output NaN-filled first.  Returns O, LSE, dQ, dK, dV in the heads view."""
    Sq, Sk, H = q.shape[2], k.shape[2], HEADS * D
    qb = torch.zeros(B * Sq, H + 8, dtype=torch.bfloat16, device=DEV)
    kvb = torch.zeros(B * Sk, 2 * H + 16, dtype=torch.bfloat16, device=DEV)
    dob = torch.zeros(B * Sq, H + 8, dtype=torch.bfloat16, device=DEV)
    qb[:, :H], kvb[:, :H], kvb[:, H + 8:2 * H + 8], dob[:, :H] = _rows(q), _rows(k), _rows(v), _rows(do)
    ob, dqb, dkvb = torch.full_like(dob, NAN), torch.full_like(qb, NAN), torch.full_like(kvb, NAN)
    lse = torch.full((B, HEADS, Sq), NAN, device=DEV)
    K, V, dK, dV = kvb[:, :H], kvb[:, H + 8:], dkvb[:, :H], dkvb[:, H + 8:]
    a = L.kzv_attn_args(Q=qb.data_ptr(), K=K.data_ptr(), V=V.data_ptr(), O=ob.data_ptr(), LSE=lse.data_ptr(), dO=dob.data_ptr(),
                        dQ=dqb.data_ptr(), dK=dK.data_ptr(), dV=dV.data_ptr(), ldq=H + 8, ldk=2 * H + 16, ldv=2 * H + 16, ldo=H + 8,
                        ids=L.ptr(ids), ld_ids=(Sk + 1 if ids is not None else 0), pad_id=1, B=B, heads=HEADS, Sq=Sq, Sk=Sk,
                        mode=mode, drop_p=drop, drop_key=key, head_dim=D)
    if fam == "stream":
        if max(Sq, Sk) > 288:
            want = L.ATTN_STREAM96 if D == 96 else L.ATTN_STREAM64
            assert lib.kzv_attn_impl_ex(C.byref(a), 0, L.MODEL_LONG_SEQ) == want
            assert lib.kzv_attn_impl_ex(C.byref(a), 1, L.MODEL_LONG_SEQ) == want
        L.check(lib.kzv_attn_stream_fwd(C.byref(a), _st()), "attn_stream_fwd")
        L.check(lib.kzv_attn_stream_bwd(C.byref(a), _st()), "attn_stream_bwd")
    else:
        assert lib.kzv_attn_impl(C.byref(a), 0) == IMPL[fam, D] and lib.kzv_attn_impl(C.byref(a), 1) == IMPL[fam, D]
        L.check(lib.kzv_attn_fwd(C.byref(a), _st()), "attn_fwd")
        L.check(lib.kzv_attn_bwd(C.byref(a), _st()), "attn_bwd")
    torch.cuda.synchronize()
    pad = torch.cat([ob[:, H:], dqb[:, H:], dkvb[:, H:H + 8], dkvb[:, 2 * H + 8:]], 0)
    assert bool(pad.isnan().all()), "a kernel wrote into the padding between the rows"
    return {"O": _heads(ob, Sq, D).clone(), "LSE": lse, "dQ": _heads(dqb, Sq, D).clone(), "dK": _heads(dK, Sk, D).clone(),
            "dV": _heads(dV, Sk, D).clone()}


@functools.lru_cache(maxsize=4)
def _case(lib, fam, D, mode, Sq, Sk, kind, drop):
    """Operands, engine outputs, float64 reference and emulation of one case."""
    gen = torch.Generator(device=DEV).manual_seed(E.case_seed(D, mode, Sq, Sk))
    q, k, v, do = E.operands(kind, B, HEADS, Sq, Sk, D, gen)
    ids = E.pad_tail_ids(B, Sk, gen) if mode == 1 else None
    mask = E.causal_pad_mask(ids, Sq, Sk) if mode == 1 else None
    key, mult = E.drop_key(Sq, Sk), None
    if drop > 0:
        mult = torch.empty(B * HEADS * Sq, Sk, device=DEV)
        L.check(lib.kzv_debug_attn_dropout_mask(key, drop, B * HEADS, Sq, Sk, mult.data_ptr(), _st()), "mask")
        mult = mult.view(B, HEADS, Sq, Sk)
    scale = E.softmax_scale(D)
    ref = E.ref64(q, k, v, do, scale, mask, mult)
    emu = E.emulate(fam, q, k, v, do, scale, mask, mult)
    got = _engine(lib, fam, D, mode, q, k, v, do, ids, drop, key)
    return types.SimpleNamespace(got=got, ref=ref, emu=emu, ids=ids, mult=mult)


def _results(got, emu, ref):
    tol, er = E.bounds(emu, ref)
    return {k: (_unit_err(got[k], ref[k], 2), tol[k]) for k in E.OUTPUTS}, er


@pytest.mark.parametrize("drop", DROPS)
@pytest.mark.parametrize("kind", E.KINDS)
@pytest.mark.parametrize("case", E.all_cases(), ids=_ids)
def test_attention_on_peaked_softmax(lib, case, kind, drop):
    """O, LSE, dQ, dK, dV of every unit within MARGIN x max(err_ref, floor) of float64."""
    c = _case(lib, *case, kind, drop)
    res, er = _results(c.got, c.emu, c.ref)
    tag = f"peaked {_ids(case)} {kind} p={drop}"
    print(f"{tag}: error / err_ref " + ", ".join(f"{k} {float((res[k][0] / er[k].clamp(min=1e-30)).max()):.2f}" for k in E.OUTPUTS))
    _check_all(tag, res)


@pytest.mark.parametrize("Sq", [23, 127])
def test_causal_first_query_row_has_zero_dq(lib, Sq):
    """Mode 1: the first query of each image sees one key, so P = 1 and dS = P (multiplier dP - delta) = 0 in exact arithmetic (the
    float64 reference: below 1e-12): those dQ rows are exactly zero on every kind, dropout off and 0.1.  The backward sets that dS
    to 0 itself (attention.hip:399-401).  Computed, it was not 0: dP comes out of two chained MFMAs and delta' out of dot8 partial
    sums of the bf16-rounded O, and these rows held up to 8.6e-7 without dropout and up to 0.043 with it (measured on an MI355X
    before the change; inside the bound of test_attention_on_peaked_softmax either way)."""
    worst = {}
    for kind in E.KINDS:
        for drop in DROPS:
            c = _case(lib, "whole", 64, 1, Sq, Sq, kind, drop)
            assert float(c.ref["dQ"][:, :, 0].abs().max()) < 1e-12
            worst[kind, drop] = float(c.got["dQ"][:, :, 0].float().abs().max())
            print(f"causal {Sq} {kind} p={drop}: largest |dQ| of the first query rows {worst[kind, drop]:.3g}")
    assert all(w == 0.0 for w in worst.values()), worst


@pytest.mark.parametrize("fam,D,mode,Sq,Sk", [("whole", 64, 0, 161, 161), ("whole", 96, 0, 161, 161), ("stream", 64, 0, 130, 200),
                                              ("stream", 96, 0, 130, 200), ("generic", 32, 0, 161, 161)])
def test_the_checker_flags_one_planted_tile(lib, fam, D, mode, Sq, Sk):
    """Once per family: one 16-row tile of one output of one unit of the engine's ``sharp`` result replaced by the ``flat`` run's;
    exactly that unit must be flagged.  Unit (1, 3) is u = 7: Q and K x 3 (the x 1 units of ``sharp`` ARE the flat ones)."""
    sharp = _case(lib, fam, D, mode, Sq, Sk, "sharp", 0.1)
    flat = _case(lib, fam, D, mode, Sq, Sk, "flat", 0.1)
    b, h, r = B - 1, HEADS - 1, 16
    for name in E.OUTPUTS:
        planted = {k: t.clone() for k, t in sharp.got.items()}
        planted[name][b, h, r:r + 16] = flat.got[name][b, h, r:r + 16]
        _assert_flags(_results(planted, sharp.emu, sharp.ref)[0], name, (b, h))
