"""TEST INFRASTRUCTURE: references, a rounding-point emulation, inputs and the bound for the training attention kernels
(csrc/attention.hip, attention_d96.hip, attention_stream.hip, attention_generic.hip).  Plain torch; runs on the CPU and on the GPU
(everything lives on the device of the operands).  Used by tests/test_attention_emul_cpu.py, which proves on the CPU that the bound
separates a correct kernel from the mistakes listed there, and by tests/test_attention_peaked_gpu.py, which holds the kernels to it.

All tensors are in the "heads view": Q, dO, O, dQ [B, heads, Sq, D]; K, V, dK, dV [B, heads, Sk, D]; LSE [B, heads, Sq]; a unit is one
(batch, head).  ``keep_mask`` is the ATTENTION mask (bool, broadcastable to [B, heads, Sq, Sk], True = the query sees the key; None =
every key), ``drop_mult`` the DROPOUT multipliers (0 or 1 / P(keep), [B, heads, Sq, Sk]; None = no dropout).

The bound, per unit and output:  MARGIN x max(err_ref, FLOOR),  err_ref = max |emulate - ref64| over the unit,
    O, dQ, dK, dV (bf16):  FLOOR = 2^-9 x the unit's largest |ref64 entry|   (half a bf16 ulp of the output format)
    LSE (fp32):            FLOOR = 2^-21 x max(1, the unit's largest |LSE|)  (about four fp32 ulps: the scaled max, the hardware
                                                                             exp2 / log2, the conversion to the natural log)
MARGIN = 2.0 as in tests/test_decode_peaked_gpu.py and tests/test_align_gpu.py, for the same reason: the engine's summation orders
(MFMA accumulation, lane partial sums) are not the emulation's.  There is no constant floor.

Resolution: a softmax scale wrong by 2, an ``alpha`` that is never applied, a missing delta, a missing 1 / P(keep), an LSE of the
dropped probabilities, a causal diagonal off by one and unmasked pad keys are each >= 3 bounds away on every unit (asserted in
test_attention_emul_cpu.py).  A delta wrong by x 0.9 is only 1 - 4 bounds away on ``flat`` inputs: that is below what this bound
resolves, and it is not tested for.
"""
import torch

MARGIN = 2.0
KINDS = ("flat", "sharp", "rise", "fall")
SHARP_LADDER = (0.5, 1.0, 2.0, 3.0)
LOG2E = 1.4426950408889634
KB = 64                         # keys per block of the streaming kernels (attention_stream.hip:29)
OUTPUTS = ("O", "LSE", "dQ", "dK", "dV")


def f32(x, like):
    return torch.tensor(x, dtype=torch.float32, device=like.device)


def softmax_scale(D):
    """head_dim^-0.5 as the kernels hold it: an fp32 (attention_common.h:38)."""
    return 0.125 if D == 64 else float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(D), dtype=torch.float32).sqrt())


# ------------------------------------------------------------------------------------------------ inputs
def operands(kind, B, heads, Sq, Sk, D, gen):
    """bf16 Q, K, V, dO (heads view) on the generator's device.
    flat   randn.
    sharp  unit u = b * heads + h multiplies Q and K by (0.5, 1, 2, 3)[u % 4]: row maxima of P from ~1 / Sk to 1.000 in one launch;
           the 0.5 units have the small gradients a constant floor hides.
    rise   a unit vector d per unit; Q += 6 c d, K[j] += d * 12 c j / (Sk - 1), c = (D / 64)^(1/4) (1 at head_dim 64; with c = 1 at
           head_dim 96 the scaled ramp is 7.3 instead of 9 and the median smallest alpha at 385 keys is 0.118, above the 0.1 that
           test_attention_emul_cpu.py asks for): the row maximum climbs through every key block, so every ``alpha`` of the online
           softmax is far from 1.
    fall   the same ramp reversed: the maximum sits in the first block, later blocks contribute exp(-large)."""
    assert kind in KINDS, kind
    dev = gen.device
    rnd = lambda *s: torch.randn(*s, device=dev, generator=gen)
    q, k, v, do = rnd(B, heads, Sq, D), rnd(B, heads, Sk, D), rnd(B, heads, Sk, D), rnd(B, heads, Sq, D)
    if kind == "sharp":
        mul = torch.tensor(SHARP_LADDER, device=dev)[torch.arange(B * heads, device=dev) % 4].view(B, heads, 1, 1)
        q, k = q * mul, k * mul
    elif kind in ("rise", "fall"):
        d = rnd(B, heads, 1, D)
        d = d / d.norm(dim=-1, keepdim=True)
        ramp = torch.arange(Sk, device=dev, dtype=torch.float32) / max(Sk - 1, 1)
        if kind == "fall":
            ramp = 1.0 - ramp
        c = (D / 64.0) ** 0.25                 # the ramp of the SCALED scores is 9 j / (Sk - 1) at every head_dim, as at 64
        q = q + 6.0 * c * d
        k = k + d * (12.0 * c * ramp).view(1, 1, Sk, 1)
    return q.bfloat16(), k.bfloat16(), v.bfloat16(), do.bfloat16()


# ------------------------------------------------------------------------------------------------ float64 reference
def ref64(q, k, v, dO, scale, keep_mask=None, drop_mult=None):
    """softmax(q k^T scale [masked]) [x drop_mult] v and its gradients for dO, float64 autograd on the bf16 operands; LSE is the
    log-sum-exp of the scaled, masked, UN-dropped scores.  Also "P", the un-dropped probabilities (not an output of the kernels)."""
    qd, kd, vd = (t.double().requires_grad_(True) for t in (q, k, v))
    s = qd @ kd.transpose(2, 3) * float(scale)
    if keep_mask is not None:
        s = s.masked_fill(~keep_mask, float("-inf"))
    p = torch.softmax(s, -1)
    pd = p if drop_mult is None else p * drop_mult.double()
    o = pd @ vd
    dq, dk, dv = torch.autograd.grad(o, (qd, kd, vd), dO.double())
    return {"O": o.detach(), "LSE": torch.logsumexp(s.detach(), -1), "dQ": dq, "dK": dk, "dV": dv, "P": p.detach()}


# ------------------------------------------------------------------------------------------------ emulation
def _bf(x):
    return x.bfloat16().float()


def _fms(a, b, c):
    """fp32 a * b - c with one rounding (the kernels' fmaf)."""
    return (a.double() * b.double() - c.double()).float()


MUTANTS = ("fwd_scale", "bwd_scale", "alpha1", "no_delta", "no_inv_keep", "lse_dropped")


def emulate(family, q, k, v, dO, scale, keep_mask=None, drop_mult=None, mutant=None):
    """The same operation in fp32, rounding to bf16 exactly where the kernels of ``family`` round.  Products of bf16 operands are
    exact in fp32 and every sum below is an fp32 sum, as in the kernels (MFMA fp32 accumulators, fp32 VALU); only the ORDER of the
    sums differs, which is what MARGIN is for.  Returns O, LSE, dQ, dK, dV (fp32 tensors holding bf16 values; LSE fp32) and, for
    "stream", "alpha_min": per query row the smallest ``alpha`` over the key blocks after the first.

    family "whole": attention.hip (head_dim 64, modes 0 and 1) and attention_d96.hip (head_dim 96).  Rounding points, in order
    (a.hip = attention.hip, d96 = attention_d96.hip, c.h = attention_common.h):
      F1  S = Q K^T: bf16 operands, fp32 accumulate (a.hip:131-132, d96:98); masked or past Sk -> -inf (a.hip:137-138, d96:101)
      F2  the row max over the WHOLE row (a.hip:141-145, d96:103-107); mref = max * sc, sc = scale * log2(e) in fp32 (a.hip:116,147;
          d96:83,108)
      F3  p = exp2(fma(S, sc, -mref)), fp32; the row sum adds these un-dropped, un-rounded p (c.h:128)
      F4  p -> bf16 (c.h:129); dropped elements zeroed AFTER the rounding, 1 / P(keep) NOT applied here (c.h:130-134)
      F5  LSE = (max * sc + log2(sum)) / log2(e), fp32 (a.hip:162, d96:123)
      F6  O = (bf16 P) V in fp32 (a.hip:173, d96:136), x (inv_keep / sum) (a.hip:178, d96:140), -> bf16 (store_bf4 c.h:69-70;
          a.hip:183, d96:145)
      B1  lse2 = LSE * log2(e) (a.hip:277, c.h:146, d96:226); delta' = rowsum(dO . O) * P(keep) from the ROUNDED O
          (a.hip:229-233, c.h:142-147, d96:222-227)
      B2  pr = exp2(fma(S, sc, -lse2)) (c.h:112), kept pr where not dropped (c.h:116); dP = dO V^T fp32 (a.hip:390-391, d96:275);
          dS = fma(kept pr, dP, -pr * delta') (c.h:117)
      B2' mode 1 (the only masked mode: a ``keep_mask`` is given): dS of query 0, which sees one key, is set to its exact value 0
          (a.hip:399-401); its kept pr still goes into dV
      B3  kept pr -> bf16, dS -> bf16 (a.hip:402-403, d96:283-284)
      B4  dV = (bf16 kept pr)^T dO x inv_keep -> bf16 (a.hip:411,481; d96:293,345); dK = (bf16 dS)^T Q x scale inv_keep -> bf16
          (a.hip:412,471,480; d96:294,335,344); dQ = (bf16 dS) K x scale inv_keep -> bf16 (a.hip:445,456,462; d96:310,323-327)

    family "stream": attention_stream.hip (s.hip), head_dim 64 and 96.  As "whole" but for the forward, an online softmax over
    blocks of 64 keys:
      F2' per block: bm = the block's max, mn = max(m, bm), alpha = exp2((m - mn) * sc) (s.hip:136-141); l *= alpha, o *= alpha
          (s.hip:143-145); mref = mn * sc (s.hip:146)
      F3' l += the block's un-dropped, un-rounded p (s.hip:151-153 through c.h:128); F4 as above; o += (bf16 P) V (s.hip:162)
      F5' LSE = (m * sc + log2(l)) / log2(e) (s.hip:175); F6' O = o x (inv_keep / l) -> bf16 (s.hip:176,180)
      B1-B4 as above: the dK / dV kernel (s.hip:228-233 delta', 297-299 elements and rounding, 322-323 stores) and the dQ kernel
          (s.hip:351-356 delta' and lse2, 400-407 elements and rounding, 424-428 store); dQ is an fp32 sum over all key blocks.

    family "generic": attention_generic.hip (g.hip), fp32 VALU, mode 0:
      G1  qf = Q * scale rounded to fp32 (g.hip:80); s = qf . K fp32 (g.hip:95); p = exp(s - max) (g.hip:102); inv = 1 / sum (g.hip:104)
      G2  LSE = max + log(sum) (g.hip:105)
      G3  pr = bf16(p * inv * multiplier): normalised and scaled by 1 / P(keep) BEFORE the rounding (g.hip:109)
      G4  O = bf16(sum pr V) (g.hip:115-116)
      G5  delta = rowsum(dO . O) from the rounded O, no P(keep) (g.hip:86); pk = exp(s - LSE) (g.hip:127); dP = dO . V (g.hip:129)
      G6  dS = bf16(pk * (dP * multiplier - delta) * scale) (g.hip:130-131,133), Pd = bf16(pk * multiplier) (g.hip:132)
      G7  dQ = bf16(sum dS K) (g.hip:141-142); dK = bf16(sum dS Q), dV = bf16(sum Pd dO) (g.hip:166-167,176-177)

    ``mutant`` plants one mistake INTO THE EMULATION (the kernels are never mutated): "fwd_scale" / "bwd_scale": the softmax scale
    x 0.5 in the forward / in the backward only; "alpha1": alpha = 1 (stream); "no_delta": delta = 0; "no_inv_keep": 1 / P(keep)
    missing from dP; "lse_dropped": LSE from the sum of the dropped probabilities.  Mask mistakes (diagonal off by one, pad keys
    unmasked) are planted by passing another ``keep_mask``."""
    assert mutant is None or mutant in MUTANTS, mutant
    qf, kf, vf, dof = q.float(), k.float(), v.float(), dO.float()
    inv_keep = f32(1.0, qf) if drop_mult is None else drop_mult.max().float()
    keep = None if drop_mult is None else (drop_mult != 0).float()
    scale_f = f32(scale, qf) * (0.5 if mutant == "fwd_scale" else 1.0)
    scale_b = f32(scale, qf) * (0.5 if mutant == "bwd_scale" else 1.0)
    dp_mult = (1.0 / inv_keep) if mutant == "no_inv_keep" else f32(1.0, qf)
    if family == "generic":
        return _emulate_generic(qf, kf, vf, dof, scale_f, scale_b, keep_mask, drop_mult, inv_keep, mutant, dp_mult)
    assert family in ("whole", "stream"), family
    neg = float("-inf")
    S = qf @ kf.transpose(2, 3)                                                          # F1
    if keep_mask is not None:
        S = S.masked_fill(~keep_mask, neg)
    sc = scale_f * f32(LOG2E, qf)
    aux = {}
    if family == "whole":
        mx = S.amax(-1, keepdim=True)                                                    # F2
        dead = mx == neg
        mref = torch.where(dead, torch.zeros_like(mx), mx * sc)
        p = torch.exp2(_fms(S, sc, mref))                                                # F3
        l = p.sum(-1, keepdim=True)
        pb = _bf(p)                                                                      # F4
        l_lse = (p * keep).sum(-1, keepdim=True) if (mutant == "lse_dropped" and keep is not None) else l
        if keep is not None:
            pb = pb * keep
        o = pb @ vf
        m_sc = mx * sc
    else:
        Sk = kf.shape[2]
        m = torch.full_like(S[..., :1], neg)
        l, l_lse = torch.zeros_like(m), torch.zeros_like(m)
        o = torch.zeros_like(qf)
        amin = torch.full_like(m, float("inf"))
        for k0 in range(0, Sk, KB):
            Sb = S[..., k0:k0 + KB]
            mn = torch.maximum(m, Sb.amax(-1, keepdim=True))                             # F2'
            alpha = torch.exp2((m - mn) * sc)
            if k0 > 0:
                amin = torch.minimum(amin, alpha)
                if mutant == "alpha1":
                    alpha = torch.ones_like(alpha)
            m = mn
            p = torch.exp2(_fms(Sb, sc, mn * sc))                                        # F3'
            l = l * alpha + p.sum(-1, keepdim=True)
            pb = _bf(p)
            kb = None if keep is None else keep[..., k0:k0 + KB]
            if kb is not None:
                pb = pb * kb
            l_lse = l_lse * alpha + ((p * kb) if (mutant == "lse_dropped" and kb is not None) else p).sum(-1, keepdim=True)
            o = o * alpha + pb @ vf[:, :, k0:k0 + KB]
        dead = m == neg
        m_sc = m * sc
        aux["alpha_min"] = amin.squeeze(-1)
    lse = torch.where(dead, torch.full_like(m_sc, float("inf")), (m_sc + torch.log2(l_lse)) * f32(1.0 / LOG2E, qf))   # F5
    onorm = torch.where(dead, torch.zeros_like(l), inv_keep / l)
    O = _bf(o * onorm)                                                                   # F6
    # ---- backward
    scb = scale_b * f32(LOG2E, qf)
    lse2 = lse * f32(LOG2E, qf)                                                          # B1
    delta = (dof * O).sum(-1, keepdim=True) * (1.0 / inv_keep)
    if mutant == "no_delta":
        delta = torch.zeros_like(delta)
    pr = torch.exp2(_fms(S, scb, lse2))                                                  # B2 (S = -inf or lse2 = +inf -> 0)
    pkept = pr if keep is None else pr * keep
    dP = dof @ vf.transpose(2, 3) * dp_mult
    dS = (pkept.double() * dP.double() - (pr * delta).double()).float()
    if keep_mask is not None:
        dS[:, :, 0] = 0.0                                                                # B2'
    pkb, dsb = _bf(pkept), _bf(dS)                                                       # B3
    out = {"O": O, "LSE": lse.squeeze(-1),                                               # B4
           "dV": _bf(pkb.transpose(2, 3) @ dof * inv_keep),
           "dK": _bf(dsb.transpose(2, 3) @ qf * (scale_b * inv_keep)),
           "dQ": _bf(dsb @ kf * (scale_b * inv_keep))}
    out.update(aux)
    return out


def _emulate_generic(qf, kf, vf, dof, scale_f, scale_b, keep_mask, drop_mult, inv_keep, mutant, dp_mult):
    assert keep_mask is None, "attention_generic.hip has no mask mode"
    mult = torch.ones((), device=qf.device) if drop_mult is None else drop_mult.float()
    s = (qf * scale_f) @ kf.transpose(2, 3)                                              # G1
    mx = s.amax(-1, keepdim=True)
    p = torch.exp(s - mx)
    l = p.sum(-1, keepdim=True)
    l_lse = (p * (mult != 0)).sum(-1, keepdim=True) if (mutant == "lse_dropped" and drop_mult is not None) else l
    lse = mx + torch.log(l_lse)                                                          # G2
    pr = _bf(p * (1.0 / l) * mult)                                                       # G3
    O = _bf(pr @ vf)                                                                     # G4
    delta = (dof * O).sum(-1, keepdim=True)                                              # G5
    if mutant == "no_delta":
        delta = torch.zeros_like(delta)
    sb = (qf * scale_b) @ kf.transpose(2, 3) if mutant == "bwd_scale" else s
    pk = torch.exp(sb - lse)
    dP = dof @ vf.transpose(2, 3)
    dS = _bf(pk * (dP * (mult * dp_mult) - delta) * scale_b)                             # G6
    Pd = _bf(pk * mult)
    return {"O": O, "LSE": lse.squeeze(-1), "dQ": _bf(dS @ kf),                          # G7
            "dK": _bf(dS.transpose(2, 3) @ qf), "dV": _bf(Pd.transpose(2, 3) @ dof)}


# ------------------------------------------------------------------------------------------------ bound
def unit_max(x):
    """max |x| over each (batch, head) unit, float64; NaN (an unwritten output) counts as inf."""
    d = torch.nan_to_num(x.double().abs(), nan=float("inf"))
    return d.reshape(*d.shape[:2], -1).amax(-1)


def err_ref(emu, ref):
    """Per unit and output: max |emulate - ref64|."""
    return {k: unit_max(emu[k].double() - ref[k]) for k in OUTPUTS}


def bounds(emu, ref):
    """Per unit and output: MARGIN x max(err_ref, FLOOR) (module docstring).  Returns (bound, err_ref), dicts of [B, heads]."""
    er = err_ref(emu, ref)
    tol = {}
    for k in OUTPUTS:
        big = unit_max(ref[k])
        floor = 2.0 ** -21 * big.clamp(min=1.0) if k == "LSE" else 2.0 ** -9 * big
        tol[k] = MARGIN * torch.maximum(er[k], floor)
    return tol, er


def causal_pad_mask(ids, Sq, Sk, pad_id=1, diag=0, pads=True):
    """[B, 1, Sq, Sk] bool: key <= query + diag, and (``pads``) key not a pad.  diag != 0 and pads = False are the mask mutants."""
    keep = torch.ones(Sq, Sk, dtype=torch.bool, device=ids.device).tril(diag)[None, None]
    if pads:
        keep = keep & (ids[:, :Sk] != pad_id)[:, None, None, :]
    return keep.expand(ids.shape[0], 1, Sq, Sk)


def pad_tail_ids(B, Sk, gen):
    """Labels with a pad tail as in tests/test_ops_gpu.py::test_attention_fwd_bwd: image b keeps its first 3 + 5 b tokens."""
    ids = torch.randint(5, 50, (B, Sk + 1), device=gen.device, generator=gen, dtype=torch.int64)
    for b in range(B):
        ids[b, 3 + 5 * b:] = 1
    return ids


# ------------------------------------------------------------------------------------------------ the cases of both test modules
# (family, head dims, mode, [(Sq, Sk)]): the smallest shapes that reach each kernel instance (tests/test_attention_peaked_gpu.py)
CASES = [
    ("whole", (64,), 0, [(161, 161), (60, 160), (100, 100), (192, 176), (257, 257), (9, 9)]),
    ("whole", (64,), 1, [(23, 23), (127, 127)]),
    ("whole", (96,), 0, [(37, 37), (161, 161), (257, 257), (60, 288)]),
    ("stream", (64, 96), 0, [(37, 37), (130, 200), (300, 385), (60, 513), (513, 40)]),
    ("generic", (32, 128), 0, [(70, 70), (161, 161)]),
]


def all_cases():
    return [(fam, D, mode, Sq, Sk) for fam, Ds, mode, shapes in CASES for D in Ds for Sq, Sk in shapes]


def case_seed(D, mode, Sq, Sk):
    return 1009 * Sq + 31 * Sk + 7 * D + mode


def drop_key(Sq, Sk):
    return 4099 + 3 * Sq + 5 * Sk

