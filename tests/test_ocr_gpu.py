"""ocr_lightning row, GPU side: every kernel of csrc/ocr.hip through the C ABI against torch's own CPU modules
(the reference's dependencies: nn.CTCLoss, nn.LSTM, nn.SmoothL1Loss, nn.Conv2d, nn.BatchNorm2d, nn.MaxPool2d, optim.Adam), then
kzv.ocr_model.OCRModel against oracle/ocr_oracle.py -- forward, _shared_step loss, every gradient, an Adam step -- and the
reference's own model tests (output shapes on randn(2, 3, 64, 128); singles == batched).  Tolerances: the GEMM operands are bf16
(2^-8 relative per operand, fp32 accumulation); the reference runs this model in fp32, so "1e-6" there is "a few 1e-2 of the
tensor's scale" here -- stated per assertion."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from kzv import _lib as L
from kzv.ocr_data import CHAR_TO_IDX, IDX_TO_CHAR
from kzv.ocr_model import OCRModel
from oracle.ocr_oracle import OCROracle

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return L.load()


@pytest.fixture(autouse=True)
def _bf16_operands_for_the_per_op_tests():
    """kzv_ocr_set_precision is process-wide (kzv.OCRModel sets it before each of its passes): the per-operator tests below pass bf16
    buffers, so each test starts from the bf16 setting whatever model ran before it."""
    L.check(L.load().kzv_ocr_set_precision(0), "ocr_set_precision")
    yield


def _st():
    return torch.cuda.current_stream().cuda_stream


def _bf(x):
    return x.to(torch.bfloat16).to(torch.float32)


# ------------------------------------------------------------------------------------------------- CTC
@pytest.mark.parametrize("T,B,Cc,lens", [(1, 6, 7, [1, 0, 2, 1, 3, 1]), (12, 5, 9, [3, 5, 0, 12, 1]), (20, 4, 5, [7, 10, 2, 13]), (6, 3, 4, [6, 7, 3])])
def test_ctc_loss_and_gradient_match_torch(lib, T, B, Cc, lens):
    """nn.CTCLoss(blank=0, zero_infinity=True) on log_softmax(logits): per-sample negative log-likelihoods and the gradient with
    respect to the LOGITS under per-sample weights (the reduction the caller folds in), T = 1 (the model's case) and T > 1, with
    repeated labels, empty targets, targets as long as the input and infeasible ones (longer than the input -> inf -> 0)."""
    torch.manual_seed(T * 10 + B)
    logits = torch.randn(T, B, Cc, requires_grad=True)
    Lmax = max(max(lens), 1)
    tg = torch.randint(1, Cc, (B, Lmax))
    tg[0, :2] = tg[0, 0] if Lmax >= 2 else tg[0, :2]                # a repeated label needs a blank between
    tl = torch.tensor(lens)
    il = torch.full((B,), T)
    w = torch.rand(B) + 0.5
    lp = F.log_softmax(logits, dim=2)
    per = F.ctc_loss(lp, tg, il, tl, blank=0, reduction="none", zero_infinity=True)
    (per * w).sum().backward()
    dlp = torch.empty(T, B, Cc, device=DEV)
    lgd, tgd, ild, tld, wd = logits.detach().to(DEV).contiguous(), tg.to(DEV), il.to(DEV), tl.to(DEV), w.to(DEV)      # kept alive across the launches
    L.check(lib.kzv_ocr_log_softmax(lgd.data_ptr(), dlp.data_ptr(), T * B, Cc, _st()), "lsm")
    assert (dlp.cpu() - lp.detach()).abs().max() < 1e-5
    S = 2 * Lmax + 1
    scratch = torch.empty(2 * B * T * S, device=DEV)
    nll, g = torch.empty(B, device=DEV), torch.empty(T, B, Cc, device=DEV)
    L.check(lib.kzv_ocr_ctc(dlp.data_ptr(), tgd.data_ptr(), Lmax, ild.data_ptr(), tld.data_ptr(), T, B, Cc, 0, 1, Lmax,
                            scratch.data_ptr(), nll.data_ptr(), wd.data_ptr(), g.data_ptr(), _st()), "ctc")
    assert torch.allclose(nll.cpu(), per.detach(), atol=2e-4, rtol=1e-5), (nll.cpu(), per)
    assert (g.cpu() - logits.grad).abs().max() < 2e-5 * max(1.0, logits.grad.abs().max().item())
    if any(n > T for n in lens):
        assert float(nll.cpu()[[i for i, n in enumerate(lens) if n > T][0]]) == 0.0


def test_ctc_whole_page_labels_against_a_length_one_sequence(lib):
    """ocr_lightning's labels are whole-page texts (dataset.py) while the model emits ONE time step: every label longer than one
    character is infeasible, and nn.CTCLoss(zero_infinity=True) gives it loss 0 and no gradient.  The launch must not be sized by
    the longest label of the batch (a 600-character label used to be refused)."""
    torch.manual_seed(9)
    T, B, Cc = 1, 4, 11
    lens = [700, 1, 0, 633]
    Lmax = max(lens)
    logits = torch.randn(T, B, Cc, requires_grad=True)
    tg = torch.randint(1, Cc, (B, Lmax))
    tl, il = torch.tensor(lens), torch.full((B,), T)
    w = torch.rand(B) + 0.5
    lp = F.log_softmax(logits, dim=2)
    per = F.ctc_loss(lp, tg, il, tl, blank=0, reduction="none", zero_infinity=True)
    (per * w).sum().backward()
    tgd, ild, tld, wd = tg.to(DEV), il.to(DEV), tl.to(DEV), w.to(DEV)
    dlp = lp.detach().to(DEV).contiguous()
    scratch = torch.empty(2 * B * T * (2 * min(Lmax, T) + 1), device=DEV)          # the documented size
    nll, g = torch.full((B,), -1.0, device=DEV), torch.full((T, B, Cc), 7.0, device=DEV)
    L.check(lib.kzv_ocr_ctc(dlp.data_ptr(), tgd.data_ptr(), Lmax, ild.data_ptr(), tld.data_ptr(), T, B, Cc, 0, 1, Lmax,
                            scratch.data_ptr(), nll.data_ptr(), wd.data_ptr(), g.data_ptr(), _st()), "ctc")
    assert torch.allclose(nll.cpu(), per.detach(), atol=2e-4, rtol=1e-5)
    assert float(nll[0]) == 0.0 and float(nll[3]) == 0.0
    assert torch.all(g[:, 0] == 0) and torch.all(g[:, 3] == 0)
    assert (g.cpu() - logits.grad).abs().max() < 2e-5 * max(1.0, logits.grad.abs().max().item())


# ------------------------------------------------------------------------------------------------- fp32 arithmetic (the reference's)
@pytest.mark.parametrize("M,N,K,nv,resid", [(100, 64, 64, 64, False), (517, 132, 192, 130, True), (16, 1024, 512, 1024, False),
                                            (512, 512, 4608, 512, True), (8200, 64, 576, 64, False)])
def test_gemm_nt_f32_matches_fp64(lib, M, N, K, nv, resid):
    """kzv_gemm_nt_f32 (f32-input MFMA: exact fp32 products, fp32 accumulation) against fp64 products of the same operands: ragged M,
    n_valid < N (zeroed columns), bias, RESID, shapes that split the reduction over workgroups (few tiles) and shapes that do not."""
    torch.manual_seed(M + K)
    A, B = torch.randn(M, K, device=DEV), torch.randn(nv, K, device=DEV) * 0.1
    bias, res = torch.randn(nv, device=DEV), torch.randn(M, N, device=DEV)
    out = torch.full((M, N), 7.0, device=DEV)
    a = L.kzv_gemm_nt_args(A=A.data_ptr(), lda=K, B=B.data_ptr(), ldb=K, C=out.data_ptr(), ldc=N, bias=bias.data_ptr(), resid=res.data_ptr() if resid else None,
                           ldr=N, aux=None, ldaux=0, M=M, N=N, K=K, n_valid=nv, drop_p=0.0, drop_key=0)
    L.check(lib.kzv_gemm_nt_f32(C.byref(a), L.EPI_RESID if resid else L.EPI_F32, _st()), "gemm_nt_f32")
    want = A.double() @ B.double().t() + bias.double()
    got = out.double()
    if resid:
        want = want + res[:, :nv].double()
        assert torch.equal(out[:, nv:], res[:, nv:])                   # padded columns: 0 + residual
    else:
        assert torch.all(out[:, nv:] == 0)
    scale = want.abs().max().item()
    assert (got[:, :nv] - want).abs().max().item() < 3e-6 * scale, (got[:, :nv] - want).abs().max().item() / scale      # fp32 accumulation order only
    first = out.clone()
    L.check(lib.kzv_gemm_nt_f32(C.byref(a), L.EPI_RESID if resid else L.EPI_F32, _st()), "gemm_nt_f32")
    assert torch.equal(out, first)                                     # fixed summation order: bit-reproducible


@pytest.mark.parametrize("Mt,N,K,ns", [(16, 1024, 512, 1024), (131, 64, 192, 64), (8200, 64, 576, 64), (512, 512, 4608, 512), (33, 192, 512, 150)])
def test_gemm_tn_f32_matches_fp64(lib, Mt, N, K, ns):
    torch.manual_seed(Mt + N)
    P, Q = torch.randn(Mt, N, device=DEV), torch.randn(Mt, K, device=DEV)
    init = torch.randn(ns, K, device=DEV)
    O, db = init.clone(), torch.ones(ns, device=DEV)
    a = L.kzv_gemm_tn_args(P=P.data_ptr(), ldp=N, Q=Q.data_ptr(), ldq=K, OUT=O.data_ptr(), ldo=K, Mtok=Mt, N=N, K=K, n_store=ns, dbias=db.data_ptr())
    L.check(lib.kzv_gemm_tn_f32(C.byref(a), _st()), "gemm_tn_f32")
    want = init.double() + (P[:, :ns].double().t() @ Q.double())
    assert (O.double() - want).abs().max().item() < 3e-6 * want.abs().max().item()
    wb = 1.0 + P[:, :ns].double().sum(0)
    assert (db.double() - wb).abs().max().item() < 3e-6 * max(1.0, wb.abs().max().item())


def test_fp32_model_singles_equal_batched_and_outputs_match_the_oracle_at_full_depth():
    """ocr_lightning/tests/test_model.py:48-76 at the reference's own precision: OCRModel(precision="fp32") at full ResNet34 depth in
    eval mode -- singles == batched within 1e-5 of the output scale (the reference asserts atol 1e-6 on outputs of order 0.1; a
    row's result does not depend on the batch here either, what remains is the split of a short reduction over workgroups) and the
    outputs within 1e-4 of the fp32 oracle (36 convolutions deep; bf16 operands gave 5e-2)."""
    c2i, i2c = _vocab()
    m = OCRModel(c2i, i2c, learning_rate=1e-4, max_boxes=10, init_seed=1, precision="fp32").eval()
    torch.manual_seed(0)
    x = torch.randn(2, 3, 64, 128)
    out = m(x)
    a, b = m(x[:1]), m(x[1:])
    for k in ("pred_boxes", "pred_logits"):
        scale = max(1.0, out[k].abs().max().item())
        assert (out[k][0] - a[k][0]).abs().max().item() < 1e-5 * scale and (out[k][1] - b[k][0]).abs().max().item() < 1e-5 * scale, k
    o = OCROracle(len(c2i), 0, max_boxes=10)
    o.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()}, strict=True)
    with torch.no_grad():
        ref = o.eval()(x)
    for k in ("pred_boxes", "pred_logits"):
        assert (out[k].cpu() - ref[k]).abs().max().item() < 1e-4 * max(1.0, ref[k].abs().max().item()), k


def _fp32_step_against_float64(blocks, widths, exact_masks):
    """One training step of OCRModel(precision="fp32") and of the oracle in fp32 and in float64 (the exact value for these weights).
    Returns per parameter (engine error, torch-fp32 error) against float64 as relative L2 norms, the number of ReLU outputs whose
    sign differs between the engine and the float64 oracle, and the losses.  exact_masks: the float64 oracle replays the ENGINE's
    ReLU masks (tests/_replay-style), so that a pre-activation within rounding of zero is not a 100 % local difference."""
    c2i, i2c = _vocab()
    mb = 6
    m = OCRModel(c2i, i2c, learning_rate=1e-3, max_boxes=mb, init_seed=2, precision="fp32", blocks=blocks, widths=widths)
    sd0 = {k: v.cpu() for k, v in m.state_dict().items()}
    batch = _batch(6, 64, 160, mb, seed=4)
    m.train(); m.zero_grad()
    got = m.training_step(batch, 0)
    masks = m.relu_masks_of_last_step()
    m.backward()
    torch.cuda.synchronize()

    def oracle(dtype, replay):
        o = OCROracle(len(c2i), 0, max_boxes=mb, blocks=blocks, widths=widths)
        o.load_state_dict(sd0, strict=True)
        o = o.to(dtype).train()
        o.relu_record["seen"] = []
        if replay:
            o.relu_masks.extend(masks)
        b = dict(batch, images=batch["images"].to(dtype), bounding_boxes_batch=batch["bounding_boxes_batch"].to(dtype))
        total, loc, rec = o.shared_step(b, c2i)
        total.backward()
        return o, float(total.detach())
    o32, t32 = oracle(torch.float32, False)
    o64, t64 = oracle(torch.float64, False)
    flips = sum(int((a != b).sum()) for a, b in zip(masks, o64.relu_record["seen"]))
    elems = sum(a.numel() for a in masks)
    if exact_masks:
        o64, t64 = oracle(torch.float64, True)
    g64 = dict(o64.named_parameters())
    errs = {}
    for name, p in o32.named_parameters():
        g = m.grad(name).cpu()
        want = p.grad if p.grad is not None else torch.zeros_like(p)
        if "weight_hh" in name:
            assert g.abs().max().item() == 0 and want.abs().max().item() == 0
            continue
        exact = g64[name].grad
        errs[name] = (float((g.double() - exact).norm() / (exact.norm() + 1e-300)), float((want.double() - exact).norm() / (exact.norm() + 1e-300)),
                      float((g - want).norm() / (want.norm() + 1e-30)), (g - want).abs().max().item() / max(want.abs().max().item(), 1e-30))
    run = {k: (m.buffers[k].cpu(), v) for k, v in o32.state_dict().items() if "running" in k}
    return errs, flips, elems, (got, t32, t64), run


def test_fp32_training_step_is_as_exact_as_torch_fp32_on_a_four_stage_trunk():
    """All four stage shapes (64 .. 512 channels, the strided 1x1 shortcuts, reductions of 576 .. 4608 split over workgroups) on a
    (1, 1, 1, 1) trunk: measured against the oracle in float64, EVERY gradient of the fp32 engine is within 3 x the error torch's own
    fp32 arithmetic makes (observed 1e-6 .. 3e-6 on both sides).  The reference trains this model in fp32
    (ocr_lightning/train.py:132-140): this is its arithmetic, not the bf16-operand approximation of round 3."""
    errs, flips, elems, (got, t32, t64), run = _fp32_step_against_float64((1, 1, 1, 1), (64, 128, 256, 512), exact_masks=False)
    assert abs(got - t64) < 1e-5 * max(1.0, t64)
    assert flips == 0, f"{flips} of {elems} ReLU signs differ from float64"
    worst = max(errs.items(), key=lambda e: e[1][0] / max(e[1][1], 1e-9))
    for name, (e_engine, e_torch, _, _) in errs.items():
        assert e_engine < 3.0 * e_torch + 2e-6, (name, e_engine, e_torch)
    print("fp32 (1,1,1,1): worst engine / torch-fp32 error against float64:", worst[0], worst[1][:2])


def test_fp32_full_depth_training_step_matches_the_oracle_without_mask_replay():
    """The whole training step of the FULL ResNet34 trunk (3, 4, 6, 3) in train mode against oracle/ocr_oracle.py -- the comparison
    round 3 could only make on a 2-block trunk and by direction.
    (1) Nothing replayed: losses within 1e-4, every parameter gradient within 1 % of torch's fp32 result in relative L2 norm (and
        5 % of its largest entry: one flipped ReLU below moves single weight-gradient entries by ~2 %), running statistics within 1e-4.
    (2) Among the ~3.5 million ReLU outputs of this step a handful of pre-activations sit within fp32 rounding of zero, and whichever
        way an implementation rounds them is a 100 % local difference of the gradient (observed: 1 - 3 of them, 0.4 % of a
        gradient's norm); any two fp32 implementations differ there.  So: at most 1e-5 of the ReLU signs may differ from the float64
        oracle's, and with the engine's masks replayed through the float64 oracle every gradient is within 3 x torch-fp32's own
        error + 1e-5 of the exact value."""
    errs, flips, elems, (got, t32, t64), run = _fp32_step_against_float64((3, 4, 6, 3), (64, 128, 256, 512), exact_masks=True)
    assert abs(got - t32) < 1e-4 * max(1.0, t32)
    assert flips <= 1e-5 * elems, f"{flips} of {elems} ReLU signs differ from float64"
    worst = ("", 0.0)
    for name, (e_engine, e_torch, rel32, max32) in errs.items():
        assert rel32 < 1e-2 and max32 < 5e-2, (name, rel32, max32)
        worst = max(worst, (name, e_engine), key=lambda e: e[1])
        assert e_engine < 3.0 * e_torch + 1e-5, (name, e_engine, e_torch)
    print(f"fp32 full depth: {flips} of {elems} ReLU signs differ from float64; worst engine error against float64 with the masks replayed", worst)
    for k, (a, v) in run.items():
        assert (a - v).abs().max().item() < 1e-4 * max(1.0, v.abs().max().item()), k


# ------------------------------------------------------------------------------------------------- LSTM cell / SmoothL1 / Adam
def test_lstm_cell_matches_nn_lstm_on_a_length_one_sequence(lib):
    """One direction of nn.LSTM on [B, 1, I] with zero state: gates from torch (fp32), cell forward and the gate gradients."""
    torch.manual_seed(3)
    B, I, H = 5, 64, 256
    lstm = nn.LSTM(I, H, num_layers=1, batch_first=True)
    x = torch.randn(B, 1, I, requires_grad=True)
    out, _ = lstm(x)
    dh = torch.randn(B, H)
    out[:, 0].backward(dh)
    gates = (x.detach()[:, 0] @ lstm.weight_ih_l0.detach().t() + lstm.bias_ih_l0.detach()).to(DEV)
    h32 = torch.empty(B, 2 * H, device=DEV); h16 = torch.empty(B, 2 * H, dtype=torch.bfloat16, device=DEV)
    bhh = lstm.bias_hh_l0.detach().to(DEV)
    L.check(lib.kzv_ocr_lstm_cell_fwd(gates.data_ptr(), bhh.data_ptr(), h32[:, H:].data_ptr(), h16[:, H:].data_ptr(), 2 * H, B, H, _st()), "cell")
    assert (h32[:, H:].cpu() - out.detach()[:, 0]).abs().max() < 1e-5
    dg = torch.empty(B, 4 * H, dtype=torch.bfloat16, device=DEV)
    dhp = torch.zeros(B, 2 * H, device=DEV); dhp[:, H:] = dh.to(DEV)
    L.check(lib.kzv_ocr_lstm_cell_bwd(gates.data_ptr(), bhh.data_ptr(), dhp[:, H:].data_ptr(), 2 * H, dg.data_ptr(), B, H, _st()), "cell_bwd")
    dgf = dg.float().cpu()
    assert (dgf.sum(0) - lstm.bias_ih_l0.grad).abs().max() < 2e-2 * lstm.bias_ih_l0.grad.abs().max()      # bf16 gate gradients
    assert (dgf.t() @ x.detach()[:, 0] - lstm.weight_ih_l0.grad).abs().max() < 2e-2 * lstm.weight_ih_l0.grad.abs().max()
    assert lstm.weight_hh_l0.grad.abs().max() == 0 and dgf[:, H:2 * H].abs().max() == 0                  # zero state: W_hh and the forget gate get nothing


def test_smooth_l1_box_loss_matches_the_reference_loop(lib):
    torch.manual_seed(4)
    B, mb, gtb = 5, 6, 8
    pred = (torch.randn(B, mb, 4) * 2).requires_grad_(True)
    gt = torch.randn(B, gtb, 4) * 2
    counts = [3, 0, 8, 6, 1]
    fn = nn.SmoothL1Loss(reduction="mean")
    tot, nv = 0.0, 0
    for i in range(B):                                   # model.py:105-120
        n = min(counts[i], mb)
        if n == 0:
            continue
        tot = tot + fn(pred[i, :n], gt[i, :n]); nv += 1
    ref = tot / nv
    ref.backward()
    loss = torch.zeros(1, device=DEV); dp = torch.empty(B, mb * 4, device=DEV)
    pd, gd, cd, zd = pred.detach().to(DEV).reshape(B, mb * 4).contiguous(), gt.to(DEV).contiguous(), torch.tensor(counts, dtype=torch.int32, device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV)
    L.check(lib.kzv_ocr_smooth_l1_boxes(pd.data_ptr(), mb, gd.data_ptr(), gtb, cd.data_ptr(), B, loss.data_ptr(), dp.data_ptr(), _st()), "sl1")
    assert abs(float(loss) - float(ref)) < 1e-5 and (dp.cpu().view(B, mb, 4) - pred.grad).abs().max() < 1e-6
    loss.zero_()
    L.check(lib.kzv_ocr_smooth_l1_boxes(pd.data_ptr(), mb, None, 0, zd.data_ptr(), B, loss.data_ptr(), dp.data_ptr(), _st()), "sl1 empty")
    assert float(loss) == 0.0 and dp.abs().max() == 0


def test_adam_matches_torch_optim(lib):
    torch.manual_seed(5)
    p0 = torch.randn(1000)
    p = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=1e-2)
    pd, m, v = p0.to(DEV), torch.zeros(1000, device=DEV), torch.zeros(1000, device=DEV)
    for step in range(1, 6):
        g = torch.randn(1000) * (0.1 if step % 2 else 3.0)
        p.grad = g.clone(); opt.step()
        gd = g.to(DEV)
        L.check(lib.kzv_ocr_adam(pd.data_ptr(), gd.data_ptr(), m.data_ptr(), v.data_ptr(), 1000, 1e-2, 0.9, 0.999, 1e-8, step, _st()), "adam")
        assert (pd.cpu() - p.detach()).abs().max() < 1e-6


# ------------------------------------------------------------------------------------------------- conv / BN / pools
def _to_nhwc16(x):
    return x.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).to(DEV)


@pytest.mark.parametrize("cin,cout,k,stride,pad,H,W", [(3, 64, 7, 2, 3, 32, 48), (64, 64, 3, 1, 1, 9, 13), (64, 128, 3, 2, 1, 16, 24), (64, 128, 1, 2, 0, 16, 24)])
def test_convolution_forward_input_and_weight_gradients(lib, cin, cout, k, stride, pad, H, W):
    """nn.Conv2d as im2col + the MFMA GEMM (forward), the GEMM against the transposed packed weight + the gather (input
    gradient) and kzv_gemm_tn on the column matrix (weight gradient), on bf16-rounded operands, against F.conv2d in fp32."""
    torch.manual_seed(k * 100 + cin)
    N = 2
    x = _bf(torch.randn(N, cin, H, W)).requires_grad_(True)
    w = _bf(torch.randn(cout, cin, k, k) / (k * k * cin) ** 0.5).requires_grad_(True)
    y = F.conv2d(x, w, stride=stride, padding=pad)
    dy = _bf(torch.randn_like(y))
    y.backward(dy)
    Ho, Wo = y.shape[2:]
    Kp = (k * k * cin + 63) // 64 * 64
    M = N * Ho * Wo
    x16 = _to_nhwc16(x.detach())
    cols = torch.empty(M, Kp, dtype=torch.bfloat16, device=DEV)
    L.check(lib.kzv_ocr_im2col(x16.data_ptr(), cols.data_ptr(), N, H, W, cin, k, k, stride, pad, Kp, _st()), "im2col")
    wp = torch.empty(cout, Kp, dtype=torch.bfloat16, device=DEV); wt = torch.empty(Kp, cout, dtype=torch.bfloat16, device=DEV)
    wd = w.detach().to(DEV).contiguous()
    L.check(lib.kzv_ocr_conv_weight(wd.data_ptr(), wp.data_ptr(), wt.data_ptr(), cout, cin, k, k, Kp, _st()), "pack")
    out = torch.empty(M, cout, device=DEV)
    a = L.kzv_gemm_nt_args(A=cols.data_ptr(), lda=Kp, B=wp.data_ptr(), ldb=Kp, C=out.data_ptr(), ldc=cout, M=M, N=cout, K=Kp, n_valid=0)
    L.check(lib.kzv_gemm_nt(C.byref(a), L.EPI_F32, _st()), "gemm")
    ref = y.detach().permute(0, 2, 3, 1).reshape(M, cout)
    assert (out.cpu() - ref).abs().max() < 2e-3 * max(1.0, ref.abs().max().item())
    dy16 = dy.permute(0, 2, 3, 1).reshape(M, cout).contiguous().to(torch.bfloat16).to(DEV)
    gp = torch.zeros(cout, Kp, device=DEV)
    t = L.kzv_gemm_tn_args(P=dy16.data_ptr(), ldp=cout, Q=cols.data_ptr(), ldq=Kp, OUT=gp.data_ptr(), ldo=Kp, Mtok=M, N=cout, K=Kp, n_store=0, dbias=None)
    L.check(lib.kzv_gemm_tn(C.byref(t), _st()), "wgrad")
    gw = torch.zeros(cout, cin, k, k, device=DEV)
    L.check(lib.kzv_ocr_conv_wgrad_unpack(gp.data_ptr(), gw.data_ptr(), cout, cin, k, k, Kp, _st()), "unpack")
    assert (gw.cpu() - w.grad).abs().max() < 5e-3 * max(1.0, w.grad.abs().max().item())
    if cin % 4 == 0:
        dcols = torch.empty(M, Kp, device=DEV)
        a = L.kzv_gemm_nt_args(A=dy16.data_ptr(), lda=cout, B=wt.data_ptr(), ldb=cout, C=dcols.data_ptr(), ldc=Kp, M=M, N=Kp, K=cout, n_valid=0)
        L.check(lib.kzv_gemm_nt(C.byref(a), L.EPI_F32, _st()), "dgrad")
        dx = torch.full((N * H * W, cin), 0.5, device=DEV)
        L.check(lib.kzv_ocr_col2im(dcols.data_ptr(), dx.data_ptr(), N, H, W, cin, k, k, stride, pad, Kp, 1, _st()), "col2im")
        want = x.grad.permute(0, 2, 3, 1).reshape(N * H * W, cin) + 0.5
        assert (dx.cpu() - want).abs().max() < 5e-3 * max(1.0, want.abs().max().item())


@pytest.mark.parametrize("train,relu,resid", [(1, 1, 1), (1, 1, 0), (1, 0, 0), (0, 1, 1)])
def test_batchnorm_relu_residual_forward_backward(lib, train, relu, resid):
    torch.manual_seed(6 + train + 2 * relu)
    N, Cc, H, W = 3, 64, 5, 7
    M = N * H * W
    y = (torch.randn(N, Cc, H, W) * 2 + 0.3).requires_grad_(True)
    r = _bf(torch.randn(N, Cc, H, W)).requires_grad_(True) if resid else None
    bn = nn.BatchNorm2d(Cc)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(Cc) + 0.5); bn.bias.copy_(torch.randn(Cc) * 0.2)
        bn.running_mean.copy_(torch.randn(Cc) * 0.1); bn.running_var.copy_(torch.rand(Cc) + 0.5)
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    bn.train(bool(train))
    z = bn(y) + (r if resid else 0)
    a = F.relu(z) if relu else z
    da = torch.randn_like(a)
    a.backward(da)
    nh = lambda t: t.detach().permute(0, 2, 3, 1).reshape(M, Cc).contiguous()
    yd = nh(y).to(DEV)
    rm, rv = rm0.to(DEV), rv0.to(DEV)
    mean, rstd = torch.empty(Cc, device=DEV), torch.empty(Cc, device=DEV)
    out = torch.empty(M, Cc, dtype=torch.bfloat16, device=DEV)
    r16 = nh(r).to(torch.bfloat16).to(DEV) if resid else None
    gam, bet, scr = bn.weight.detach().to(DEV), bn.bias.detach().to(DEV), torch.empty(lib.kzv_ocr_bn_scratch_floats(M, Cc), device=DEV)
    L.check(lib.kzv_ocr_bn_fwd(yd.data_ptr(), M, Cc, gam.data_ptr(), bet.data_ptr(), rm.data_ptr(), rv.data_ptr(),
                               mean.data_ptr(), rstd.data_ptr(), L.ptr(r16), out.data_ptr(), relu, train, 1e-5, 0.1, scr.data_ptr(), _st()), "bn")
    assert (out.float().cpu() - nh(a)).abs().max() < 1e-2 * max(1.0, a.abs().max().item())                # bf16 output
    if train:
        assert (rm.cpu() - bn.running_mean).abs().max() < 1e-5 and (rv.cpu() - bn.running_var).abs().max() < 1e-4
    dz, dy = torch.empty(M, Cc, device=DEV), torch.empty(M, Cc, dtype=torch.bfloat16, device=DEV)
    dg, db = torch.zeros(Cc, device=DEV), torch.zeros(Cc, device=DEV)
    dad = nh(da).to(DEV)
    L.check(lib.kzv_ocr_bn_bwd(dad.data_ptr(), out.data_ptr(), yd.data_ptr(), M, Cc, mean.data_ptr(), rstd.data_ptr(),
                               gam.data_ptr(), dz.data_ptr(), dg.data_ptr(), db.data_ptr(), dy.data_ptr(), relu, train, scr.data_ptr(), _st()), "bn_bwd")
    if train:
        assert (dg.cpu() - bn.weight.grad).abs().max() < 2e-3 * max(1.0, bn.weight.grad.abs().max().item())
        assert (db.cpu() - bn.bias.grad).abs().max() < 2e-3 * max(1.0, bn.bias.grad.abs().max().item())
    assert (dy.float().cpu() - nh(y.grad)).abs().max() < 1e-2 * max(1.0, y.grad.abs().max().item())
    if resid:
        assert (dz.cpu() - nh(r.grad)).abs().max() < 1e-5


def test_pooling_forward_backward(lib):
    torch.manual_seed(8)
    N, Cc, H, W = 2, 64, 9, 14
    x = _bf(torch.randn(N, Cc, H, W)).requires_grad_(True)
    mp = F.max_pool2d(x, 3, 2, 1)
    g = torch.randn_like(mp)
    mp.backward(g)
    Ho, Wo = mp.shape[2:]
    x16 = _to_nhwc16(x.detach())
    out = torch.empty(N * Ho * Wo, Cc, dtype=torch.bfloat16, device=DEV); idx = torch.empty(N * Ho * Wo, Cc, dtype=torch.uint8, device=DEV)
    L.check(lib.kzv_ocr_maxpool_fwd(x16.data_ptr(), out.data_ptr(), idx.data_ptr(), N, H, W, Cc, _st()), "mp")
    assert torch.equal(out.float().cpu(), mp.detach().permute(0, 2, 3, 1).reshape(-1, Cc))
    dx = torch.empty(N * H * W, Cc, device=DEV)
    gd = g.permute(0, 2, 3, 1).reshape(-1, Cc).contiguous().to(DEV)
    L.check(lib.kzv_ocr_maxpool_bwd(gd.data_ptr(), idx.data_ptr(), dx.data_ptr(), N, H, W, Cc, _st()), "mp_bwd")
    assert (dx.cpu() - x.grad.permute(0, 2, 3, 1).reshape(-1, Cc)).abs().max() < 1e-6
    f32 = torch.empty(N, Cc, device=DEV); f16 = torch.empty(N, Cc, dtype=torch.bfloat16, device=DEV)
    L.check(lib.kzv_ocr_avgpool_fwd(x16.data_ptr(), f32.data_ptr(), f16.data_ptr(), N, H * W, Cc, _st()), "ap")
    assert (f32.cpu() - x.detach().mean((2, 3))).abs().max() < 1e-5
    dfe = torch.randn(N, Cc)
    dxa = torch.empty(N * H * W, Cc, device=DEV)
    dfd = dfe.to(DEV)
    L.check(lib.kzv_ocr_avgpool_bwd(dfd.data_ptr(), dxa.data_ptr(), N, H * W, Cc, _st()), "ap_bwd")
    assert (dxa.cpu().view(N, H * W, Cc) - dfe[:, None, :] / (H * W)).abs().max() < 1e-7


# ------------------------------------------------------------------------------------------------- the model
def _vocab():
    """A duplicate-free character set with the blank at index 0.  (The reference's placeholder VOCAB = '<blank>' + 'abc...' spells the
    blank token out character by character, so 'b', 'l', 'a', 'n', 'k' occur twice: the dict then has FEWER entries than its largest
    index, num_chars = len(char_to_idx) is too small and labels such as '7' index past the logits -- undefined behaviour in
    nn.CTCLoss.  The kernels clamp labels into the class range; the parity tests use a vocabulary where the question does not arise.)"""
    v = "_" + "abcdefghijklmnopqrstuvwxyz0123456789"
    return {ch: i for i, ch in enumerate(v)}, {i: ch for i, ch in enumerate(v)}


def test_model_forward_shapes_batch_consistency_and_hparams():
    """ocr_lightning/tests/test_model.py:28-86 against kzv.OCRModel at full ResNet34 depth (eval mode: running statistics)."""
    c2i, i2c = _vocab()
    m = OCRModel(c2i, i2c, learning_rate=1e-4, max_boxes=10, init_seed=1, precision="bf16").eval()
    torch.manual_seed(0)
    x = torch.randn(2, 3, 64, 128)
    out = m(x)
    assert set(out) == {"pred_boxes", "pred_logits"}
    assert out["pred_boxes"].shape == (2, 10, 4) and out["pred_logits"].shape == (2, 1, len(c2i))
    a, b = m(x[:1]), m(x[1:])
    for k in ("pred_boxes", "pred_logits"):        # reference: atol 1e-6 in fp32; here the GEMMs round their operands to bf16 (row results do not depend on the batch)
        scale = out[k].abs().max().item()
        assert (out[k][0] - a[k][0]).abs().max().item() < 1e-3 * max(1.0, scale) and (out[k][1] - b[k][0]).abs().max().item() < 1e-3 * max(1.0, scale)
    hp = m.hparams
    assert hp.max_boxes == 10 and hp.char_to_idx["a"] == c2i["a"] and hp.idx_to_char[1] == i2c[1] and hp.learning_rate == 1e-4
    assert hp.num_chars == len(c2i) and hp.blank_char_idx == c2i.get("<blank>", 0) == 0
    # the reference's key names and registration order (checked against the oracle built from torch modules the same way)
    o = OCROracle(len(c2i), 0, max_boxes=10)
    assert list(m.state_dict()) != [] and set(m.state_dict()) == set(o.state_dict())
    assert [k for k in o.state_dict() if k in m.offsets] == list(m.offsets)
    o.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()}, strict=True)
    with torch.no_grad():
        ref = o.eval()(x)
    for k in ("pred_boxes", "pred_logits"):        # 36 bf16 convolutions deep: a few 1e-2 of the output scale
        assert (out[k].cpu() - ref[k]).abs().max().item() < 5e-2 * max(1.0, ref[k].abs().max().item()), k


def _batch(B, H, W, max_boxes, seed):
    g = torch.Generator().manual_seed(seed)
    texts = ["a", "", "7", "zz", "q", "b"][:B]
    counts = [2, 0, max_boxes + 2, 1, 3, 1][:B]
    mc = max(counts)
    gt = torch.full((B, mc, 4), -1.0)
    for i, n in enumerate(counts):
        gt[i, :n] = torch.rand(n, 4, generator=g) * 3
    return {"images": torch.rand(B, 3, H, W, generator=g), "label_texts": texts, "bounding_boxes_batch": gt, "target_lengths": [len(t) for t in texts],
            "bbox_counts": counts, "image_paths": [""] * B}


def test_two_block_trunk_forward_loss_backward_and_adam_step_match_the_oracle():
    """The whole training step on a 2-stage trunk (one BasicBlock of 64, one of 128 with the strided 1x1 shortcut) in TRAIN mode
    (batch statistics): loc / rec / total loss of _shared_step (boxes: a sample without boxes and one with more than max_boxes;
    labels: an empty one and one longer than the length-1 sequence), every parameter gradient, the running statistics, and the
    parameters after one optim.Adam step.

    Gradients are compared twice.  (1) Against the plain fp32 oracle: the heads within 2 %; the trunk by direction (cosine) and
    relative L2 norm only, because the bf16 forward (~1 % error per activation) flips the ReLU mask of the ~0.5 % of pre-activations
    nearest to zero and every flipped element is a 100 % local error (observed: relative L2 7 - 16 %, cosine 0.985 - 0.999).
    (2) With the engine's own ReLU masks REPLAYED through the oracle (like the dropout-mask replay of the TrOCR path): what
    remains is GEMM-operand rounding, and every tensor must agree within 5 % of its largest entry."""
    c2i, i2c = _vocab()
    mb = 4
    m = OCRModel(c2i, i2c, learning_rate=1e-3, max_boxes=mb, blocks=(1, 1), widths=(64, 128), init_seed=3, precision="bf16")
    o = OCROracle(len(c2i), 0, max_boxes=mb, blocks=(1, 1), widths=(64, 128))
    sd0 = {k: v.cpu() for k, v in m.state_dict().items()}
    o.load_state_dict(sd0, strict=True)
    o.train()
    batch = _batch(6, 64, 96, mb, seed=9)
    total, loc, rec = o.shared_step(batch, c2i)
    total.backward()
    m.train(); m.zero_grad()
    got = m.training_step(batch, 0)
    assert abs(m.logged["train/loc_loss"][-1] - float(loc)) < 2e-2 * max(1.0, float(loc))
    assert abs(m.logged["train/rec_loss"][-1] - float(rec)) < 2e-2 * max(1.0, float(rec)) and abs(got - float(total)) < 2e-2 * max(1.0, float(total))
    masks = m.relu_masks_of_last_step()
    m.backward()
    torch.cuda.synchronize()
    for name, p in o.named_parameters():
        g = m.grad(name).cpu()
        want = p.grad if p.grad is not None else torch.zeros_like(p)
        if "weight_hh" in name:
            assert g.abs().max().item() == 0 and want.abs().max().item() == 0
            continue
        rel = float((g - want).norm() / (want.norm() + 1e-30))
        cos = float((g * want).sum() / (g.norm() * want.norm() + 1e-30))
        if name.startswith("feature_extractor"):
            assert rel < 0.3 and cos > 0.96, (name, rel, cos)
        else:
            assert (g - want).abs().max().item() < 0.02 * want.abs().max().item(), (name, rel)
    for k, v in o.state_dict().items():
        if "running" in k:
            assert (m.buffers[k].cpu() - v).abs().max().item() < 2e-2 * max(1.0, v.abs().max().item()), k
    # (2) mask replay
    o2 = OCROracle(len(c2i), 0, max_boxes=mb, blocks=(1, 1), widths=(64, 128))
    o2.load_state_dict(sd0, strict=True)
    o2.train()
    assert len(masks) == 5                                   # stem + 2 per BasicBlock
    o2.relu_masks.extend(masks)
    t2, _, _ = o2.shared_step(batch, c2i)
    assert not o2.relu_masks and abs(float(t2) - got) < 2e-2 * max(1.0, float(t2))
    t2.backward()
    worst = ("", 0.0)
    for name, p in o2.named_parameters():
        if "weight_hh" in name:
            continue
        g, want = m.grad(name).cpu(), p.grad
        err = (g - want).abs().max().item() / max(want.abs().max().item(), 1e-12)
        if name == "feature_extractor.0.weight":
            # the stem convolution sits below the max-pool, whose argmax is NOT replayed: window maxima that differ in fp32 but
            # round to the same bf16 value route their gradient to different pixels (observed: relative L2 0.086)
            assert float((g - want).norm() / want.norm()) < 0.2, (name, err)
            continue
        worst = max(worst, (name, err), key=lambda e: e[1])
        assert err < 0.05, (name, err)                       # observed: <= 0.02 everywhere
    print("mask replay: worst relative gradient error", worst)
    # one Adam step from the ORACLE's gradients on both sides isolates the optimizer kernel from the gradient tolerance
    opt = torch.optim.Adam(o.parameters(), lr=1e-3)
    opt.step()
    m.configure_optimizers()
    for name, p in o.named_parameters():
        m.grad(name).copy_((p.grad if p.grad is not None else torch.zeros_like(p)).to(DEV))
    m.optimizer_step()
    for name, p in o.named_parameters():
        assert (m.param(name).cpu() - p.detach()).abs().max().item() < 1e-6, name


def test_fit_steps_reduce_the_loss_and_eval_uses_running_statistics():
    c2i, i2c = _vocab()
    m = OCRModel(c2i, i2c, learning_rate=2e-3, max_boxes=4, blocks=(1, 1), widths=(64, 128), init_seed=5)
    m.configure_optimizers()
    batch = _batch(6, 32, 48, 4, seed=11)
    losses = [m.fit_step(batch, i) for i in range(25)]
    assert all(np.isfinite(losses)) and losses[-1] < 0.6 * losses[0], losses[::6]
    m.eval()
    v1 = m.validation_step(batch, 0); v2 = m.validation_step(batch, 0)
    assert abs(v1 - v2) < 1e-6 and np.isfinite(v1) and "val/total_loss" in m.logged      # (the box loss is summed with float atomics)
    from kzv.ocr_data import decode_ctc_output
    out = m(batch["images"])
    dec = [decode_ctc_output(out["pred_logits"][i].cpu(), i2c, 0) for i in range(6)]
    assert all(isinstance(d, str) and len(d) <= 1 for d in dec)      # a length-1 sequence decodes to one character or ''
    m.train()
    out = m(batch["images"])                               # batch statistics, as during the fit: the one-character labels are fitted
    dec = [decode_ctc_output(out["pred_logits"][i].cpu(), i2c, 0) for i in range(6)]
    assert dec[0] == "a" and dec[2] == "7" and dec[4] == "q" and dec[5] == "b", dec


def test_graph_replayed_fit_steps_equal_eager_ones():
    """fit_step replays the whole optimisation step (zero_grad, forward, losses, backward, Adam, operand refresh: ~200 launches on this
    trunk) from one captured hipGraph from the third step of a batch geometry on; the batch contents, the label texts and Adam's bias
    corrections reach it through device buffers.  Same parameters and losses as the launch-by-launch path on a stream of DIFFERENT
    batches (the box loss sums with float atomics: 1e-6)."""
    c2i, i2c = _vocab()
    ms = [OCRModel(c2i, i2c, learning_rate=2e-3, max_boxes=4, blocks=(1, 1), widths=(64, 128), init_seed=5) for _ in range(2)]
    ms[1].use_graph = False
    for m in ms:
        m.configure_optimizers()
    batches = [_batch(6, 32, 48, 4, seed=20 + i) for i in range(3)]
    batches[1]["label_texts"] = ["q", "zz", "", "a", "7", "abc" * 100]
    losses = [[m.fit_step(batches[i % 3], i) for i in range(7)] for m in ms]
    assert ms[0]._graphs and all(e.graph is not None for e in ms[0]._graphs.values()) and not ms[1]._graphs
    assert np.allclose(losses[0], losses[1], rtol=1e-5, atol=1e-6), (losses[0], losses[1])
    for name in ms[0].offsets:
        a, b = ms[0].param(name), ms[1].param(name)
        assert (a - b).abs().max().item() <= 1e-6 * max(1.0, b.abs().max().item()), name
    for k in ms[0].buffers:
        assert torch.allclose(ms[0].buffers[k].float(), ms[1].buffers[k].float(), rtol=1e-4, atol=1e-5), k      # (7 Adam steps amplify the 1e-7 of the atomics)
    assert ms[0]._optimizer.step_count == ms[1]._optimizer.step_count == 7


def test_a_captured_step_survives_a_workspace_that_grows_under_it():
    """a captured fit step bakes in the pointer of the fp32 GEMMs' split-K workspace, a later batch geometry with a larger
    request moves that workspace, and the earlier graph is replayed afterwards.  The workspace retires its old block instead of freeing
    it (csrc/dev_buf.h), so the replays compute what the launch-by-launch replica computes.  Geometry A (batch 6: split-K launches
    within the 1 MiB the workspace starts with) is captured, B (batch 12: on an MI355X a fresh process grows at batch 8, 16 and 32)
    must move a workspace -- kzv_scratch_growths() rises, or this test has not tested anything -- and A runs again from its old graph.  The workspaces are
    process-wide, so the scenario runs in a process of its own (tests/_ocr_growth_worker.py).  Tolerances: those of
    test_graph_replayed_fit_steps_equal_eager_ones (the same arithmetic on both sides; the box loss sums with float atomics)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _ocr_growth_worker as W
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_ocr_growth_worker.py"), "6", "12"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    g, e = out["graph"], out["eager"]
    a_end, b_end = W.A_FIRST - 1, W.A_FIRST + W.B_STEPS - 1
    print("growths", g["growths"], "captured", g["captured"], "param_err", out["param_err"])
    assert g["captured"][a_end] == 1, g["captured"]                          # A's step is a graph before B starts
    assert g["growths"][b_end] > g["growths"][a_end], g["growths"]           # B moved a workspace that A's graph points into
    assert g["captured"][b_end:] == [2] * (1 + W.A_AGAIN), g["captured"]     # A again: replayed, nothing captured anew
    assert e["captured"] == [0] * len(out["plan"])
    assert np.allclose(g["losses"], e["losses"], rtol=1e-5, atol=1e-6), (g["losses"], e["losses"])
    assert out["param_err"] <= 1e-6, out["param_err"]
    assert out["buffers_close"]
    assert out["steps"] == [len(out["plan"])] * 2


def test_optimizer_state_round_trips_in_adams_own_layout_and_a_resumed_run_continues_exactly():
    """the OCR checkpoints carry optim.Adam's state (Lightning's ``optimizer_states[0]``).  (1) The state_dict loads into a
    torch.optim.Adam over the oracle's parameters (same registration order) and equals what torch computes from the same gradients;
    (2) a second model that loads weights + optimizer state after 3 steps and takes 2 more ends where the uninterrupted 5-step run ends."""
    c2i, i2c = _vocab()
    kw = dict(learning_rate=2e-3, max_boxes=4, blocks=(1, 1), widths=(64, 128), init_seed=5)
    full, part = OCRModel(c2i, i2c, **kw), OCRModel(c2i, i2c, **kw)
    for m in (full, part):
        m.configure_optimizers(); m.use_graph = False
    batches = [_batch(6, 32, 48, 4, seed=40 + i) for i in range(5)]
    for i in range(5):
        full.fit_step(batches[i], i)
    o = OCROracle(len(c2i), 0, max_boxes=4, blocks=(1, 1), widths=(64, 128))
    o.load_state_dict({k: v.cpu() for k, v in part.state_dict().items()}, strict=True)
    opt = torch.optim.Adam(o.parameters(), lr=2e-3)
    for i in range(3):
        part.zero_grad(); part.training_step(batches[i], i); part.backward()
        for name, p in o.named_parameters():                     # torch's Adam on the ENGINE's gradients: isolates the state layout
            p.grad = part.grad(name).cpu().clone()
        part.optimizer_step(); opt.step()
        o.load_state_dict({k: v.cpu() for k, v in part.state_dict().items()}, strict=True)      # keep BN buffers / weights in step
    sd = part.optimizer_state_dict()
    ref = opt.state_dict()
    assert sd["param_groups"][0]["params"] == ref["param_groups"][0]["params"] and set(sd["state"]) == set(ref["state"])
    for i in ref["state"]:
        assert float(sd["state"][i]["step"]) == float(ref["state"][i]["step"]) == 3.0
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.allclose(sd["state"][i][k], ref["state"][i][k], rtol=1e-5, atol=1e-9), (i, k)
    torch.optim.Adam(o.parameters(), lr=1.0).load_state_dict(sd)                                   # torch accepts the layout
    resumed = OCRModel(c2i, i2c, **dict(kw, init_seed=99))
    resumed.use_graph = False
    resumed.load_state_dict(part.state_dict(), strict=True)
    resumed.load_optimizer_state_dict(sd)
    assert resumed._optimizer.step_count == 3
    for i in (3, 4):
        resumed.fit_step(batches[i], i)
    for name in full.offsets:
        a, b = resumed.param(name), full.param(name)
        assert (a - b).abs().max().item() <= 1e-6 * max(1.0, b.abs().max().item()), name


def test_training_step_accepts_whole_page_label_texts():
    """A page text of several hundred characters (what ocr_lightning's dataset yields) in the batch: the step runs, the long
    sample contributes rec loss 0 like nn.CTCLoss(zero_infinity=True) against one time step, the short ones still train."""
    c2i, i2c = _vocab()
    m = OCRModel(c2i, i2c, learning_rate=1e-3, max_boxes=4, blocks=(1, 1), widths=(64, 128), init_seed=5)
    m.configure_optimizers()
    batch = _batch(4, 32, 48, 4, seed=3)
    ref_loss = m.training_step(batch, 0)
    rec_short = m.logged["train/rec_loss"][-1]
    long_batch = dict(batch, label_texts=["a", "", "7", "abq7z" * 130], target_lengths=[1, 0, 1, 650])
    total = m.training_step(long_batch, 0)
    assert np.isfinite(total)
    # samples 0 and 2 are unchanged; sample 3 ('zz' before: infeasible too) still contributes 0: the mean over the three
    # non-empty labels is what it was
    assert abs(m.logged["train/rec_loss"][-1] - rec_short) < 1e-5 * max(1.0, abs(rec_short)), (m.logged["train/rec_loss"], rec_short, ref_loss)


def test_cli_trains_the_ocr_model_on_a_folder_dataset(tmp_path):
    """`python -m kzv.train --model ocr` with ocr_lightning/train.py's flags on a temp-dir dataset (the reference's test-fixture
    layout): exit 0, no traceback, metrics and checkpoints written, a checkpoint loads back."""
    from PIL import Image
    rng = np.random.default_rng(0)
    for split, n in (("train", 6), ("val", 3)):
        for i in range(n):
            for sub in ("images", "labels", "bounding_boxes"):
                os.makedirs(tmp_path / split / sub / "book", exist_ok=True)
            Image.fromarray(rng.integers(0, 255, (32 + 4 * (i % 2), 48, 3), dtype=np.uint8)).save(tmp_path / split / "images" / "book" / f"p{i}.png")
            (tmp_path / split / "labels" / "book" / f"p{i}.txt").write_text("abc7"[i % 4], encoding="utf-8")
            (tmp_path / split / "bounding_boxes" / "book" / f"p{i}.json").write_text(json.dumps([[1, 2, 10, 12]] * (1 + i % 3)))
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "kuzushiji-vision_amd"))
    r = subprocess.run([sys.executable, "-m", "kzv.train", "--model", "ocr", "--train_data_dir", str(tmp_path / "train"), "--val_data_dir", str(tmp_path / "val"),
                        "--checkpoint_dir", str(tmp_path / "ck"), "--log_dir", str(tmp_path / "logs"), "--batch_size", "3", "--epochs", "2", "--max_boxes", "5",
                        "--learning_rate", "1e-3", "--seed", "1", "--accelerator", "gpu", "--devices", "1"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "Traceback" not in r.stderr, r.stdout[-1500:] + r.stderr[-3000:]
    recs = [json.loads(ln) for ln in (tmp_path / "logs" / "metrics.jsonl").read_text().splitlines()]
    assert len(recs) == 2 and all(np.isfinite(x["train/total_loss"]) and np.isfinite(x["val/total_loss"]) for x in recs)
    ck = torch.load(tmp_path / "ck" / "last.ckpt", weights_only=False)
    assert "feature_extractor.7.2.bn2.running_var" in ck["state_dict"] and ck["hyper_parameters"]["max_boxes"] == 5
    m = OCRModel(CHAR_TO_IDX, IDX_TO_CHAR, max_boxes=5)
    m.load_state_dict(ck["state_dict"], strict=True)
    # --resume: weights, Adam state and epoch come back (pl.Trainer.fit(ckpt_path=...)); one more epoch is appended to the log
    assert ck["epoch"] == 1 and len(ck["optimizer_states"][0]["state"]) == len(m.offsets) and ck["global_step"] == 4
    r = subprocess.run([sys.executable, "-m", "kzv.train", "--model", "ocr", "--train_data_dir", str(tmp_path / "train"), "--val_data_dir", str(tmp_path / "val"),
                        "--checkpoint_dir", str(tmp_path / "ck"), "--log_dir", str(tmp_path / "logs"), "--batch_size", "3", "--epochs", "3", "--max_boxes", "5",
                        "--learning_rate", "1e-3", "--seed", "1", "--accelerator", "gpu", "--devices", "1", "--resume", str(tmp_path / "ck" / "last.ckpt")],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "Traceback" not in r.stderr and "Resumed from" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
    recs = [json.loads(ln) for ln in (tmp_path / "logs" / "metrics.jsonl").read_text().splitlines()]
    assert [x["epoch"] for x in recs] == [0, 1, 2]
    assert torch.load(tmp_path / "ck" / "last.ckpt", weights_only=False)["global_step"] == 6


def test_two_rank_data_parallel_fit_steps(tmp_path):
    """pl.Trainer(devices=2) for this model = DDP: each rank its own shard and its own BatchNorm statistics, gradients averaged
    before Adam.  Two ranks of the real fit_step on one GPU over gloo: identical replicas afterwards, equal (to float-atomic order) to
    one process that computes the two shards' gradients one after the other and averages them by hand."""
    import socket
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _ocr_ddp_worker as W
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   KZV_DIST_BACKEND="gloo", KZV_FORCE_DEVICE="0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_ocr_ddp_worker.py"), str(tmp_path)], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=600)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(o[-2000:] for o in outs)
    r0, r1 = (torch.load(tmp_path / f"ocr_rank{r}.pt")["params"] for r in range(2))
    assert torch.equal(r0, r1)
    m = W.make()
    init = m.flat_params.clone()
    for step in range(W.STEPS):
        acc = torch.zeros_like(m.flat_grads)
        for rank in range(2):
            m.train(); m.zero_grad()
            m.training_step(W.shard(step, rank, 2), step)
            m.backward()
            acc += m.flat_grads
        m.flat_grads.copy_(acc / 2)
        m.optimizer_step()
    torch.cuda.synchronize()
    # The forward is bit-reproducible (BatchNorm statistics are reduced in a fixed order); what is left between the two runs is the
    # summation order of the weight-gradient split-K atomics and of the all-reduce, which Adam can turn into a +-lr difference only
    # where a gradient element is ~0.  Compare the UPDATE as a whole.
    upd_a, upd_b = (m.flat_params - init).cpu(), r0 - init.cpu()
    moved = upd_a.abs().max().item()
    rel = float((upd_a - upd_b).norm() / upd_b.norm())
    frac = float(((upd_a - upd_b).abs() > 0.02 * moved).float().mean())
    print(f"two-rank OCR step vs hand-averaged: relative L2 of the update difference {rel:.4f}, elements off by > 2 % of a step: {frac:.2e}")
    assert moved > 1e-4 and rel < 0.01 and frac < 1e-3
