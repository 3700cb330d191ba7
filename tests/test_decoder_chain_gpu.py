"""The decoder layer's linear chains as two launches (csrc/decoder_chain.hip; their backward: csrc/decoder_chain_bwd.hip) against the launch-per-operation forward they replace
(HF RobertaLayer, modeling_roberta.py:421-464, under src/models/trocr_model.py:258-297): same model, same batch, same dropout seed,
`kzv_set_dec_chain(0 / 1)` -- loss, logits and EVERY gradient (the backward reads the tensors the chains wrote: sums, LayerNorm
statistics, bf16 operands, the saved GELU derivative, and regenerates their dropout masks).  The oracle-side parity of the chain
path is what test_model_gpu.py / test_parity_gpu.py / test_configs_gpu.py assert at the same geometry (the chains are the default)."""
import dataclasses

import numpy as np
import pytest
import torch

from kzv import _lib as L
from kzv.config import small_config, tiny_config
from kzv.data import build_decoder_dir, synthetic_batch
from kzv.model import TrOCRModel

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _default_mode_afterwards():
    yield
    L.load().kzv_set_dec_chain(-1)
    L.load().kzv_set_head_ce(-1)


def _run(cfg, tmp_path, B, Lh, train, seed):
    lib = L.load()
    d = build_decoder_dir(str(tmp_path / "dec"), cfg)
    m = TrOCRModel(cfg.encoder_config_dict(), d, init_seed=seed, load_tokenizer=False)
    px, lab = synthetic_batch(cfg, B, Lh, seed=seed, min_chars=1, max_chars=Lh - 2)
    pxt, ids = torch.from_numpy(px).cuda(), torch.from_numpy(lab).cuda()
    out = []
    for mode in (0, 1, 2):
        L.check(lib.kzv_set_dec_chain(mode), "mode")
        m.train() if train else m.eval()
        m.zero_grad()
        loss, logits = m.forward_loss(pxt, ids, want_logits=True, seed=11)
        grads = None
        if train:
            m.backward()
            grads = m.flat_grads.clone()
        torch.cuda.synchronize()
        out.append((float(loss), logits.clone(), grads))
    return out


@pytest.mark.parametrize("B,Lh,train", [(5, 30, True), (3, 12, True), (7, 23, False)])
def test_chains_equal_the_launch_per_operation_forward(tmp_path, B, Lh, train):
    cfg = dataclasses.replace(tiny_config(), dec_hidden=256, dec_heads=4, dec_ffn=768, dec_layers=3)       # dropout 0.1 stays on
    (l0, z0, g0), (l1, z1, g1), (l2, z2, g2) = _run(cfg, tmp_path, B, Lh, train, seed=4 + B)
    dz = float((z0 - z1).abs().max())
    print(f"B={B} L={Lh} train={train}: loss {l0:.6f} / {l1:.6f}, largest logit difference {dz:.2e}", end="")
    assert abs(l0 - l1) < 1e-5 * max(1.0, abs(l0)) and dz < 1e-4
    assert abs(l2 - l1) < 2e-6 * max(1.0, abs(l1)) and torch.equal(z1, z2)      # mode 2 changes the backward only (the loss is a sum of float atomics)
    if train:
        dg = float((g0 - g1).abs().max()); sc = float(g0.abs().max())
        dg2 = float((g1 - g2).abs().max())
        print(f", largest gradient difference {dg:.2e} (forward chains) / {dg2:.2e} (backward segments vs launches) of {sc:.2e}")
        assert dg < 1e-4 * sc                                   # same arithmetic, same dropout bits: differences are summation order at most
        assert dg2 < 1e-6 * sc      # the segments: the launches' arithmetic bit for bit (kzv_common.h ln_bwd_*); what differs is float-atomic order


@pytest.mark.parametrize("B,Lh,train,vocab", [(5, 30, True, 4300), (3, 12, True, 100), (7, 23, False, 777), (70, 9, True, 4300)])
def test_one_launch_lm_head_and_cross_entropy_equals_gemm_plus_ce_kernel(tmp_path, B, Lh, train, vocab):
    """kzv_set_head_ce(1) (default): lm_head.decoder + log-softmax + NLL + dlogits in one launch, logits never written (SURVEY K9;
    csrc/cross_entropy.hip head_ce_kernel) against the head GEMM + ce_kernel it replaces -- same model, batch and dropout seed: the loss
    and EVERY gradient (the head's two gradient GEMMs read the bf16 dlogits the kernel wrote).  Vocabularies that end inside a
    256-column chunk and inside a 64-column pad (100 -> Vp 128, 777 -> 832), rows past M in the last workgroup, ignored (pad) targets,
    and the validation form (no gradient buffer)."""
    cfg = dataclasses.replace(tiny_config(), dec_hidden=256, dec_heads=4, dec_ffn=768, dec_layers=2, vocab=vocab)
    lib = L.load()
    d = build_decoder_dir(str(tmp_path / "dec"), cfg)
    m = TrOCRModel(cfg.encoder_config_dict(), d, init_seed=3 + B, load_tokenizer=False)
    px, lab = synthetic_batch(cfg, B, Lh, seed=5 + B, min_chars=1, max_chars=Lh - 2)
    pxt, ids = torch.from_numpy(px).cuda(), torch.from_numpy(lab).cuda()
    out = []
    for mode in (0, 1):
        L.check(lib.kzv_set_head_ce(mode), "mode")
        m.train() if train else m.eval()
        m.zero_grad()
        loss, _ = m.forward_loss(pxt, ids, want_logits=False, seed=13)
        grads = None
        if train:
            m.backward()
            grads = m.flat_grads.clone()
        torch.cuda.synchronize()
        out.append((float(loss), grads))
    (l0, g0), (l1, g1) = out
    assert np.isfinite(l1) and abs(l0 - l1) < 2e-6 * max(1.0, abs(l0)), (l0, l1)
    if train:
        dg = float((g0 - g1).abs().max()); sc = float(g0.abs().max())
        print(f"B={B} L={Lh} V={vocab}: loss {l0:.6f} / {l1:.6f}, largest gradient difference {dg:.2e} of {sc:.2e}")
        assert dg < 2e-3 * sc        # dlogits are bf16 on both sides: an fp32 summation-order difference of a logit moves single entries by one bf16 ulp


def test_chains_at_the_benchmark_decoder_geometry(tmp_path):
    """12 layers, 15 sequences of up to 127 tokens (rows not a multiple of the 64-row workgroup tile), dropout on."""
    cfg = small_config()
    (l0, z0, g0), (l1, z1, g1), (l2, z2, g2) = _run(cfg, tmp_path, 15, cfg.max_pos - cfg.pad_id - 1, True, seed=2)
    dz = float((z0 - z1).abs().max()); dg = float((g0 - g1).abs().max()); sc = float(g0.abs().max())
    dg2 = float((g1 - g2).abs().max())
    print(f"loss {l0:.6f} / {l1:.6f}, largest logit difference {dz:.2e}, largest gradient difference {dg:.2e} / {dg2:.2e} (backward segments) of {sc:.2e}")
    assert abs(l0 - l1) < 1e-5 * max(1.0, abs(l0)) and dz < 1e-4 and dg < 1e-4 * sc
    assert abs(l2 - l1) < 2e-6 * max(1.0, abs(l1)) and torch.equal(z1, z2) and dg2 < 1e-6 * sc


def test_chains_with_more_workgroups_than_compute_units(tmp_path):
    """256 sequences x 127 positions = 32,512 decoder rows = 508 workgroups of 64 rows on 256 CUs (the untrimmed benchmark step), the INPUT
    changing from step to step: logits bit-identical to the launch-per-operation path in every step.  Rounds 3 - 4 failed this (found in
    round 4's second session: tools/dev/r5_det3.py): the residual epilogue consumed registers whose loads -- issued early, some inside a
    uniform branch -- had not landed, hipcc's own vmcnt wait being too lenient; 2 - 5 % of chain A's workgroups then added `beta` instead
    of the LayerNorm output for 16 rows (logits off by 0.2), only once a launch had more workgroups than CUs (slower loads), and repeated
    inputs hid nothing.  csrc/dec_rows.h now retires such loads by hand (retire_loads + pin)."""
    cfg = dataclasses.replace(tiny_config(), dec_hidden=256, dec_heads=4, dec_ffn=768, dec_layers=4, max_pos=130)
    lib = L.load()
    d = build_decoder_dir(str(tmp_path / "dec"), cfg)
    m = TrOCRModel(cfg.encoder_config_dict(), d, init_seed=9, load_tokenizer=False)
    ins = []
    for seed in (1, 2):
        px, lab = synthetic_batch(cfg, 256, 128, seed=seed, min_chars=1, max_chars=126)
        ins.append((torch.from_numpy(px).cuda(), torch.from_numpy(lab).cuda()))
    m.train()

    def logits(i, mode):
        L.check(lib.kzv_set_dec_chain(mode), "mode")
        _, z = m.forward_loss(ins[i][0], ins[i][1], want_logits=True, seed=11)
        torch.cuda.synchronize()
        return z.clone()

    ref = [logits(0, 0), logits(1, 0)]
    assert ref[0].shape[0] * ref[0].shape[1] > 256 * 64
    for mode in (1, 2):
        for i in (0, 1, 1, 0, 1, 0):
            z = logits(i, mode)
            bad = int(((z - ref[i]).abs().amax(-1) > 0).sum())
            assert bad == 0, f"mode {mode}, input {i}: {bad} rows differ from the launch-per-operation path"

    # the same for the backward (the segments and the row-panel input gradients run 508 workgroups too): every gradient against mode 0
    def grads(i, mode):
        L.check(lib.kzv_set_dec_chain(mode), "mode")
        m.zero_grad()
        m.forward_loss(ins[i][0], ins[i][1], want_logits=True, seed=11)
        m.backward()
        torch.cuda.synchronize()
        return m.flat_grads.clone()

    gref = [grads(0, 0), grads(1, 0)]
    for mode in (1, 2):
        for i in (0, 1, 0):
            g = grads(i, mode)
            sc = float(gref[i].abs().max()); dg = float((g - gref[i]).abs().max())
            assert dg < 1e-5 * sc, f"mode {mode}, input {i}: largest gradient difference {dg:.2e} of {sc:.2e}"

    # ... and the one-launch LM head + cross-entropy (508 workgroups as well) against the head GEMM + ce_kernel, logits not returned
    def step(i, head):
        L.check(lib.kzv_set_dec_chain(2), "mode"); L.check(lib.kzv_set_head_ce(head), "head")
        m.zero_grad()
        loss, _ = m.forward_loss(ins[i][0], ins[i][1], want_logits=False, seed=11)
        m.backward()
        torch.cuda.synchronize()
        return float(loss), m.flat_grads.clone()

    m.trim_padding = False
    for i in (0, 1, 0):
        (l0, g0), (l1, g1) = step(i, 0), step(i, 1)
        sc = float(g0.abs().max()); dg = float((g0 - g1).abs().max())
        # the loss is a float-atomic sum over 32 k rows (508 workgroups / 32 k ce_kernel rows in another order); bf16 dlogits on both sides (see the head test above)
        assert abs(l0 - l1) < 1e-5 * max(1.0, abs(l0)) and dg < 2e-3 * sc, (i, l0, l1, dg, sc)
