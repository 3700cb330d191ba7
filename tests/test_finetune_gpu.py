"""Fine-tuning on the GPU: the grouped norm and clip + RAdamScheduleFree kernels (csrc/optim.hip) against the plain kernels and the
float64 restatement in tests/_finetune_ref.py, frozen encoder layers and gradient accumulation on the model, the data-parallel window
and the CLI.  The optimizer bounds are those of tests/test_parity_gpu.py::test_clip_and_radam_schedulefree_kernels_match_oracle:
1e-5 relative + 1e-8 (v: 1e-14), the norm within 1e-5."""
import dataclasses
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from kzv import _lib as L
from kzv import finetune as FT
from kzv import params as P
from kzv.config import tiny_config
from kzv.data import build_decoder_dir, synthetic_batch
from kzv.model import TrOCRModel
from kzv.optim import RAdamScheduleFree
from kzv.trainer import Stepper
from oracle import trocr_oracle as O

from _finetune_ref import GroupedRef

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _FlatModel:
    """What kzv.optim.RAdamScheduleFree needs of a model: the flat buffers."""

    def __init__(self, p):
        self.flat_params = p
        self.flat_grads = torch.zeros_like(p)

    def sync_weights(self):
        pass


def _no_dropout(cfg):
    return dataclasses.replace(cfg, enc_hidden_dropout=0.0, enc_attn_dropout=0.0, dec_hidden_dropout=0.0, dec_attn_dropout=0.0)


def _make(tmp_path, seed=5, tag="m", **kw):
    cfg = _no_dropout(tiny_config())
    d = build_decoder_dir(str(tmp_path / f"dec{tag}"), cfg)
    m = TrOCRModel(cfg.encoder_config_dict(), d, init_seed=seed, load_tokenizer=False, **kw)
    m.train()
    return cfg, m


def _batch(cfg, lines, length, seed):
    px, lab = synthetic_batch(cfg, lines, length, seed=seed, min_chars=2, max_chars=length - 1)
    return px, lab


# ------------------------------------------------------------------------------------------------ (a) one group = the plain kernels
@pytest.mark.parametrize("with_ema", [False, True])
def test_single_group_equals_the_plain_kernels_bit_for_bit(with_ema):
    n = 1_000_448
    rng = np.random.default_rng(5)
    p0 = torch.from_numpy((rng.standard_normal(n) * 0.02).astype(np.float32)).cuda()
    plain_m, group_m = _FlatModel(p0.clone()), _FlatModel(p0.clone())
    plain = RAdamScheduleFree(plain_m, lr=1e-3, weight_decay=0.01)
    group = RAdamScheduleFree(group_m, lr=1e-3, weight_decay=0.01)
    group.set_groups([(0, n, 1.0, 1.0)])
    emas = [None, None]
    if with_ema:
        emas = [p0.clone(), p0.clone()]
        plain.attach_ema(emas[0], 0.99); group.attach_ema(emas[1], 0.99)
    for step in range(12):
        g = torch.from_numpy((rng.standard_normal(n) * 3e-3 * (1 + step % 3)).astype(np.float32)).cuda()
        plain_m.flat_grads.copy_(g); group_m.flat_grads.copy_(g)
        plain.step(max_grad_norm=1.0); group.step(max_grad_norm=1.0)
        assert torch.equal(plain._sq, group._sq), step
        assert torch.equal(plain_m.flat_params, group_m.flat_params) and torch.equal(plain.z, group.z) and torch.equal(plain.v, group.v), step
        if with_ema:
            assert torch.equal(emas[0], emas[1]), step
    assert plain.scheduled_lr > 0 and not torch.equal(plain_m.flat_params, p0)
    if with_ema:
        assert group.ema_fused_steps == 12 and not torch.equal(emas[1], p0)


def test_group_entry_points_refuse_bad_arguments():
    lib = L.load()
    n = 256
    t = torch.zeros(n, device="cuda")
    one = torch.zeros(1, device="cuda"); scratch = torch.zeros(2048, device="cuda")
    opt = RAdamScheduleFree(_FlatModel(t.clone()))
    opt.set_groups([(0, 64, 0.0, 1.0), (64, n, 1.0, 1.0)])
    tab, s = opt._d_groups.data_ptr(), L.kzv_opt_step(lr_t=0.0, ckp1=1.0, beta1=0.9, beta2=0.999, eps=1e-8, bias_correction2=1e-3, one_minus_beta2=1e-3)
    import ctypes as C
    st = L.stream_handle()
    E_ARG = lib.kzv_grad_sqnorm_groups(None, n, tab, 2, one.data_ptr(), scratch.data_ptr(), st)
    assert E_ARG != 0
    for args in ((t.data_ptr(), n, None, 2, one.data_ptr(), scratch.data_ptr(), st), (t.data_ptr(), n + 2, tab, 2, one.data_ptr(), scratch.data_ptr(), st),
                 (t.data_ptr(), n, tab, 0, one.data_ptr(), scratch.data_ptr(), st), (t.data_ptr(), n, tab, 4097, one.data_ptr(), scratch.data_ptr(), st),
                 (t.data_ptr(), n, tab, 2, None, scratch.data_ptr(), st)):
        assert lib.kzv_grad_sqnorm_groups(*args) == E_ARG
    p = t.data_ptr()
    for args in ((None, p, p, p, n, one.data_ptr(), C.byref(s), tab, 2, None, 0.0, st), (p, p, p, p, n + 1, one.data_ptr(), C.byref(s), tab, 2, None, 0.0, st),
                 (p, p, p, p, n, one.data_ptr(), C.byref(s), None, 2, None, 0.0, st), (p, p, p, p, n, one.data_ptr(), C.byref(s), tab, 0, None, 0.0, st),
                 (p, p, p, p, n, one.data_ptr(), C.byref(s), tab, 4097, None, 0.0, st), (p, p, p, p, n, one.data_ptr(), None, tab, 2, None, 0.0, st)):
        assert lib.kzv_clip_and_step_groups(*args) == E_ARG
    with pytest.raises(ValueError):
        opt.set_groups([(0, 64, 1.0, 1.0)])             # does not cover the buffer
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ (b), (c) grouped arithmetic
def _run_grouped(n, groups, frozen_g_norm, gstd, max_norm, grad_scale, steps, seed):
    """`steps` steps of the grouped kernels and of the float64 restatement on the same inputs; asserts the bounds every step."""
    rng = np.random.default_rng(seed)
    p0 = (rng.standard_normal(n) * 0.02).astype(np.float32)
    fm = _FlatModel(torch.from_numpy(p0).cuda())
    opt = RAdamScheduleFree(fm, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    opt.set_groups(groups)
    ema = fm.flat_params.clone()
    opt.attach_ema(ema, 0.99)
    ref = GroupedRef(p0, groups, lr=1e-3, weight_decay=0.01, ema_decay=0.99)
    frozen = np.zeros(n, dtype=bool)
    for lo, hi, ls, _ in groups:
        frozen[lo:hi] = ls == 0.0
    init = {"p": torch.from_numpy(p0).cuda(), "z": opt.z.clone(), "v": opt.v.clone(), "ema": ema.clone()}
    fz = torch.from_numpy(frozen).cuda()
    seen = set()
    for step in range(steps):
        g = (rng.standard_normal(n) * gstd * (1 + step % 3)).astype(np.float32)
        if frozen.any():      # large gradients where nothing trains: the norm and the clip coefficient must not see them
            g[frozen] = (rng.standard_normal(int(frozen.sum())) * frozen_g_norm / np.sqrt(frozen.sum())).astype(np.float32)
        fm.flat_grads.copy_(torch.from_numpy(g))
        opt.step(max_grad_norm=max_norm, grad_scale=grad_scale)
        total, coef = ref.step(g, max_norm=max_norm, grad_scale=grad_scale)
        seen.add(opt.scheduled_lr > 0)
        if max_norm > 0:
            seen.add(("clip", coef < 1.0))
            assert abs(opt.grad_norm() - total) <= 1e-5 * total, (step, opt.grad_norm(), total)
        got = {"p": fm.flat_params, "z": opt.z, "v": opt.v, "ema": ema}
        for name, want in (("p", ref.y), ("z", ref.z), ("v", ref.v), ("ema", ref.ema)):
            assert torch.equal(got[name][fz], init[name][fz]), (step, name)                # frozen: bit for bit what it was
            d = np.abs(got[name].double().cpu().numpy() - want)
            tol = 1e-5 * np.abs(want) + (1e-8 if name != "v" else 1e-14)
            assert (d <= tol).all(), (step, name, float((d / (np.abs(want) + 1e-30)).max()))
    assert seen >= {True, False}       # the silent and the adaptive phase
    return seen


@pytest.mark.parametrize("max_norm,gstd", [(1.0, 0.0946), (1.0, 1e-3), (0.0, 1e-3)])
def test_grouped_step_matches_the_restatement(max_norm, gstd):
    """A frozen group at the head, groups of 64 / 192 / 64,000 floats, a frozen group in the middle, a trailing group of 64 floats; the
    scaled norm of the trainable gradient is ~3 (clip active) or ~0.03 (inactive), the frozen gradients' norm is 100."""
    u = 64
    sizes = [(1, 0.0, 1.0), (1, 0.5, 0.0), (3, 0.75, 1.0), (1000, 1.0, 1.0), (4099 - 1006, 0.0, 1.0), (1, 0.25, 0.0)]
    groups, at = [], 0
    for units, ls, ws in sizes:
        groups.append((at, at + units * u, ls, ws)); at += units * u
    assert at == 64 * 4099
    seen = _run_grouped(at, groups, 100.0, gstd, max_norm, 0.125, 12, seed=6)
    if max_norm > 0:
        assert ("clip", gstd > 0.01) in seen


def test_many_groups_and_grid_wrap():
    """4,096 groups of alternating scale over 64 * 40,000 floats: more groups than workgroups, more floats than one grid pass of
    2048 x 256 x 4, a group boundary inside nearly every wave."""
    units, ngr = 40_000, 4096
    groups, at = [], 0
    for i in range(ngr):
        k = 10 if i < units - 9 * ngr else 9
        groups.append((at, at + 64 * k, 0.5 if i % 2 else 1.0, 1.0 if i % 2 else 0.0)); at += 64 * k
    assert at == 64 * units and at > 2048 * 256 * 4
    _run_grouped(at, groups, 0.0, 3e-3, 1.0, 0.125, 7, seed=7)


# ------------------------------------------------------------------------------------------------ (d) frozen layers on the model
def _fwd_bwd(m, px, lab, seed=11, accumulate=False):
    loss, _ = m.forward_loss(torch.from_numpy(px), torch.from_numpy(lab), seed=seed)
    m.backward(accumulate=accumulate)
    torch.cuda.synchronize()
    return float(loss.item()), {k: v.clone() for k, v in m.grad_dict().items()}


def _is_frozen(name, n, Le):
    return n > 0 and FT.layer_id(name, Le) <= n


@pytest.mark.parametrize("n_frozen", [1, 2])
def test_frozen_encoder_layers_on_the_model(tmp_path, n_frozen):
    cfg, m = _make(tmp_path)
    Le = cfg.enc_layers
    assert n_frozen <= Le and m.frozen_encoder_layers == 0 and L.load().kzv_get_frozen_encoder_layers(m._h) == 0
    px, lab = _batch(cfg, 4, 20, seed=2)
    _, g0 = _fwd_bwd(m, px, lab)
    _, g1 = _fwd_bwd(m, px, lab)                      # the unfrozen backward twice: the run-to-run difference of float atomics
    for bad in (-1, Le + 1, 1.5, True):
        with pytest.raises(ValueError):
            m.frozen_encoder_layers = bad
    assert L.load().kzv_set_frozen_encoder_layers(m._h, Le + 1) != 0 and L.load().kzv_set_frozen_encoder_layers(m._h, -1) != 0
    opt = m.configure_optimizers()
    groups = FT.apply(m, opt, freeze_encoder_layers=n_frozen)
    assert m.frozen_encoder_layers == n_frozen == L.load().kzv_get_frozen_encoder_layers(m._h) == m.hparams.frozen_encoder_layers
    assert groups[0][2] == 0.0 and len(groups) == 2
    _, gf = _fwd_bwd(m, px, lab)
    _, gf2 = _fwd_bwd(m, px, lab)                     # the same window again: a missing side-stream join would show here
    checked = 0
    for k, v in gf.items():
        if _is_frozen(k, n_frozen, Le):
            assert not v.any() and not gf2[k].any(), k                   # exactly zero
            assert g0[k].any() or k.endswith("key.bias"), k              # ... where the unfrozen backward has a gradient
            continue
        tol = max(2.0 ** -22 * float(g0[k].abs().max()), float((g0[k] - g1[k]).abs().max()))
        if not torch.equal(v, g0[k]):
            assert float((v - g0[k]).abs().max()) <= tol, (k, float((v - g0[k]).abs().max()), tol)
        if not torch.equal(gf2[k], v):
            assert float((gf2[k] - v).abs().max()) <= tol, (k, float((gf2[k] - v).abs().max()), tol)
        checked += 1
    assert checked > 20
    # one optimizer step (out of the silent phase, with weight decay): frozen parameters keep their bits, the others move
    opt.k, opt.weight_decay = 10, 0.01
    before = {k: v.clone() for k, v in m.state_dict_views().items()}
    opt.step(max_grad_norm=1.0)
    torch.cuda.synchronize()
    for k, v in m.state_dict_views().items():
        if _is_frozen(k, n_frozen, Le):
            assert torch.equal(v, before[k]), k
        elif not k.endswith("key.bias") and "token_type" not in k:
            assert not torch.equal(v, before[k]), k
    # the Stepper's buckets leave the frozen ranges out
    st = Stepper(m, opt, world=1, dp_path=False)
    cut = groups[0][1]
    assert len(st.seg_ranges) == Le - n_frozen + 1 and min(lo for lo, _ in st.seg_ranges) == cut
    m.frozen_encoder_layers = 0
    _, g2 = _fwd_bwd(m, px, lab)
    assert all(g2[k].any() for k in g2 if _is_frozen(k, n_frozen, Le) and not k.endswith("key.bias"))


# ------------------------------------------------------------------------------------------------ (e) accumulation on the model
def test_accumulation_on_the_model(tmp_path):
    cfg, m = _make(tmp_path, seed=5)
    a, b = _batch(cfg, 3, 5, seed=21), _batch(cfg, 2, 29, seed=22)
    _, ga = _fwd_bwd(m, *a)
    _, ga2 = _fwd_bwd(m, *a)                          # pass a twice: the run-to-run difference of a single pass
    _, gb = _fwd_bwd(m, *b)
    _fwd_bwd(m, *a)
    _, gacc = _fwd_bwd(m, *b, accumulate=True)        # no zeroing in between: the buffer holds g_a + g_b
    for k, v in gacc.items():
        want = ga[k] + gb[k]
        tol = 2.0 ** -22 * float(want.abs().max()) + 2.0 * float((ga[k] - ga2[k]).abs().max())
        d = float((v - want).abs().max())
        assert d <= tol, (k, d, tol)
    # against the float64 oracle, summed over the two batches (the criterion of test_model_gpu.py::test_tiny_matches_reference_fixture)
    sd = P.state_dict_from_flat(cfg, P.recipe_flat(cfg, 5))
    ra, rb = O.forward_backward(cfg, sd, *a), O.forward_backward(cfg, sd, *b)
    worst = {}
    for name, wa in ra["grads"].items():
        if name.startswith("decoder.lm_head.decoder."):
            continue
        want = wa + rb["grads"][name]
        got = gacc[name].cpu().numpy()
        if name.endswith("key.bias"):
            assert np.abs(got).max() < 1e-4, name
            continue
        worst[name] = np.abs(got - want).max() / (np.abs(want).max() + 1e-9)
    bad = {k: v for k, v in worst.items() if v > 0.05}
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1])[:8]
    assert np.median(list(worst.values())) < 0.02
    # Stepper(accumulate_grad_batches=2) over [a, b] == one opt.step(grad_scale=0.5) on that buffer
    _, m2 = _make(tmp_path, seed=5, tag="s")
    opt2 = m2.configure_optimizers()
    opt2.k = 10                                       # past RAdam's silent phase: the step moves the parameters
    st = Stepper(m2, opt2, world=1, max_grad_norm=1.0, accumulate_grad_batches=2)
    tb = [{"pixel_values": torch.from_numpy(x[0]), "labels": torch.from_numpy(x[1])} for x in (a, b)]
    assert st.step(tb[0], 0) is None and not st.stepped and opt2.k == 10
    la = float(m2._loss.item())
    mean = st.step(tb[1], 1)
    assert st.stepped and opt2.k == 11
    assert abs(float(mean.item()) - 0.5 * (la + float(m2._loss.item()))) < 1e-6
    _, m3 = _make(tmp_path, seed=5, tag="t")
    opt3 = m3.configure_optimizers()
    opt3.k = 10
    m3.flat_grads.copy_(m2.flat_grads)
    opt3.step(max_grad_norm=1.0, grad_scale=0.5)
    torch.cuda.synchronize()
    assert torch.equal(m3.flat_params, m2.flat_params) and torch.equal(opt3.z, opt2.z) and torch.equal(opt3.v, opt2.v)
    assert not torch.equal(m3.flat_params, torch.from_numpy(P.recipe_flat(cfg, 5)).cuda())
    for k, v in m2.grad_dict().items():               # and that buffer is g_a + g_b again
        want = ga[k] + gb[k]
        assert float((v - want).abs().max()) <= 2.0 ** -22 * float(want.abs().max()) + 2.0 * float((ga[k] - ga2[k]).abs().max()), k


# ------------------------------------------------------------------------------------------------ (f) data-parallel window
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_rank_accumulation_window_with_frozen_layer(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _finetune_dp_worker as W
    port = _free_port()
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   KZV_DIST_BACKEND="gloo", KZV_FORCE_DEVICE="0")
        procs.append(subprocess.Popen(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tests", "_finetune_dp_worker.py"), str(tmp_path)],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate()[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(o[-2000:] for o in outs)
    r0, r1 = (torch.load(tmp_path / f"rank{r}.pt") for r in range(2))
    assert r0["dp_path"] and torch.equal(r0["params"], r1["params"]) and r0["norms"] == r1["norms"]
    # all-reduce only in a window's last backward, and never over the frozen range
    cfg, m, opt = W.make(str(tmp_path), "single")
    cut = opt.groups[0][1]
    assert opt.groups[0][2] == 0.0 and len(r0["seg_ranges"]) == cfg.enc_layers - W.FREEZE + 1
    assert len(r0["reduced"]) == W.WINDOWS * len(r0["buckets"]) and len(r0["buckets"]) >= 2
    assert all(micro == W.K and off // 4 >= cut for micro, off, _ in r0["reduced"])
    assert sum(nel for _, _, nel in r0["reduced"]) == W.WINDOWS * (m.flat_params.numel() - cut)
    # single process over the same four micro-batches per window: each rank's window buffer, their sum, grad_scale 1/4
    init = m.flat_params.clone()
    for w in range(W.WINDOWS):
        total = torch.zeros_like(m.flat_grads)
        for rank in range(2):
            for j in range(W.K):
                bt = W.micro_batch(cfg, w, j, rank)
                m.forward_loss(bt["pixel_values"], bt["labels"])
                m.backward(accumulate=j > 0)
            total += m.flat_grads
        m.flat_grads.copy_(total)
        opt.step(max_grad_norm=1.0, grad_scale=1.0 / (W.K * 2))
        assert abs(opt.grad_norm() - r0["norms"][w]) <= 1e-5 * r0["norms"][w]
    torch.cuda.synchronize()
    assert torch.equal(m.flat_params[:cut], init[:cut]) and torch.equal(r0["params"][:cut], init[:cut].cpu())
    mine, theirs = P.state_dict_from_flat(cfg, m.flat_params.double().cpu().numpy()), P.state_dict_from_flat(cfg, r0["params"].double().numpy())
    moved, worst = 0.0, 0.0
    for k in mine:
        if k.endswith("key.bias"):      # exactly-zero true gradient: Adam normalises float-atomic noise there
            continue
        d = np.abs(mine[k] - theirs[k])
        tol = 1e-5 * np.abs(mine[k]) + 1e-8
        worst = max(worst, float((d / tol).max()))
        moved = max(moved, float(np.abs(mine[k] - P.state_dict_from_flat(cfg, init.double().cpu().numpy())[k]).max()))
    print(f"two ranks x k=2 vs single process: worst |difference| / bound = {worst:.3g}, largest update {moved:.3g}")
    assert moved > 1e-3
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ (g) CLI
def test_cli_finetune_checkpoint_resume_and_init_from(tmp_path, capsys):
    from kzv.train import main
    common = ["--synthetic", "32", "--batch_size", "4", "--encoder_hidden_size", "128", "--encoder_num_layers", "2", "--encoder_num_heads", "2",
              "--image_size", "32", "64", "--max_length", "16", "--max_epochs", "1", "--skip_test", "--output_dir", str(tmp_path)]
    main(common + ["--experiment_name", "a", "--max_steps", "4", "--accumulate_grad_batches", "2", "--freeze_encoder_layers", "1", "--layer_decay", "0.75"])
    out = capsys.readouterr().out
    assert "parameter groups: 3" in out and "accumulate_grad_batches 2" in out and "lr scale 0.75 .. 1" in out
    path = tmp_path / "a" / "checkpoints" / "last.ckpt"
    ck = torch.load(path, map_location="cpu", weights_only=False)
    hp = ck["hyper_parameters"]
    assert (hp["accumulate_grad_batches"], hp["frozen_encoder_layers"], hp["layer_decay"], hp["decay_exempt"]) == (2, 1, 0.75, "none")
    assert ck["global_step"] == 4 and ck["optimizer_states"][0]["param_groups"][0]["k"] == 4
    # --resume: weights, optimizer state, step and the checkpoint's settings
    main(common + ["--experiment_name", "b", "--max_steps", "6", "--resume", str(path)])
    out = capsys.readouterr().out
    assert main.start[1] == 4 and "global step 4" in out and "parameter groups: 3" in out and "accumulate_grad_batches 2" in out
    ck2 = torch.load(tmp_path / "b" / "checkpoints" / "last.ckpt", map_location="cpu", weights_only=False)
    assert ck2["global_step"] == 6 and ck2["optimizer_states"][0]["param_groups"][0]["k"] == 6
    assert ck2["hyper_parameters"]["frozen_encoder_layers"] == 1 and ck2["hyper_parameters"]["accumulate_grad_batches"] == 2
    frozen = "encoder.encoder.layer.0.output.dense.weight"
    assert torch.equal(ck2["state_dict"][frozen], ck["state_dict"][frozen])
    assert not torch.equal(ck2["state_dict"]["encoder.encoder.layer.1.output.dense.weight"], ck["state_dict"]["encoder.encoder.layer.1.output.dense.weight"])
    # --init_from: the weights alone -- step 0, a fresh optimizer, the flags' own settings (none here)
    import kzv.trainer as T
    seen = {}
    real_fit = T.fit

    def fit_probe(model, *a, **kw):
        seen["params"], seen["k"], seen["kw"] = model.flat_params.detach().cpu().clone(), kw["optimizer"].k, kw
        seen["z_is_p"] = torch.equal(kw["optimizer"].z, model.flat_params)
        return []
    T.fit = fit_probe                   # main() imports fit when it runs: the run stops where training would begin
    try:
        main(common + ["--experiment_name", "c", "--init_from", str(path)])
    finally:
        T.fit = real_fit
    assert main.start == (0, 0) and seen["k"] == 0 and seen["kw"]["start_step"] == 0 and seen["kw"]["accumulate_grad_batches"] == 1 and seen["z_is_p"]
    assert seen["kw"]["optimizer"].groups is None and seen["kw"]["optimizer"].model.frozen_encoder_layers == 0
    # equal weights: every tensor of the checkpoint, through the HF-named views
    from kzv.checkpoint import read_checkpoint
    model_cfg = seen["kw"]["optimizer"].model.cfg
    views = P.state_dict_from_flat(model_cfg, seen["params"])
    sd, _ = read_checkpoint(ck, model_cfg)
    assert len(sd) > 40
    for k, v in sd.items():
        mine = views[P.canonical_hf_name(k)]
        assert torch.equal(mine, torch.as_tensor(v).reshape(mine.shape)), k
