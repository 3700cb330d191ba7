#!/usr/bin/env python3
"""What the fine-tuning options cost or save (profiles/finetune.md).  Every figure is taken in ONE process, the arms alternating,
around work that ends in a device synchronise.

  python tools/finetune_time.py kernels [--repeats 5] [--calls 10]
      the grouped norm and the grouped clip + step kernels against the plain ones over the flat buffer of bench.py's model
      (ViT-B/16 encoder, 6 decoder layers): plain / one group / the 14-group layer-decay table / the bias_norm table; device events.
  python tools/finetune_time.py steps [--repeats 3] [--steps 8]
      bench.py's step (256 crops of 64x640, labels of 128) with 0 / 6 / 12 frozen encoder layers, and batch 64 with
      accumulate_grad_batches 1 against 4 (ms per micro-batch).
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "kuzushiji-vision_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def _cfg():
    from kzv.config import vit_b_config
    return vit_b_config(dec_layers=6)


def run_kernels(args):
    import torch
    from kzv import finetune as FT
    from kzv import params as P
    from kzv.optim import RAdamScheduleFree
    cfg = _cfg()
    _, n = P.param_offsets(cfg)
    table = FT.model_param_table(cfg)
    tables = {"plain": None, "one group": [(0, n, 1.0, 1.0)],
              "layer decay 0.75": FT.build_groups(table, cfg.enc_layers, layer_decay=0.75),
              "decay 0.75 + bias_norm": FT.build_groups(table, cfg.enc_layers, layer_decay=0.75, decay_exempt="bias_norm"),
              "6 layers frozen": FT.build_groups(table, cfg.enc_layers, freeze_encoder_layers=6)}

    class Flat:
        def __init__(self):
            self.flat_params = torch.randn(n, device="cuda") * 0.02
            self.flat_grads = torch.randn(n, device="cuda") * 1e-3

        def sync_weights(self):
            pass
    fm = Flat()
    opt = RAdamScheduleFree(fm, lr=1e-4, weight_decay=0.01)
    opt.k = 10                                   # the adaptive branch, as in a run past its first steps
    opt.attach_ema(None, 0.0)
    print(f"{n:,} floats; groups: " + ", ".join(f"{k}: {len(v) if v else 0}" for k, v in tables.items()))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    out = {k: ([], []) for k in tables}
    import ctypes as C
    from kzv import _lib as L
    lib = L.load()
    st = L.stream_handle()
    s = L.kzv_opt_step(lr_t=1e-4, ckp1=0.1, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, bias_correction2=0.01, adaptive=1,
                       max_grad_norm=1.0, grad_scale=1.0, one_minus_beta2=0.001)
    g, p, z, v = fm.flat_grads.data_ptr(), fm.flat_params.data_ptr(), opt.z.data_ptr(), opt.v.data_ptr()
    sq, scr = opt._sq.data_ptr(), opt._scratch.data_ptr()

    def norm(tab, ng):
        if not tab:
            L.check(lib.kzv_grad_sqnorm(g, n, sq, scr, st))
        else:
            L.check(lib.kzv_grad_sqnorm_groups(g, n, tab, ng, sq, scr, st))

    def step(tab, ng):
        if not tab:
            L.check(lib.kzv_clip_and_step_ema(p, z, v, g, n, sq, C.byref(s), None, 0.0, st))
        else:
            L.check(lib.kzv_clip_and_step_groups(p, z, v, g, n, sq, C.byref(s), tab, ng, None, 0.0, st))
    dev = {}
    for name, groups in tables.items():
        opt.set_groups(groups)
        dev[name] = (opt._d_groups, len(groups) if groups else 0)
        norm(L.ptr(dev[name][0]), dev[name][1]); step(L.ptr(dev[name][0]), dev[name][1])      # every kernel loaded before anything is timed
    torch.cuda.synchronize()
    for _ in range(args.repeats):
        for name in tables:
            tab, ng = L.ptr(dev[name][0]), dev[name][1]
            ev[0].record()
            for _ in range(args.calls):
                norm(tab, ng)
            ev[1].record()
            for _ in range(args.calls):
                step(tab, ng)
            ev[2].record()
            torch.cuda.synchronize()
            out[name][0].append(ev[0].elapsed_time(ev[1]) / args.calls * 1e3)
            out[name][1].append(ev[1].elapsed_time(ev[2]) / args.calls * 1e3)
    for name, (a, b) in out.items():
        train = sum(hi - lo for lo, hi, ls, _ in (tables[name] or [(0, n, 1.0, 1.0)]) if ls != 0.0)
        print(f"{name:24s} norm us: median {statistics.median(a):7.1f} min {min(a):7.1f} max {max(a):7.1f} | step us: median {statistics.median(b):7.1f} "
              f"min {min(b):7.1f} max {max(b):7.1f} | {train * 28 / (statistics.median(b) * 1e-6) / 1e12:.2f} TB/s over the trainable floats")


def _model(batch, label_len=128):
    import torch
    from kzv.data import build_decoder_dir, synthetic_batch
    from kzv.model import TrOCRModel
    cfg = _cfg()
    with tempfile.TemporaryDirectory() as tmp:
        model = TrOCRModel(cfg.encoder_config_dict(), build_decoder_dir(os.path.join(tmp, "dec"), cfg), init_seed=42, load_tokenizer=False)
    opt = model.configure_optimizers()
    opt.k = 10                                   # past RAdam's silent phase
    model.train()
    px, lab = synthetic_batch(cfg, batch, label_len, seed=1)
    return cfg, model, opt, {"pixel_values": torch.from_numpy(px).cuda(), "labels": torch.from_numpy(lab).cuda()}


def _time(stepper, batch, steps):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        stepper.step(batch, i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def run_steps(args):
    from kzv import finetune as FT
    from kzv.trainer import Stepper
    cfg, model, opt, batch = _model(256)
    arms = {}
    for frozen in (0, 6, 12):
        FT.apply(model, opt, freeze_encoder_layers=frozen)
        st = Stepper(model, opt, world=1, max_grad_norm=1.0, dp_path=False)
        _time(st, batch, 3)
        arms[frozen] = (st, [])
    for _ in range(args.repeats):
        for frozen, (st, ms) in arms.items():
            FT.apply(model, opt, freeze_encoder_layers=frozen)
            st.step(batch, 0)
            ms.append(_time(st, batch, args.steps))
    for frozen, (_, ms) in arms.items():
        print(f"batch 256, {frozen:2d} frozen encoder layers: ms per step " + " / ".join(f"{x:.2f}" for x in ms))
    FT.apply(model, opt)
    del model, opt, arms
    cfg, model, opt, batch = _model(64)
    arms = {k: (Stepper(model, opt, world=1, max_grad_norm=1.0, dp_path=False, accumulate_grad_batches=k), []) for k in (1, 4)}
    for k, (st, _) in arms.items():
        _time(st, batch, 8)
    for _ in range(args.repeats):
        for k, (st, ms) in arms.items():
            ms.append(_time(st, batch, 4 * args.steps))
    for k, (_, ms) in arms.items():
        print(f"batch 64, accumulate_grad_batches {k}: ms per micro-batch " + " / ".join(f"{x:.2f}" for x in ms))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    k = sub.add_parser("kernels"); k.add_argument("--repeats", type=int, default=5); k.add_argument("--calls", type=int, default=10)
    s = sub.add_parser("steps"); s.add_argument("--repeats", type=int, default=3); s.add_argument("--steps", type=int, default=8)
    a = ap.parse_args()
    {"kernels": run_kernels, "steps": run_steps}[a.cmd](a)
