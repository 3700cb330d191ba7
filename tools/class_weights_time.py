#!/usr/bin/env python3
"""What class weights and the focal term cost (profiles/class_weights.md): bench.py's model and batch (ViT-B/16 encoder, 6 decoder
layers, 256 crops of 64x640, labels of 128, kzv.trainer.Stepper), everything off against weights, weights + eps 0.1 and weights + gamma 2.

  python tools/class_weights_time.py steps [--repeats 3] [--steps 10] [--warmup 3]
      host clock around steps that end in a device synchronise, the arms alternating inside one process; prints ms per step.
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/class_weights_time.py plan
      runs the phases (arm, trim) in a fixed order, PLAN_STEPS steps each, twice over; every step launches head_ce_kernel once and, in
      the arms that are not "off", target_weight_sum_kernel once.
  python tools/class_weights_time.py parse DIR
      groups the head_ce_kernel / target_weight_sum_kernel dispatches of that trace by phase (their order is the plan's) and prints the
      median and the minimum.
"""
from __future__ import annotations

import argparse
import csv
import glob
import math
import os
import re
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "kuzushiji-vision_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

PLAN_STEPS = 6
ARMS = {"off": (False, 0.0, 0.0), "weights": (True, 0.0, 0.0), "weights+eps0.1": (True, 0.1, 0.0), "weights+gamma2": (True, 0.0, 2.0)}      # (weights, eps, gamma)
PLAN = [(arm, trim) for _ in range(2) for trim in (True, False) for arm in ARMS]      # alternated: every arm twice


def make():
    import torch
    from kzv.config import vit_b_config
    from kzv.data import build_decoder_dir, synthetic_batch
    from kzv.model import TrOCRModel
    from kzv.trainer import Stepper
    cfg = vit_b_config(dec_layers=6)
    with tempfile.TemporaryDirectory() as tmp:
        model = TrOCRModel(cfg.encoder_config_dict(), build_decoder_dir(os.path.join(tmp, "dec"), cfg), init_seed=42, load_tokenizer=False)
    opt = model.configure_optimizers()
    model.train()
    stepper = Stepper(model, opt, world=1, max_grad_norm=1.0, dp_path=False)
    px, lab = synthetic_batch(cfg, 256, 128, seed=1)
    batch = {"pixel_values": torch.from_numpy(px).cuda(), "labels": torch.from_numpy(lab).cuda()}
    g = torch.Generator().manual_seed(7)
    weights = torch.exp((torch.rand(cfg.vocab, generator=g, dtype=torch.float64) * 2 - 1) * math.log(4.0)).float()      # exp(U(-ln 4, ln 4))
    return model, stepper, batch, weights


def set_arm(model, weights, arm):
    on, eps, gamma = ARMS[arm]
    model.focal_gamma = 0.0
    model.label_smoothing = eps
    model.focal_gamma = gamma
    model.class_weights = weights if on else None


def run_steps(args):
    import torch
    model, stepper, batch, weights = make()
    for i in range(args.warmup):
        stepper.step(batch, i)
    for arm in reversed(ARMS):                  # every instantiation loaded before anything is timed
        set_arm(model, weights, arm)
        stepper.step(batch, 0)
    torch.cuda.synchronize()
    out, last = {a: [] for a in ARMS}, {}
    for _ in range(args.repeats):
        for arm in ARMS:
            set_arm(model, weights, arm)
            stepper.step(batch, 0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.steps):
                loss = stepper.step(batch, i)
            torch.cuda.synchronize()
            out[arm].append((time.perf_counter() - t0) / args.steps * 1e3)
            last[arm] = float(loss)
    for arm, v in out.items():
        print(f"{arm:15s}: ms per step " + " / ".join(f"{x:.3f}" for x in v) + f"   (decoder positions {model.last_active_length}, last loss {last[arm]:.4f})")
    for arm in list(ARMS)[1:]:
        print(f"{arm}: difference of the minima against off: {min(out[arm]) - min(out['off']):+.3f} ms")


def run_plan(_args):
    import torch
    model, stepper, batch, weights = make()
    for arm, trim in PLAN:
        set_arm(model, weights, arm)
        model.trim_padding = trim
        for i in range(PLAN_STEPS):
            stepper.step(batch, i)
        torch.cuda.synchronize()
        print(f"phase {arm} trim {trim}: decoder positions {model.last_active_length}", file=sys.stderr)


def parse(args):
    files = sorted(glob.glob(os.path.join(args.dir, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {args.dir}")
    head, norm = [], []
    for f in files:
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                row = (int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"])
                if "head_ce_kernel" in r["Kernel_Name"]:
                    head.append(row)
                elif "target_weight_sum_kernel" in r["Kernel_Name"]:
                    norm.append(row)
    head.sort(); norm.sort()
    if len(head) != len(PLAN) * PLAN_STEPS:
        raise SystemExit(f"{len(head)} head_ce_kernel dispatches, the plan has {len(PLAN) * PLAN_STEPS}")
    n_on = sum(arm != "off" for arm, _ in PLAN) * PLAN_STEPS
    if len(norm) != n_on:
        raise SystemExit(f"{len(norm)} target_weight_sum_kernel dispatches, the plan has {n_on}")
    k_norm = 0
    for k, (arm, trim) in enumerate(PLAN):
        part = head[k * PLAN_STEPS:(k + 1) * PLAN_STEPS][1:]            # the first step of a phase left out (cold instruction cache)
        us = [(e - s) / 1e3 for s, e, _ in part]
        names = {re.search(r"head_ce_kernel<[^>]*>", n).group(0) if re.search(r"head_ce_kernel<[^>]*>", n) else n for _, _, n in part}
        line = f"{arm:15s} {'trimmed  ' if trim else 'untrimmed'}: head_ce median {statistics.median(us):7.1f} us, min {min(us):7.1f} us over {len(us)}   {sorted(names)}"
        if arm != "off":
            nus = [(e - s) / 1e3 for s, e, _ in norm[k_norm * PLAN_STEPS:(k_norm + 1) * PLAN_STEPS][1:]]
            k_norm += 1
            line += f"   target_weight_sum median {statistics.median(nus):5.1f} us, min {min(nus):5.1f} us"
        print(line)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    s = sub.add_parser("steps"); s.add_argument("--repeats", type=int, default=3); s.add_argument("--steps", type=int, default=10); s.add_argument("--warmup", type=int, default=3)
    sub.add_parser("plan")
    q = sub.add_parser("parse"); q.add_argument("dir")
    a = ap.parse_args()
    {"steps": run_steps, "plan": run_plan, "parse": parse}[a.cmd](a)
