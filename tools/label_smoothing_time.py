#!/usr/bin/env python3
"""What label smoothing costs (profiles/label_smoothing.md): bench.py's model and batch (ViT-B/16 encoder, 6 decoder layers, 256 crops of
64x640, labels of 128, kzv.trainer.Stepper), eps 0 against eps 0.1.

  python tools/label_smoothing_time.py steps [--repeats 3] [--steps 10] [--warmup 3]
      host clock around steps that end in a device synchronise, the two arms alternating inside one process; prints ms per step.
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/label_smoothing_time.py plan
      runs the phases (eps, trim) in a fixed order, PLAN_STEPS steps each, twice over; every step launches head_ce_kernel once.
  python tools/label_smoothing_time.py parse DIR
      groups the head_ce_kernel dispatches of that trace by phase (their order is the plan's) and prints the median and the minimum.
"""
from __future__ import annotations

import argparse
import csv
import glob
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
PLAN = [(eps, trim) for _ in range(2) for trim in (True, False) for eps in (0.0, 0.1)]      # alternated: every arm twice


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
    return model, stepper, batch


def run_steps(args):
    import torch
    model, stepper, batch = make()
    for i in range(args.warmup):
        stepper.step(batch, i)
    for eps in (0.1, 0.0):                      # both instantiations loaded before anything is timed
        model.label_smoothing = eps
        stepper.step(batch, 0)
    torch.cuda.synchronize()
    out, last = {0.0: [], 0.1: []}, {}
    for _ in range(args.repeats):
        for eps in (0.0, 0.1):
            model.label_smoothing = eps
            stepper.step(batch, 0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.steps):
                loss = stepper.step(batch, i)
            torch.cuda.synchronize()
            out[eps].append((time.perf_counter() - t0) / args.steps * 1e3)
            last[eps] = float(loss)
    for eps, v in out.items():
        print(f"eps {eps}: ms per step " + " / ".join(f"{x:.3f}" for x in v) + f"   (decoder positions {model.last_active_length}, last loss {last[eps]:.4f})")
    print(f"difference of the minima: {min(out[0.1]) - min(out[0.0]):+.3f} ms")


def run_plan(_args):
    import torch
    model, stepper, batch = make()
    for eps, trim in PLAN:
        model.label_smoothing, model.trim_padding = eps, trim
        for i in range(PLAN_STEPS):
            stepper.step(batch, i)
        torch.cuda.synchronize()
        print(f"phase eps {eps} trim {trim}: decoder positions {model.last_active_length}", file=sys.stderr)


def parse(args):
    files = sorted(glob.glob(os.path.join(args.dir, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {args.dir}")
    rows = []
    for f in files:
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                if "head_ce_kernel" in r["Kernel_Name"]:
                    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    if len(rows) != len(PLAN) * PLAN_STEPS:
        raise SystemExit(f"{len(rows)} head_ce_kernel dispatches, the plan has {len(PLAN) * PLAN_STEPS}")
    for k, (eps, trim) in enumerate(PLAN):
        part = rows[k * PLAN_STEPS:(k + 1) * PLAN_STEPS][1:]            # the first step of a phase left out (cold instruction cache)
        us = [(e - s) / 1e3 for s, e, _ in part]
        names = {re.search(r"head_ce_kernel<[^>]*>", n).group(0) if re.search(r"head_ce_kernel<[^>]*>", n) else n for _, _, n in part}
        print(f"eps {eps} {'trimmed  ' if trim else 'untrimmed'}: median {statistics.median(us):7.1f} us, min {min(us):7.1f} us over {len(us)}   {sorted(names)}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    s = sub.add_parser("steps"); s.add_argument("--repeats", type=int, default=3); s.add_argument("--steps", type=int, default=10); s.add_argument("--warmup", type=int, default=3)
    sub.add_parser("plan")
    q = sub.add_parser("parse"); q.add_argument("dir")
    a = ap.parse_args()
    {"steps": run_steps, "plan": run_plan, "parse": parse}[a.cmd](a)
