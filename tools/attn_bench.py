#!/usr/bin/env python3
"""Times the encoder attention and the whole training step at the reference CLI's defaults; prints one JSON line.

  python tools/attn_bench.py [--B 64 --heads 8 --S 257 --D 96] [--step-batch 64] [--iters 20 --warmup 5]

* op: kzv_attn_fwd and kzv_attn_bwd on the model's packed strides (Q | K | V column blocks of one [B * S, 3 * heads * D]
  buffer, O / dO [B * S, heads * D]), dropout 0.1 as in training; device-event timing, mean per launch;
* step: Stepper.step (forward, backward, clip, optimizer) of reference_cli_config() at batch --step-batch (0 skips it), the
  CLI's dropout and labels of length 128; img/s over --step-iters steps after warm-up, host clock around a synchronise.

KZV_LIB selects the library (kzv/_lib.py), so one job can time an older build against this one.  Symbols the Python binding
declares but an older library lacks are left unbound (reported under "unbound"); kzv_attn_impl is then not asked.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "kuzushiji-vision_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from kzv import _lib as L  # noqa: E402


def load_tolerant():
    probe = C.CDLL(L.LIB_PATH)
    unbound = sorted(n for n in L.SYMBOLS if not hasattr(probe, n))
    for n in unbound:
        del L.SYMBOLS[n]
    return L.load(), unbound


def time_op(lib, B, heads, S, D, iters, warmup):
    H = heads * D
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    qkv = torch.randn(B * S, 3 * H, device="cuda", generator=gen).bfloat16()
    dqkv = torch.empty_like(qkv)
    O = torch.empty(B * S, H, dtype=torch.bfloat16, device="cuda")
    dO = torch.randn(B * S, H, device="cuda", generator=gen).bfloat16()
    LSE = torch.empty(B, heads, S, device="cuda")
    a = L.kzv_attn_args(Q=qkv.data_ptr(), K=qkv[:, H:].data_ptr(), V=qkv[:, 2 * H:].data_ptr(), O=O.data_ptr(), LSE=LSE.data_ptr(),
                        dO=dO.data_ptr(), dQ=dqkv.data_ptr(), dK=dqkv[:, H:].data_ptr(), dV=dqkv[:, 2 * H:].data_ptr(),
                        ldq=3 * H, ldk=3 * H, ldv=3 * H, ldo=H, B=B, heads=heads, Sq=S, Sk=S, mode=0, drop_p=0.1, drop_key=7,
                        head_dim=0 if D == 64 else D)
    st = torch.cuda.current_stream().cuda_stream
    res = {}
    for name, fn in (("fwd", lib.kzv_attn_fwd), ("bwd", lib.kzv_attn_bwd)):
        for _ in range(warmup):
            L.check(fn(C.byref(a), st), name)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            L.check(fn(C.byref(a), st), name)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / iters
        flop = (4.0 if name == "fwd" else 10.0) * B * heads * S * S * D
        res[name] = {"us": round(us, 2), "tflops": round(flop / us * 1e-6, 1)}
    return res


def time_step(batch, iters, warmup):
    from kzv.config import reference_cli_config
    from kzv.data import build_decoder_dir, synthetic_batch
    from kzv.model import TrOCRModel
    from kzv.trainer import Stepper
    cfg = reference_cli_config()
    with tempfile.TemporaryDirectory() as tmp:
        m = TrOCRModel(cfg.encoder_config_dict(), build_decoder_dir(os.path.join(tmp, "dec"), cfg), device="cuda:0", init_seed=42,
                       load_tokenizer=False)
    opt = m.configure_optimizers()
    m.train()
    stepper = Stepper(m, opt, world=1, max_grad_norm=1.0, dp_path=False)
    px, lab = synthetic_batch(cfg, batch, 128, seed=1)
    b = {"pixel_values": torch.from_numpy(px).cuda(), "labels": torch.from_numpy(lab).cuda()}
    for i in range(warmup):
        stepper.step(b, i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(iters):
        loss = stepper.step(b, warmup + i)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"batch": batch, "ms_per_step": round(dt * 1e3 / iters, 2), "img_per_s": round(batch * iters / dt, 1),
            "loss": round(float(loss), 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--heads", type=int, default=8)
    ap.add_argument("--S", type=int, default=257)
    ap.add_argument("--D", type=int, default=96)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step-batch", type=int, default=64)
    ap.add_argument("--step-iters", type=int, default=10)
    args = ap.parse_args()
    lib, unbound = load_tolerant()
    out = {"lib": L.LIB_PATH, "unbound": unbound, "geometry": {"B": args.B, "heads": args.heads, "S": args.S, "D": args.D}}
    if "kzv_attn_impl" not in unbound:
        out["impl"] = L.attention_impl(args.D, args.S, args.S, heads=args.heads)
    out["op"] = time_op(lib, args.B, args.heads, args.S, args.D, args.iters, args.warmup)
    if args.step_batch > 0:
        out["step"] = time_step(args.step_batch, args.step_iters, 2)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
