#!/usr/bin/env python3
"""Times the encoder attention and the whole training step at the reference CLI's defaults; prints one JSON line.

  python tools/attn_bench.py [--B 64 --heads 8 --S 257 --D 96] [--step-batch 64] [--iters 20 --warmup 5]
  python tools/attn_bench.py --long [--iters 20 --warmup 5] [--step-batch 64]

--long measures the K/V-streaming kernels (kzv_attn_stream_fwd / _bwd) next to what kzv_attn_fwd / _bwd run on the same launch
(the whole-head MFMA kernels at 257 tokens, the VALU kernel at head_dim 96 and 384 tokens), the streaming kernels alone at
head_dim 64, B * heads = 32 * 12, 1,025 tokens, and the step of the reference CLI model built with long_sequences=True on
1024 x 64, 1536 x 64 and 2048 x 64 columns (257, 385 and 513 tokens).

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


def time_op(lib, B, heads, S, D, iters, warmup, stream=False):
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
    fns = (("fwd", lib.kzv_attn_stream_fwd), ("bwd", lib.kzv_attn_stream_bwd)) if stream else (("fwd", lib.kzv_attn_fwd), ("bwd", lib.kzv_attn_bwd))
    for name, fn in fns:
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


def time_step(batch, iters, warmup, image_h=1024, long_sequences=False):
    import dataclasses
    from kzv.config import reference_cli_config
    from kzv.data import build_decoder_dir, synthetic_batch
    from kzv.model import TrOCRModel
    from kzv.trainer import Stepper
    cfg = dataclasses.replace(reference_cli_config(), image_h=image_h)
    with tempfile.TemporaryDirectory() as tmp:
        kw = {"long_sequences": True} if long_sequences else {}
        m = TrOCRModel(cfg.encoder_config_dict(), build_decoder_dir(os.path.join(tmp, "dec"), cfg), device="cuda:0", init_seed=42,
                       load_tokenizer=False, **kw)
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
    out = {"batch": batch, "ms_per_step": round(dt * 1e3 / iters, 2), "img_per_s": round(batch * iters / dt, 1),
           "loss": round(float(loss), 4)}
    del stepper, opt, m
    torch.cuda.empty_cache()
    return out


def long_table(lib, iters, warmup, step_batch, step_iters):
    """--long: streaming against whole-head / VALU on the same launches, the 1,025-token throughput, the long-column steps."""
    ops = []
    for B, heads, S, D, other in ((64, 8, 257, 96, True), (64, 12, 257, 64, True), (64, 8, 384, 96, True), (32, 12, 1025, 64, False)):
        row = {"B": B, "heads": heads, "S": S, "D": D, "stream": time_op(lib, B, heads, S, D, iters, warmup, stream=True)}
        if other:
            row["impl"] = L.attention_impl(D, S, S, heads=heads)
            row[row["impl"]] = time_op(lib, B, heads, S, D, iters if row["impl"] != "valu" else max(2, iters // 5), warmup, stream=False)
        ops.append(row)
    steps = []
    if step_batch > 0:
        for h in (1024, 1536, 2048):
            steps.append(dict(image=f"{h}x64", tokens=h // 16 * 4 + 1, **time_step(step_batch, step_iters, 2, image_h=h, long_sequences=True)))
    return {"op": ops, "step": steps}


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
    ap.add_argument("--long", action="store_true", help="the streaming-kernel table (see above)")
    ap.add_argument("--stream", action="store_true", help="time kzv_attn_stream_fwd / _bwd instead of kzv_attn_fwd / _bwd")
    args = ap.parse_args()
    lib, unbound = load_tolerant()
    if args.long:
        print(json.dumps({"lib": L.LIB_PATH, **long_table(lib, args.iters, args.warmup, args.step_batch, args.step_iters)}), flush=True)
        return
    out = {"lib": L.LIB_PATH, "unbound": unbound, "geometry": {"B": args.B, "heads": args.heads, "S": args.S, "D": args.D}}
    if "kzv_attn_impl" not in unbound:
        out["impl"] = L.attention_impl(args.D, args.S, args.S, heads=args.heads, long_sequences=args.stream)
    out["op"] = time_op(lib, args.B, args.heads, args.S, args.D, args.iters, args.warmup, stream=args.stream)
    if args.step_batch > 0:
        out["step"] = time_step(args.step_batch, args.step_iters, 2)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
