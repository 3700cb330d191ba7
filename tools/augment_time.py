"""Timing of the augmentation kernel (csrc/augment.hip) against its two yardsticks: a copy of the same tensors (the byte floor,
2 * n*3*H*W*4 bytes) and the training step it joins.  Needs an MI355X; prints one JSON object.

  python tools/augment_time.py                     # kernel vs out.copy_(in) at batch 256 on 64x640 and 1024x64, then the step
  python tools/augment_time.py --no-step           # kernel and copy only

Kernel: HIP events around 50 launches after a warm-up, alternating with 50 copies of the same tensors, three repeats (the spread
is printed); parameter sets: every operation on for every crop, the reference preset's mix, the identity, and each operation alone.
Step: bench.py's model and batch (ViT-B encoder, 6 decoder layers, batch 256 of 64x640 crops) through kzv.trainer.Stepper, with and
without the per-step work `--augment reference` adds (host draw of the parameters, their upload, the kernel); host clock around
steps that end in a device synchronise."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kuzushiji-vision_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from kzv import augment as A  # noqa: E402


def event_ms(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches


def all_on(n, H, W):
    rng = np.random.default_rng(0)
    p = A.identity_params(n)
    p["m"] = A.inverse_affine(rng.uniform(-7, 7, n), (np.round(rng.uniform(-5, 5, n)), np.round(rng.uniform(-3, 3, n))), rng.uniform(0.93, 1.07, n),
                              (rng.uniform(-5, 5, n), rng.uniform(-5, 5, n)), H, W)
    p["morph"] = 1 + np.arange(n) % 2
    p["blur"] = A.blur_weights(rng.uniform(0.5, 1.5, n))
    p["contrast"], p["brightness"], p["noise_sigma"] = 1.2, -0.1, 0.05
    p["noise_key"] = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    return p


def time_kernel(n, H, W, launches, repeats):
    from kzv import _lib as L
    lib = L.load()
    x = torch.rand(n, 3, H, W, device="cuda") * 2 - 1
    out = torch.empty_like(x)
    on = all_on(n, H, W)
    sets = {"all_on": on, "reference_mix": A.sample_params(A.preset("reference"), n, H, W, seed=1), "identity": A.identity_params(n)}
    for name, fields in (("warp_only", ("m",)), ("morph_only", ("morph",)), ("blur_only", ("blur",)), ("noise_only", ("noise_sigma", "noise_key"))):
        sets[name] = A.identity_params(n)                 # one operation for every crop: which stage costs what
        for f in fields:
            sets[name][f] = on[f]
    res = {"shape": [n, 3, H, W], "floor_mb": 2 * x.numel() * 4 / 1e6}
    copies = []
    for name, p in sets.items():
        d_p = torch.from_numpy(p.view(np.uint8).reshape(-1).copy()).cuda()

        def launch():
            L.check(lib.kzv_augment_lines(x.data_ptr(), d_p.data_ptr(), n, H, W, out.data_ptr(), L.stream_handle()), "augment_lines")
        for _ in range(5):
            launch(); out.copy_(x)
        torch.cuda.synchronize()
        ks, cs = [], []
        for _ in range(repeats):                         # alternate the two, so that they see the same machine
            ks.append(event_ms(launch, launches))
            cs.append(event_ms(lambda: out.copy_(x), launches))
        copies += cs
        res[name] = {"kernel_us": [round(k * 1e3, 1) for k in ks], "copy_us": [round(c * 1e3, 1) for c in cs],
                     "ratio_to_copy": round(min(ks) / min(cs), 2), "floor_tb_s": round(res["floor_mb"] / 1e6 / (min(ks) * 1e-3), 2)}
    res["copy_tb_s"] = round(res["floor_mb"] / 1e6 / (min(copies) * 1e-3), 2)
    return res


def time_step(steps, warmup):
    from kzv.config import vit_b_config
    from kzv.data import build_decoder_dir, synthetic_batch
    from kzv.model import TrOCRModel
    from kzv.trainer import Stepper
    cfg = vit_b_config(dec_layers=6)
    with tempfile.TemporaryDirectory() as tmp:
        model = TrOCRModel(cfg.encoder_config_dict(), build_decoder_dir(os.path.join(tmp, "dec"), cfg), device="cuda:0", init_seed=42, load_tokenizer=False)
    opt = model.configure_optimizers()
    model.train()
    stepper = Stepper(model, opt, world=1, max_grad_norm=1.0, dp_path=False)
    px, lab = synthetic_batch(cfg, 256, 128, seed=1)
    px = np.clip(px, -1, 1)
    batch = {"pixel_values": torch.from_numpy(px).cuda(), "labels": torch.from_numpy(lab).cuda()}
    aug, acfg = A.DeviceAugment("cuda:0"), A.preset("reference")
    n, _, H, W = batch["pixel_values"].shape
    out = torch.empty_like(batch["pixel_values"])

    def plain(i):
        stepper.step(batch, i)

    def augmented(i):
        p = A.sample_params(acfg, n, H, W, seed=42, rank=0, epoch=0, step=i)
        stepper.step({"pixel_values": aug(batch["pixel_values"], p, out=out), "labels": batch["labels"]}, i)

    def run(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            fn(i)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3
    for i in range(warmup):
        plain(i); augmented(i)
    t = {"plain_ms": [], "augmented_ms": []}
    for _ in range(3):
        t["plain_ms"].append(round(run(plain), 3)); t["augmented_ms"].append(round(run(augmented), 3))
    t0 = time.perf_counter()
    for i in range(20):
        A.sample_params(acfg, n, H, W, seed=42, step=i)
    t["host_draw_ms"] = round((time.perf_counter() - t0) / 20 * 1e3, 3)
    t["share_of_step"] = round(min(t["augmented_ms"]) / min(t["plain_ms"]) - 1.0, 4)
    t["images_per_s"] = {"plain": round(256 / min(t["plain_ms"]) * 1e3), "augmented": round(256 / min(t["augmented_ms"]) * 1e3)}
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_time.py measures on an MI355X: no GPU here, nothing measured")
    res = {"kernel": [time_kernel(args.batch, H, W, args.launches, args.repeats) for H, W in ((64, 640), (1024, 64))]}
    if not args.no_step:
        res["step"] = time_step(args.steps, args.warmup)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
