"""dev: what top-k alternatives cost (the figures of profiles/alternatives.md).

   python tools/dev/alternatives_bench.py kernels [--reps 5] [--k 5]
       kzv_token_scores and kzv_token_topk on the same fp32 logits, the benchmark geometry: 256 x 127 rows of 4,300 columns in the
       4,352 stride (559 MB).  Meant to run under `rocprofv3 --kernel-trace --stats -- python ...`: token_scores_kernel and
       token_topk_kernel then stand side by side in the kernel statistics; the wall times printed here include the launch.
   python tools/dev/alternatives_bench.py stream [--images 4096] [--layers 6 12] [--reps 3] [--k 5]
       generate_stream on the workload of profiles/decode_stream.md (ViT-B encoder, 64 x 640 crops, the reference decoder, 256 slots,
       limits 2 + U{8..60}, bf16) with top_k = 0 and top_k = k, alternated in one process; every timing includes the encoder and ends
       on a synchronise; per cell the median of --reps and the spread (max - min)."""
import argparse, os, statistics, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.environ.get("KZV_PKG") or os.path.join(ROOT, "kuzushiji-vision_amd"))
import torch
from kzv import _lib as L

ap = argparse.ArgumentParser()
ap.add_argument("what", choices=["kernels", "stream"])
ap.add_argument("--images", type=int, default=4096)
ap.add_argument("--layers", type=int, nargs="*", default=[6, 12])
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--k", type=int, default=5)
a = ap.parse_args()
lib = L.load()

if a.what == "kernels":
    B, T, V, ld = 256, 127, 4300, 4352
    rows = B * T
    logits = torch.randn(rows, ld, device="cuda")
    targets = torch.randint(4, V, (B, T + 1), device="cuda")
    logprob = torch.empty(rows, device="cuda")
    top1 = torch.empty(rows, dtype=torch.int64, device="cuda")
    top1_lp = torch.empty(rows, device="cuda")
    ids = torch.empty(rows, a.k, dtype=torch.int32, device="cuda")
    lp = torch.empty(rows, a.k, device="cuda")
    st = L.stream_handle()

    def scores():
        L.check(lib.kzv_token_scores(logits.data_ptr(), ld, targets.data_ptr(), T + 1, B, T, V, 1, logprob.data_ptr(), top1.data_ptr(), top1_lp.data_ptr(), st), "token_scores")

    def topk():
        L.check(lib.kzv_token_topk(logits.data_ptr(), ld, rows, V, a.k, ids.data_ptr(), lp.data_ptr(), st), "token_topk")

    ts = {"token_scores": [], "token_topk": []}
    for rep in range(a.reps + 1):                              # the first round warms both
        for name, fn in (("token_scores", scores), ("token_topk", topk)):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep:
                ts[name].append((time.perf_counter() - t0) * 1e6)
    assert bool(torch.equal(ids[:, 0].long(), top1)) and float((lp[:, 0] - top1_lp).abs().max()) <= 1e-6
    gb = rows * V * 4 / 1e9
    for name, v in ts.items():
        med = statistics.median(v)
        print(f"{name}: {rows} rows x {V} columns (stride {ld}), k = {a.k}: median {med:.0f} us wall (spread {max(v) - min(v):.0f}), {gb / med * 1e6:.0f} GB/s of logits")
    sys.exit(0)

from kzv.config import vit_b_config
from kzv.data import build_decoder_dir, synthetic_batch
from kzv.model import TrOCRModel

print(f"library {L.LIB_PATH}; {a.images} crops; top_k 0 against {a.k}")
print("| layers | stream steps | top_k = 0 ms (spread) | top_k = %d ms (spread) | ratio |" % a.k)
print("|---|---|---|---|---|")
for layers in a.layers:
    cfg = vit_b_config(dec_layers=layers)
    Lh = min(128, cfg.max_pos - cfg.pad_id - 1)
    x = torch.from_numpy(synthetic_batch(cfg, 256, 16, seed=3)[0]).cuda()
    x = x.repeat(-(-a.images // 256), 1, 1, 1)[:a.images].contiguous()
    g = torch.Generator().manual_seed(5)
    limits = (2 + torch.randint(8, 61, (a.images,), generator=g)).clamp(max=Lh).to(torch.int32)
    with tempfile.TemporaryDirectory() as tmp:
        m = TrOCRModel(cfg.encoder_config_dict(), build_decoder_dir(os.path.join(tmp, "d"), cfg), init_seed=1, load_tokenizer=False)
    m.eval()
    want = m.generate_stream(x, max_length=Lh, limits=limits)                      # warm both: binds, packs, graphs
    got = m.generate_stream(x, max_length=Lh, limits=limits, top_k=a.k)
    assert m.stream_decode_impl == "slot-refill" and bool(torch.equal(got[0], want))
    ts = {0: [], a.k: []}
    for _ in range(a.reps):
        for k in ts:
            torch.cuda.synchronize(); t0 = time.perf_counter()
            m.generate_stream(x, max_length=Lh, limits=limits, top_k=k)
            torch.cuda.synchronize(); ts[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: statistics.median(v) for k, v in ts.items()}
    spr = {k: max(v) - min(v) for k, v in ts.items()}
    print(f"| {layers} | {m.last_stream_steps} | {med[0]:.1f} ({spr[0]:.1f}) | {med[a.k]:.1f} ({spr[a.k]:.1f}) | {med[a.k] / med[0]:.3f} |", flush=True)
    del m, x
    torch.cuda.empty_cache()
