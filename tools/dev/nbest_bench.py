"""dev: what n-best lists and per-token log-probabilities cost the beam search on refilled slots (the table of profiles/nbest.md).
The job of tools/dev/decode_stream_bench.py --beams 4: ViT-B encoder, 64 x 640 crops (160 patch keys), the reference decoder, N resident
crops on the device's compute-unit count of slots, limits = 2 + U{8..60} (seeded) and every limit = Lh; the padding bias lowered by 8.
Modes, alternated inside one process, each timing with the encoder and ending on a synchronise; per cell the median of --reps and the
spread (max - min):
   off      generate_stream(num_beams=4)                                                   -- the call without the new keywords
   nbest    generate_stream(num_beams=4, num_return_sequences=4)                            -- more written when a search ends
   nbest+lp generate_stream(num_beams=4, num_return_sequences=4, return_logprobs=True)      -- the LP instance: one more staged row copy per step
KZV_PKG=<another tree's package> with --modes off times a tree that has no such keywords (the parent commit).
   python tools/dev/nbest_bench.py [--images 4096] [--layers 6] [--reps 3] [--modes off nbest nbest+lp]"""
import argparse, os, statistics, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.environ.get("KZV_PKG") or os.path.join(ROOT, "kuzushiji-vision_amd"))
import torch
from kzv import _lib as L
from kzv.config import vit_b_config
from kzv.data import build_decoder_dir, synthetic_batch
from kzv.model import TrOCRModel

ap = argparse.ArgumentParser()
ap.add_argument("--images", type=int, default=4096)
ap.add_argument("--layers", type=int, nargs="*", default=[6])
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--beams", type=int, default=4)
ap.add_argument("--modes", nargs="*", default=["off", "nbest", "nbest+lp"])
a = ap.parse_args()
L.load()
KW = {"off": {}, "nbest": {"num_return_sequences": a.beams}, "nbest+lp": {"num_return_sequences": a.beams, "return_logprobs": True}}
print(f"library {L.LIB_PATH}; {a.images} crops; {a.beams} beams; modes {a.modes}")
print("| layers | limits | steps | " + " | ".join(f"{m} ms (spread)" for m in a.modes) + " |")
print("|---|---|---|" + "---|" * len(a.modes))
for layers in a.layers:
    cfg = vit_b_config(dec_layers=layers)
    Lh = min(128, cfg.max_pos - cfg.pad_id - 1)
    x = torch.from_numpy(synthetic_batch(cfg, 256, 16, seed=3)[0]).cuda()
    x = x.repeat(-(-a.images // 256), 1, 1, 1)[:a.images].contiguous()
    g = torch.Generator().manual_seed(5)
    cases = {"2 + U{8..60}": (2 + torch.randint(8, 61, (a.images,), generator=g)).clamp(max=Lh).to(torch.int32),
             f"all {Lh}": torch.full((a.images,), Lh, dtype=torch.int32)}
    with tempfile.TemporaryDirectory() as tmp:
        m = TrOCRModel(cfg.encoder_config_dict(), build_decoder_dir(os.path.join(tmp, "d"), cfg), init_seed=1, load_tokenizer=False)
    m.state_dict_views()["decoder.lm_head.bias"][cfg.pad_id] -= 8.0
    m.eval()
    for name, limits in cases.items():
        for mode in a.modes:                                                          # warm: binds, packs, graphs
            m.generate_stream(x, max_length=Lh, limits=limits, num_beams=a.beams, **KW[mode])
            assert m.stream_beam_impl == "slot-refill" and m.last_stream_pad_fallbacks == 0
        ts = {mode: [] for mode in a.modes}
        for _ in range(a.reps):
            for mode in a.modes:
                torch.cuda.synchronize(); t0 = time.perf_counter()
                m.generate_stream(x, max_length=Lh, limits=limits, num_beams=a.beams, **KW[mode])
                torch.cuda.synchronize(); ts[mode].append((time.perf_counter() - t0) * 1e3)
        print(f"| {layers} | {name} | {m.last_stream_steps} | " +
              " | ".join(f"{statistics.median(v):.1f} ({max(v) - min(v):.1f})" for v in ts.values()) + " |", flush=True)
    del m, x
    torch.cuda.empty_cache()
