"""dev: what forced prefixes cost decoding on refilled slots (the tables of profiles/prefix.md).
The job of tools/dev/controls_bench.py: ViT-B encoder, 64 x 640 crops (160 patch keys), the reference decoder, N resident crops on the
device's compute-unit count of slots, limits = 2 + U{8..60} (seeded: line lengths pinned), greedy and 4 beams; the padding bias lowered
by 8.  Modes, alternated inside one process, each timing with the encoder and ending on a synchronise; per cell the median of --reps and
the spread (max - min):
   off     generate_stream(...)                                   -- the call without the new keyword
   prefix  generate_stream(..., prefix_ids = 4 tokens per image)  -- one more node per step; a beam wave on the rank-log-probabilities route
Under the pinned limits a forced token takes the place of a free one, so both modes take the same number of steps and "prefix - off" is the
node's cost (beams: plus the route's).
KZV_PKG=<another tree's package> with --modes off times a tree that has no such keyword (the parent commit).
   python tools/dev/prefix_bench.py [--images 4096] [--layers 6] [--reps 3] [--beams 1 4] [--modes off prefix] [--forced 4]"""
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
ap.add_argument("--layers", type=int, default=6)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--beams", type=int, nargs="*", default=[1, 4])
ap.add_argument("--forced", type=int, default=4)
ap.add_argument("--modes", nargs="*", default=["off", "prefix"])
a = ap.parse_args()
L.load()
print(f"library {L.LIB_PATH}; {a.images} crops; {a.forced} forced tokens; modes {a.modes}")
print("| beams | steps | " + " | ".join(f"{m} ms (spread)" for m in a.modes) + " |")
print("|---|---|" + "---|" * len(a.modes))
cfg = vit_b_config(dec_layers=a.layers)
Lh = min(128, cfg.max_pos - cfg.pad_id - 1)
x = torch.from_numpy(synthetic_batch(cfg, 256, 16, seed=3)[0]).cuda()
x = x.repeat(-(-a.images // 256), 1, 1, 1)[:a.images].contiguous()
g = torch.Generator().manual_seed(5)
limits = (2 + torch.randint(8, 61, (a.images,), generator=g)).clamp(max=Lh).to(torch.int32)
prefix = torch.randint(5, cfg.vocab, (a.images, a.forced), generator=g)
KW = {"off": {}, "prefix": {"prefix_ids": prefix}}
with tempfile.TemporaryDirectory() as tmp:
    m = TrOCRModel(cfg.encoder_config_dict(), build_decoder_dir(os.path.join(tmp, "d"), cfg), init_seed=1, load_tokenizer=False)
m.state_dict_views()["decoder.lm_head.bias"][cfg.pad_id] -= 8.0
m.eval()
for nb in a.beams:
    kw = {} if nb == 1 else {"num_beams": nb}
    steps = {}
    for mode in a.modes:                                                              # warm: binds, packs, graphs
        m.generate_stream(x, max_length=Lh, limits=limits, **kw, **KW[mode])
        steps[mode] = m.last_stream_steps
        assert (m.stream_decode_impl if nb == 1 else m.stream_beam_impl) == "slot-refill" and m.last_stream_pad_fallbacks == 0
    ts = {mode: [] for mode in a.modes}
    for _ in range(a.reps):
        for mode in a.modes:
            torch.cuda.synchronize(); t0 = time.perf_counter()
            m.generate_stream(x, max_length=Lh, limits=limits, **kw, **KW[mode])
            torch.cuda.synchronize(); ts[mode].append((time.perf_counter() - t0) * 1e3)
    print(f"| {nb} | {' / '.join(str(steps[mode]) for mode in a.modes)} | " +
          " | ".join(f"{statistics.median(v):.1f} ({max(v) - min(v):.1f})" for v in ts.values()) + " |", flush=True)
