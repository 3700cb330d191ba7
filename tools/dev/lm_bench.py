"""dev: what the language-model fusion costs (the tables of profiles/lm_fusion.md); the method of tools/dev/controls_bench.py.
(a) kzv_lm_fuse alone: --kernel times it at 256 and 1,024 rows x 4,300 tokens with histories of 64 by device events around --iters
    back-to-back launches; the order-3 LM is fitted on synthetic labels of the benchmark's length distribution (2 + U{8..60}).
(b) the 4,096-crop waves of tools/dev/controls_bench.py: generate_stream greedy and with 4 beams, alternated inside one process; per arm
    the median of --reps and the spread (max - min); every timing includes the encoder and ends on a synchronise.  Arms: "off"; "on" (the
    LM at weight 0.4: on an untrained model it changes where lines end, so its steps differ); "pin" (min_length=128: no EOS before a
    line's limit, every line runs to its limit) and "pin+lm" (the same with the LM): equal steps, so pin+lm - pin is the node's cost and
    pin+lm - off the cost of the pair.  --arms off pin runs on a build without the fusion too (KZV_PKG / KZV_LIB name it): the parent.
   python tools/dev/lm_bench.py [--kernel] [--images 4096] [--layers 6] [--reps 3] [--beams 1 4] [--arms off on pin pin+lm]"""
import argparse, os, statistics, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.environ.get("KZV_PKG") or os.path.join(ROOT, "kuzushiji-vision_amd"))
import ctypes as C
import torch
from kzv import _lib as L
from kzv.config import vit_b_config
from kzv.data import build_decoder_dir, synthetic_batch
from kzv.model import TrOCRModel

ap = argparse.ArgumentParser()
ap.add_argument("--kernel", action="store_true")
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--images", type=int, default=4096)
ap.add_argument("--layers", type=int, nargs="*", default=[6])
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--beams", type=int, nargs="*", default=[1, 4])
ap.add_argument("--arms", nargs="*", default=["off", "on", "pin", "pin+lm"])
a = ap.parse_args()
lib = L.load()
print(f"library {L.LIB_PATH}")


def synthetic_lm(cfg, vocab):
    """order 3, fitted on 2,048 synthetic label rows whose lengths are 2 + U{8..60}"""
    from kzv import lm as LM
    g = torch.Generator().manual_seed(11)
    lens = (torch.randint(8, 61, (2048,), generator=g)).tolist()
    body = torch.randint(5, min(vocab, 600), (2048, 60), generator=g).tolist()      # a character set of a few hundred: contexts recur
    return LM.NGramLM.fit([[cfg.bos_id] + body[i][:lens[i]] + [cfg.eos_id] for i in range(2048)], 3, vocab)


if a.kernel:
    V, n = 4300, 64
    cfg = vit_b_config()
    lm = synthetic_lm(cfg, V)
    d = lm.to_device("cuda")
    print(f"{lm}")
    print("| rows | us per launch | bytes moved | GB/s |")
    print("|---|---|---|---|")
    for rows in (256, 1024):
        g = torch.Generator().manual_seed(rows)
        x = (torch.randn(rows, V, generator=g) * 3).cuda()
        ids = torch.randint(5, 600, (rows, 128), generator=g).cuda()
        args = L.kzv_lm_fuse_args(logits=x.data_ptr(), ld=V, rows=rows, vocab=V, ids=ids.data_ptr(), ld_ids=128, t=n - 1, group=1, weight=0.4,
                                  lm=C.pointer(d.struct))
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for it in range(2):                                            # the first pass warms
            ev[0].record()
            for _ in range(a.iters):
                L.check(lib.kzv_lm_fuse(C.byref(args), L.stream_handle()), "lm_fuse")
            ev[1].record()
            torch.cuda.synchronize()
        us = ev[0].elapsed_time(ev[1]) * 1e3 / a.iters
        nbytes = 2 * rows * V * 4
        print(f"| {rows} | {us:.2f} | {nbytes / 1e6:.1f} MB | {nbytes / us / 1e3:.0f} |", flush=True)
    sys.exit(0)

print("| layers | beams | arm | steps | ms (spread) | ms per step |")
print("|---|---|---|---|---|---|")
for layers in a.layers:
    cfg = vit_b_config(dec_layers=layers)
    Lh = min(128, cfg.max_pos - cfg.pad_id - 1)
    x = torch.from_numpy(synthetic_batch(cfg, 256, 16, seed=3)[0]).cuda()
    x = x.repeat(-(-a.images // 256), 1, 1, 1)[:a.images].contiguous()
    g = torch.Generator().manual_seed(5)
    limits = (2 + torch.randint(8, 61, (a.images,), generator=g)).clamp(max=Lh).to(torch.int32)
    with tempfile.TemporaryDirectory() as tmp:
        m = TrOCRModel(cfg.encoder_config_dict(), build_decoder_dir(os.path.join(tmp, "d"), cfg), init_seed=1, load_tokenizer=False)
    m.state_dict_views()["decoder.lm_head.bias"][cfg.pad_id] -= 8.0   # as decode_stream_bench.py: no running beam takes padding
    m.eval()
    arms = {"off": {}, "pin": {"min_length": 128}}
    if "on" in a.arms or "pin+lm" in a.arms:
        arms["on"] = {"lm": synthetic_lm(cfg, cfg.vocab), "lm_weight": 0.4}
        arms["pin+lm"] = dict(arms["on"], min_length=128)
    for nb in a.beams:
        kw = {} if nb == 1 else {"num_beams": nb}
        ts, steps = {k: [] for k in a.arms}, {}
        for arm in a.arms:                                             # warm: binds, packs, graphs
            m.generate_stream(x, max_length=Lh, limits=limits, **kw, **arms[arm])
            assert m.last_stream_pad_fallbacks == 0
        for _ in range(a.reps):
            for arm in a.arms:
                torch.cuda.synchronize(); t0 = time.perf_counter()
                m.generate_stream(x, max_length=Lh, limits=limits, **kw, **arms[arm])
                torch.cuda.synchronize(); ts[arm].append((time.perf_counter() - t0) * 1e3)
                steps[arm] = m.last_stream_steps
        for arm in a.arms:
            med, spr = statistics.median(ts[arm]), max(ts[arm]) - min(ts[arm])
            print(f"| {layers} | {nb} | {arm} | {steps[arm]} | {med:.1f} ({spr:.1f}) | {med / steps[arm]:.3f} |", flush=True)
