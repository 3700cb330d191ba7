"""dev: generation time of the one-launch decoder step against the launch-per-operation step at 161 / 256 / 320 patch keys
(the table of profiles/decode_wide.md and DESIGN.md section 7, N1).  256 crops, max_length 128, early_stopping=False, beam-4 and
greedy, 6 and 12 decoder layers; per cell a warm call, then the median of REPS timed calls between synchronisations.
   python tools/dev/decode_wide_bench.py [--patches 161 256 320] [--layers 6 12] [--reps 3]
KZV_LIB points at a variant library (-DKZV_DF_CHUNKS=2|4|8); KZV_PKG at another tree's kuzushiji-vision_amd (the parent commit's, whose
mode 0 must not have moved)."""
import argparse, dataclasses, os, statistics, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.environ.get("KZV_PKG") or os.path.join(ROOT, "kuzushiji-vision_amd"))
import torch
from kzv import _lib as L
from kzv.config import reference_cli_config
from kzv.data import build_decoder_dir, synthetic_batch
from kzv.model import TrOCRModel

GEOM = {161: dict(image_h=16, image_w=2576), 256: dict(image_h=1024, image_w=64), 320: dict(image_h=64, image_w=1280, enc_heads=12)}
ap = argparse.ArgumentParser()
ap.add_argument("--patches", type=int, nargs="*", default=[161, 256, 320])
ap.add_argument("--layers", type=int, nargs="*", default=[6, 12])
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--images", type=int, default=256)
a = ap.parse_args()
lib = L.load()
print(f"library {L.LIB_PATH}")
print("| patch keys | decoder layers | rows per image | per-operation ms | one-launch ms | ratio | step |")
print("|---|---|---|---|---|---|---|")
for patches in a.patches:
    for layers in a.layers:
        cfg = dataclasses.replace(reference_cli_config(), dec_layers=layers, **GEOM[patches])
        assert cfg.num_patches == patches
        with tempfile.TemporaryDirectory() as tmp:
            m = TrOCRModel(cfg.encoder_config_dict(), build_decoder_dir(os.path.join(tmp, "d"), cfg), init_seed=1, load_tokenizer=False,
                           long_sequences=cfg.enc_seq > 288)
        m.eval()
        x = torch.from_numpy(synthetic_batch(cfg, a.images, 128, seed=3)[0]).cuda()
        for beams in (4, 1):
            ms, how = [], "?"
            for mode in (0, 1):
                L.check(lib.kzv_set_decode_one_launch(mode), "mode")
                m.generate(x, max_length=128, num_beams=beams, early_stopping=False)      # warm: binds, captures the step's graph
                if mode and hasattr(m, "decode_step_impl"):
                    how = m.decode_step_impl
                ts = []
                for _ in range(a.reps):
                    torch.cuda.synchronize(); t0 = time.perf_counter()
                    m.generate(x, max_length=128, num_beams=beams, early_stopping=False)
                    torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
                ms.append(statistics.median(ts))
            print(f"| {patches} | {layers} | {beams} | {ms[0]:.1f} | {ms[1]:.1f} | {ms[1] / ms[0]:.3f} | {how} |", flush=True)
        del m, x
        torch.cuda.empty_cache()
