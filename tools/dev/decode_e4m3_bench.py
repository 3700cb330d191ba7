"""dev: generation time with the decoder's streamed linears read as bf16 against e4m3 (kzv_set_decode_weights; the table of
profiles/decode_e4m3.md and DESIGN.md section 7, N1).  256 crops x 128 tokens, encoder included, early_stopping=False; 160 / 256 / 320
patch keys, 6 / 12 decoder layers, 4 / 1 rows per image.  The formats are timed ALTERNATELY on one model inside this one process,
REPS times each, between synchronisations: median and (min - max) per format.  A switch of format re-captures the step's graphs
(their key holds the format), so every timed call follows an UNTIMED one in the same format that has done that.  (Two handles,
one per format, do not fit at 320 patch keys x 1,024 rows: the long-sequence workspace is 152 GiB.)  (What a weight
change costs in e4m3 mode is one quant_pack8_kernel launch: read it from a kernel trace, profiles/decode_e4m3.md.)
   python tools/dev/decode_e4m3_bench.py [--patches 160 256 320] [--layers 6 12] [--rows 4 1] [--reps 5] [--weights bf16 e4m3]
KZV_PKG points at another tree's kuzushiji-vision_amd (the parent commit's, with --weights bf16: its default path must not have moved);
KZV_LIB at a variant library (-DKZV_DF_WIN8=32: time it with --weights e4m3 and compare with the stock build's bf16 column)."""
import argparse, dataclasses, os, statistics, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.environ.get("KZV_PKG") or os.path.join(ROOT, "kuzushiji-vision_amd"))
import torch
from kzv import _lib as L
from kzv.config import reference_cli_config
from kzv.data import build_decoder_dir, synthetic_batch
from kzv.model import TrOCRModel

GEOM = {160: dict(image_h=16, image_w=2560), 161: dict(image_h=16, image_w=2576), 256: dict(image_h=1024, image_w=64),
        320: dict(image_h=64, image_w=1280, enc_heads=12)}
ap = argparse.ArgumentParser()
ap.add_argument("--patches", type=int, nargs="*", default=[160, 256, 320])
ap.add_argument("--layers", type=int, nargs="*", default=[6, 12])
ap.add_argument("--rows", type=int, nargs="*", default=[4, 1])
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--images", type=int, default=256)
ap.add_argument("--tokens", type=int, default=128)
ap.add_argument("--weights", nargs="*", default=["bf16", "e4m3"], choices=["bf16", "e4m3"])
a = ap.parse_args()
lib = L.load()
print(f"library {L.LIB_PATH}; {a.images} crops x {a.tokens} tokens; median (min - max) of {a.reps}, ms per generate")
print("| patch keys | layers | rows | " + " | ".join(a.weights) + " | e4m3 / bf16 | read |")
print("|---|---|---|" + "---|" * len(a.weights) + "---|---|")


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


for patches in a.patches:
    for layers in a.layers:
        cfg = dataclasses.replace(reference_cli_config(), dec_layers=layers, **GEOM[patches])
        assert cfg.num_patches == patches
        with tempfile.TemporaryDirectory() as tmp:
            m = TrOCRModel(cfg.encoder_config_dict(), build_decoder_dir(os.path.join(tmp, "d"), cfg), init_seed=1, load_tokenizer=False,
                           long_sequences=cfg.enc_seq > 288)
        m.eval()
        x = torch.from_numpy(synthetic_batch(cfg, a.images, a.tokens, seed=3)[0]).cuda()
        for rows in a.rows:
            def gen():
                m.generate(x, max_length=a.tokens, num_beams=rows, early_stopping=False)

            def use(fmt):                                             # the format, and an untimed call that captures its graphs
                if fmt != "bf16" or hasattr(m, "set_decode_weights"):
                    m.set_decode_weights(fmt)
                gen()
            read = {}
            for fmt in a.weights:                                     # warm: binds, packs
                use(fmt)
                read[fmt] = getattr(m, "decode_weights_impl", "bf16")
            ts = {fmt: [] for fmt in a.weights}
            for _ in range(a.reps):
                for fmt in a.weights:
                    use(fmt)
                    ts[fmt].append(timed(gen))
            med = {fmt: statistics.median(v) for fmt, v in ts.items()}
            cells = " | ".join(f"{med[f]:.1f} ({min(ts[f]):.1f} - {max(ts[f]):.1f})" for f in a.weights)
            both = len(a.weights) == 2
            ratio = f"{med['e4m3'] / med['bf16']:.3f}" if both else "-"
            print(f"| {patches} | {layers} | {rows} | {cells} | {ratio} | {' / '.join(read[f] for f in a.weights)} |", flush=True)
        if hasattr(m, "set_decode_weights"):
            m.set_decode_weights("bf16")
        del m, x
        torch.cuda.empty_cache()
