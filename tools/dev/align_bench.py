"""TrOCRModel.align at the benchmark geometry (ViT-B on 64 x 640 crops = 160 patches, the reference decoder, batch 256, labels of
128): wall time of one call with and without the maps, and -- run under `rocprofv3 --kernel-trace --stats -- python
tools/dev/align_bench.py` -- the times of attn_probs_kernel / token_scores_kernel beside the cross-attention forward kernel's."""
import sys, tempfile, time
sys.path.insert(0, "kuzushiji-vision_amd")
import torch
from kzv.config import vit_b_config
from kzv.data import build_decoder_dir, synthetic_batch
from kzv.model import TrOCRModel
cfg = vit_b_config(int(sys.argv[1]) if len(sys.argv) > 1 else 12)
d = build_decoder_dir(tempfile.mkdtemp(), cfg)
m = TrOCRModel(cfg.encoder_config_dict(), d, init_seed=1, load_tokenizer=False)
m.eval()
px, lab = synthetic_batch(cfg, 256, 128, seed=3, min_chars=100, max_chars=127)
x, ids = torch.from_numpy(px).cuda(), torch.from_numpy(lab).cuda()
for want_map in (False, True):
    out = m.align(x, ids, want_map=want_map)              # the first call binds the workspace
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(3):
        out = m.align(x, ids, want_map=want_map)
    torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / 3
    live = out["live"]
    print(f"align(want_map={want_map}): {dt * 1e3:.1f} ms for 256 crops x {m.last_active_length} positions; "
          f"mean logprob {float(out['logprob'][live].mean()):.3f}, max |row sum - 1| {float((out['row_sum'][live] - 1).abs().max()):.2g}")
