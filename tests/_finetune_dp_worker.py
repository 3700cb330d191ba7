"""Worker of tests/test_finetune_gpu.py::test_two_rank_accumulation_window_with_frozen_layer: one rank of a data-parallel run of
kzv.trainer.Stepper with accumulate_grad_batches = 2 and one frozen encoder layer -- the ranks share GPU 0 and talk over gloo
(KZV_DIST_BACKEND=gloo KZV_FORCE_DEVICE=0), like tests/_stepper_worker.py."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "kuzushiji-vision_amd")):
    sys.path.insert(0, p)

from kzv import finetune  # noqa: E402
from kzv.data import build_decoder_dir, synthetic_batch  # noqa: E402
from kzv.model import TrOCRModel  # noqa: E402
from kzv.trainer import Stepper, init_distributed  # noqa: E402

WINDOWS, K, FREEZE, PER_RANK, LR, BETA2, SEED = 7, 2, 1, 2, 5e-3, 0.99, 4     # beta2 0.99: RAdam leaves its silent phase at step 6


def run_config():
    import dataclasses
    from kzv.config import tiny_config
    return dataclasses.replace(tiny_config(), enc_hidden_dropout=0.0, enc_attn_dropout=0.0, dec_hidden_dropout=0.0, dec_attn_dropout=0.0)


def micro_batch(cfg, window, j, rank):
    px, lab = synthetic_batch(cfg, PER_RANK, 18, seed=900 + 16 * window + 4 * j + rank, min_chars=3, max_chars=17)
    return {"pixel_values": torch.from_numpy(px), "labels": torch.from_numpy(lab)}


def make(out, tag, device="cuda:0"):
    cfg = run_config()
    d = build_decoder_dir(os.path.join(out, f"dec{tag}"), cfg)
    m = TrOCRModel(cfg.encoder_config_dict(), d, learning_rate=LR, beta2=BETA2, init_seed=SEED, load_tokenizer=False, device=device)
    opt = m.configure_optimizers()
    finetune.apply(m, opt, freeze_encoder_layers=FREEZE)
    m.train()
    return cfg, m, opt


def main():
    out = sys.argv[1]
    rank, world, local = init_distributed()
    cfg, m, opt = make(out, rank, f"cuda:{local}")
    st = Stepper(m, opt, world=world, max_grad_norm=1.0, bucket_mb=0.2, accumulate_grad_batches=K)
    import torch.distributed as dist
    reduced = []
    real = dist.all_reduce

    def counting(t, *a, **kw):              # which ranges are all-reduced, and in which micro-batch
        reduced.append((st._micro, t.data_ptr() - m.flat_grads.data_ptr(), t.numel()))
        return real(t, *a, **kw)
    dist.all_reduce = counting
    norms = []
    for w in range(WINDOWS):
        for j in range(K):
            st.step(micro_batch(cfg, w, j, rank), w * K + j)
        assert st.stepped
        norms.append(opt.grad_norm())
    torch.cuda.synchronize()
    torch.save({"params": m.flat_params.cpu(), "norms": norms, "buckets": st.buckets, "seg_ranges": st.seg_ranges, "reduced": reduced,
                "dp_path": st.dp_path}, os.path.join(out, f"rank{rank}.pt"))
    dist.all_reduce = real
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
