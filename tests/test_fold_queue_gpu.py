"""The deferred LayerNorm folds past their last free region (csrc/fold_queue.h behind KzvLnDeferScope, csrc/layernorm.hip): a model with
30 encoder layers issues 69 LayerNorm backwards inside the one scope of `kzv_backward` (the decoder's 9, then two per layer) against 63
regions, so the 64th finds none free and what is pending is folded first -- inside the nested scope of a segment.  The reference is the
same backward as `Le + 2` calls of `kzv_backward_segment`, whose scopes each close on 9 pending folds at most: same model, input, labels
and dropout seed, an identical forward before each."""
import dataclasses

import numpy as np
import pytest
import torch

from kzv import _lib as L
from kzv import params as P
from kzv.config import tiny_config
from kzv.data import build_decoder_dir, synthetic_batch
from kzv.model import TrOCRModel

pytestmark = pytest.mark.gpu


def test_one_backward_past_the_last_free_region_equals_the_segments(tmp_path):
    cfg = dataclasses.replace(tiny_config(), enc_layers=30)      # hidden 128, decoder 2 x 64; dropout 0.1 stays on
    B, Lh = 8, 12                                                # 72 encoder rows: two LayerNorm-backward workgroups
    lib = L.load()
    d = build_decoder_dir(str(tmp_path / "dec"), cfg)
    m = TrOCRModel(cfg.encoder_config_dict(), d, init_seed=3, load_tokenizer=False)
    px, lab = synthetic_batch(cfg, B, Lh, seed=3, min_chars=1, max_chars=Lh - 2)
    pxt, ids = torch.from_numpy(px).cuda(), torch.from_numpy(lab).cuda()
    m.train()
    st = L.stream_handle()

    m.forward_loss(pxt, ids, seed=11)
    m.backward()                                                 # zeroes the gradients, then ONE kzv_backward
    whole = m.flat_grads.clone()

    m.forward_loss(pxt, ids, seed=11)
    L.check(lib.kzv_zero_grads(m._h, st), "zero_grads")
    n = lib.kzv_backward_segments(m._h)
    assert n == cfg.enc_layers + 2
    for seg in range(n):
        L.check(lib.kzv_backward_segment(m._h, seg, st), "backward_segment")
    torch.cuda.synchronize()
    parts = m.flat_grads

    offsets, total = P.param_offsets(cfg)
    assert whole.numel() == total and float(whole.abs().max()) > 0
    worst = (0.0, "")
    for name, (off, shape) in offsets.items():
        k = int(np.prod(shape))
        a, b = whole[off:off + k], parts[off:off + k]
        diff, scale = float((a - b).abs().max()), float(b.abs().max())
        worst = max(worst, (diff / scale if scale > 0 else float(diff > 0), name))
        # the two differ in float-atomic order only: the bound tests/test_decoder_chain_gpu.py applies to such gradients
        assert diff <= 1e-6 * scale, f"{name}: max|diff| {diff:.3e} of max|tensor| {scale:.3e}"
    print(f"{len(offsets)} tensors, largest max|diff| / max|tensor| = {worst[0]:.2e} ({worst[1]})")
