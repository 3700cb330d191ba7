"""The sharpened model of tests/_peaked.py without a GPU: for the three crops the GPU tests decode (160, 320 and 512 patch keys), on a
batch of 3 rows,

  * peaked() reaches both of its conditions (peaks above 0.3; min(sens_self, sens_cross) >= 6 x err_ref);
  * the recipe model reaches neither: its cross-attention is uniform and halving the cross softmax scale moves its fp64 logits by less
    than 1e-3 -- a tenth of the 1e-2 the path-against-path tests of the generation step allow;
  * every returned tensor is bf16-exact;
  * O.stepwise_logits on the sharpened weights equals the teacher-forced O.decoder_forward column: the reference the GPU tests use
    reads a prefix the way a teacher-forced pass reads a whole line.
Figures on the CPU (query factors self / cross, peaks, err_ref, sens_self, sens_cross): see DESIGN.md section 7."""
import numpy as np
import pytest
import torch

import _peaked as PK
from kzv import params as P
from oracle import trocr_oracle as O

SEED, LH = 21, 30
CROPS = {160: dict(image_h=64, image_w=640), 320: dict(image_h=64, image_w=1280), 512: dict(image_h=2048, image_w=64, dec_layers=2)}


@pytest.fixture(scope="module", params=list(CROPS))
def built(request):
    keys = request.param
    cfg = PK.geometry(**CROPS[keys])
    assert cfg.num_patches == keys
    px, lab = PK.batch(cfg, 3, 1, LH, seed=24)
    sd, px16, info = PK.peaked(cfg, SEED, px, lab)
    print(f"\n{keys} keys, {cfg.dec_layers} layers: " + PK.describe(info))
    return keys, cfg, px, lab, sd, px16, info


def test_peaked_reaches_both_conditions(built):
    keys, cfg, px, lab, sd, px16, info = built
    assert info["peak_self"] > PK.PEAK and info["peak_cross"] > PK.PEAK
    assert min(info["sens_self"], info["sens_cross"]) >= PK.RATIO * info["err_ref"]
    assert 1 < info["factor_self"] <= 2 ** PK.ROUNDS and 1 < info["factor_cross"] <= 2 ** PK.ROUNDS
    assert info["ratio"] == min(info["sens_self"], info["sens_cross"]) / info["err_ref"]


def test_the_recipe_model_reaches_neither(built):
    keys, cfg, px, lab, *_ = built
    sd = {k: PK.bf16_exact(v) for k, v in P.state_dict_from_flat(cfg, P.recipe_flat(cfg, SEED)).items()}
    info = PK.conditions(cfg, sd, PK.bf16_exact(px), lab, check=False)
    print(f"\n{keys} keys, recipe weights: " + PK.describe(info))
    assert info["peak_cross"] < 2.0 / keys and info["peak_self"] < PK.PEAK
    assert info["sens_cross"] < 1e-3
    assert min(info["sens_self"], info["sens_cross"]) < PK.RATIO * info["err_ref"]
    with pytest.raises(AssertionError):
        PK.conditions(cfg, sd, PK.bf16_exact(px), lab)


def test_returned_tensors_are_bf16_exact(built):
    keys, cfg, px, lab, sd, px16, info = built
    recipe = P.state_dict_from_flat(cfg, P.recipe_flat(cfg, SEED))
    assert set(sd) == set(recipe)
    for k, v in sd.items():
        assert v.dtype == np.float32 and v.shape == recipe[k].shape, k
        assert np.array_equal(v, PK.bf16_exact(v)), k
    assert px16.dtype == np.float32 and np.array_equal(px16, PK.bf16_exact(px16))
    assert np.array_equal(px16, PK.bf16_exact(px))
    # what was scaled and by how much; everything else is the recipe's tensor, rounded
    q, v = "decoder.roberta.encoder.layer.0.{}.self.query.weight", "decoder.roberta.encoder.layer.0.{}.self.value.bias"
    for block, factor in (("attention", info["factor_self"]), ("crossattention", info["factor_cross"])):
        assert np.array_equal(sd[q.format(block)], PK.bf16_exact(recipe[q.format(block)]) * np.float32(factor))
        assert np.array_equal(sd[v.format(block)], PK.bf16_exact(recipe[v.format(block)]) * np.float32(PK.VALUE_GAIN))
    k = "decoder.roberta.encoder.layer.0.attention.self.key.weight"
    assert np.array_equal(sd[k], PK.bf16_exact(recipe[k]))


def test_stepwise_logits_equal_the_teacher_forced_column(built):
    keys, cfg, px, lab, sd, px16, info = built
    sd64, enc64 = PK.encode(cfg, sd, px16, torch.float64)
    ids = torch.from_numpy(lab)
    whole = PK.decode(cfg, sd64, ids[:, :-1].contiguous(), enc64)
    step = O.stepwise_logits(cfg, sd64, torch.from_numpy(px16).double())
    live, _ = PK.live_rows(cfg, ids[:, :-1])
    worst = 0.0
    for t in (0, 1, 7, 8, 17, LH - 2):
        rows = live[:, t]
        if bool(rows.any()):
            worst = max(worst, float((step(t, ids) - whole[:, t])[rows].abs().max()))
    print(f"\n{keys} keys: stepwise against teacher-forced, fp64: {worst:.2e}")
    assert worst <= 1e-9
