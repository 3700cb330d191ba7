"""Fine-tuning, the parts that need no GPU: the float64 restatement of the grouped step against the oracle (and what licenses ONE ckp1
for all groups), kzv.finetune.build_groups, the accumulation schedule of kzv.trainer.Stepper, the CLI's checks."""
import numpy as np
import pytest

from kzv import finetune as FT
from kzv.optim import check_groups
from kzv.train import parse_args
from kzv.trainer import Stepper
from oracle import trocr_oracle as O

from _finetune_ref import GroupedRef


# ------------------------------------------------------------------------------------------------ the restatement
def test_one_group_is_the_oracle_step_exactly():
    n = 4096
    rng = np.random.default_rng(3)
    p0 = rng.standard_normal(n) * 0.02
    ref = GroupedRef(p0, [(0, n, 1.0, 1.0)], lr=1e-3, weight_decay=0.01)
    st = O.RAdamScheduleFreeState(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01)
    y = p0.copy(); z = y.copy(); v = np.zeros(n)
    for step in range(12):
        g = (rng.standard_normal(n) * 0.05).astype(np.float32)
        total, coef = ref.step(g, max_norm=1.0, grad_scale=0.5)
        gs = g.astype(np.float64) * 0.5
        t2, c2 = O.clip_grad_norm([gs], 1.0)
        O.radam_schedulefree_step(st, y, z, v, gs * c2)
        assert (total, coef) == (t2, c2)
        assert np.array_equal(ref.y, y) and np.array_equal(ref.z, z) and np.array_equal(ref.v, v)


def test_scaled_groups_share_ckp1_over_both_phases():
    """schedulefree keeps lr_max and weight_sum per group; a learning-rate scale that is constant in time multiplies the weight and every
    term of weight_sum by scale ** weight_lr_power and cancels in ckp1 = weight / weight_sum -- the kernel's single ckp1."""
    n = 64 * 6
    groups = [(0, 64, 0.0, 1.0), (64, 128, 0.5, 0.0), (128, 256, 0.75, 1.0), (256, 320, 0.0316, 1.0), (320, 384, 1.0, 1.0)]
    rng = np.random.default_rng(4)
    ref = GroupedRef(rng.standard_normal(n) * 0.02, groups, lr=1e-3, weight_decay=0.01)
    plain = O.RAdamScheduleFreeState(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01)
    phases = set()
    for step in range(12):
        ref.step((rng.standard_normal(n) * 0.01).astype(np.float32), max_norm=1.0)
        lr, ckp1, _, adaptive = plain.next_scalars()
        phases.add(bool(adaptive))
        assert len(ref.last_ckp1) == 4
        for c in ref.last_ckp1:
            assert c == pytest.approx(ckp1, rel=1e-12, abs=0.0), (step, c, ckp1)
    assert phases == {True, False}        # the silent and the adaptive phase


def test_frozen_slices_are_untouched_and_outside_the_norm():
    n = 256
    groups = [(0, 64, 0.0, 1.0), (64, 256, 1.0, 1.0)]
    rng = np.random.default_rng(5)
    p0 = rng.standard_normal(n) * 0.02
    ref = GroupedRef(p0, groups, lr=1e-3, weight_decay=0.01, ema_decay=0.9)
    g = np.concatenate([np.full(64, 100.0), rng.standard_normal(192) * 0.01]).astype(np.float32)
    for _ in range(8):
        total, _ = ref.step(g, max_norm=1.0)
    assert total < 1.0
    assert np.array_equal(ref.y[:64], p0[:64]) and np.array_equal(ref.z[:64], p0[:64]) and not ref.v[:64].any()
    assert np.array_equal(ref.ema[:64], p0[:64]) and not np.array_equal(ref.y[64:], p0[64:])


# ------------------------------------------------------------------------------------------------ build_groups
LE = 3


def _table(Le=LE, He=96, Hd=64):
    """A synthetic parameter table in the engine's order: every tensor starts on a multiple of 64 floats."""
    names = [("encoder.patch_embeddings.projection.weight", He * 48), ("encoder.patch_embeddings.projection.bias", He),
             ("encoder.cls_token", He), ("encoder.position_embeddings", 17 * He)]
    for i in range(Le):
        h = f"encoder.encoder.layer.{i}."
        names += [(h + "layernorm_before.weight", He), (h + "layernorm_before.bias", He),
                  (h + "attention.attention.query.weight", He * He), (h + "attention.attention.query.bias", He),
                  (h + "output.dense.weight", He * 4 * He), (h + "output.dense.bias", He)]
    names += [("encoder.layernorm.weight", He), ("encoder.layernorm.bias", He), ("encoder_decoder_proj.weight", Hd * He), ("encoder_decoder_proj.bias", Hd),
              ("decoder.roberta.embeddings.word_embeddings.weight", 70 * Hd), ("decoder.roberta.embeddings.LayerNorm.weight", Hd),
              ("decoder.roberta.encoder.layer.0.attention.self.query.weight", Hd * Hd), ("decoder.roberta.encoder.layer.0.attention.self.query.bias", Hd),
              ("decoder.lm_head.layer_norm.weight", Hd), ("decoder.lm_head.bias", 70)]
    table, off = [], 0
    for name, size in names:
        table.append((name, off, size))
        off += (size + 63) // 64 * 64
    return table, off


def _scale_of(groups, off):
    for lo, hi, ls, ws in groups:
        if lo <= off < hi:
            return ls, ws
    raise AssertionError(off)


def test_build_groups_defaults_are_one_plain_group():
    table, n = _table()
    assert FT.build_groups(table, LE) == [(0, n, 1.0, 1.0)]
    assert FT.build_groups(list(reversed(table)), LE) == [(0, n, 1.0, 1.0)]      # any order in


@pytest.mark.parametrize("decay,freeze,exempt", [(0.75, 0, "none"), (0.75, 1, "none"), (1.0, 2, "none"), (0.9, 3, "bias_norm"), (1.0, 0, "bias_norm"),
                                                 (0.65, 0, "bias_norm")])
def test_build_groups_cover_align_and_scale(decay, freeze, exempt):
    table, n = _table()
    groups = FT.build_groups(table, LE, layer_decay=decay, freeze_encoder_layers=freeze, decay_exempt=exempt)
    assert check_groups(groups, n) == groups                # sorted, contiguous, covers [0, n), multiples of 64
    for a, b in zip(groups, groups[1:]):
        assert a[2:] != b[2:]                               # merged
    for name, off, size in table:
        lid = FT.layer_id(name, LE)
        for at in (off, off + size - 1, (off + size + 63) // 64 * 64 - 1):       # first float, last float, last float of the padding
            ls, ws = _scale_of(groups, at)
            if freeze > 0 and lid <= freeze:
                assert ls == 0.0, name
            else:
                assert ls == decay ** (LE + 1 - lid) and ls > 0.0, name
            named = (name.endswith(".bias") or name in ("encoder.cls_token", "encoder.position_embeddings")
                     or name.endswith(("layernorm.weight", "layernorm_before.weight", "LayerNorm.weight", "layer_norm.weight")))
            assert ws == (0.0 if exempt == "bias_norm" and named else 1.0), name


def test_layer_ids_follow_beit():
    assert FT.layer_id("encoder.patch_embeddings.projection.weight", LE) == 0
    assert FT.layer_id("encoder.cls_token", LE) == 0 and FT.layer_id("encoder.position_embeddings", LE) == 0
    assert [FT.layer_id(f"encoder.encoder.layer.{i}.output.dense.bias", LE) for i in range(LE)] == [1, 2, 3]
    for name in ("encoder.layernorm.weight", "encoder_decoder_proj.bias", "decoder.roberta.encoder.layer.0.output.dense.weight", "decoder.lm_head.bias"):
        assert FT.layer_id(name, LE) == LE + 1
    assert FT.is_decay_exempt("decoder.roberta.embeddings.LayerNorm.weight") and FT.is_decay_exempt("encoder.encoder.layer.0.layernorm_after.weight")
    assert FT.is_decay_exempt("decoder.lm_head.layer_norm.weight") and not FT.is_decay_exempt("decoder.roberta.embeddings.position_embeddings.weight")
    assert not FT.is_decay_exempt("encoder.encoder.layer.0.output.dense.weight")


def test_build_groups_on_the_real_table():
    from kzv import params as P
    from kzv.config import tiny_config, vit_b_config
    for cfg in (tiny_config(), vit_b_config()):
        _, total = P.param_offsets(cfg)
        table = FT.model_param_table(cfg)
        Le = cfg.enc_layers
        assert FT.build_groups(table, Le) == [(0, total, 1.0, 1.0)]
        g = FT.build_groups(table, Le, layer_decay=0.75)
        assert len(g) == Le + 2 and check_groups(g, total) == g           # the embeddings, Le layers, the rest
        g = FT.build_groups(table, Le, layer_decay=0.75, freeze_encoder_layers=1, decay_exempt="bias_norm")
        assert check_groups(g, total) == g and g[0][2] == 0.0 and len(g) <= 4096
        offs, _ = P.param_offsets(cfg)
        cut = offs["enc.1.ln1.w"][0] if Le > 1 else offs["enc.lnf.w"][0]
        assert all((ls == 0.0) == (hi <= cut) for lo, hi, ls, ws in g)     # frozen exactly below the backward's cut


@pytest.mark.parametrize("bad", [dict(layer_decay=0.0), dict(layer_decay=1.5), dict(freeze_encoder_layers=-1), dict(freeze_encoder_layers=LE + 1),
                                 dict(decay_exempt="bias")])
def test_build_groups_refuses_bad_settings(bad):
    with pytest.raises(ValueError):
        FT.build_groups(_table()[0], LE, **bad)


@pytest.mark.parametrize("groups", [[], [(0, 64, 1.0, 1.0)], [(0, 32, 1.0, 1.0), (32, 128, 1.0, 1.0)], [(64, 128, 1.0, 1.0)],
                                    [(0, 64, 1.0, 1.0), (128, 192, 1.0, 1.0)], [(0, 128, -1.0, 1.0)], [(0, 128, float("nan"), 1.0)],
                                    [(64 * i, 64 * i + 64, 1.0, 1.0) for i in range(4097)]])
def test_check_groups_refuses(groups):
    with pytest.raises(ValueError):
        check_groups(groups, 128 if len(groups) < 4097 else 64 * 4097)


# ------------------------------------------------------------------------------------------------ the accumulation schedule
class _FakeStepper(Stepper):
    """Stepper.step with the four device operations replaced by records."""

    def __init__(self, k, world=1):
        self.world, self.dp_path, self.log = world, world > 1, []
        self._init_window(k)

    def _forward(self, batch):
        import torch
        self.log.append(("forward", batch))
        return torch.tensor([float(batch)])

    def _zero(self):
        self.log.append(("zero",))

    def _backward(self, sync):
        self.log.append(("backward", sync))

    def _opt_step(self, grad_scale):
        self.log.append(("step", grad_scale))


def test_accumulation_schedule_k3_over_7_batches():
    st = _FakeStepper(3)
    gstep, losses = 0, []
    for i in range(7):
        loss = st.step(i + 1, i, last_batch=i == 6)
        if st.stepped:
            gstep += 1
            losses.append(float(loss))
        else:
            assert loss is None
    assert gstep == 3
    assert losses == [2.0, 5.0, 7.0]                     # the mean of each window's micro-batch losses
    want = []
    for b in range(1, 8):
        want.append(("forward", b))
        if b in (1, 4, 7):
            want.append(("zero",))                       # once per window, before its first backward
        want.append(("backward", b in (3, 6, 7)))        # the all-reduce only in the window's last backward
        if b in (3, 6, 7):
            want.append(("step", 1.0 / 3.0))             # the short window too: Lightning divides every micro-batch loss by k
    assert st.log == want


def test_accumulation_scale_counts_the_ranks_and_k1_is_a_plain_step():
    st = _FakeStepper(2, world=4)
    st.step(1.0); st.step(3.0)
    assert st.log[-1] == ("step", 1.0 / 8.0) and [e for e in st.log if e[0] == "backward"] == [("backward", False), ("backward", True)]
    st = _FakeStepper(1)
    loss = st.step(5.0)
    assert st.stepped and float(loss) == 5.0 and st.log == [("forward", 5.0), ("zero",), ("backward", True), ("step", 1.0)]
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            _FakeStepper(bad)


# ------------------------------------------------------------------------------------------------ CLI, checkpoints
def test_cli_defaults_and_values():
    a = parse_args([])
    assert (a.init_from, a.resume, a.freeze_encoder_layers, a.layer_decay, a.decay_exempt, a.accumulate_grad_batches) == (None, None, 0, 1.0, "none", 1)
    a = parse_args(["--freeze_encoder_layers", "12", "--layer_decay", "0.75", "--decay_exempt", "bias_norm", "--accumulate_grad_batches", "4",
                    "--init_from", "x.ckpt"])
    assert (a.init_from, a.freeze_encoder_layers, a.layer_decay, a.decay_exempt, a.accumulate_grad_batches) == ("x.ckpt", 12, 0.75, "bias_norm", 4)
    assert parse_args(["--resume", "x.ckpt"]).resume == "x.ckpt"


@pytest.mark.parametrize("argv", [["--layer_decay", "0"], ["--layer_decay", "1.01"], ["--layer_decay", "-0.5"], ["--freeze_encoder_layers", "-1"],
                                  ["--freeze_encoder_layers", "13"], ["--encoder_num_layers", "4", "--freeze_encoder_layers", "5"],
                                  ["--decay_exempt", "bias"], ["--accumulate_grad_batches", "0"], ["--init_from", "a", "--resume", "b"]])
def test_cli_refuses_bad_ranges(argv, capsys):
    with pytest.raises(SystemExit) as e:
        parse_args(argv)
    assert e.value.code == 2
    assert argv[-2] in capsys.readouterr().err


@pytest.mark.parametrize("argv", [["--init_from", "a.ckpt"], ["--freeze_encoder_layers", "1"], ["--layer_decay", "0.9"], ["--decay_exempt", "bias_norm"],
                                  ["--accumulate_grad_batches", "2"]])
def test_cli_ocr_refuses_each_flag_with_a_reason(argv, capsys):
    with pytest.raises(SystemExit) as e:
        parse_args(["--model", "ocr"] + argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert argv[0] in err and "TrOCR model only" in err
    assert parse_args(["--model", "ocr", "--resume", "x.ckpt"]).resume == "x.ckpt"      # ocr's own resume stays


def test_checkpoint_without_the_keys_is_off():
    import types
    off = {"layer_decay": 1.0, "freeze_encoder_layers": 0, "decay_exempt": "none", "accumulate_grad_batches": 1}
    assert FT.settings_from_hparams(None) == off
    assert FT.settings_from_hparams({"learning_rate": 1e-4, "label_smoothing": 0.1}) == off
    assert FT.settings_from_hparams(types.SimpleNamespace(learning_rate=1e-4)) == off
    assert FT.is_default(**{k: v for k, v in off.items() if k != "accumulate_grad_batches"})
    hp = {"layer_decay": 0.75, "frozen_encoder_layers": 1, "decay_exempt": "bias_norm", "accumulate_grad_batches": 2}
    assert FT.settings_from_hparams(hp) == {"layer_decay": 0.75, "freeze_encoder_layers": 1, "decay_exempt": "bias_norm", "accumulate_grad_batches": 2}
