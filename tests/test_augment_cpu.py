"""Training-time augmentation without a GPU: the fp64 restatement the GPU tests use (tests/_augment_ref.py) is pinned, stage by
stage, to the torch statement include/kzv.h gives for it; the host sampler (kzv.augment.sample_params) is deterministic in its
arguments and returns exact identity parameters for every coin it loses; the CLI flags and the loader wrapper do their bookkeeping."""
import dataclasses

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _augment_ref as R
from kzv import augment as A
from kzv.config import tiny_config
from kzv.data import SyntheticLineDataset, make_loader

SHAPES = [(5, 3), (19, 37), (70, 9)]


def _image(H, W, seed=0):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (3, H, W))


def _m32(*a, **kw):
    return A.inverse_affine(*a, **kw).astype(np.float32)


@pytest.mark.parametrize("H,W", SHAPES)
def test_restated_warp_equals_grid_sample(H, W):
    x = _image(H, W)
    for m in (_m32(30.0, (0, 0), 1.0, (0, 0), H, W), _m32(0.0, (2, -1), 0.5, (0, 0), H, W), _m32(-7.0, (1, 3), 1.07, (10.0, -5.0), H, W),
              np.array([1, 0, -(W + 5), 0, 1, 0], np.float32), np.array(A.IDENTITY_M, np.float32)):
        sx, sy = R.source_coords(m, H, W)
        grid = torch.from_numpy(np.stack([(2 * sx + 1) / W - 1, (2 * sy + 1) / H - 1], -1))[None]
        want = F.grid_sample(torch.from_numpy(x)[None] - 1, grid, "bilinear", "zeros", align_corners=False)[0] + 1
        assert np.abs(R.warp(x, m) - want.numpy()).max() < 1e-12
    assert np.array_equal(R.warp(x, np.array(A.IDENTITY_M, np.float32)), x)


@pytest.mark.parametrize("H,W", SHAPES)
def test_restated_morphology_equals_pooling(H, W):
    x = _image(H, W, 1)
    t = torch.from_numpy(x)[None]
    assert np.array_equal(R.morph(x, 1), F.max_pool2d(t, 3, 1, 1)[0].numpy())
    assert np.array_equal(R.morph(x, 2), (-F.max_pool2d(-t, 3, 1, 1))[0].numpy())
    assert R.morph(x, 0) is x


@pytest.mark.parametrize("H,W", SHAPES)
def test_restated_blur_equals_conv_on_replicate_padding(H, W):
    x = _image(H, W, 2)
    w = A.blur_weights(1.5).astype(np.float32).astype(np.float64)
    t = torch.from_numpy(x)[:, None]                                    # channels as batch: one filter
    k = torch.from_numpy(w)
    h = F.conv2d(F.pad(t, (3, 3, 0, 0), mode="replicate"), k.view(1, 1, 1, 7))
    v = F.conv2d(F.pad(h, (0, 0, 3, 3), mode="replicate"), k.view(1, 1, 7, 1))
    assert np.abs(R.blur(x, w) - v[:, 0].numpy()).max() < 1e-12
    assert np.array_equal(R.blur(x, A.IDENTITY_BLUR), x)


def test_restated_noise_is_the_dropout_sites_hash():
    # kzv_hash32 by hand for two counters (csrc/kzv_common.h), and unit variance of g over a crop
    def h(x):
        x &= 0xffffffff
        x ^= x >> 16; x = (x * 0x7feb352d) & 0xffffffff
        x ^= x >> 15; x = (x * 0x846ca68b) & 0xffffffff
        return x ^ (x >> 16)
    key = 0xC0FFEE11
    got = R.noise_sums(key, 4, 5)
    for e in (0, 37):
        v = h(e * 0x9E3779B9 + key)
        assert got.reshape(-1)[e] == sum((v >> s) & 0xff for s in (0, 8, 16, 24))
    g = R.noise_g(key, 64, 640)
    assert abs(g.mean()) < 5 / np.sqrt(g.size) and abs(g.var() - 1.0) < 0.03


def test_sample_params_is_a_function_of_its_arguments():
    cfg = A.preset("reference")
    base = dict(n=16, H=64, W=640, seed=7, rank=0, epoch=0, step=0)
    a, b = A.sample_params(cfg, **base), A.sample_params(cfg, **base)
    assert a.dtype == A.PARAMS_DTYPE and a.dtype.itemsize == 72 and a.shape == (16,)
    assert a.tobytes() == b.tobytes()
    for key in ("rank", "epoch", "step", "seed"):
        other = A.sample_params(cfg, **dict(base, **{key: base[key] + 1}))
        assert other.tobytes() != a.tobytes(), key
    # the reference preset moves something in a batch of 16, and its weights are weights
    assert a.tobytes() != A.identity_params(16).tobytes()
    assert np.all(np.abs(a["blur"].astype(np.float64).sum(1) - 1.0) < 1e-7)
    assert set(np.unique(a["morph"])) <= {0, 1, 2}


def test_no_two_seeds_ranks_epochs_or_steps_share_a_variate():
    """Philox advances its counter from the low word, one per four outputs: an argument placed there would make neighbouring epochs
    overlapping windows of ONE stream (epoch e + 4 = epoch e slid by one crop).  Every (seed, rank, epoch, step) must own its stream:
    the [n, 16] uniforms and the noise keys of any two of them share no value, and no parameter record recurs."""
    n, base = 64, dict(seed=7, rank=0, epoch=0, step=3)
    u0, k0 = A.draw_variates(n, **base)
    assert u0.shape == (n, 16) and len(np.unique(u0)) == u0.size
    cfg = A.preset("reference")
    p0 = A.sample_params(cfg, n, 64, 640, **base)
    ident = np.array(A.IDENTITY_M, np.float32).tobytes()
    rec0 = {p0["m"][i].tobytes() for i in range(n)} - {ident}            # the continuous part of a record: the drawn matrices
    assert len(rec0) > n // 4
    for key in ("epoch", "step", "rank", "seed"):
        for k in list(range(1, 18)) + [64, 1 << 20, 1 << 40]:
            other = dict(base, **{key: base[key] + k})
            u, keys = A.draw_variates(n, **other)
            assert not np.intersect1d(u0, u).size, (key, k)
            assert np.intersect1d(k0, keys).size <= 1, (key, k)          # 64 x 64 pairs of 32-bit keys: a chance hit is 1e-6
            p = A.sample_params(cfg, n, 64, 640, **other)
            assert not rec0 & {p["m"][i].tobytes() for i in range(n)}, (key, k)
    # the stream is a function of the arguments, and a longer batch continues a shorter one (same stream, more of it)
    assert np.array_equal(A.draw_variates(n, **base)[0], u0) and np.array_equal(A.draw_variates(8, **base)[0], u0[:8])


def test_lost_coins_give_exact_identity_parameters():
    cfg = dataclasses.replace(A.preset("reference"), p_affine=0.0, p_thin=0.0, p_thick=0.0, p_blur=0.0, p_photometric=0.0, p_noise=0.0)
    assert not cfg.enabled and not A.preset("off").enabled and A.preset("reference").enabled
    p = A.sample_params(cfg, 8, 32, 64, seed=3, rank=1, epoch=2, step=5)
    assert p.tobytes() == A.identity_params(8).tobytes()
    one = A.identity_params(1)[0]
    assert tuple(one["m"]) == A.IDENTITY_M and tuple(one["blur"]) == A.IDENTITY_BLUR
    assert one["contrast"] == 1 and one["brightness"] == 0 and one["noise_sigma"] == 0 and one["morph"] == 0


def test_integer_translations_alone_are_exactly_that_shift():
    for H, W in ((64, 640), (1024, 64), (5, 3), (19, 37)):
        for tx, ty in ((3, -2), (0, 0), (-W - 4, 1)):
            m = _m32(0.0, (tx, ty), 1.0, (0.0, 0.0), H, W)
            assert np.array_equal(m, np.array([1, 0, -tx, 0, 1, -ty], np.float32)), (H, W, tx, ty, m)
    # through the sampler: degrees 0, unit scale, no shear -> whole-pixel shifts within the translate range
    cfg = A.AugmentConfig(translate=(0.07, 0.07), p_affine=1.0)
    p = A.sample_params(cfg, 32, 64, 640, seed=11)
    m = p["m"]
    assert np.all(m[:, [0, 4]] == 1) and np.all(m[:, [1, 3]] == 0)
    assert np.all(m[:, [2, 5]] == np.round(m[:, [2, 5]])) and np.abs(m[:, 2]).max() <= 45 and np.abs(m[:, 5]).max() <= 4
    assert len(np.unique(m[:, 2])) > 4


def test_blur_weights_sum_to_one():
    for s in (0.3, 0.5, 1.0, 1.5):
        w = A.blur_weights(s)
        assert abs(w.sum() - 1.0) < 1e-15 and np.all(w == w[::-1])
        assert abs(w.astype(np.float32).astype(np.float64).sum() - 1.0) < 1e-7


# ---- CLI and loader plumbing -------------------------------------------------------------------------------------------------
def test_cli_flags_parse():
    from kzv.train import parse_args
    a = parse_args([])
    assert a.augment == "off" and a.augment_seed is None
    a = parse_args(["--augment", "reference", "--augment_seed", "9"])
    assert a.augment == "reference" and a.augment_seed == 9
    with pytest.raises(SystemExit):
        parse_args(["--augment", "heavy"])
    with pytest.raises(ValueError):
        A.preset("heavy")


def test_ocr_model_refuses_augmentation(capsys):
    from kzv.train import main
    with pytest.raises(SystemExit) as e:
        main(["--model", "ocr", "--augment", "reference", "--train_data_dir", "x", "--val_data_dir", "y"])
    assert "--augment" in str(e.value) and "ocr" in str(e.value)


class _StubAugment:
    """stands in for DeviceAugment on the CPU: marks what it was given"""
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def __call__(self, px, params, out=None):
        self.calls.append(params)
        return px + 1000.0


def test_make_loader_wraps_training_loaders_only():
    ds = SyntheticLineDataset(tiny_config(), 8, 12, seed=3)
    stub = _StubAugment()
    ref, off = A.preset("reference"), A.preset("off")
    assert not isinstance(make_loader(ds, 4, True, seed=1), A.AugmentLoader)
    assert not isinstance(make_loader(ds, 4, True, seed=1, augment=None), A.AugmentLoader)
    assert not isinstance(make_loader(ds, 4, True, seed=1, augment=(stub, off, 1)), A.AugmentLoader)       # off builds no wrapper
    assert not isinstance(make_loader(ds, 4, False, seed=1), A.AugmentLoader)                              # validation / test
    assert isinstance(make_loader(ds, 4, True, seed=1, augment=(stub, ref, 1)), A.AugmentLoader)
    # augment= on a loader that is not a training loader is an error, not a silent no-op; train= overrides the guess from shuffle
    with pytest.raises(ValueError, match="training loaders"):
        make_loader(ds, 4, False, seed=1, augment=(stub, ref, 1))
    with pytest.raises(ValueError, match="train=False"):
        make_loader(ds, 4, True, seed=1, augment=(stub, ref, 1), train=False)
    unshuffled = make_loader(ds, 4, False, seed=1, augment=(stub, ref, 1), train=True)                     # an overfit / debug run
    assert isinstance(unshuffled, A.AugmentLoader) and len(unshuffled) == 2
    bucketed = SyntheticLineDataset(tiny_config(), 8, 12, seed=3, width_buckets=(32, 64))
    assert isinstance(make_loader(bucketed, 4, True, seed=1, augment=(stub, ref, 1)), A.AugmentLoader)
    assert not stub.calls


class _StubLoader:
    def __init__(self):
        self.epochs = []

    def __len__(self):
        return 3

    def set_epoch(self, e):
        self.epochs.append(e)

    def __iter__(self):
        for i in range(3):
            yield {"pixel_values": torch.full((2, 3, 4, 6), float(i)), "labels": torch.tensor([[i, 7]]), "text": [f"t{i}"], "image_path": ["p"]}


def test_augment_loader_bookkeeping():
    stub, inner, cfg = _StubAugment(), _StubLoader(), A.preset("reference")
    ld = A.AugmentLoader(inner, stub, cfg, seed=5, rank=2)
    assert len(ld) == 3
    for epoch in (0, 4):
        ld.set_epoch(epoch)
        stub.calls.clear()
        got = list(ld)
        assert ld.epoch == epoch and ld.step == 3 and inner.epochs[-1] == epoch
        for i, b in enumerate(got):
            assert set(b) == {"pixel_values", "labels", "text", "image_path"}
            assert torch.equal(b["pixel_values"], torch.full((2, 3, 4, 6), float(i)) + 1000.0)
            assert torch.equal(b["labels"], torch.tensor([[i, 7]])) and b["text"] == [f"t{i}"]
            want = A.sample_params(cfg, 2, 4, 6, seed=5, rank=2, epoch=epoch, step=i)
            assert stub.calls[i].tobytes() == want.tobytes()
    # a second pass over the same epoch repeats the draws
    first = [c.tobytes() for c in stub.calls]
    stub.calls.clear()
    list(ld)
    assert [c.tobytes() for c in stub.calls] == first


def test_launches_too_large_for_one_grid_are_refused_before_any_launch():
    """a tile is 256 threads and a launch carries fewer than 2^32 of them: 2^24 tiles or more is KZV_E_ARG with a message, before the
    pointers are looked at twice (none is dereferenced on the host; nothing is launched)"""
    from kzv import _lib as L
    lib = L.load()
    n = (1 << 24) // 3 + 1                          # 1x1 crops: one tile per channel
    assert lib.kzv_augment_lines(1 << 20, 1 << 12, n, 1, 1, 1 << 40, None) == -1
    assert b"2^32" in lib.kzv_last_error() and b"tiles" in lib.kzv_last_error()
    assert lib.kzv_augment_lines(1 << 20, 1 << 12, 1, 65536, 65536, 1 << 40, None) == -1
    assert b"3*H*W" in lib.kzv_last_error()
