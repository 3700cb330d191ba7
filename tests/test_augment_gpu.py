"""kzv_augment_lines (csrc/augment.hip) on the GPU: exact where the contract says exact, and against the fp64 restatement
(tests/_augment_ref.py, fed the same fp32 parameters) elsewhere.

Shapes are the smallest at which the kernel can still go wrong: a canvas smaller than the halo, canvases ragged in both directions
and narrower than a tile, the benchmark's 64x640 (2 x 10 tiles) and the reference CLI's tall 1024x64 column (32 tiles down).

The tolerance against fp64 is derived, not fitted:

    atol = 1e-5 + 12 * contrast * spacing_fp32(max(H, W))

The only device-versus-double difference that matters is the rounding of the source coordinates sx and sy: the device evaluates
m0*x + m1*y + m2 in fp32, at most three roundings at a magnitude of up to max(H, W) (beyond [-1, W] / [-1, H] the coordinate is
clamped and every tap is fill), each at most one spacing of fp32 there.  The pixels lie in [-1, 1], so the bilinear interpolant
(fill included: it is continuous in sx and sy, across pixel boundaries and across the clamp) has slope at most 2 per pixel in
each of the two directions: 3 roundings * slope 2 * 2 directions = 12 spacings.  The 3x3 maximum / minimum and the blur
(non-negative weights summing to 1) are non-expansive, `contrast` scales what reaches it, the clamp to [-1, 1] is non-expansive
again.  Everything else (fp32 interpolation, seven fp32 products, the noise scale) is of order 1e-6.
If the kernel misses this bound, the kernel is wrong."""
import numpy as np
import pytest
import torch

import _augment_ref as R
from kzv import _lib as L
from kzv import augment as A

pytestmark = pytest.mark.gpu

SHAPES = [(3, 5, 3), (2, 19, 37), (2, 70, 9), (2, 64, 640), (1, 1024, 64)]
IDS = [f"{n}x{h}x{w}" for n, h, w in SHAPES]


@pytest.fixture(scope="module")
def aug():
    return A.DeviceAugment("cuda:0")


@pytest.fixture(scope="module", params=SHAPES, ids=IDS)
def batch(request):
    n, H, W = request.param
    x = np.random.default_rng(1000 + H * W).uniform(-1.0, 1.0, (n, 3, H, W)).astype(np.float32)
    x.setflags(write=False)
    return x, torch.from_numpy(x.copy()).cuda()


def _params(n, **fields):
    p = A.identity_params(n)
    for k, v in fields.items():
        p[k] = v
    return p


def test_identity_parameters_return_the_input_bit_for_bit(aug, batch):
    x, d = batch
    out = aug(d, A.identity_params(len(x)))
    assert out.data_ptr() != d.data_ptr()
    assert torch.equal(out, d)
    assert torch.equal(d.cpu(), torch.from_numpy(x.copy()))          # a pure function: the input is untouched


@pytest.mark.parametrize("dx,dy", [(1, 0), (0, -1), (2, 3), (-3, 2), (10**6, 0), (0, -(10**6))])
def test_integer_translations_are_exact_shifts_with_white_fill(aug, batch, dx, dy):
    x, d = batch
    n, _, H, W = x.shape
    shifts = [(dx, dy), (W + 5, 0), (0, -H)][:n]                      # the second and third: just beyond the canvas, all fill
    p = A.identity_params(n)
    want = np.ones_like(x)
    for i, (sx, sy) in enumerate(shifts):
        p["m"][i] = (1, 0, -sx, 0, 1, -sy)
        ys, xs = np.arange(H) - sy, np.arange(W) - sx                 # out[y, x] = in[y - sy, x - sx]
        oky, okx = np.nonzero((ys >= 0) & (ys < H))[0], np.nonzero((xs >= 0) & (xs < W))[0]
        want[i][np.ix_(np.arange(3), oky, okx)] = x[i][np.ix_(np.arange(3), ys[oky], xs[okx])]
    assert torch.equal(aug(d, p).cpu(), torch.from_numpy(want))


def test_noise_is_the_counter_hash_exactly(aug, batch):
    x, d = batch
    n, _, H, W = x.shape
    keys = [0xC0FFEE11, 7, 0xFFFFFFFF][:n]
    p = _params(n, noise_sigma=0.25)
    p["noise_key"] = keys
    out = aug(torch.zeros_like(d), p).cpu().double().numpy()
    got = np.rint(out * 4 * 147.80).astype(np.int64) + 510
    for i, k in enumerate(keys):
        assert np.array_equal(got[i], R.noise_sums(k, H, W)), (i, k)


def test_noise_statistics(aug):
    z = torch.zeros(1, 3, 64, 640, device="cuda")
    p = _params(1, noise_sigma=0.25)
    p["noise_key"] = 0x5EED1234
    v = aug(z, p).double().cpu().numpy().reshape(-1)
    assert abs(v.mean() / 0.25) < 5 / np.sqrt(v.size)
    assert abs(v.var() / 0.25 ** 2 - 1.0) < 0.03


def test_out_overlapping_in_is_refused_and_launches_nothing(aug):
    d = torch.rand(2, 3, 19, 37, device="cuda") * 2 - 1
    keep = d.clone()
    p = _params(2, contrast=0.5)
    with pytest.raises(L.KzvError, match="overlaps"):
        aug(d, p, out=d)
    flat = torch.zeros(d.numel() + 64, device="cuda")
    src, dst = flat[:d.numel()].view_as(d), flat[64:].view_as(d)     # partial overlap
    src.copy_(keep)
    with pytest.raises(L.KzvError, match="overlaps"):
        aug(src, p, out=dst)
    torch.cuda.synchronize()
    assert torch.equal(d, keep) and torch.equal(src, keep)
    lib = L.load()
    assert lib.kzv_augment_lines(d.data_ptr(), 0, 2, 19, 37, flat.data_ptr(), 0) == -1              # null params
    assert lib.kzv_augment_lines(d.data_ptr(), flat.data_ptr(), 2, 0, 37, flat.data_ptr(), 0) == -1  # H < 1


def _cases(H, W):
    ident = np.array(A.IDENTITY_M)
    rot = A.inverse_affine(30.0, (0, 0), 1.0, (0.0, 0.0), H, W)       # gathers leave the canvas on every side
    half = A.inverse_affine(0.0, (0, 0), 0.5, (0.0, 0.0), H, W)
    shear = A.inverse_affine(0.0, (0, 0), 1.0, (10.0, 0.0), H, W)
    everything = A.inverse_affine(-7.0, (2, -1), 0.93, (5.0, -5.0), H, W)
    b03, b15 = A.blur_weights(0.3), A.blur_weights(1.5)
    return {
        "rotate30": dict(m=rot), "scale0.5": dict(m=half), "shear10": dict(m=shear),
        "thin": dict(m=ident, morph=1), "thick": dict(m=ident, morph=2),
        "blur0.3": dict(m=ident, blur=b03), "blur1.5": dict(m=ident, blur=b15),
        "photometric": dict(m=ident, contrast=1.3, brightness=-0.2),
        "noise": dict(m=ident, noise_sigma=0.05, noise_key=12345),
        # the kernel's stage skips in the combinations the cases above do not reach
        "rotate_noise": dict(m=rot, noise_sigma=0.05, noise_key=777), "shift_blur": dict(m=np.array([1, 0, -2, 0, 1, 3.0]), blur=b15),
        "shift_thick_photometric": dict(m=np.array([1, 0, 1, 0, 1, -1.0]), morph=2, contrast=1.3, brightness=-0.2),
        "all_thin": dict(m=everything, morph=1, blur=b15, contrast=1.3, brightness=-0.2, noise_sigma=0.05, noise_key=99),
        "all_thick": dict(m=rot, morph=2, blur=b03, contrast=1.3, brightness=-0.2, noise_sigma=0.03, noise_key=3),
    }


def test_each_operation_and_all_together_against_fp64(aug, batch):
    x, d = batch
    n, _, H, W = x.shape
    spacing = float(np.spacing(np.float32(max(H, W))))
    worst = {}
    for name, f in _cases(H, W).items():
        p = _params(n, **f)                                          # rounded once to fp32, here; the reference reads the same records
        got = aug(d, p).cpu().double().numpy()
        want = R.augment(x, p)
        err = float(np.abs(got - want).max())
        atol = 1e-5 + 12 * float(p["contrast"][0]) * spacing
        worst[name] = (err, atol)
        print(f"augment {n}x3x{H}x{W} {name}: max|err| {err:.3g} (atol {atol:.3g})")
    bad = {k: v for k, v in worst.items() if not v[0] <= v[1]}
    assert not bad, bad


def test_mixed_batch_each_crop_takes_its_own_parameters(aug):
    """one launch, a different operation per crop (the block-uniform stage skips must follow the crop, not the launch)"""
    n, H, W = 6, 40, 100
    x = np.random.default_rng(5).uniform(-1, 1, (n, 3, H, W)).astype(np.float32)
    c = _cases(H, W)
    p = A.identity_params(n)
    for i, name in enumerate(("rotate30", "thin", "blur1.5", "photometric", "all_thin")):
        for k, v in c[name].items():
            p[k][i] = v
    got = aug(torch.from_numpy(x).cuda(), p).cpu().double().numpy()
    want = R.augment(x, p)
    assert np.abs(got - want).max() <= 1e-5 + 12 * 1.3 * float(np.spacing(np.float32(W)))
    assert np.array_equal(got[5], x[5].astype(np.float64))


# ---- the training CLI ----------------------------------------------------------------------------------------------------------
def test_train_cli_augments_training_batches_only(tmp_path, monkeypatch, capsys):
    """kzv.train.main(["--synthetic", "64", "--augment", "reference", "--max_steps", "4", ...]) on the tiny encoder, IN this process, so
    that the loaders it built can be read afterwards: it returns (no SystemExit), the loss is finite, training batches differ from the
    un-augmented ones and repeat for the same seed, validation and test batches are the un-augmented ones.  This calls `main`, not the
    module's `__main__` entry: the exit status of `python -m kzv.train` itself is test_python_m_kzv_train_exits_zero's subject."""
    from kzv import data as D
    from kzv.train import main
    made = []
    real = D.make_loader

    def spy(dataset, batch_size, shuffle, *a, **kw):
        ld = real(dataset, batch_size, shuffle, *a, **kw)
        made.append((dataset, batch_size, shuffle, ld))
        return ld
    monkeypatch.setattr(D, "make_loader", spy)
    hist = main(["--synthetic", "64", "--augment", "reference", "--max_steps", "4", "--batch_size", "8", "--image_size", "32", "64",
                 "--encoder_hidden_size", "128", "--encoder_num_layers", "2", "--encoder_num_heads", "2", "--max_length", "16", "--max_epochs", "1",
                 "--skip_test", "--output_dir", str(tmp_path), "--experiment_name", "aug"])
    assert hist and all(np.isfinite(v) for _, v in hist)
    assert "augmentation: reference" in capsys.readouterr().out
    assert [s for _, _, s, _ in made] == [True, False, False]
    (tds, bs, _, train), (vds, _, _, val), (sds, _, _, test) = made
    assert isinstance(train, A.AugmentLoader) and not isinstance(val, A.AugmentLoader) and not isinstance(test, A.AugmentLoader)

    def batches(ld, epoch=0):
        ld.set_epoch(epoch)
        return [b for b in ld]
    plain = batches(real(tds, bs, True, 42, 0, 1))
    first, second = batches(train), batches(train)
    again = batches(real(tds, bs, True, 42, 0, 1, augment=(A.DeviceAugment("cuda:0"), A.preset("reference"), 42)))
    other = batches(real(tds, bs, True, 42, 0, 1, augment=(A.DeviceAugment("cuda:0"), A.preset("reference"), 43)))
    assert len(plain) == len(first) == 8
    for a, b, c, e, f in zip(plain, first, second, again, other):
        assert b["pixel_values"].is_cuda and b["pixel_values"].shape == a["pixel_values"].shape
        assert torch.equal(a["labels"], b["labels"]) and a["text"] == b["text"]
        assert not torch.equal(b["pixel_values"].cpu(), a["pixel_values"])
        assert torch.equal(b["pixel_values"], c["pixel_values"]) and torch.equal(b["pixel_values"], e["pixel_values"])
        assert not torch.equal(b["pixel_values"], f["pixel_values"])
    assert not torch.equal(batches(train, 1)[0]["pixel_values"], first[0]["pixel_values"])       # a new epoch, new draws (and a new order)
    for ds, ld in ((vds, val), (sds, test)):
        for a, b in zip(batches(real(ds, bs, False, 42, 0, 1)), batches(ld)):
            assert torch.equal(a["pixel_values"], b["pixel_values"]) and torch.equal(a["labels"], b["labels"])


def test_python_m_kzv_train_exits_zero(tmp_path):
    """the command the users type, as a process of its own: `python -m kzv.train --synthetic 64 --augment reference --max_steps 4` exits
    with status 0, says which preset it runs, and every loss it prints is finite"""
    import os
    import re
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([root, os.path.join(root, "kuzushiji-vision_amd")]))
    cmd = [sys.executable, "-m", "kzv.train", "--synthetic", "64", "--augment", "reference", "--max_steps", "4", "--batch_size", "8", "--image_size", "32", "64",
           "--encoder_hidden_size", "128", "--encoder_num_layers", "2", "--encoder_num_heads", "2", "--max_length", "16", "--max_epochs", "1",
           "--skip_test", "--num_workers", "0", "--output_dir", str(tmp_path / "out")]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "augmentation: reference (seed 42, training batches only)" in out, out[-4000:]
    losses = [float(v) for v in re.findall(r"(?:train|val)_loss (\S+)", out)]
    assert losses and all(np.isfinite(v) for v in losses), out[-4000:]


def test_off_builds_no_wrapper_and_launches_nothing(tmp_path, monkeypatch):
    from kzv import data as D
    from kzv.train import main
    made = []
    real = D.make_loader
    monkeypatch.setattr(D, "make_loader", lambda *a, **kw: made.append((real(*a, **kw), kw)) or made[-1][0])
    monkeypatch.setattr(A.DeviceAugment, "__call__", lambda *a, **kw: pytest.fail("augmentation ran with --augment off"))
    hist = main(["--synthetic", "16", "--max_steps", "2", "--batch_size", "8", "--image_size", "32", "64", "--encoder_hidden_size", "128",
                 "--encoder_num_layers", "2", "--encoder_num_heads", "2", "--max_length", "16", "--max_epochs", "1", "--skip_test",
                 "--output_dir", str(tmp_path), "--experiment_name", "off"])
    assert hist and all(np.isfinite(v) for _, v in hist)
    assert all(kw.get("augment") is None and not isinstance(ld, A.AugmentLoader) for ld, kw in made)
