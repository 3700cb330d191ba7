"""Class weights and the focal term of the training loss, the parts that need no GPU: kzv.classweights (counts -> weights), the four
flags of python -m kzv.train, and the ctypes bindings of the six new symbols (include/kzv.h)."""
import ctypes as C

import numpy as np
import pytest

from kzv import _lib as L
from kzv import classweights as CW
from kzv.train import parse_args

COUNTS = np.array([0, 100000, 1, 7, 0, 250, 3, 90000, 12, 4000, 2, 1], dtype=np.int64)      # a long tail, two classes never seen


# ================================================================================================ from_counts / count_targets
def _closed_form(counts, raw, cap):
    lo = raw.min()
    w = np.clip(raw, lo, lo * cap)
    return w * (counts.sum() / (counts * w).sum())


@pytest.mark.parametrize("power,cap", [(0.5, 10.0), (1.0, 10.0), (0.5, 1e9), (0.5, 1.0)])
def test_inv_pow_is_the_closed_form(power, cap):
    n = np.maximum(COUNTS, 1).astype(np.float64)
    want = _closed_form(COUNTS, n ** -power, cap)
    got = CW.from_counts(COUNTS, "inv_pow", power=power, cap=cap)
    assert got.dtype == np.float32 and got.shape == COUNTS.shape
    np.testing.assert_allclose(got, want, rtol=1e-6)
    assert got.max() / got.min() <= cap * (1 + 1e-6)
    assert abs(float((COUNTS * got.astype(np.float64)).sum()) / COUNTS.sum() - 1.0) < 1e-6
    assert got[0] == got[4] == got[2] == got[11]                 # a class never seen weighs like one seen once
    if cap == 1.0:
        np.testing.assert_allclose(got, 1.0, rtol=1e-6)


@pytest.mark.parametrize("beta,cap", [(0.999, 10.0), (0.9, 10.0), (0.9999, 3.0)])
def test_effective_is_the_closed_form(beta, cap):
    n = np.maximum(COUNTS, 1).astype(np.float64)
    want = _closed_form(COUNTS, (1 - beta) / (1 - beta ** n), cap)
    got = CW.from_counts(COUNTS, "effective", beta=beta, cap=cap)
    assert got.dtype == np.float32
    np.testing.assert_allclose(got, want, rtol=1e-6)
    assert got.max() / got.min() <= cap * (1 + 1e-6)
    assert abs(float((COUNTS * got.astype(np.float64)).sum()) / COUNTS.sum() - 1.0) < 1e-6
    assert got[0] == got[4] == got[2]


def test_the_cap_binds_where_the_raw_spread_is_wider():
    w = CW.from_counts(COUNTS, "inv_pow", power=0.5, cap=10.0)           # raw spread sqrt(100000) = 316
    assert abs(w.max() / w.min() - 10.0) < 1e-5
    assert (w == w.max()).sum() >= 5 and (w == w.min()).sum() == 1


@pytest.mark.parametrize("kw", [{"scheme": "nope"}, {"cap": 0.5}, {"scheme": "effective", "beta": 1.0}, {"power": -1.0}])
def test_from_counts_refuses(kw):
    with pytest.raises(ValueError):
        CW.from_counts(COUNTS, **kw)


def test_count_targets_counts_what_the_loss_scores():
    pad, bos, eos = 1, 0, 2
    rows = [[bos, 5, 6, 5, eos, pad, pad], np.array([bos, 7, eos, pad, pad, pad, pad]), [5, 9]]      # padded or not; the first id is never a target
    c = CW.count_targets(rows, 12, pad)
    assert c.dtype == np.int64 and c.shape == (12,)
    want = np.zeros(12, dtype=np.int64)
    want[5], want[6], want[7], want[9], want[eos] = 2, 1, 1, 1, 2
    assert (c == want).all() and c[bos] == 0 and c[pad] == 0
    lab = np.array([[0, 5, 6, 2, 1, 1], [0, 2, 1, 1, 1, 1]])
    assert int(CW.count_targets(lab, 12, pad).sum()) == int((lab[:, 1:] != pad).sum())


# ================================================================================================ flags
def test_flag_defaults_and_values(tmp_path):
    a = parse_args([])
    assert a.class_weights == "none" and a.class_weight_beta == 0.999 and a.class_weight_cap == 10.0 and a.focal_gamma == 0.0
    a = parse_args(["--class_weights", "inv_sqrt", "--class_weight_cap", "4", "--focal_gamma", "2"])
    assert a.class_weights == "inv_sqrt" and a.class_weight_cap == 4.0 and a.focal_gamma == 2.0
    a = parse_args(["--class_weights", "effective", "--class_weight_beta", "0.99"])
    assert a.class_weights == "effective" and a.class_weight_beta == 0.99
    path = str(tmp_path / "w.npy")
    assert parse_args(["--class_weights", path]).class_weights == path
    assert parse_args(["--label_smoothing", "0.1", "--class_weights", "inv_sqrt"]).label_smoothing == 0.1      # weights and smoothing combine
    assert parse_args(["--model", "ocr"]).focal_gamma == 0.0


@pytest.mark.parametrize("argv,word", [
    (["--class_weights", "inv_sqrt", "--model", "ocr"], "--class_weights"),
    (["--class_weight_beta", "0.99", "--model", "ocr"], "--class_weight_beta"),
    (["--class_weight_cap", "3", "--model", "ocr"], "--class_weight_cap"),
    (["--focal_gamma", "1", "--model", "ocr"], "--focal_gamma"),
    (["--focal_gamma", "2", "--label_smoothing", "0.1"], "--focal_gamma"),
    (["--focal_gamma", "-0.1"], "--focal_gamma"),
    (["--focal_gamma", "5.1"], "--focal_gamma"),
    (["--focal_gamma", "nan"], "--focal_gamma"),
    (["--class_weights", "sqrt"], "--class_weights"),
    (["--class_weight_beta", "1.0"], "--class_weight_beta"),
    (["--class_weight_cap", "0.5"], "--class_weight_cap"),
])
def test_flag_refusals(argv, word, capsys):
    with pytest.raises(SystemExit) as e:
        parse_args(argv)
    assert e.value.code == 2                                   # argparse's error exit
    assert word in capsys.readouterr().err


def test_help_says_what_train_loss_and_val_loss_are(capsys):
    with pytest.raises(SystemExit):
        parse_args(["--help"])
    out = " ".join(capsys.readouterr().out.split())      # (argparse may break a line behind the hyphen of cross-entropy: the phrases end before it)
    assert "--class_weights {none,inv_sqrt,effective,PATH.npy}" in out
    assert "train_loss in the logs is then the WEIGHTED loss, while val_loss and the test losses stay the plain" in out
    assert "train_loss in the logs is then the FOCAL loss, while val_loss and the test losses stay the plain" in out
    assert "--class_weight_beta" in out and "--class_weight_cap" in out and "--focal_gamma" in out


# ================================================================================================ bindings
def test_bindings_of_the_new_symbols():
    assert L.SYMBOLS["kzv_set_class_weights"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int])
    assert L.SYMBOLS["kzv_get_class_weights"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int])
    assert L.SYMBOLS["kzv_set_focal_gamma"] == (C.c_int, [C.c_void_p, C.c_float])
    assert L.SYMBOLS["kzv_get_focal_gamma"] == (C.c_float, [C.c_void_p])
    res, args = L.SYMBOLS["kzv_ce_fwd_bwd_w"]
    ls = L.SYMBOLS["kzv_ce_fwd_bwd_ls"][1]
    assert res is C.c_int and args == ls[:-1] + [C.c_void_p, C.c_float] + ls[-1:]      # kzv_ce_fwd_bwd_ls's list, weights and gamma before the stream
    res, args = L.SYMBOLS["kzv_target_weight_sum"]
    assert res is C.c_int and args == [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p] * 3
