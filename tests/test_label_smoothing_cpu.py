"""Label smoothing, the parts that need no GPU: the --label_smoothing flag of python -m kzv.train and the ctypes bindings of the three
new symbols (include/kzv.h)."""
import ctypes as C

import pytest

from kzv import _lib as L
from kzv.train import parse_args


def test_flag_default_and_value():
    assert parse_args([]).label_smoothing == 0.0
    assert parse_args(["--label_smoothing", "0.1"]).label_smoothing == 0.1
    assert parse_args(["--label_smoothing", "0"]).label_smoothing == 0.0


@pytest.mark.parametrize("argv", [["--label_smoothing", "1.0"], ["--label_smoothing", "-0.1"], ["--label_smoothing", "nan"],
                                  ["--label_smoothing", "0.1", "--model", "ocr"]])
def test_flag_rejections(argv, capsys):
    with pytest.raises(SystemExit) as e:
        parse_args(argv)
    assert e.value.code == 2                                   # argparse's error exit
    assert "--label_smoothing" in capsys.readouterr().err


def test_ocr_model_without_the_flag_still_parses():
    assert parse_args(["--model", "ocr"]).label_smoothing == 0.0


def test_help_says_what_train_loss_and_val_loss_are(capsys):
    with pytest.raises(SystemExit):
        parse_args(["--help"])
    out = " ".join(capsys.readouterr().out.split())
    assert "--label_smoothing" in out and "an extension" in out and "train_loss in the logs is then the SMOOTHED loss" in out
    assert "val_loss and the test losses stay the plain cross-entropy" in out


def test_bindings_of_the_new_symbols():
    res, args = L.SYMBOLS["kzv_set_label_smoothing"]
    assert res is C.c_int and args == [C.c_void_p, C.c_float]
    res, args = L.SYMBOLS["kzv_get_label_smoothing"]
    assert res is C.c_float and args == [C.c_void_p]
    res, args = L.SYMBOLS["kzv_ce_fwd_bwd_ls"]
    plain = L.SYMBOLS["kzv_ce_fwd_bwd"][1]
    assert res is C.c_int and args == plain[:-1] + [C.c_float] + plain[-1:]      # kzv_ce_fwd_bwd's list with eps before the stream
