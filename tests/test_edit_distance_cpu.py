"""Edit distance / CER / alignment on token ids (kzv/metrics.py, include/kzv.h: kzv_edit_distance), the parts that need no GPU:

  * edit_stats_reference -- the numpy statement the kernel is tested against -- returns, over ids with the specials dropped, the distances
    kzv.model._levenshtein returns over the strings batch_decode(skip_special_tokens=True) makes of the same rows, and its edit counts add up;
  * it reproduces the reference's CER values of tests/golden/cer_kat.npz and the 2/9 corpus example through a char -> id map;
  * hand-checkable alignments pin the preference: diagonal, then deletion, then insertion;
  * the ABI: the symbol is bound, and every argument error returns before a device is touched (without a GPU a launch would have been a
    HIP error instead);
  * is_one_char_tokenizer accepts build_decoder_dir's tokenizer and refuses a vocabulary with a two-character entry."""
import ctypes as C
import os

import numpy as np
import pytest

from kzv import _lib as L
from kzv import metrics as M
from kzv.config import tiny_config
from kzv.data import build_decoder_dir
from kzv.model import _levenshtein

SPECIAL = [0, 1, 2, 3, 4]


@pytest.fixture(scope="module")
def tokenizer(tmp_path_factory):
    from transformers import AutoTokenizer
    return AutoTokenizer.from_pretrained(build_decoder_dir(str(tmp_path_factory.mktemp("dec")), tiny_config()))


def _random_pairs(n, vocab, width, seed):
    """Label rows of 0..width-4 characters, predictions = the label with ~15 % substitutions / deletions / insertions (or an unrelated
    line), specials sprinkled at the front, in the middle and after the end of both."""
    rng = np.random.default_rng(seed)
    ref = np.full((n, width), 1, dtype=np.int64)
    pred = np.full((n, width), 1, dtype=np.int64)
    for k in range(n):
        m = int(rng.integers(0, width - 3))
        r = rng.integers(5, vocab, m).tolist()
        if rng.random() < 0.2:
            p = rng.integers(5, vocab, int(rng.integers(0, width - 3))).tolist()
        else:
            p = []
            for t in r:
                u = rng.random()
                if u < 0.05:
                    continue
                p.append(int(rng.integers(5, vocab)) if u < 0.10 else t)
                if u > 0.95:
                    p.append(int(rng.integers(5, vocab)))
            p = p[:width - 3]
        for row, line in ((ref[k], r), (pred[k], [2] + p + [3])):
            line = list(line)
            if line and rng.random() < 0.3:
                line.insert(int(rng.integers(0, len(line))), int(rng.choice([0, 4])))      # [UNK] / [MASK] inside the line
            row[:len(line)] = line[:width]
            if rng.random() < 0.2 and len(line) + 2 <= width:
                row[len(line) + 1] = int(rng.integers(5, vocab))                             # a character after the padding began
    return pred, ref


def test_reference_equals_the_string_path(tokenizer):
    V = tiny_config().vocab
    pred, ref = _random_pairs(300, V, 24, seed=3)
    st = M.edit_stats_reference(pred, ref, tokenizer.all_special_ids, V, align=True, char_stats=True)
    ps = tokenizer.batch_decode(pred, skip_special_tokens=True)
    ts = tokenizer.batch_decode(ref, skip_special_tokens=True)
    assert st["dist"].tolist() == [_levenshtein(p, t) for p, t in zip(ps, ts)]
    assert st["ref_len"].tolist() == [len(t) for t in ts] and st["pred_len"].tolist() == [len(p) for p in ps]
    assert max(st["dist"]) > 0 and min(st["dist"]) == 0
    o = st["ops"].astype(np.int64)
    assert (o[:, 1] + o[:, 2] + o[:, 3] == st["dist"]).all()
    assert (o[:, 0] + o[:, 1] + o[:, 2] == st["ref_len"]).all() and (o[:, 0] + o[:, 1] + o[:, 3] == st["pred_len"]).all()
    cs = st["char_stats"].astype(np.int64)
    assert (cs[:, 0] == cs[:, 1] + cs[:, 2] + cs[:, 3]).all() and cs[:5].sum() == 0
    assert cs.sum(axis=0).tolist() == [int(st["ref_len"].sum())] + o.sum(axis=0).tolist()
    # the CER values are the string path's, ==
    from kzv.model import TrOCRModel
    want = [TrOCRModel.calculate_cer(None, p, t) for p, t in zip(ps, ts)]
    assert M.cer_values(st["dist"], st["ref_len"], st["pred_len"]) == want


def _encode(strings, table, width):
    out = np.full((len(strings), width), 1, dtype=np.int64)
    for k, s in enumerate(strings):
        out[k, :len(s)] = [table.setdefault(ch, 5 + len(table)) for ch in s]
    return out


def test_reference_reproduces_the_golden_cer(golden_dir):
    g = np.load(os.path.join(golden_dir, "cer_kat.npz"), allow_pickle=False)
    preds, tgts = [str(p) for p in g["preds"]], [str(t) for t in g["targets"]]
    table = {}
    width = max(1, max(map(len, preds + tgts)))
    st = M.edit_stats_reference(_encode(preds, table, width), _encode(tgts, table, width), SPECIAL, 5 + len(table) + 1)
    got = M.cer_values(st["dist"], st["ref_len"], st["pred_len"])
    for c, want in zip(got, g["cer"]):
        assert c == pytest.approx(float(want))
    assert got == [(1.0 if p else 0.0) if not t else _levenshtein(p, t) / len(t) for p, t in zip(preds, tgts)]
    # the reference's corpus example: 2 edits over 9 characters
    table = {}
    st = M.edit_stats_reference(_encode(["ac", "cot", "test"], table, 4), _encode(["ab", "cat", "test"], table, 4), SPECIAL, 32)
    assert int(st["dist"].sum()) == 2 and int(st["ref_len"].sum()) == 9
    assert st["ops"].tolist() == [[1, 1, 0, 0], [2, 1, 0, 0], [4, 0, 0, 0]]


def test_the_alignment_preference_is_diagonal_then_deletion_then_insertion():
    a, b, c = 5, 6, 7

    def one(ref, pred):
        width = 4
        r = np.full((1, width), 1, dtype=np.int64); r[0, :len(ref)] = ref
        p = np.full((1, width), 1, dtype=np.int64); p[0, :len(pred)] = pred
        st = M.edit_stats_reference(p, r, SPECIAL, 8, align=True, char_stats=True)
        return int(st["dist"][0]), st["ops"][0].tolist(), st["ref_to_pred"][0].tolist(), st["pred_to_ref"][0].tolist(), st["char_stats"]

    # abc against ac: b is deleted, a and c stay
    d, ops, r2p, p2r, cs = one([a, b, c], [a, c])
    assert (d, ops, r2p, p2r) == (1, [2, 0, 1, 0], [0, -1, 1, -2], [0, 2, -2, -2])
    assert cs[b].tolist() == [1, 0, 0, 1, 0] and cs[a].tolist() == [1, 1, 0, 0, 0]
    # ab against ba: distance 2 three ways (two substitutions; delete + insert either way round): the diagonal wins
    d, ops, r2p, p2r, cs = one([a, b], [b, a])
    assert (d, ops, r2p, p2r) == (2, [0, 2, 0, 0], [0, 1, -2, -2], [0, 1, -2, -2])
    # aa against a: the walk back from the end takes the diagonal first, so the FIRST a is the deleted one
    d, ops, r2p, p2r, cs = one([a, a], [a])
    assert (d, ops, r2p, p2r) == (1, [1, 0, 1, 0], [-1, 0, -2, -2], [1, -2, -2, -2])
    # ab against abc, then against cab: insertions at the end and at the front
    assert one([a, b], [a, b, c])[1:4] == ([2, 0, 0, 1], [0, 1, -2, -2], [0, 1, -1, -2])
    assert one([a, b], [c, a, b])[1:4] == ([2, 0, 0, 1], [1, 2, -2, -2], [-1, 0, 1, -2])
    # ab against bc: substitute twice (diagonal) rather than delete a, keep b, insert c -- both cost 2
    assert one([a, b], [b, c])[1:3] == ([0, 2, 0, 0], [0, 1, -2, -2])
    # up before left: abc against bd costs 2 as (delete a, keep b, c -> d) only; ab against ca ...
    d, ops, r2p, p2r, cs = one([a, b, c], [b, a])
    assert d == 2 and ops[1] + ops[2] + ops[3] == 2
    # empty sides
    assert one([], [a, b])[:2] == (2, [0, 0, 0, 2]) and one([a, b], [])[:2] == (2, [0, 0, 2, 0]) and one([], [])[:2] == (0, [0, 0, 0, 0])
    assert M.cer_values([2, 2, 0], [0, 2, 0], [2, 0, 0]) == [1.0, 1.0, 0.0]


def test_out_of_range_ids_and_specials_vanish():
    r = np.array([[2, 5, -100, 6, 0, 7, 3, 1, 9, 1]], dtype=np.int64)           # 9 == vocab: outside
    p = np.array([[2, 5, 6, 7, 3, 1, 1, 1, 4, 8]], dtype=np.int64)
    st = M.edit_stats_reference(p, r, SPECIAL, 9, align=True, char_stats=True)
    assert (int(st["dist"][0]), int(st["ref_len"][0]), int(st["pred_len"][0])) == (1, 3, 4)
    assert st["ops"][0].tolist() == [3, 0, 0, 1] and st["char_stats"][8].tolist() == [0, 0, 0, 0, 1]
    assert st["char_stats"].shape == (9, 5) and st["char_stats"][:5].sum() == 0


def test_character_table_sorts_by_errors_then_id():
    cs = np.zeros((10, 5), dtype=np.int32)
    cs[5] = [4, 2, 1, 1, 0]; cs[6] = [3, 3, 0, 0, 2]; cs[7] = [1, 1, 0, 0, 0]; cs[9] = [0, 0, 0, 0, 3]
    rows = M.character_table(cs, None, top=3)
    assert [r["id"] for r in rows] == [9, 5, 6]
    assert rows[1] == {"char": None, "id": 5, "count": 4, "correct": 2, "substituted": 1, "deleted": 1, "inserted": 0, "error_rate": 0.5}
    assert [r["id"] for r in M.character_table(cs, None, top=None)] == [9, 5, 6, 7]


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load()


def _args(**kw):
    p = 4096                                                 # never dereferenced: the checks come before any launch
    base = dict(pred=p, ld_pred=16, ref=p, ld_ref=16, n=3, width_pred=16, width_ref=16, vocab=50, n_special=5,
                special=(C.c_int32 * 8)(0, 1, 2, 3, 4), dist=p, ref_len=p, pred_len=p, ops=None, ref_to_pred=None, pred_to_ref=None,
                ld_align=16, char_stats=None)
    base.update(kw)
    return L.kzv_edit_args(**base)


def test_symbol_is_bound(lib):
    assert "kzv_edit_distance" in L.SYMBOLS and lib.kzv_edit_distance.argtypes is not None
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kzv.h")) as f:
        hdr = f.read()
    assert "int kzv_edit_distance(const kzv_edit_args* a, void* stream);" in hdr
    # the ctypes mirror has the C layout: 4 x 8 bytes, 13 int32 (+ 4 bytes of padding), 6 pointers, ld_align, 1 pointer
    assert C.sizeof(L.kzv_edit_args) == 32 + 56 + 6 * 8 + 8 + 8 and L.kzv_edit_args.dist.offset == 88


@pytest.mark.parametrize("kw,word", [
    (dict(pred=None), b"pred"), (dict(ref=None), b"ref"), (dict(dist=None), b"dist"), (dict(ref_len=None), b"ref_len"),
    (dict(pred_len=None), b"pred_len"),
    (dict(width_pred=0), b"width"), (dict(width_pred=129, ld_pred=129), b"width"), (dict(width_ref=0), b"width"),
    (dict(width_ref=129, ld_ref=129), b"width"),
    (dict(ld_pred=15), b"ld_pred"), (dict(ld_ref=15), b"ld_ref"),
    (dict(n_special=-1), b"n_special"), (dict(n_special=9), b"n_special"),
    (dict(vocab=0), b"vocab"),
    (dict(ref_to_pred=4096), b"together"), (dict(pred_to_ref=4096), b"together"),
    (dict(ref_to_pred=4096, pred_to_ref=4096, ld_align=15), b"ld_align"),
    (dict(n=-1), b"n must"),
])
def test_bad_arguments_are_refused_before_any_launch(lib, kw, word):
    a = _args(**kw)
    assert lib.kzv_edit_distance(C.byref(a), None) == -1      # KZV_E_ARG
    msg = lib.kzv_last_error()
    assert b"edit_distance" in msg and word in msg, msg


def test_null_arguments_and_no_pairs(lib):
    assert lib.kzv_edit_distance(None, None) == -1 and b"edit_distance" in lib.kzv_last_error()
    a = _args(n=0)
    assert lib.kzv_edit_distance(C.byref(a), None) == 0       # KZV_OK: nothing is launched
    a = _args(n=0, width_ref=0)
    assert lib.kzv_edit_distance(C.byref(a), None) == -1      # ... but the shape is still checked


# ---- the tokenizer test ----------------------------------------------------------------------------------------------------------------
def test_one_char_tokenizer(tokenizer):
    assert M.is_one_char_tokenizer(tokenizer)
    assert len(tokenizer.all_special_ids) == 5 and sorted(tokenizer.all_special_ids) == SPECIAL

    from tokenizers import Regex, Tokenizer, decoders, pre_tokenizers
    from tokenizers.models import WordLevel
    from transformers import PreTrainedTokenizerFast
    from kzv.data import SPECIAL_TOKENS

    def make(entries):
        vocab = {t: i for i, t in enumerate(SPECIAL_TOKENS + entries)}
        tok = Tokenizer(WordLevel(vocab=vocab, unk_token="[UNK]"))
        tok.pre_tokenizer = pre_tokenizers.Split(Regex(r"[\s\S]"), behavior="isolated")
        tok.decoder = decoders.Sequence([])
        tok.add_special_tokens(SPECIAL_TOKENS)
        return PreTrainedTokenizerFast(tokenizer_object=tok, unk_token="[UNK]", pad_token="[PAD]", cls_token="[CLS]", sep_token="[SEP]",
                                       mask_token="[MASK]", bos_token="[CLS]", eos_token="[SEP]")

    assert M.is_one_char_tokenizer(make(["a", "b", "c"]))
    assert not M.is_one_char_tokenizer(make(["a", "bc", "d"]))
    assert not M.is_one_char_tokenizer(object())
