"""The character n-gram language model on the host (kzv/lm.py): normalisation of the fitted model, ``row`` against a brute-force
recursion and on hand-built tables, file round trips, ARPA import, ``fuse_reference`` and the CLI surface.  No GPU."""
import math

import numpy as np
import pytest
import torch

from kzv import lm as LM
from kzv.lm import NGramLM

from _trained import load as load_trained


@pytest.fixture(scope="module")
def fixture_sequences():
    gold, cfg, sd, data = load_trained()
    labs = np.concatenate([data["fit"][1], data["unseen"][1]])
    seqs = LM.sequences_from_labels(labs, cfg.pad_id, cfg.eos_id)
    assert len(seqs) == 12 and all(s[0] == cfg.bos_id and s[-1] == cfg.eos_id for s in seqs)
    return cfg, seqs


# ---- 1. normalisation -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [2, 3, 4])
def test_fitted_model_is_normalised_after_every_prefix(order, fixture_sequences):
    cfg, seqs = fixture_sequences
    lm = NGramLM.fit(seqs, order, cfg.vocab, discount=0.75)
    assert lm.n_contexts() == [71, 100, 88][:order - 1]
    e64 = e32 = 0.0
    for s in seqs:
        for i in range(1, len(s) + 1):
            e64 = max(e64, abs(float(lm.prob64(s[:i]).sum()) - 1.0))
            e32 = max(e32, abs(float(np.exp(lm.row(s[:i]).astype(np.float64)).sum()) - 1.0))
    print(f"order {order}: |sum - 1| float64 {e64:.3g}, exp(row) {e32:.3g}")
    assert e64 < 1e-12 and e32 < 1e-6


# ---- 2. row against brute force and on hand-built tables --------------------------------------------------------------------------------
def _brute(seqs, order, vocab, D):
    """P_k by the recursion of the issue, straight from the sequences (no shared code with kzv/lm.py)."""
    def count(ctx):
        out = {}
        k = len(ctx)
        for s in seqs:
            for i in range(max(1, k), len(s)):
                if tuple(s[i - k:i]) == tuple(ctx):
                    out[s[i]] = out.get(s[i], 0) + 1
        return out

    def P(ctx):
        c = count(ctx)
        if not ctx:
            T = sum(c.values())
            return np.array([max(c.get(v, 0) - D, 0.0) / T + (D * len(c) / T) / vocab for v in range(vocab)])
        low = P(ctx[1:])
        if not c:
            return low
        tot = sum(c.values())
        return np.array([max(c.get(v, 0) - D, 0.0) / tot for v in range(vocab)]) + (D * len(c) / tot) * low
    return P


@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_row_equals_the_brute_force_recursion(order):
    rng = np.random.default_rng(order)
    vocab, pool = 40, rng.choice(np.arange(4, 40), size=12, replace=False)
    seqs = [[0] + [int(v) for v in pool[rng.integers(0, 12, size=rng.integers(2, 14))]] + [2] for _ in range(30)]
    lm = NGramLM.fit(seqs, order, vocab, discount=0.75)
    P = _brute(seqs, order, vocab, 0.75)
    worst, exact = 0.0, 0
    for s in seqs[:8] + [[0, 39, 38], [0, int(pool[0]), 39, int(pool[1])]]:      # seen prefixes, and contexts never seen
        for i in range(1, len(s) + 1):
            h = s[:i]
            want = np.log(P(tuple(h[max(0, len(h) - (order - 1)):]) if order > 1 else ()))
            got = lm.row(h)
            worst = max(worst, float(np.abs(got - want).max()))
            # the same path, no back-off in it (acc == 0): the stored value is the brute-force one rounded once -- equal, not close
            k = min(order - 1, len(h))
            if k == 0:
                assert np.array_equal(got, want.astype(np.float32)), h
                exact += vocab
            else:
                j = lm._find(h[len(h) - k:])
                if j >= 0:
                    tok = lm.succ_tok[lm.off[k - 1][j]:lm.off[k - 1][j + 1]]
                    assert tok.size and np.array_equal(got[tok], want.astype(np.float32)[tok]), (h, tok)
                    exact += int(tok.size)
    assert exact > 50, exact
    print(f"order {order}: {exact} elements equal to the brute force rounded to fp32; max |row - log P_k| = {worst:.3g}")
    # both take the same path; row sums up to three fp32-rounded back-offs and one rounded leaf, each add rounded again: at most 7
    # roundings of half an ulp of values below 16 (9.5e-7), 3.4e-6
    assert worst < 3.4e-6


def _hand_table():
    """vocab 8, order 3: the context (1, 2) exists, its suffix (2,) does not; token 5 is listed under (1, 2) and under (3,);
    (4, 3) and (3,) both list token 6."""
    uni = np.log(np.array([0.05, 0.1, 0.1, 0.15, 0.2, 0.1, 0.25, 0.05]))
    ctx = {(1, 2): (math.log(0.4), {5: math.log(0.5), 7: math.log(0.1)}),
           (3,): (math.log(0.3), {5: math.log(0.6), 6: math.log(0.1)}),
           (4, 3): (math.log(0.2), {6: math.log(0.7)})}
    return NGramLM.from_tables(3, 8, uni, ctx), uni, ctx


def test_row_follows_the_stated_rule_on_a_hand_built_table():
    lm, uni, ctx = _hand_table()
    f = np.float32
    # (1, 2) found, (2,) absent: skipped, acc = bo(1, 2) alone
    r = lm.row([0, 1, 2])
    acc = f(0) + f(ctx[(1, 2)][0])
    assert r[5] == f(math.log(0.5)) and r[7] == f(math.log(0.1))
    for v in (0, 1, 2, 3, 4, 6):
        assert r[v] == f(acc + f(uni[v]))
    # a token under several orders takes the highest order's value: 6 from (4, 3), 5 from (3,) + bo(4, 3)
    r = lm.row([0, 4, 3])
    a1 = f(ctx[(4, 3)][0])
    assert r[6] == f(math.log(0.7)) and r[5] == f(a1 + f(math.log(0.6)))
    a2 = f(a1 + f(ctx[(3,)][0]))
    assert r[0] == f(a2 + f(uni[0]))
    # a token outside the vocabulary in the context: not found
    assert np.array_equal(lm.row([0, 99, 3]), lm.row([0, 7, 3])) and lm.row([0, 7, 3])[6] == f(f(0) + f(math.log(0.1)))
    # BOS alone and the empty history
    assert np.array_equal(lm.row([0]), uni.astype(f)) and np.array_equal(lm.row([]), uni.astype(f))


# ---- 3. round trips and import --------------------------------------------------------------------------------------------------------------
def test_save_load_round_trip_is_bitwise_and_needs_no_pickle(tmp_path, fixture_sequences):
    cfg, seqs = fixture_sequences
    lm = NGramLM.fit(seqs, 4, cfg.vocab)
    path = str(tmp_path / "lm.npz")
    lm.save(path)
    with np.load(path, allow_pickle=False) as z:
        assert set(z.files) == set(lm.tables()) and all(z[k].dtype != object for k in z.files)
    back = NGramLM.load(path)
    assert back.order == 4 and back.vocab == cfg.vocab
    for k, v in lm.tables().items():
        assert np.array_equal(v, back.tables()[k]) and v.dtype == back.tables()[k].dtype, k
    assert np.array_equal(back.row(seqs[0][:4]).view(np.uint32), lm.row(seqs[0][:4]).view(np.uint32))


ARPA = """\\data\\
ngram 1=5
ngram 2=4

\\1-grams:
-1.0\t<s>\t-0.5
-0.7\t</s>
-0.5\ta\t-0.3
-0.6\tb\t-0.2
-0.9\tq\t-0.1

\\2-grams:
-0.2\t<s>\ta
-0.4\ta\tb
-0.3\tb\t</s>
-0.1\tq\ta

\\end\\
"""


def test_from_arpa_gives_the_stated_values():
    ln10 = math.log(10.0)
    f = np.float32
    lm = NGramLM.from_arpa(ARPA, {"a": 4, "b": 5, "c": 6}, bos_id=0, eos_id=2, vocab=7)      # q is unmapped; c has no unigram; no <unk>
    assert lm.order == 2 and lm.n_contexts() == [3]                    # <s>, a, b (q dropped with its back-off and its bigram)
    assert lm.uni[4] == f(-0.5 * ln10) and lm.uni[5] == f(-0.6 * ln10) and lm.uni[0] == f(-1.0 * ln10) and lm.uni[2] == f(-0.7 * ln10)
    assert lm.uni[6] == f(-1.0 * ln10) and lm.uni[1] == f(-1.0 * ln10) and lm.uni[3] == f(-1.0 * ln10)      # the smallest unigram value
    r = lm.row([0])
    assert r[4] == f(-0.2 * ln10) and r[5] == f(f(-0.5 * ln10) + f(-0.6 * ln10))
    r = lm.row([0, 4])
    assert r[5] == f(-0.4 * ln10) and r[2] == f(f(-0.3 * ln10) + f(-0.7 * ln10))
    r = lm.row([0, 4, 5])
    assert r[2] == f(-0.3 * ln10) and r[4] == f(f(-0.2 * ln10) + f(-0.5 * ln10))
    with_unk = ARPA.replace("ngram 1=5", "ngram 1=6").replace("-0.9\tq\t-0.1", "-0.9\tq\t-0.1\n-2.5\t<unk>")
    assert NGramLM.from_arpa(with_unk, {"a": 4, "b": 5, "c": 6}, 0, 2, 7).uni[6] == f(-2.5 * ln10)


def test_logprob_and_perplexity_of_a_known_sequence():
    lm, uni, ctx = _hand_table()
    s = [0, 1, 2, 5, 3, 6]
    f = np.float32
    want = [f(uni[1]),                                                     # after [0]: no context of 0
            f(uni[2]),                                                     # after [0, 1]: (0, 1) and (1,) absent
            f(math.log(0.5)),                                              # after (1, 2): 5 is listed
            f(uni[3]),                                                     # after (2, 5), (5,): absent
            f(math.log(0.1))]                                              # after (5, 3) absent, (3,): 6 listed
    total = float(sum(float(v) for v in want))
    assert lm.logprob(s) == total
    assert lm.perplexity([s]) == math.exp(-total / 5)
    assert lm.perplexity([s, s]) == pytest.approx(math.exp(-total / 5), rel=1e-15)


# ---- 4. fuse_reference ---------------------------------------------------------------------------------------------------------------------
def test_fuse_reference_keeps_minus_infinity_skips_dead_rows_and_is_the_identity_at_weight_zero():
    lm, _, _ = _hand_table()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(4, 8, generator=g)
    x[0, 5] = x[2, 0] = float("-inf")
    hist = torch.tensor([[0, 1, 2, 0], [0, 4, 3, 0], [0, 3, 0, 0], [0, 0, 0, 0]])
    y = LM.fuse_reference(x, hist[:, :3], lm, 0.7)
    assert y.dtype == torch.float32 and y[0, 5] == float("-inf") and y[2, 0] == float("-inf")
    w = np.float32(0.7)
    want = x[1].numpy() + (lm.row([0, 4, 3]) * w).astype(np.float32)
    assert np.array_equal(y[1].numpy(), want.astype(np.float32))
    assert torch.equal(LM.fuse_reference(x, hist[:, :3], lm, 0.0), x)
    lens, live = torch.tensor([3, 3, 2, 1]), torch.tensor([True, False, True, False])
    z = LM.fuse_rows_reference(x, hist, lens, lm, 0.7, live)
    assert torch.equal(z[1], x[1]) and torch.equal(z[3], x[3]) and torch.equal(z[0], y[0])
    assert torch.equal(z[2:3], LM.fuse_reference(x[2:3], hist[2:3, :2], lm, 0.7))


# ---- 5. CLI surface and refusals -----------------------------------------------------------------------------------------------------------
def test_cli_surface_and_python_level_refusals(capsys):
    from kzv.train import parse_args
    a = parse_args([])
    assert a.lm_weight == 0.0 and a.lm_order == 0 and a.lm_path is None
    assert parse_args(["--lm_order", "3", "--lm_weight", "0.4"]).lm_order == 3
    with pytest.raises(SystemExit):
        parse_args(["--model", "ocr", "--lm_weight", "0.3"])
    assert "--lm_" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        parse_args(["--lm_order", "5"])
    with pytest.raises(ValueError, match="order"):
        NGramLM(5, 100)
    with pytest.raises(ValueError, match="vocab"):
        NGramLM(2, 16385)
    lm, _, _ = _hand_table()
    with pytest.raises(ValueError, match="vocabulary"):
        LM.resolve(lm, 0.5, 9)
    with pytest.raises(ValueError, match="finite"):
        LM.resolve(lm, float("nan"), 8)
    with pytest.raises(ValueError, match="NGramLM"):
        LM.resolve(object(), 0.5, 8)
    assert LM.resolve(None, 0.5, 8) is None and LM.resolve(lm, 0.0, 8) is None
    assert LM.resolve(lm, 0.5, 8)[0] is lm


# ---- 6. the CLIs fit on label rows that hold no BOS / EOS --------------------------------------------------------------------------------------
def _starts_and_ends(lm, cfg, first_tokens):
    """the (BOS,) context exists with the lines' first characters as successors, and EOS is a seen successor of some context"""
    j = lm._find([cfg.bos_id])
    assert j >= 0, "no (BOS,) context: the fit never saw a line start"
    succ = set(lm.succ_tok[lm.off[0][j]:lm.off[0][j + 1]].tolist())
    assert succ == set(first_tokens)
    assert cfg.eos_id in set(lm.succ_tok.tolist()), "EOS is no seen successor: every step would tax it by the unigram floor"
    assert lm.uni[cfg.eos_id] > lm.uni[cfg.pad_id] and cfg.bos_id not in set(lm.succ_tok.tolist())


def test_train_cli_start_up_fit_wraps_the_label_rows_and_saves_the_model(tmp_path, capsys):
    import types
    from kzv.config import tiny_config
    from kzv.data import SyntheticLineDataset
    from kzv.train import _decode_lm, parse_args
    cfg = tiny_config()
    ds = SyntheticLineDataset(cfg, 24, 20, seed=4)
    firsts = [int(ds[i]["labels"][0]) for i in range(24)]
    assert cfg.bos_id not in firsts                                    # the labels hold no BOS: the recipe of kzv/data.py
    model = types.SimpleNamespace(cfg=cfg, tokenizer=None)
    out = str(tmp_path / "run")
    lm = _decode_lm(parse_args(["--lm_order", "3", "--lm_weight", "0.4"]), model, ds, out, 0)
    path = tmp_path / "run" / "checkpoints" / "lm.npz"
    assert path.exists() and lm.order == 3 and lm.vocab == cfg.vocab
    assert "order 3" in capsys.readouterr().out
    _starts_and_ends(lm, cfg, firsts)
    saved = NGramLM.load(str(path))
    assert all(np.array_equal(v, saved.tables()[k]) for k, v in lm.tables().items())
    # a decode's history [BOS] then finds its context: the first step is no unigram row
    assert not np.array_equal(lm.row([cfg.bos_id]), lm.uni)
    # weight 0: fitted and saved all the same, and off
    out2 = str(tmp_path / "run2")
    assert _decode_lm(parse_args(["--lm_order", "2"]), model, ds, out2, 0) is None
    assert (tmp_path / "run2" / "checkpoints" / "lm.npz").exists()
    assert _decode_lm(parse_args([]), model, ds, str(tmp_path / "run3"), 0) is None and not (tmp_path / "run3").exists()


def test_lm_cli_fit_wraps_every_line(tmp_path, capsys):
    from kzv.config import tiny_config
    from kzv.data import build_decoder_dir, synthetic_charset
    cfg = tiny_config()
    d = build_decoder_dir(str(tmp_path / "dec"), cfg)
    chars = synthetic_charset(cfg.vocab - 5)
    lines = ["".join(chars[(7 * i + 3 * j) % 40] for j in range(3 + i % 5)) for i in range(30)]
    text = tmp_path / "labels.txt"
    text.write_text("\n".join(lines) + "\n", encoding="utf-8")
    out = str(tmp_path / "lm.npz")
    assert LM._main(["fit", str(text), "--tokenizer", d, "--order", "3", "--out", out]) == 0
    lm = NGramLM.load(out)
    _starts_and_ends(lm, cfg, [5 + (7 * i) % 40 for i in range(30)])
    assert LM._main(["info", out]) == 0 and LM._main(["perplexity", out, str(text), "--tokenizer", d]) == 0
    said = capsys.readouterr().out
    assert "perplexity" in said and "order=3" in said
    with_wrap = lm.perplexity([[cfg.bos_id] + [5 + (7 * i + 3 * j) % 40 for j in range(3 + i % 5)] + [cfg.eos_id] for i in range(30)])
    assert f"{with_wrap:.4f}" in said
