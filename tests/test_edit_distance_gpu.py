"""kzv_edit_distance on the GPU (include/kzv.h; csrc/edit_distance.hip; kzv/metrics.py) against metrics.edit_stats_reference -- the numpy
statement: full matrix, walk back preferring diagonal, then deletion, then insertion.  Every comparison is exact.

Op level.  Compacted lengths (m label, n prediction) over {0, 1, 2, 63, 64, 65, 127, 128}^2 in one batch of 128-column rows: empty sides,
both lane-ownership boundaries (a lane owns two columns: 64 / 65 and 127 / 128), identical rows, rows with no character in common, a
prediction that repeats its label (CER > 1), predictions that are edits of the label over a 12-character alphabet (many ties for the
walk); the batch is ordered so that the four waves of a workgroup get very different lengths.  Raw rows carry [CLS] at the front,
specials in the middle, [SEP] followed by padding and by stray characters, and the ids -100, vocab and vocab + 7, which must vanish and
never reach char_stats.  Further shapes: widths 70 / 33 inside 160-column buffers (ld larger than the width), N = 1, 3, 5 (a partial
last workgroup), N = 1,100 lines of <= 12 characters (more waves than the part holds at once).  Every shape runs on two different
inputs.  The distance-only instance equals the full one's dist; char_stats accumulates over two calls on the halves of a batch.

Model level, on the reference-fitted fixture (tests/_trained.py) with some labels perturbed so that errors exist: evaluate_many and cer_of
equal generate_stream + batch_decode + calculate_cer for 1 and 4 beams; trainer.test(stream_decode=True) returns the same CER values
whether the tokenizer is recognised as one character per token (device path) or not (string path)."""
import numpy as np
import pytest
import torch

from kzv import metrics as M
from kzv.data import build_decoder_dir
from kzv.model import TrOCRModel

from _trained import load as load_trained

pytestmark = pytest.mark.gpu

SPECIAL = [0, 1, 2, 3, 4]
V = 40
LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128]
JUNK = [0, 1, 2, 3, 4, -100, V, V + 7]


def _raw(line, width, rng, lead=None):
    """`line` with dropped-by-rule ids put around and between its characters, as far as `width` allows; [SEP] and padding after it, with
    one more dropped id somewhere in the padding (nothing may be cut at the first [SEP])."""
    row = list(line)
    room = width - len(row)
    if lead is not None and room > 0:
        row.insert(0, lead); room -= 1
    for _ in range(min(room, int(rng.integers(0, 4)))):
        row.insert(int(rng.integers(0, len(row) + 1)), int(rng.choice(JUNK)))
    if len(row) < width:
        row.append(3)                                        # [SEP]
    out = np.full(width, 1, dtype=np.int64)
    out[:len(row)] = row
    if len(row) + 2 <= width:
        out[int(rng.integers(len(row) + 1, width))] = int(rng.choice([4, -100, V, 0]))
    return out


def _edited(r, n, rng, lo, hi):
    """n characters: r with ~10 % substituted, ~5 % dropped, ~5 % doubled, then cut or filled to n"""
    p = []
    for t in r:
        u = rng.random()
        if u < 0.05:
            continue
        p.append(int(rng.integers(lo, hi)) if u < 0.15 else t)
        if u > 0.95:
            p.append(int(rng.integers(lo, hi)))
    p = p[:n]
    return p + rng.integers(lo, hi, n - len(p)).tolist()


def _grid(seed):
    rng = np.random.default_rng(seed)
    lines = []
    for m in LENGTHS:
        for n in LENGTHS:
            r = rng.integers(5, 17, m).tolist()              # 12 characters: ties everywhere
            lines.append((r, _edited(r, n, rng, 5, 17)))
    ident = rng.integers(5, V, 128).tolist()
    lines += [(ident, list(ident)), (ident[:65], list(ident[:65])), (ident[:1], list(ident[:1]))]
    lines += [(rng.integers(5, 20, 128).tolist(), rng.integers(20, V, 128).tolist()), (rng.integers(5, 20, 63).tolist(), rng.integers(20, V, 65).tolist())]
    half = rng.integers(5, V, 64).tolist()
    lines += [(half, half + half), (half[:1], half[:1] * 2), (half[:32], half[:32] * 3)]
    order = rng.permutation(len(lines)).tolist()             # neighbours in a workgroup: unrelated lengths
    lead = [(128, 128), (0, 0), (1, 127), (64, 2)]           # ... and one workgroup of extremes in front
    first = [next(k for k in order if (len(lines[k][0]), len(lines[k][1])) == mn) for mn in lead]
    order = first + [k for k in order if k not in first]
    ref = np.stack([_raw(lines[k][0], 128, rng) for k in order])
    pred = np.stack([_raw(lines[k][1], 128, rng, lead=2) for k in order])
    return pred, ref


def _short(n, width, max_chars, seed, lo=5, hi=V):
    rng = np.random.default_rng(seed)
    ref, pred = [], []
    for _ in range(n):
        r = rng.integers(lo, hi, int(rng.integers(0, max_chars + 1))).tolist()
        p = _edited(r, int(rng.integers(0, max_chars + 1)), rng, lo, hi) if rng.random() < 0.8 else list(r)
        ref.append(_raw(r, width, rng)); pred.append(_raw(p, width, rng, lead=2))
        for row in (ref[-1], pred[-1]):
            if row[-1] == 1 and rng.random() < 0.3:
                row[-1] = int(rng.integers(lo, hi))           # a character after [SEP] and padding: it belongs to the line
    return np.stack(pred), np.stack(ref)


def _in_wider_buffer(x, ld):
    buf = torch.full((x.shape[0], ld), 7, dtype=torch.int64, device="cuda")         # 7 is a character: a read past the width would count
    buf[:, :x.shape[1]] = torch.from_numpy(x).cuda()
    return buf[:, :x.shape[1]]


def _check(tag, pred, ref, ld=None):
    want = M.edit_stats_reference(pred, ref, SPECIAL, V, align=True, char_stats=True)
    dp = _in_wider_buffer(pred, ld) if ld else torch.from_numpy(pred).cuda()
    dr = _in_wider_buffer(ref, ld) if ld else torch.from_numpy(ref).cuda()
    if ld and pred.shape[0] > 1:
        assert dp.stride(0) == ld and dr.stride(0) == ld
    got = M.edit_stats(dp, dr, SPECIAL, V, align=True, char_stats=True)
    torch.cuda.synchronize()
    assert set(got) == set(want)
    for k in ("dist", "ref_len", "pred_len", "ops", "ref_to_pred", "pred_to_ref", "char_stats"):
        g = got[k].cpu().numpy()
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, (tag, k, g.shape, want[k].shape)
        bad = np.argwhere(g != want[k])
        assert bad.size == 0, (tag, k, bad[:4].tolist(), g[tuple(bad[0])], want[k][tuple(bad[0])])
    assert want["char_stats"][:5].sum() == 0 and want["char_stats"].shape == (V, 5)
    only = M.edit_stats(dp, dr, SPECIAL, V, ops=False)                              # the distance-only instance
    assert set(only) == {"dist", "ref_len", "pred_len"}
    for k in only:
        assert torch.equal(only[k], got[k]), (tag, "distance-only", k)
    return want, got


@pytest.mark.parametrize("seed", [1, 2])
def test_lengths_grid_equals_the_reference(seed):
    pred, ref = _grid(seed)
    want, _ = _check(("grid", seed), pred, ref)
    seen = set(zip(want["ref_len"].tolist(), want["pred_len"].tolist()))
    assert {(m, n) for m in LENGTHS for n in LENGTHS} <= seen
    cer = M.cer_values(want["dist"], want["ref_len"], want["pred_len"])
    assert max(cer) > 1.0 and min(cer) == 0.0
    assert want["ops"][:, 1:].max(axis=0).min() > 0                                  # substitutions, deletions and insertions all occur


@pytest.mark.parametrize("seed", [3, 4])
@pytest.mark.parametrize("n", [1, 3, 5])
def test_partial_workgroups_and_rows_inside_wider_buffers(n, seed):
    rng = np.random.default_rng(100 * n + seed)
    pred, _ = _short(n, 33, 30, seed=int(rng.integers(1 << 30)), lo=5, hi=12)        # one small alphabet on both sides
    _, ref = _short(n, 70, 66, seed=int(rng.integers(1 << 30)), lo=5, hi=12)
    _check(("wide", n, seed), pred, ref, ld=160)


@pytest.mark.parametrize("seed", [5, 6])
def test_more_waves_than_fit_at_once(seed):
    pred, ref = _short(1100, 16, 12, seed=seed)
    want, _ = _check(("many", seed), pred, ref)
    assert want["dist"].max() > 0


def test_char_stats_accumulate_over_calls():
    pred, ref = _short(202, 24, 20, seed=7)
    whole = M.edit_stats_reference(pred, ref, SPECIAL, V, char_stats=True)["char_stats"]
    dp, dr = torch.from_numpy(pred).cuda(), torch.from_numpy(ref).cuda()
    table = torch.zeros(V, 5, dtype=torch.int32, device="cuda")
    a = M.edit_stats(dp[:101], dr[:101], SPECIAL, V, char_stats=table)
    first = table.cpu().numpy().copy()
    b = M.edit_stats(dp[101:], dr[101:], SPECIAL, V, char_stats=table)
    assert a["char_stats"] is table and b["char_stats"] is table
    assert np.array_equal(first, M.edit_stats_reference(pred[:101], ref[:101], SPECIAL, V, char_stats=True)["char_stats"])
    assert np.array_equal(table.cpu().numpy(), whole)
    assert np.array_equal(M.edit_stats(dp, dr, SPECIAL, V, char_stats=True)["char_stats"].cpu().numpy(), whole)
    # a given table is a base for the reference too
    assert np.array_equal(M.edit_stats_reference(pred[101:], ref[101:], SPECIAL, V, char_stats=first)["char_stats"], whole)
    assert M.edit_stats(dp[:0], dr[:0], SPECIAL, V)["dist"].numel() == 0             # no pairs: no launch, empty results


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted(tmp_path_factory):
    g, cfg, sd, data = load_trained()
    m = TrOCRModel(cfg.encoder_config_dict(), build_decoder_dir(str(tmp_path_factory.mktemp("dec")), cfg), load_tokenizer=True)
    m.load_state_dict(sd, strict=True)
    m.eval()
    px = torch.from_numpy(np.concatenate([data["fit"][0], data["unseen"][0]]))
    lab = np.concatenate([data["fit"][1], data["unseen"][1]]).copy()
    assert px.shape[0] == 12
    # perturb the labels of some fitted lines so that errors of every kind exist whatever the model reads: a character replaced, the
    # first one removed, the first one doubled
    pad = cfg.pad_id
    lab[1, 1] = 5 + (lab[1, 1] - 5 + 1) % (cfg.vocab - 5)
    lab[2, :-1] = lab[2, 1:]; lab[2, -1] = pad
    lab[3, 1:] = lab[3, :-1]
    return m, cfg, px, torch.from_numpy(lab), int(g["label_len"])


def _string_path(m, gen, lab):
    preds = m.tokenizer.batch_decode(gen, skip_special_tokens=True)
    tgts = m.tokenizer.batch_decode(lab, skip_special_tokens=True)
    return [m.calculate_cer(p, t) for p, t in zip(preds, tgts)], preds, tgts


@pytest.mark.parametrize("beams", [1, 4])
def test_evaluate_many_equals_the_string_path(fitted, beams):
    m, cfg, px, lab, Lh = fitted
    assert m.one_char_tokenizer
    gen = m.generate_stream(px, max_length=Lh, slots=5, num_beams=beams)
    want, preds, tgts = _string_path(m, gen, lab)
    ev = m.evaluate_many(px, lab, num_beams=beams, max_length=Lh, slots=5)
    assert torch.equal(ev["ids"], gen)
    assert ev["per_line"]["cer"].tolist() == want and ev["cer"] == sum(want) / len(want)
    assert max(want) > 0.0, "the perturbed labels must produce errors"
    assert m.cer_of(gen, lab) == want
    assert m.cer_of(gen.cpu().numpy(), lab.numpy()) == want
    # the rest of the report, from the same integers
    pl = ev["per_line"]
    assert pl["ref_len"].tolist() == [len(t) for t in tgts] and pl["pred_len"].tolist() == [len(p) for p in preds]
    assert ev["ref_chars"] == sum(map(len, tgts)) and ev["cer_corpus"] == int(pl["dist"].sum()) / ev["ref_chars"]
    assert ev["substitutions"] + ev["deletions"] + ev["insertions"] == int(pl["dist"].sum())
    assert ev["exact"] == sum(1 for p, t in zip(preds, tgts) if p == t) / len(tgts)
    ref = M.edit_stats_reference(gen, lab, m.tokenizer.all_special_ids, cfg.vocab, char_stats=True)
    assert ev["characters"] == M.character_table(ref["char_stats"], m.tokenizer, top=20) and ev["characters"]
    assert np.array_equal(pl["ops"], ref["ops"])
    errs = [r["substituted"] + r["deleted"] + r["inserted"] for r in ev["characters"]]
    assert errs == sorted(errs, reverse=True) and all(len(r["char"]) == 1 for r in ev["characters"])


def test_trainer_test_reports_the_same_cer_on_both_paths(fitted, monkeypatch):
    from kzv import trainer as T
    m, cfg, px, lab, Lh = fitted
    loader = [{"pixel_values": px[:6], "labels": lab[:6]}, {"pixel_values": px[6:], "labels": lab[6:]}]
    lines = []
    m._one_char = None
    dev = T.test(m, loader, log=lines.append, stream_decode=True)
    dev_logged = list(m.logged["test_cer_greedy"])
    assert m.one_char_tokenizer and len(lines) == 2 and lines[1].startswith("edits S ") and "corpus CER" in lines[1]
    monkeypatch.setattr(M, "is_one_char_tokenizer", lambda tok: False)
    m._one_char = None
    lines2 = []
    host = T.test(m, loader, log=lines2.append, stream_decode=True)
    assert not m.one_char_tokenizer and len(lines2) == 1
    m._one_char = None
    assert list(dev) == list(host) == ["test_loss", "test_cer", "test_cer_greedy"]
    assert dev["test_cer_greedy"] == host["test_cer_greedy"] and dev["test_cer"] == host["test_cer"]
    assert dev_logged == m.logged["test_cer_greedy"] and len(dev_logged) == 12 and max(dev_logged) > 0.0
    # test_loss comes from two separate forward passes whose loss is a float-atomic sum over workgroups: not this feature's number
    assert dev["test_loss"] == pytest.approx(host["test_loss"], rel=1e-5)
    assert lines[0].split()[2:] == lines2[0].split()[2:]
