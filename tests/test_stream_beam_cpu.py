"""Beam search on device-refilled slots (kzv/stream.py: beam_stream / beam_select_seat, include/kzv.h: kzv_stream_begin_beams, kzv_stream_beam_*),
the parts that need no GPU:

  * beam_stream over the seeded fake decoder of tests/test_stream_cpu.py (logits depend only on (image, prefix); V = 11, max length 14, 23
    images) equals beam.beam_search run on each image ALONE, token for token, and its scores equal the alone search's best finished score
    bit for bit -- nb in {2, 4} x early_stopping x length_penalty in {1.0, 0.6} x (more images than slots, fewer, as many); with limits,
    each image against beam_search(max_len = limit); ended slots are given the waiting images in ascending slot order; the steps stay
    within the list-scheduling bound; a running continuation that takes pad_id is counted;
  * the condition the comparison needs, asserted on the alone searches before any stream runs: at least a quarter of the searches end
    before the last possible step (LMAX - 1 = 13) and at least one runs to the length cap.  Observed (searches of 23 ending early / at
    the cap, fewest steps), per (nb, early_stopping, length_penalty): (2, T, 1.0) 17 / 6, 3; (2, T, 0.6) 17 / 6, 3; (2, F, 1.0) 14 / 9, 4;
    (2, F, 0.6) 17 / 6, 4; (4, T, 1.0) 19 / 4, 3; (4, T, 0.6) 19 / 4, 3; (4, F, 1.0) 3 / 20, 4; (4, F, 0.6) 18 / 5, 4 -- 124 of 184 early.
    Seven cells hold a quarter each; without early stopping four beams at length_penalty 1.0 keep searching to the cap on 20 of 23 images
    (that is the reference's own behaviour on these inputs), so the quarter is asserted over the searches of the whole grid, and every cell
    must still hold both kinds;
  * the ABI: kzv_stream_begin_beams and the per-op entries refuse bad arguments before they touch the device (this machine has none).
"""
import ctypes as C
import os
import zlib

import pytest
import torch

from kzv import _lib as L
from kzv import beam as BM
from kzv import stream as ST
from kzv.config import tiny_config

PAD, BOS, EOS, V, LMAX, N = 1, 2, 3, 11, 14, 23
GRID = [(nb, early, lp) for nb in (2, 4) for early in (True, False) for lp in (1.0, 0.6)]


def _logits(image: int, prefix) -> torch.Tensor:
    """[V] logits of (image, prefix): the fake decoder of tests/test_stream_cpu.py, seed for seed."""
    g = torch.Generator().manual_seed(zlib.crc32(repr((int(image), [int(x) for x in prefix])).encode()))
    x = torch.randn(V, generator=g)
    x[PAD] = -10.0
    return x


def _step_fn(nb, seen=None):
    def step(st):
        slots = st["slot_image"].numel()
        out = torch.zeros(slots * nb, V)
        for s, (i, t) in enumerate(zip(st["slot_image"].tolist(), st["slot_t"].tolist())):
            if i < 0:
                continue
            for k in range(nb):
                prefix = st["run_seq"][s, k, :t + 1]
                assert int(st["tokens"][s * nb + k]) == int(prefix[-1]) and int(st["posids"][s * nb + k]) == t + 1 + PAD
                out[s * nb + k] = _logits(i, prefix)
        if seen is not None:
            seen.append(st["slot_image"].clone())
        return out
    return step


_ALONE = {}


def _alone(image, nb, early, lp, max_len=LMAX):
    """(row padded to LMAX, best finished score, steps) of beam_search on one image; computed once per case."""
    key = (image, nb, early, lp, max_len)
    if key not in _ALONE:
        steps, score = [0], {}

        def step(t, ids):
            steps[0] += 1
            return torch.stack([_logits(image, ids[r, :t + 1]) for r in range(nb)])

        def topk(raw, run_sc):                                   # the torch expression of beam_search, kept to read the final scores off
            acc = torch.log_softmax(raw.float(), dim=-1).view(1, nb, V) + run_sc.unsqueeze(-1)
            return acc.view(1, nb * V).topk(2 * nb, dim=1)

        ids = BM.beam_search(step, lambda rows, t: None, 1, nb, max_len, V, PAD, BOS, EOS, "cpu", early_stopping=early, length_penalty=lp, topk=topk)
        row = torch.full((LMAX,), PAD, dtype=torch.int64)
        row[:ids.shape[1]] = ids[0]
        _ALONE[key] = (row, _score_of(image, row, lp), steps[0])
    return _ALONE[key]


def _score_of(image, row, lp):
    """sum log p / generated length ** length_penalty of a finished row, accumulated in fp32 in beam_search's order."""
    n = int((row != PAD).sum())
    acc = torch.zeros((), dtype=torch.float32)
    for j in range(1, n):
        acc = torch.log_softmax(_logits(image, row[:j]).float(), -1)[row[j]] + acc
    return acc / ST.divisor_table(LMAX, lp)[n - 1]


@pytest.mark.parametrize("n,slots", [(23, 4), (3, 8), (5, 5)])
@pytest.mark.parametrize("nb,early,lp", GRID)
def test_beam_stream_equals_each_image_alone(nb, early, lp, n, slots):
    want = [_alone(i, nb, early, lp) for i in range(N)]
    ends = [w[2] for w in want]
    pool = [_alone(i, *cell)[2] for cell in GRID for i in range(N)]
    assert sum(e < LMAX - 1 for e in pool) * 4 >= len(pool) and any(e == LMAX - 1 for e in pool), pool
    assert any(e < LMAX - 1 for e in ends) and any(e == LMAX - 1 for e in ends), ends
    (out, score), st = ST.beam_stream(_step_fn(nb), n, slots, nb, LMAX, V, PAD, BOS, EOS, "cpu", early_stopping=early, length_penalty=lp,
                                      return_state=True)
    assert torch.equal(out, torch.stack([w[0] for w in want[:n]]))
    assert torch.equal(score, torch.stack([w[1] for w in want[:n]]))
    c = st["counters"].tolist()
    assert c[0] == n and c[1] == n and c[3] == 0
    assert max(ends[:n]) <= c[2] <= ST.step_bound(n, slots, LMAX)
    assert (st["slot_image"] == -1).all()


@pytest.mark.parametrize("nb", [2, 4])
def test_limits_are_each_image_at_its_own_max_len(nb):
    n, slots = N, 4
    g = torch.Generator().manual_seed(5)
    limits = torch.randint(2, LMAX + 1, (n,), generator=g)
    limits[0], limits[1] = 2, LMAX
    out, score = ST.beam_stream(_step_fn(nb), n, slots, nb, LMAX, V, PAD, BOS, EOS, "cpu", limits=limits)
    for i in range(n):
        row, sc, _ = _alone(i, nb, True, 1.0, int(limits[i]))
        assert torch.equal(out[i], row), i
        assert torch.equal(score[i], sc), i
        assert int((out[i] != PAD).sum()) <= int(limits[i])


def test_seats_are_given_in_ascending_slot_order():
    n, slots, nb = N, 4, 4
    seen = []
    ST.beam_stream(_step_fn(nb, seen), n, slots, nb, LMAX, V, PAD, BOS, EOS, "cpu", poll=1)
    assert seen[0].tolist() == [0, 1, 2, 3]
    nxt = slots
    for before, after in zip(seen, seen[1:]):
        for b in [b for b in range(slots) if int(after[b]) != int(before[b])]:
            if nxt < n:
                assert int(after[b]) == nxt
                nxt += 1
            else:
                assert int(after[b]) == -1
    assert nxt == n


def test_a_running_beam_that_takes_padding_is_counted():
    nb, Lm = 2, 6
    st = ST.new_beam_state(3, 2, nb, Lm, PAD, BOS, "cpu")
    lp = torch.tensor([[-0.1, -0.2, -0.3, -0.4], [-0.1, -0.2, -0.3, -0.4]])
    ix = torch.tensor([[PAD, 5, 6, 7], [EOS, 5, PAD, 7]])       # slot 0: the best continuation is padding; slot 1: EOS, then 5, then padding
    st = ST.beam_select_seat(lp, ix, st, n_images=3, num_beams=nb, max_len=Lm, vocab=V, pad_id=PAD, bos_id=BOS, eos_id=EOS)
    assert st["counters"].tolist() == [2, 0, 1, 2]
    assert st["tokens"].tolist() == [PAD, 5, 5, PAD] and st["slot_t"].tolist() == [1, 1]
    assert st["run_seq"][0, :, :2].tolist() == [[BOS, PAD], [BOS, 5]]
    assert st["fin_done"].tolist() == [[0, 0], [1, 0]] and st["fin_len"][1, 0] == 2
    assert float(st["fin_sc"][1, 0]) == pytest.approx(-0.1)


def test_ties_rank_by_the_smaller_index_and_an_ended_slot_is_reseated_clean():
    nb, Lm = 2, 5
    st = ST.new_beam_state(3, 2, nb, Lm, PAD, BOS, "cpu")
    lp = torch.tensor([[-0.5, -0.5, -0.5, -0.5], [-0.1, -0.2, -0.3, -0.4]])
    ix = torch.tensor([[7, 5, 6, 8], [EOS, V + EOS, 5, 6]])     # slot 1: both first ranks stop -> its finished list is full: the search ends
    st = ST.beam_select_seat(lp, ix, st, n_images=3, num_beams=nb, max_len=Lm, vocab=V, pad_id=PAD, bos_id=BOS, eos_id=EOS)
    assert st["tokens"].tolist() == [7, 5, BOS, BOS]
    assert st["slot_image"].tolist() == [0, 2] and st["slot_t"].tolist() == [1, 0]
    assert st["out_ids"][1].tolist() == [BOS, EOS, PAD, PAD, PAD] and float(st["out_score"][1]) == pytest.approx(-0.1)
    assert st["run_sc"][1].tolist() == [0.0, ST.NEG] and st["fin_sc"][1].tolist() == [ST.NEG, ST.NEG]
    assert st["fin_done"][1].tolist() == [0, 0] and st["fin_len"][1].tolist() == [1, 1] and int(st["unsat"][1]) == 1
    assert st["posids"].tolist() == [2 + PAD, 2 + PAD, PAD + 1, PAD + 1]
    assert st["counters"].tolist() == [3, 1, 1, 0]


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load()


def _handle(lib):
    cfg = tiny_config()
    c = L.kzv_config(image_h=cfg.image_h, image_w=cfg.image_w, patch_h=cfg.patch_h, patch_w=cfg.patch_w, channels=cfg.channels,
                     enc_hidden=cfg.enc_hidden, enc_layers=cfg.enc_layers, enc_heads=cfg.enc_heads, enc_ffn=cfg.enc_ffn,
                     dec_hidden=cfg.dec_hidden, dec_layers=cfg.dec_layers, dec_heads=cfg.dec_heads, dec_ffn=cfg.dec_ffn,
                     vocab=cfg.vocab, max_pos=cfg.max_pos, type_vocab=cfg.type_vocab, pad_id=cfg.pad_id, ln_eps=1e-12)
    h = C.c_void_p()
    L.check(lib.kzv_model_create(C.byref(c), C.byref(h)), "create")
    return h


def test_begin_beams_refuses_bad_arguments_without_a_launch(lib):
    h = _handle(lib)
    out = 4096                                                   # never dereferenced: only its presence is checked
    try:
        begin = lambda nb, *rest: lib.kzv_stream_begin_beams(h, nb, 1, 1.0, None, *rest)
        assert begin(3, 8, 8, 16, BOS, EOS, out, 16, None, 0, None, None) == -1 and b"num_beams" in lib.kzv_last_error()
        assert begin(1, 8, 8, 16, BOS, EOS, out, 16, None, 0, None, None) == -1
        assert begin(4, 8, 8, 16, BOS, EOS, None, 16, None, 0, None, None) == -1 and b"out_ids" in lib.kzv_last_error()
        assert begin(4, 8, 8, 1, BOS, EOS, out, 16, None, 0, None, None) == -1 and b"max_len" in lib.kzv_last_error()
        assert begin(4, 4, 8, 16, BOS, EOS, out, 16, None, 0, None, None) == -1 and b"pool" in lib.kzv_last_error()
        assert begin(4, 8, 8, 16, BOS, EOS, out, 16, out, 16, None, None) == -1 and b"log-prob" in lib.kzv_last_error()
        assert begin(4, 8, 8, 16, BOS, EOS, out, 16, None, 0, None, None) == -3                     # well-formed, but not bound
        assert lib.kzv_stream_beam_impl(h, 4) == -3 and b"stream_beam_impl" in lib.kzv_last_error()
        assert lib.kzv_stream_beam_impl(None, 4) < 0
        c4 = C.c_int32(0)
        assert lib.kzv_stream_poll_beams(h, c4, c4, c4, None) == -3 and b"stream_poll_beams" in lib.kzv_last_error()
        # the bookkeeping entries by themselves: the same refusals, before their launches
        st = L.kzv_stream_beam_state(slots=4, n_images=8, num_beams=4, max_len=16, vocab=V, bos_id=BOS, eos_id=EOS, pad_id=PAD, early_stopping=1,
                                     slot_image=out, slot_t=out, tokens=out, posids=out, run_seq=out, fin_seq=out, run_scores=out, fin_scores=out,
                                     fin_done=out, fin_len=out, unsatisfied=out, counters=out, scratch=out, out_ids=None, ld_ids=16,
                                     divisors=out)
        assert lib.kzv_stream_beam_update(C.byref(st), out, out, None) == -1 and b"out_ids" in lib.kzv_last_error()
        st.out_ids, st.max_len = out, 1
        assert lib.kzv_stream_beam_seat_first(C.byref(st), None) == -1 and b"max_len" in lib.kzv_last_error()
        st.max_len, st.num_beams = 16, 3
        assert lib.kzv_stream_beam_update(C.byref(st), out, out, None) == -1 and b"num_beams" in lib.kzv_last_error()
        st.num_beams, st.divisors = 4, None
        assert lib.kzv_stream_beam_update(C.byref(st), out, out, None) == -1 and b"divisors" in lib.kzv_last_error()
        st.divisors, st.rows, st.ld_rows = out, out, 8
        assert lib.kzv_stream_beam_update(C.byref(st), out, out, None) == -1 and b"row table" in lib.kzv_last_error()
        st.ld_rows = 16
        assert lib.kzv_stream_beam_update(C.byref(st), None, out, None) == -1
        assert lib.kzv_stream_beam_update(None, out, out, None) == -1
    finally:
        lib.kzv_model_destroy(h)
