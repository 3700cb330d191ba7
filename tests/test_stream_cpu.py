"""Slot-refill greedy decoding (kzv/stream.py, include/kzv.h: kzv_stream_*), the parts that need no GPU:

  * greedy_stream over a seeded fake decoder whose logits depend only on (image, prefix): per image the tokens of beam.greedy run on
    that image alone -- more images than slots, fewer images than slots, as many; with limits, the same rows cut at the limit; ended
    slots are given the waiting images in ascending slot order; the steps stay within the list-scheduling bound;
  * the ABI: the query before kzv_model_bind is a state error that names itself; kzv_stream_begin refuses a null out_ids, max_len < 2
    and a wave larger than its pool as argument errors before it touches the device (this machine has none: a launch would have been
    a HIP error instead).  The pool-smaller-than-the-slots refusal needs a bound handle: tests/test_stream_gpu.py."""
import ctypes as C
import os
import zlib

import pytest
import torch

from kzv import _lib as L
from kzv import beam as BM
from kzv import stream as ST
from kzv.config import tiny_config

PAD, BOS, EOS, V, LMAX = 1, 2, 3, 11, 14


def _logits(image: int, prefix) -> torch.Tensor:
    """[V] logits of (image, prefix): seeded by both, so that any schedule must see the same numbers."""
    g = torch.Generator().manual_seed(zlib.crc32(repr((int(image), [int(x) for x in prefix])).encode()))
    x = torch.randn(V, generator=g)
    x[PAD] = -10.0                               # a greedy prefix holds no padding
    return x


def _step_fn(seen=None):
    def step(st):
        out = torch.zeros(st["slot_image"].numel(), V)
        for b, (i, t) in enumerate(zip(st["slot_image"].tolist(), st["slot_t"].tolist())):
            if i >= 0:
                prefix = st["out_ids"][i, :t + 1]
                assert int(st["tokens"][b]) == int(prefix[-1]) and int(st["posids"][b]) == t + 1 + PAD
                out[b] = _logits(i, prefix)
        if seen is not None:
            seen.append(st["slot_image"].clone())
        return out
    return step


def _alone(image: int, limit=None) -> torch.Tensor:
    ids = BM.greedy(lambda t, ids: _logits(image, ids[0, :t + 1]).view(1, V), 1, LMAX, PAD, BOS, EOS, "cpu")
    row = torch.full((LMAX,), PAD, dtype=torch.int64)
    row[:ids.shape[1]] = ids[0]
    if limit is not None:
        row[limit:] = PAD
    return row


@pytest.mark.parametrize("n,slots", [(23, 4), (3, 8), (5, 5)])
def test_stream_equals_each_image_alone(n, slots):
    out, st = ST.greedy_stream(_step_fn(), n, slots, LMAX, PAD, BOS, EOS, "cpu", return_state=True)
    want = torch.stack([_alone(i) for i in range(n)])
    assert torch.equal(out, want)
    lengths = (want != PAD).sum(1)
    assert lengths.min() < LMAX and (want == EOS).any(), "the fake decoder must end some lines by EOS"
    c = st["counters"].tolist()
    assert c[0] == n and c[1] == n
    assert c[2] <= ST.step_bound(n, slots, LMAX)
    assert c[2] >= int(lengths.max()) - 1                   # no fewer steps than the longest line
    assert (st["slot_image"] == -1).all()


def test_limits_cut_the_same_rows():
    n, slots = 23, 4
    g = torch.Generator().manual_seed(5)
    limits = torch.randint(2, LMAX + 1, (n,), generator=g)
    limits[0], limits[1] = 2, LMAX
    out, lp = ST.greedy_stream(_step_fn(), n, slots, LMAX, PAD, BOS, EOS, "cpu", limits=limits, return_logprobs=True)
    want = torch.stack([_alone(i, int(limits[i])) for i in range(n)])
    assert torch.equal(out, want)
    for i in range(n):                                       # log-probabilities sit at the emitted tokens' columns, nowhere else
        k = int((want[i] != PAD).sum())
        for j in range(1, k):
            ref = torch.log_softmax(_logits(i, want[i, :j]), -1)[want[i, j]]
            assert abs(float(lp[i, j]) - float(ref)) < 1e-6
        assert (lp[i, k:] == 0).all() and lp[i, 0] == 0


def test_seats_are_given_in_ascending_slot_order():
    n, slots = 23, 4
    seen = []
    ST.greedy_stream(_step_fn(seen), n, slots, LMAX, PAD, BOS, EOS, "cpu", poll=1)
    assert seen[0].tolist() == [0, 1, 2, 3]
    nxt = slots
    for before, after in zip(seen, seen[1:]):
        changed = [b for b in range(slots) if int(after[b]) != int(before[b])]
        for b in changed:                                    # ascending slots take ascending images; once none is left, -1
            if nxt < n:
                assert int(after[b]) == nxt
                nxt += 1
            else:
                assert int(after[b]) == -1
    assert nxt == n


def test_first_maximum_wins_ties():
    st = ST.new_state(2, 2, 6, PAD, BOS, "cpu", want_logprobs=True)
    x = torch.zeros(2, V)
    x[0, 5] = x[0, 7] = 2.0
    x[1, EOS] = x[1, 9] = 2.0                                # EOS is column 3: it wins and the line ends
    st = ST.select_seat(x, st, n_images=2, max_len=6, pad_id=PAD, bos_id=BOS, eos_id=EOS)
    assert st["out_ids"][:, 1].tolist() == [5, EOS]
    assert st["slot_image"].tolist() == [0, -1] and st["slot_t"].tolist() == [1, 0]
    assert st["tokens"].tolist() == [5, BOS] and st["posids"].tolist() == [2 + PAD, PAD + 1]
    assert st["counters"].tolist() == [2, 1, 1]


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


def test_query_before_bind_is_an_error(lib):
    h = _handle(lib)
    try:
        assert lib.kzv_stream_decode_impl(h) == -3           # KZV_E_STATE
        assert b"stream_decode_impl" in lib.kzv_last_error()
        assert lib.kzv_stream_decode_impl(None) < 0
        for fn in (lib.kzv_stream_start, ):
            assert fn(h, None) == -3
        assert lib.kzv_stream_step(h, 0, None) == -3 and b"stream_step" in lib.kzv_last_error()
    finally:
        lib.kzv_model_destroy(h)


def test_begin_refuses_bad_arguments_without_a_launch(lib):
    h = _handle(lib)
    out = 4096                                               # never dereferenced: only its presence is checked
    try:
        assert lib.kzv_stream_begin(h, 8, 8, 16, BOS, EOS, None, 16, None, 0, None, None) == -1
        assert b"stream_begin" in lib.kzv_last_error() and b"out_ids" in lib.kzv_last_error()
        assert lib.kzv_stream_begin(h, 8, 8, 1, BOS, EOS, out, 16, None, 0, None, None) == -1
        assert b"max_len" in lib.kzv_last_error()
        assert lib.kzv_stream_begin(h, 4, 8, 16, BOS, EOS, out, 16, None, 0, None, None) == -1       # a wave larger than its pool
        assert b"pool" in lib.kzv_last_error()
        assert lib.kzv_stream_begin(h, 8, 8, 16, BOS, EOS, out, 8, None, 0, None, None) == -1        # rows shorter than max_len
        assert lib.kzv_stream_begin(h, 8, 8, 16, BOS, EOS, out, 16, None, 0, None, None) == -3       # well-formed, but not bound
        # the bookkeeping entry by itself: the same refusals, before its launches
        st = L.kzv_stream_state(slots=4, n_images=8, max_len=16, vocab=V, bos_id=BOS, eos_id=EOS, pad_id=PAD, slot_image=out, slot_t=out,
                                tokens=out, posids=out, counters=out, scratch=out, out_ids=None, ld_ids=16)
        assert lib.kzv_stream_update(C.byref(st), out, V, None) == -1 and b"out_ids" in lib.kzv_last_error()
        st.out_ids, st.max_len = out, 1
        assert lib.kzv_stream_seat_first(C.byref(st), None) == -1 and b"max_len" in lib.kzv_last_error()
        st.max_len = 16
        assert lib.kzv_stream_update(C.byref(st), out, V - 1, None) == -1                            # ld < vocab
        assert lib.kzv_stream_update(None, out, V, None) == -1
    finally:
        lib.kzv_model_destroy(h)
