"""The top-k row reduction on the GPU (include/kzv.h: kzv_token_topk, kzv_stream_topk; csrc/token_topk.hip), op level.

kzv_token_topk against torch on the same fp32 rows: ids = the first k indices of torch.sort(descending=True, stable=True) (ties by
ascending column), log-probabilities = float64 log-softmax.  vocab 1 / 7 / 63 / 64 / 65 / 257 / 4300 with ld = vocab or padded to a
multiple of 64 (the scalar and the 16-byte path, a scalar tail, the project's vocabulary in its 4,352 stride; the padding holds 1e9:
a column read past `vocab` would win), rows 1 / 5 / 130 (partial workgroups), k 1 / 5 / 8 (k > vocab included).  Rows are randn plus
planted rows: the k largest values in consecutive columns and at column strides 4 / 64 / 256 (all winners in one lane's list,
whichever columns a lane owns), exact ties of the maximum and of ranks 2-4 across distant columns, an all-equal row, a row that is
-inf except for 3 columns.  ids exactly, surplus entries -1 / -inf, log-probabilities within 1e-4 where finite (the bound
tests/test_align_gpu.py::test_token_scores_of_the_fitted_model asserts for the same kind of reduction) and -inf exactly where the
reference is -inf.  The argument refusals return KZV_E_ARG without launching.

kzv_stream_topk on the harness of tests/test_stream_gpu.py::test_select_and_seat_kernels_equal_the_torch_statement (7 slots, 157
columns, 30 images, 12 output columns, limits, planted ties, EOS ties, mass endings): every step calls kzv_stream_topk and then
kzv_stream_update on the same logits; after every step the device arrays equal kzv/stream.py's statement (ids exactly,
log-probabilities to 1e-4) and alternative 0 equals out_ids at every written column."""
import ctypes as C

import pytest
import torch

from kzv import _lib as L
from kzv import stream as ST

pytestmark = pytest.mark.gpu
NEG = float("-inf")
KINDS = 9


def _plant(x, r, kind, k, g):
    """Row r of x [rows, vocab] (randn) becomes a planted row of `kind`; kinds that need more columns than there are stay randn."""
    V = x.shape[1]
    top = float(x[r].max())
    if kind == 1:                                            # the k largest in consecutive columns, in a random order of size
        n = min(k, V)
        c0 = int(torch.randint(0, V - n + 1, (1,), generator=g))
        x[r, c0:c0 + n] = top + 1.0 + torch.randperm(n, generator=g).float()
    elif kind in (2, 3, 4):                                  # ... at a column stride: one lane's columns on one of the two paths
        s = {2: 4, 3: 64, 4: 256}[kind]
        c0 = int(torch.randint(0, min(s, V), (1,), generator=g))
        cols = [c0 + j * s for j in range(k) if c0 + j * s < V]
        x[r, cols] = top + 1.0 + torch.randperm(len(cols), generator=g).float()
    elif kind == 5 and V >= 3:                               # the maximum three times, far apart: ascending columns
        cols = torch.tensor(sorted({0 if V < 8 else 3, V // 2, V - 1}))
        x[r, cols] = top + 1.0
    elif kind == 6 and V >= 7:                               # ranks 2-4 tied across distant columns under a single maximum
        x[r, V // 3] = top + 2.0
        x[r, torch.tensor([V - 2, 1, V // 2 + 1])] = top + 1.0
    elif kind == 7:                                          # an all-equal row: columns 0 .. k - 1
        x[r] = 0.75
    elif kind == 8:                                          # -inf except for 3 columns: the -inf columns follow by column
        keep = torch.randperm(V, generator=g)[:3]
        vals = x[r, keep].clone()
        x[r] = NEG
        x[r, keep] = vals


def _reference(x, k):
    V = x.shape[1]
    order = torch.sort(x, dim=-1, descending=True, stable=True).indices[:, :k]
    lp = torch.log_softmax(x.double(), -1).gather(1, order)
    ids = order.to(torch.int32)
    if V < k:
        ids = torch.cat((ids, torch.full((x.shape[0], k - V), -1, dtype=torch.int32)), 1)
        lp = torch.cat((lp, torch.full((x.shape[0], k - V), NEG, dtype=torch.float64)), 1)
    return ids, lp


def _run(buf, ld, rows, V, k):
    ids = torch.full((rows, k), -7, dtype=torch.int32, device="cuda")
    lp = torch.full((rows, k), 7.0, dtype=torch.float32, device="cuda")
    L.check(L.load().kzv_token_topk(buf.data_ptr(), ld, rows, V, k, ids.data_ptr(), lp.data_ptr(), L.stream_handle()), "token_topk")
    torch.cuda.synchronize()
    return ids.cpu(), lp.cpu()


def _compare(tag, got_ids, got_lp, x, k):
    want_ids, want_lp = _reference(x, k)
    assert torch.equal(got_ids, want_ids), (tag, (got_ids != want_ids).nonzero()[:4], got_ids[(got_ids != want_ids).any(1)][:2], want_ids[(got_ids != want_ids).any(1)][:2])
    inf = torch.isinf(want_lp)
    assert bool((got_lp[inf] == NEG).all()), tag
    assert bool(torch.isfinite(got_lp[~inf]).all()), tag
    return float((got_lp.double() - want_lp)[~inf].abs().max()) if bool((~inf).any()) else 0.0


@pytest.mark.parametrize("padded", [False, True], ids=["ld=vocab", "ld=64n"])
@pytest.mark.parametrize("V", [1, 7, 63, 64, 65, 257, 4300])
def test_token_topk_against_torch(V, padded):
    ld = -(-V // 64) * 64 if padded else V
    g = torch.Generator().manual_seed(1000 * V + padded)
    worst = 0.0
    for rows in (1, 5, 130):
        for k in (1, 5, 8):
            x = torch.randn(rows, V, generator=g)
            for r in range(rows):                            # 130 rows: every kind 14 times; 1 and 5 rows: kinds that move with k
                _plant(x, r, (r + k + rows) % KINDS, k, g)
            buf = torch.full((rows, ld), 1e9)
            buf[:, :V] = x
            got_ids, got_lp = _run(buf.cuda(), ld, rows, V, k)
            worst = max(worst, _compare((V, ld, rows, k), got_ids, got_lp, x, k))
            if V < k:
                assert bool((got_ids[:, V:] == -1).all()) and bool((got_lp[:, V:] == NEG).all())
            assert bool((got_ids[:, :min(k, V)] >= 0).all()) and bool((got_ids < V).all())
    print(f"vocab {V}, ld {ld}: largest |log-probability - float64 log-softmax| {worst:.2e}")
    assert worst <= 1e-4


def test_token_topk_every_kind_at_every_k_and_an_unaligned_base():
    """Each planted kind at each k on the project's vocabulary, 4,352 stride -- and the same rows from a base that is not 16-byte
    aligned (the scalar path over 4,300 columns).  Two runs give the same bits."""
    V, ld = 4300, 4352
    g = torch.Generator().manual_seed(77)
    for k in (1, 5, 8):
        x = torch.randn(KINDS, V, generator=g)
        for r in range(KINDS):
            _plant(x, r, r, k, g)
        flat = torch.full((KINDS * ld + 1,), 1e9)
        for off in (0, 1):
            view = flat[off:off + KINDS * ld].view(KINDS, ld)
            view[:, :V] = x
            view[:, V:] = 1e9
            dev = flat.cuda()
            buf = dev[off:off + KINDS * ld]
            assert (buf.data_ptr() % 16 == 0) == (off == 0)
            got_ids, got_lp = _run(buf, ld, KINDS, V, k)
            assert _compare((k, off), got_ids, got_lp, x, k) <= 1e-4
            again_ids, again_lp = _run(buf, ld, KINDS, V, k)
            assert torch.equal(got_ids, again_ids) and torch.equal(got_lp, again_lp)
    # -inf except 3 columns, k = 8: three finite candidates, then the first five -inf columns
    x = torch.full((1, V), NEG)
    x[0, [4000, 17, 2222]] = torch.tensor([0.5, 0.25, 1.0])
    got_ids, got_lp = _run(x.cuda(), V, 1, V, 8)
    assert got_ids.tolist() == [[2222, 4000, 17, 0, 1, 2, 3, 4]]
    assert bool((got_lp[0, 3:] == NEG).all()) and bool(torch.isfinite(got_lp[0, :3]).all())


def test_token_topk_rows_with_nan_keep_their_ids_in_range():
    V = 257
    x = torch.randn(9, V, generator=torch.Generator().manual_seed(5))
    x[0, 3] = x[1, 256] = x[2, 0] = float("nan")
    x[3] = float("nan")
    got_ids, _ = _run(x.cuda(), V, 9, V, 8)
    assert bool((got_ids >= -1).all()) and bool((got_ids < V).all())
    want_ids, _ = _reference(x[4:], 8)
    assert torch.equal(got_ids[4:], want_ids)


def test_token_topk_refuses_bad_arguments():
    lib = L.load()
    x = torch.zeros(4, 64, device="cuda")
    ids = torch.full((4, 8), -7, dtype=torch.int32, device="cuda")
    lp = torch.full((4, 8), 7.0, device="cuda")
    st = L.stream_handle()
    p, i, l = x.data_ptr(), ids.data_ptr(), lp.data_ptr()
    for why, args in {"null logits": (None, 64, 4, 64, 5, i, l), "null ids": (p, 64, 4, 64, 5, None, l), "null logprob": (p, 64, 4, 64, 5, i, None),
                      "k = 0": (p, 64, 4, 64, 0, i, l), "k = 9": (p, 64, 4, 64, 9, i, l), "vocab = 0": (p, 64, 4, 0, 5, i, l),
                      "ld < vocab": (p, 63, 4, 64, 5, i, l), "rows = 0": (p, 64, 0, 64, 5, i, l), "rows = 2^31": (p, 64, 1 << 31, 64, 5, i, l),
                      "rows < 0": (p, 64, -1, 64, 5, i, l)}.items():
        assert lib.kzv_token_topk(*args, st) == -1, why
        assert b"token_topk" in lib.kzv_last_error(), why
    torch.cuda.synchronize()
    assert bool((ids == -7).all()) and bool((lp == 7.0).all())          # nothing was launched


def test_stream_topk_kernel_equals_the_torch_statement():
    lib = L.load()
    slots, V, N, ML, pad, bos, eos, K = 7, 157, 30, 12, 1, 2, 3, 5
    g = torch.Generator().manual_seed(11)
    limits = torch.randint(2, ML + 1, (N,), generator=g, dtype=torch.int32)
    lim_d = limits.cuda()
    ref = ST.new_state(N, slots, ML, pad, bos, "cpu", want_logprobs=True, top_k=K)
    dev = {k: v.clone().cuda() for k, v in ref.items()}
    scratch = torch.zeros(2 * slots, dtype=torch.int32, device="cuda")
    st = L.kzv_stream_state(slots=slots, n_images=N, max_len=ML, vocab=V, bos_id=bos, eos_id=eos, pad_id=pad,
                            slot_image=dev["slot_image"].data_ptr(), slot_t=dev["slot_t"].data_ptr(), tokens=dev["tokens"].data_ptr(),
                            posids=dev["posids"].data_ptr(), counters=dev["counters"].data_ptr(), scratch=scratch.data_ptr(),
                            out_ids=dev["out_ids"].data_ptr(), ld_ids=ML, out_logprob=dev["out_logprob"].data_ptr(), ld_logprob=ML,
                            limit=lim_d.data_ptr())
    L.check(lib.kzv_stream_seat_first(C.byref(st), L.stream_handle()), "seat_first")
    alt_i, alt_l = dev["alt_ids"].data_ptr(), dev["alt_logprob"].data_ptr()
    # the refusals of kzv_token_topk, and rows too short for max_len * k entries
    xz = torch.zeros(slots, V, device="cuda")
    for why, args in {"k = 0": (C.byref(st), xz.data_ptr(), V, 0, alt_i, alt_l, ML * K), "k = 9": (C.byref(st), xz.data_ptr(), V, 9, alt_i, alt_l, ML * 9),
                      "null logits": (C.byref(st), None, V, K, alt_i, alt_l, ML * K), "null ids": (C.byref(st), xz.data_ptr(), V, K, None, alt_l, ML * K),
                      "null logprob": (C.byref(st), xz.data_ptr(), V, K, alt_i, None, ML * K), "ld < vocab": (C.byref(st), xz.data_ptr(), V - 1, K, alt_i, alt_l, ML * K),
                      "short rows": (C.byref(st), xz.data_ptr(), V, K, alt_i, alt_l, ML * K - 1), "null state": (None, xz.data_ptr(), V, K, alt_i, alt_l, ML * K)}.items():
        assert lib.kzv_stream_topk(*args, L.stream_handle()) == -1, why
    torch.cuda.synchronize()
    assert bool((dev["alt_ids"] == -1).all())
    worst, seen_tie, seen_eos, wrote = 0.0, 0, 0, torch.zeros(N, ML, dtype=torch.bool)
    for step in range(50):
        x = torch.randn(slots, V, generator=g)
        x[:, pad] = -20.0
        for b in range(slots):
            r = int(torch.randint(0, 6, (1,), generator=g))
            if r == 0:                                      # an exact tie of the maximum: the first column wins, the others follow by column
                cols = torch.randperm(V - 4, generator=g)[:3] + 4
                x[b, cols] = x[b].max() + 1.0
                seen_tie += 1
            elif r == 1:                                    # EOS as the maximum, tied with a later column
                x[b, eos] = x[b, 100] = x[b].max() + 0.5
                seen_eos += 1
        if step % 9 == 4:                                   # every live line ends in this step
            x[:, eos] = 50.0
        xd = x.cuda()
        for b in range(slots):
            if int(ref["slot_image"][b]) >= 0:
                wrote[int(ref["slot_image"][b]), int(ref["slot_t"][b]) + 1] = True
        L.check(lib.kzv_stream_topk(C.byref(st), xd.data_ptr(), V, K, alt_i, alt_l, ML * K, L.stream_handle()), "stream_topk")
        L.check(lib.kzv_stream_update(C.byref(st), xd.data_ptr(), V, L.stream_handle()), "stream_update")
        ref = ST.select_seat(x, ref, n_images=N, max_len=ML, pad_id=pad, bos_id=bos, eos_id=eos, limit=limits)
        for k in ("slot_image", "slot_t", "tokens", "posids", "counters", "out_ids", "alt_ids"):
            assert torch.equal(dev[k].cpu(), ref[k]), (step, k, dev[k].cpu(), ref[k])
        worst = max(worst, float((dev["alt_logprob"].cpu() - ref["alt_logprob"]).abs().max()))
        assert torch.equal(dev["alt_ids"].cpu()[..., 0][wrote].long(), dev["out_ids"].cpu()[wrote]), step
    assert ref["counters"].tolist()[:2] == [N, N] and (ref["slot_image"] == -1).all()
    assert seen_tie >= 5 and seen_eos >= 5
    got_i, got_l = dev["alt_ids"].cpu(), dev["alt_logprob"].cpu()
    assert bool((got_i[~wrote] == -1).all()) and bool((got_l[~wrote] == 0).all()) and bool((got_i[wrote] >= 0).all())
    assert not bool(wrote[:, 0].any()) and int(wrote.sum()) == int((ref["out_ids"][:, 1:] != pad).sum())
    lp0 = float((got_l[..., 0] - dev["out_logprob"].cpu())[wrote].abs().max())
    print(f"alternatives: largest difference to torch.log_softmax {worst:.2e}; entry 0 against out_logprob {lp0:.2e}")
    assert worst <= 1e-4 and lp0 <= 1e-4
