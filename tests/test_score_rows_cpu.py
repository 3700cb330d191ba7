"""The argument checks the three score-chain entries share (csrc/score_rows.h: score_rows_check, called by kzv_logits_process,
kzv_lm_fuse and kzv_force_prefix with their own checks around it).  Every refusal comes before any launch, so this runs without a GPU.

One bad argument at a time, taken from the lists of tests/test_controls_cpu.py, tests/test_lm_gpu.py and tests/test_prefix_cpu.py, and for
each the exact (return code, kzv_last_error) pair.  The expected texts are written out here as the entries' sources stated them BEFORE
the checks were shared (one kzv_fail per condition and entry, the entry's name spelled in each): nothing below is formatted by the code
under test.  With one condition violated the pair is fixed; with several at once only the code is (the message may be any of theirs),
which is why every case here violates exactly one.

The lockstep call with group = 0: kzv_force_prefix refuses it (the rows of an image form a group in every case); kzv_logits_process and
kzv_lm_fuse accept it, which needs a launch to show and is asserted in tests/test_stream_gpu.py.
"""
import ctypes as C
import os

import pytest

from kzv import _lib as L

P = 4096                     # a pointer that is never dereferenced: only its presence is checked
E_ARG = -1


def _lm(**kw):
    return C.pointer(L.kzv_ngram_lm(**dict(dict(order=1, vocab=41, uni=P), **kw)))


_ROWS = dict(logits=P, ld=48, rows=4, vocab=41, ids=P, ld_ids=16, t=3, group=1, slot_image=None, slot_t=None, by_image=0, n_images=0)
_SLOTS = dict(slot_image=P, slot_t=P, n_images=5)

ENTRIES = {
    "logits_process": dict(
        fn="kzv_logits_process", args=L.kzv_logits_process_args, calls="kzv_test_logits_process_calls",
        good=dict(_ROWS, no_repeat_ngram_size=2, min_length=0, eos_id=3, normalise=0, repetition_penalty=1.2, reserved=0, suppress_mask=None),
        null="logits_process: null arguments",
        bad=[
            (dict(logits=None), "logits_process: null logits / ids"),
            (dict(ids=None), "logits_process: null logits / ids"),
            (dict(rows=0), "logits_process: rows must be positive (got 0)"),
            (dict(vocab=0), "logits_process: vocab 0 outside 1..16384"),
            (dict(vocab=16385, ld=16388), "logits_process: vocab 16385 outside 1..16384"),
            (dict(ld=40), "logits_process: ld 40 < vocab 41"),
            (dict(ld_ids=0), "logits_process: ld_ids must be positive"),
            (dict(slot_image=P), "logits_process: slot_image and slot_t go together"),
            (dict(slot_t=P), "logits_process: slot_image and slot_t go together"),
            (dict(_SLOTS, group=3), "logits_process: 4 rows are no multiple of 3 rows per slot"),
            (dict(_SLOTS, group=0), "logits_process: 4 rows are no multiple of 0 rows per slot"),
            (dict(_SLOTS, n_images=0), "logits_process: n_images must be positive"),
            (dict(t=-1), "logits_process: step -1 is negative"),
            # the entry's own checks, around the shared block
            (dict(no_repeat_ngram_size=9), "logits_process: no_repeat_ngram_size 9 outside 0..8"),
            (dict(no_repeat_ngram_size=-1), "logits_process: no_repeat_ngram_size -1 outside 0..8"),
            (dict(repetition_penalty=0.0), "logits_process: repetition_penalty must be positive (got 0)"),
            (dict(repetition_penalty=-2.0), "logits_process: repetition_penalty must be positive (got -2)"),
            (dict(min_length=-1), "logits_process: min_length must not be negative"),
            (dict(min_length=2, eos_id=41), "logits_process: EOS 41 outside the vocabulary"),
        ]),
    "lm_fuse": dict(
        fn="kzv_lm_fuse", args=L.kzv_lm_fuse_args, calls="kzv_test_lm_fuse_calls",
        good=dict(_ROWS, weight=0.5, reserved=0, lm=_lm()),
        null="lm_fuse: null arguments",
        bad=[
            (dict(logits=None), "lm_fuse: null logits / ids"),
            (dict(ids=None), "lm_fuse: null logits / ids"),
            (dict(rows=0), "lm_fuse: rows must be positive (got 0)"),
            (dict(vocab=0), "lm_fuse: vocab 0 outside 1..16384"),
            (dict(vocab=16385, ld=16388), "lm_fuse: vocab 16385 outside 1..16384"),
            (dict(ld=40), "lm_fuse: ld 40 < vocab 41"),
            (dict(ld_ids=0), "lm_fuse: ld_ids must be positive"),
            (dict(slot_image=P), "lm_fuse: slot_image and slot_t go together"),
            (dict(slot_t=P), "lm_fuse: slot_image and slot_t go together"),
            (dict(_SLOTS, group=3), "lm_fuse: 4 rows are no multiple of 3 rows per slot"),
            (dict(_SLOTS, group=0), "lm_fuse: 4 rows are no multiple of 0 rows per slot"),
            (dict(_SLOTS, n_images=0), "lm_fuse: n_images must be positive"),
            (dict(t=-1), "lm_fuse: step -1 is negative"),
            (dict(lm=None), "lm_fuse: null language model"),
            (dict(lm=_lm(order=5)), "lm_fuse: order outside 1..4"),
            (dict(vocab=40), "lm_fuse: the language model's vocabulary differs from the scores'"),
            (dict(lm=_lm(uni=None)), "lm_fuse: null unigram table"),
            (dict(weight=float("nan")), "lm_fuse: the weight must be finite (got nan)"),
            (dict(weight=float("inf")), "lm_fuse: the weight must be finite (got inf)"),
        ]),
    "force_prefix": dict(
        fn="kzv_force_prefix", args=L.kzv_force_prefix_args, calls="kzv_test_force_prefix_calls",
        good=dict(logits=P, ld=45, rows=8, vocab=41, t=0, group=2, slot_image=None, slot_t=None, by_image=0, n_images=4, prefix=P, ld_prefix=3,
                  prefix_len=P, normalised=0, reserved=0, forced_logprob=None, ld_forced_logprob=0),
        null="force_prefix: null arguments",
        bad=[
            (dict(logits=None), "force_prefix: null logits"),
            (dict(rows=0), "force_prefix: rows must be positive (got 0)"),
            (dict(vocab=0), "force_prefix: vocab 0 outside 1..16384"),
            (dict(vocab=16385, ld=16400), "force_prefix: vocab 16385 outside 1..16384"),
            (dict(ld=40), "force_prefix: ld 40 < vocab 41"),
            (dict(group=0), "force_prefix: 8 rows are no multiple of 0 rows per image"),         # lockstep too: refused here, accepted by the other two
            (dict(group=3), "force_prefix: 8 rows are no multiple of 3 rows per image"),
            (dict(slot_image=P, slot_t=P, group=3), "force_prefix: 8 rows are no multiple of 3 rows per image"),
            (dict(slot_image=P), "force_prefix: slot_image and slot_t go together"),
            (dict(slot_t=P), "force_prefix: slot_image and slot_t go together"),
            (dict(slot_image=P, slot_t=P, n_images=0), "force_prefix: n_images must be positive"),
            (dict(t=-1), "force_prefix: step -1 is negative"),
            (dict(prefix=None), "force_prefix: null prefix / prefix_len"),
            (dict(prefix_len=None), "force_prefix: null prefix / prefix_len"),
            (dict(ld_prefix=0), "force_prefix: ld_prefix must be positive"),
            (dict(forced_logprob=P, ld_forced_logprob=3), "force_prefix: forced_logprob rows of 3 columns are shorter than BOS + the 3 prefix columns"),
        ]),
}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load()


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_one_bad_argument_gives_the_code_and_text_it_always_gave(lib, entry):
    e = ENTRIES[entry]
    fn, calls = getattr(lib, e["fn"]), getattr(lib, e["calls"])
    before = calls()
    for kw, text in e["bad"]:
        rc = fn(C.byref(e["args"](**dict(e["good"], **kw))), None)
        assert (rc, lib.kzv_last_error()) == (E_ARG, text.encode()), (entry, kw)
    assert (fn(None, None), lib.kzv_last_error()) == (E_ARG, e["null"].encode())
    assert calls() == before                     # nothing reached a launch
