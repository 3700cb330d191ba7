"""The attention checker of tests/_attn_emul.py proves itself without a GPU: the emulation stays inside the bound it defines, the
input recipes do what they promise, and every mistake of the list below, planted into the EMULATION (never into a kernel), lands
outside the bound on every (batch, head) unit by a factor >= 3.  The cases are those of tests/test_attention_peaked_gpu.py (the
streaming ones up to 385 keys) at 4 units instead of 8; the dropout masks are oracle/attn_dropout.py's.

Mutants: forward softmax scale x 0.5; backward softmax scale x 0.5; alpha = 1 (streaming, more than one key block, on flat / sharp /
rise); delta omitted; 1 / P(keep) omitted from dP (dropout); LSE from the dropped probabilities (dropout); the causal diagonal off by
one either way and pad keys unmasked (mode 1).  ``alpha = 1`` on ``fall`` is left out on purpose: the maximum sits in the first block,
so the correction it skips is (nearly) 1 and the mutant computes the right thing.  A delta wrong by x 0.9 is only 1 - 4 bounds away on
``flat``: the resolution limit of this bound, not tested for."""
import functools

import pytest
import torch

import _attn_emul as E
from oracle import attn_dropout as AD

DROPS = (0.0, 0.1)
CPU_CASES = [c for c in E.all_cases() if not (c[0] == "stream" and c[4] > 385)]
FAMILIES = sorted({(fam, D, mode) for fam, D, mode, _, _ in CPU_CASES})


def _ids(c):
    return f"{c[0]}-d{c[1]}-m{c[2]}-{c[3]}x{c[4]}"


def _geometry(mode):
    return (2, 2) if mode == 1 else (1, 4)          # the pad tails of mode 1 differ per image; 4 units: the whole sharp ladder


@functools.lru_cache(maxsize=None)
def _inputs(fam, D, mode, Sq, Sk, kind, drop):
    B, heads = _geometry(mode)
    gen = torch.Generator().manual_seed(E.case_seed(D, mode, Sq, Sk))
    q, k, v, do = E.operands(kind, B, heads, Sq, Sk, D, gen)
    ids = E.pad_tail_ids(B, Sk, gen) if mode == 1 else None
    mult = None
    if drop > 0:
        mult = torch.from_numpy(AD.multiplier(E.drop_key(Sq, Sk), drop, B * heads, Sq, Sk)).view(B, heads, Sq, Sk)
    return q, k, v, do, ids, mult


@functools.lru_cache(maxsize=None)
def _clean(fam, D, mode, Sq, Sk, kind, drop):
    """(reference, emulation, bound, err_ref) of one case: computed once, shared by every test, never modified."""
    q, k, v, do, ids, mult = _inputs(fam, D, mode, Sq, Sk, kind, drop)
    mask = E.causal_pad_mask(ids, Sq, Sk) if mode == 1 else None
    scale = E.softmax_scale(D)
    ref = E.ref64(q, k, v, do, scale, mask, mult)
    emu = E.emulate(fam, q, k, v, do, scale, mask, mult)
    tol, er = E.bounds(emu, ref)
    return ref, emu, tol, er


@pytest.mark.parametrize("case", CPU_CASES, ids=_ids)
def test_the_emulation_is_within_half_its_own_bound(case):
    """Trivially true at MARGIN, so asserted at 0.5 x bound = max(err_ref, floor): a NaN, an inf or a shape mistake in the helper
    shows here.  Prints err_ref as a fraction of the unit's largest entry."""
    for kind in E.KINDS:
        for drop in DROPS:
            ref, emu, tol, er = _clean(*case, kind, drop)
            frac = {}
            for k in E.OUTPUTS:
                assert torch.isfinite(emu[k]).all() and torch.isfinite(ref[k]).all(), (kind, drop, k)
                assert bool((E.unit_max(emu[k].double() - ref[k]) <= 0.5 * tol[k]).all()), (kind, drop, k)
                frac[k] = float((er[k] / E.unit_max(ref[k]).clamp(min=1e-30)).max())
            print(f"{_ids(case)} {kind} p={drop}: err_ref / largest entry " + ", ".join(f"{k} {f:.2g}" for k, f in frac.items()))


LONG = [c for c in CPU_CASES if c[2] == 0 and c[4] >= 128 and c[3] >= 60]


@pytest.mark.parametrize("case", LONG, ids=_ids)
def test_sharp_is_sharp(case):
    """Mode 0 with at least 128 keys (a row of 9 or 37 keys cannot have a maximum below 0.05): the largest row maximum of P is
    >= 0.99, the median row maximum of the flattest unit is <= 0.05, and at least one unit has its largest |dQ| below 0.3: the small
    gradients that a bound of 0.03 x max(1, ...) cannot judge."""
    ref, _, _, _ = _clean(*case, "sharp", 0.0)
    rowmax = ref["P"].amax(-1)                                   # [B, heads, Sq]
    med = rowmax.flatten(2).median(-1).values
    dq = E.unit_max(ref["dQ"])
    print(f"{_ids(case)}: largest row max {float(rowmax.max()):.4f}, unit medians {[round(float(x), 3) for x in med.flatten()]}, "
          f"largest |dQ| per unit {[round(float(x), 3) for x in dq.flatten()]}")
    assert float(rowmax.max()) >= 0.99
    assert float(med.min()) <= 0.05
    assert float(dq.min()) < 0.3


MULTI = [c for c in CPU_CASES if c[0] == "stream" and c[4] > E.KB]


@pytest.mark.parametrize("case", MULTI, ids=_ids)
def test_rise_moves_the_max(case):
    """Streaming families, more than one key block: the median over rows of the smallest alpha (blocks after the first) is below
    0.1 on ``rise``; on ``fall`` it is 1 for most rows (which is why alpha = 1 is not a mutant there)."""
    _, emu, _, _ = _clean(*case, "rise", 0.0)
    med = float(emu["alpha_min"].flatten().median())
    _, emu_f, _, _ = _clean(*case, "fall", 0.0)
    print(f"{_ids(case)}: median over rows of min alpha: rise {med:.3g}, fall {float(emu_f['alpha_min'].flatten().median()):.3g}")
    assert med < 0.1


# ------------------------------------------------------------------------------------------------ mutants
def _mutant_cases(name, fam, D, mode):
    """(case, kind, drop) on which mutant ``name`` applies for family (fam, D, mode)."""
    out = []
    for c in CPU_CASES:
        if c[:3] != (fam, D, mode):
            continue
        for kind in E.KINDS:
            for drop in DROPS:
                if name in ("no_inv_keep", "lse_dropped") and drop == 0.0:
                    continue
                if name == "alpha1" and (fam != "stream" or c[4] <= E.KB or kind == "fall"):
                    continue
                if name in ("diag+1", "diag-1", "no_pad") and mode != 1:
                    continue
                out.append((c, kind, drop))
    return out


ALL_MUTANTS = E.MUTANTS + ("diag+1", "diag-1", "no_pad")


def _run_mutant(name, case, kind, drop):
    fam, D, mode, Sq, Sk = case
    q, k, v, do, ids, mult = _inputs(*case, kind, drop)
    scale = E.softmax_scale(D)
    if name in E.MUTANTS:
        mask = E.causal_pad_mask(ids, Sq, Sk) if mode == 1 else None
        return E.emulate(fam, q, k, v, do, scale, mask, mult, mutant=name)
    mask = {"diag+1": lambda: E.causal_pad_mask(ids, Sq, Sk, diag=1), "diag-1": lambda: E.causal_pad_mask(ids, Sq, Sk, diag=-1),
            "no_pad": lambda: E.causal_pad_mask(ids, Sq, Sk, pads=False)}[name]()
    return E.emulate(fam, q, k, v, do, scale, mask, mult)


@pytest.mark.parametrize("name", ALL_MUTANTS)
def test_mutants_of_the_emulation_are_flagged(name):
    """Per mutant and family one line: the minimum over the units of every applicable (case, kind, dropout) of the maximum over the
    outputs of error / bound (and the same without LSE, for the record).  Every line must be >= 3."""
    lines = []
    for fam, D, mode in FAMILIES:
        todo = _mutant_cases(name, fam, D, mode)
        if not todo:
            continue
        worst, worst_g, where = float("inf"), float("inf"), None
        for case, kind, drop in todo:
            ref, _, tol, _ = _clean(*case, kind, drop)
            mut = _run_mutant(name, case, kind, drop)
            ratio = {k: E.unit_max(mut[k].double() - ref[k]) / tol[k] for k in E.OUTPUTS}
            per_unit = torch.stack(list(ratio.values())).amax(0)
            grads = torch.stack([ratio[k] for k in E.OUTPUTS if k != "LSE"]).amax(0)
            if float(per_unit.min()) < worst:
                worst, where = float(per_unit.min()), (_ids(case), kind, drop)
            worst_g = min(worst_g, float(grads.min()))
        lines.append((f"{fam} d{D} mode {mode}", worst, worst_g, where, len(todo)))
    assert lines, name
    for fam, worst, worst_g, where, n in lines:
        print(f"mutant {name:12s} {fam:18s}: min over units of max over outputs of error / bound = {worst:8.3g} "
              f"(without LSE {worst_g:8.3g}) at {where}, {n} runs")
    for fam, worst, _, where, _ in lines:
        assert worst >= 3.0, (name, fam, worst, where)
