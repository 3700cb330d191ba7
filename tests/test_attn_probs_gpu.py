"""kzv_attn_probs (csrc/attention_probs.hip) at the op level: head-averaged attention probabilities, their centroid, peak and row
sum, recomputed from bf16 Q, K and a forward's LSE, against an fp32 torch softmax of the SAME bf16 values averaged over heads.

LSE comes once from the engine's own forward on the same tensors (kzv_attn_fwd up to 288 keys, kzv_attn_stream_fwd beyond, as a
model does: the contract kzv_cross_attention relies on) and once from torch.logsumexp in fp32.  Both sides start from identical
operands; what differs is the fp32 summation order of 64 exact products and the exp: expected 1e-5, asserted 1e-4 absolute on the
map and on the row sum, 1e-4 of the grid extent on the centroids, and the same peak wherever the reference's two largest weights are
more than 2e-4 apart (at least 95 % of the rows; the reference alone is checked for that first).  Rows are peaked (every head of a
query looks at one key), so the median peak weight is above 0.2 as in a trained decoder.

Shapes, the smallest that reach every edge: B = 3 images; 1 and 4 heads (single and summed); Sq 1, 19, 127 (tails of the 16-row
tile, two workgroups per image); Sk 8 (one partial key tile), 160 (exact tiles), 257 (tile + 1), 1030 (many blocks); K inside a
wider buffer (ldk != heads * 64, as crosskv is); grid_w 4 and 40; float4 and scalar map rows; map == NULL."""
import ctypes as C

import numpy as np
import pytest
import torch

from kzv import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
TOL = 1e-4


@pytest.fixture(scope="module")
def lib():
    return L.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _operands(B, heads, Sq, Sk, seed):
    """bf16 Q [B, Sq, H], K, V [B, Sk, H] on the CPU: every head of query (b, q) is its target key's vector times 0.6 .. 1.2 plus
    half-size noise, so all heads peak on that key (scores ~ 8 a against N(0, a^2) elsewhere)."""
    gen = torch.Generator().manual_seed(seed)
    H = heads * 64
    K = torch.randn(B, Sk, H, generator=gen).bfloat16()
    V = torch.randn(B, Sk, H, generator=gen).bfloat16()
    tgt = torch.randint(0, Sk, (B, Sq), generator=gen)
    a = 0.6 + 0.6 * torch.rand(B, Sq, 1, generator=gen)
    Q = (a * (torch.gather(K.float(), 1, tgt[:, :, None].expand(B, Sq, H)) + 0.5 * torch.randn(B, Sq, H, generator=gen))).bfloat16()
    return Q, K, V


def _reference(Q, K, heads, grid_w):
    """fp32 softmax of the bf16 values, mean over heads; its centroid, peak, top-2 gap and fp32 log-sum-exp."""
    B, Sq, H = Q.shape
    Sk = K.shape[1]
    qh = Q.float().view(B, Sq, heads, 64).transpose(1, 2)
    kh = K.float().view(B, Sk, heads, 64).transpose(1, 2)
    s = qh @ kh.transpose(2, 3) * 0.125
    p = torch.softmax(s, -1).mean(1)                                      # [B, Sq, Sk]
    k = torch.arange(Sk)
    row, col = (k // grid_w).float(), (k % grid_w).float()
    top2 = torch.topk(p, min(2, Sk), dim=-1).values
    gap = top2[..., 0] - top2[..., 1] if Sk > 1 else torch.ones(B, Sq)
    return {"map": p, "row": (p * row).sum(-1), "col": (p * col).sum(-1), "peak_w": p.max(-1).values, "peak": p.argmax(-1),
            "gap": gap, "lse": torch.logsumexp(s, -1)}


class _Dev:
    """The operands as the model lays them out: Q in a [B * Sq, H + 8] buffer, K and V as column blocks of one
    [B * Sk, 2 H + 16] buffer starting at column 8 (ldk != heads * 64)."""

    def __init__(self, Q, K, V, heads):
        B, Sq, H = Q.shape
        Sk = K.shape[1]
        self.B, self.Sq, self.Sk, self.heads, self.H = B, Sq, Sk, heads, H
        self.q = torch.full((B * Sq, H + 8), NAN, dtype=torch.bfloat16, device=DEV)
        self.kv = torch.full((B * Sk, 2 * H + 16), NAN, dtype=torch.bfloat16, device=DEV)
        self.q[:, :H] = Q.reshape(B * Sq, H).to(DEV)
        self.kv[:, 8:8 + H] = K.reshape(B * Sk, H).to(DEV)
        self.kv[:, H + 8:2 * H + 8] = V.reshape(B * Sk, H).to(DEV)
        self.Q, self.K, self.V = self.q[:, :H], self.kv[:, 8:8 + H], self.kv[:, H + 8:2 * H + 8]
        self.ldq, self.ldk = H + 8, 2 * H + 16

    def engine_lse(self, lib):
        O = torch.empty(self.B * self.Sq, self.H, dtype=torch.bfloat16, device=DEV)
        lse = torch.full((self.B, self.heads, self.Sq), NAN, device=DEV)
        a = L.kzv_attn_args(Q=self.Q.data_ptr(), K=self.K.data_ptr(), V=self.V.data_ptr(), O=O.data_ptr(), LSE=lse.data_ptr(),
                            ldq=self.ldq, ldk=self.ldk, ldv=self.ldk, ldo=self.H, B=self.B, heads=self.heads, Sq=self.Sq, Sk=self.Sk,
                            mode=0, drop_p=0.0, drop_key=0, head_dim=64)
        if self.Sk <= 288:
            L.check(lib.kzv_attn_fwd(C.byref(a), _st()), "attn_fwd")
        else:
            L.check(lib.kzv_attn_stream_fwd(C.byref(a), _st()), "attn_stream_fwd")
        return lse

    def probs(self, lib, lse, grid_w, ld_map=None, **over):
        """-> (map [B, Sq, ld_map] or None, pos [B, Sq, 4], peak [B, Sq]); outputs start as NaN / -1."""
        amap = None if ld_map is None else torch.full((self.B, self.Sq, ld_map), NAN, device=DEV)
        pos = torch.full((self.B, self.Sq, 4), NAN, device=DEV)
        peak = torch.full((self.B, self.Sq), -1, dtype=torch.int32, device=DEV)
        a = L.kzv_attn_probs_args(Q=self.Q.data_ptr(), K=self.K.data_ptr(), ldq=self.ldq, ldk=self.ldk, LSE=lse.data_ptr(),
                                  map=None if amap is None else amap.data_ptr(), ld_map=ld_map or 0, pos=pos.data_ptr(), peak=peak.data_ptr(),
                                  B=self.B, heads=self.heads, Sq=self.Sq, Sk=self.Sk, grid_w=grid_w, head_dim=0, mode=0)
        for k, v in over.items():
            setattr(a, k, v)
        rc = lib.kzv_attn_probs(C.byref(a), _st())
        if over:
            return rc
        L.check(rc, "kzv_attn_probs")
        torch.cuda.synchronize()
        return amap, pos, peak


def _compare(tag, ref, amap, pos, peak, Sk, grid_w):
    assert bool(torch.isfinite(pos).all()) and int(peak.min()) >= 0 and int(peak.max()) < Sk, tag
    pos, peak = pos.cpu(), peak.cpu().long()
    figures = {}
    if amap is not None:
        assert bool(torch.isfinite(amap[..., :Sk]).all()), tag
        assert bool(torch.isnan(amap[..., Sk:]).all()), f"{tag}: columns past Sk were written"
        figures["map"] = float((amap[..., :Sk].cpu() - ref["map"]).abs().max())
    figures["sum"] = float((pos[..., 3] - 1).abs().max())
    figures["peak_w"] = float((pos[..., 2] - ref["peak_w"]).abs().max())
    n_rows = (Sk + grid_w - 1) // grid_w
    figures["row"] = float((pos[..., 0] - ref["row"]).abs().max()) / n_rows
    figures["col"] = float((pos[..., 1] - ref["col"]).abs().max()) / grid_w
    decided = ref["gap"] > 2e-4
    print(f"{tag}: " + " ".join(f"{k}={v:.3g}" for k, v in figures.items()) + f" decided={float(decided.float().mean()):.3f}")
    for k, v in figures.items():
        assert v <= TOL, (tag, k, v)
    assert bool((peak[decided] == ref["peak"][decided]).all()), tag


@pytest.mark.parametrize("Sk", [8, 160, 257, 1030])
@pytest.mark.parametrize("Sq", [1, 19, 127])
@pytest.mark.parametrize("heads", [1, 4])
def test_attn_probs_against_fp32_softmax(lib, heads, Sq, Sk):
    B = 3
    Q, K, V = _operands(B, heads, Sq, Sk, seed=1000 * heads + 10 * Sq + Sk)
    refs = {gw: _reference(Q, K, heads, gw) for gw in (4, 40)}
    ref = refs[4]
    # the reference alone: peaked rows, and decided peaks in at least 95 % of them
    assert float(ref["peak_w"].median()) > 0.2
    assert float((ref["gap"] > 2e-4).float().mean()) >= 0.95
    d = _Dev(Q, K, V, heads)
    lse_engine = d.engine_lse(lib)
    torch.cuda.synchronize()
    assert float((lse_engine.cpu() - ref["lse"]).abs().max()) < 1e-3           # the forward's LSE is the same quantity
    ld_vec = (Sk + 3) // 4 * 4 + 4                                                # float4 rows, with columns to spare
    ld_odd = Sk + 1 if (Sk + 1) % 4 else Sk + 2                                   # rows not 16-byte aligned: scalar stores
    for src, lse in (("engine LSE", lse_engine), ("torch LSE", ref["lse"].to(DEV).contiguous())):
        for gw, ld in ((4, ld_vec), (40, ld_odd)):
            amap, pos, peak = d.probs(lib, lse, gw, ld)
            _compare(f"h{heads} Sq{Sq} Sk{Sk} gw{gw} {src}", refs[gw], amap, pos, peak, Sk, gw)
            # map == NULL: the same pos / peak bit for bit (the same arithmetic, nothing of size Sk written), and again run to run
            _, pos0, peak0 = d.probs(lib, lse, gw, None)
            assert torch.equal(pos0, pos) and torch.equal(peak0, peak)
            amap2, pos2, peak2 = d.probs(lib, lse, gw, ld)
            assert torch.equal(amap2[..., :Sk], amap[..., :Sk]) and torch.equal(pos2, pos) and torch.equal(peak2, peak)


def test_first_argmax_and_rows_past_the_end_contribute_nothing(lib):
    """Identical keys give identical weights: the peak is the FIRST of them, also when the equal keys sit in different lanes,
    tiles and blocks; and the NaN padding behind the operands' last rows (the buffers are NaN-filled) reaches no output."""
    B, heads, Sq, Sk = 1, 2, 5, 200
    Q, K, V = _operands(B, heads, Sq, Sk, seed=7)
    K[:, 3] = K[:, 150]; K[:, 77] = K[:, 150]                                     # keys 3, 77, 150 tie ...
    Q[:, :] = (0.8 * K[:, 150].float()).bfloat16()[:, None]                       # ... and every query peaks on them
    ref = _reference(Q, K, heads, 10)
    d = _Dev(Q, K, V, heads)
    amap, pos, peak = d.probs(lib, d.engine_lse(lib), 10, Sk)
    assert peak.cpu().tolist() == [[3] * Sq]
    m = amap.cpu()
    assert torch.equal(m[..., 3], m[..., 77]) and torch.equal(m[..., 3], m[..., 150])
    assert float((m - ref["map"]).abs().max()) <= TOL and float((pos[..., 3].cpu() - 1).abs().max()) <= TOL


def test_attn_probs_refusals(lib):
    Q, K, V = _operands(1, 1, 4, 16, seed=1)
    d = _Dev(Q, K, V, 1)
    lse = torch.zeros(1, 1, 289, device=DEV)
    for over, msg in (({"mode": 1}, b"mode 0"), ({"head_dim": 96}, b"head_dim"), ({"Sq": 289}, b"1..288"), ({"Sk": 4098}, b"1..4097")):
        assert d.probs(lib, lse, 4, None, **over) == -1, over          # KZV_E_ARG, before any launch
        assert msg in lib.kzv_last_error(), (over, lib.kzv_last_error())


@pytest.mark.parametrize("T,vocab,ld", [(5, 157, 192), (3, 4300, 4352), (4, 63, 67)])
def test_token_scores_against_log_softmax(lib, T, vocab, ld):
    """kzv_token_scores on fp32 rows against torch.log_softmax of the same rows: 1e-4 (an fp32 reduction over <= 4,300 entries of
    magnitude <= ~20: 4300 * 2^-24 * e^0 relative on the sum, far below); first arg-max on ties; pad targets score 0."""
    B, pad = 3, 1
    gen = torch.Generator().manual_seed(vocab)
    logits = torch.full((B * T, ld), NAN)
    logits[:, :vocab] = 6 * torch.randn(B * T, vocab, generator=gen)
    logits[1, 40] = logits[1, 17] = logits[1, :vocab].max() + 1                  # a tie: the first wins
    labels = torch.randint(2, vocab, (B, T + 3), generator=gen)
    labels[0, 2] = pad
    labels[2, T] = pad
    dl, dlab = logits.to(DEV), labels.to(DEV)
    if ld % 4:
        assert dl.data_ptr() % 16 == 0 and ld % 4 != 0                            # rows not 16-byte aligned: the by-column path
    lp = torch.full((B, T), NAN, device=DEV)
    top = torch.full((B, T), -1, dtype=torch.int64, device=DEV)
    tlp = torch.full((B, T), NAN, device=DEV)
    L.check(lib.kzv_token_scores(dl.data_ptr(), ld, dlab.data_ptr(), T + 3, B, T, vocab, pad, lp.data_ptr(), top.data_ptr(), tlp.data_ptr(), _st()),
            "token_scores")
    torch.cuda.synchronize()
    ref = torch.log_softmax(logits[:, :vocab].double(), -1).view(B, T, vocab)
    tgt = labels[:, 1:T + 1]
    want = torch.gather(ref, 2, tgt[:, :, None]).squeeze(-1)
    want[tgt == pad] = 0.0
    err = float((lp.cpu().double() - want).abs().max())
    err_top = float((tlp.cpu().double() - ref.max(-1).values).abs().max())
    print(f"token_scores T{T} V{vocab}: max|dlogprob|={err:.3g} max|dtop1_logprob|={err_top:.3g}")
    assert err <= 1e-4 and err_top <= 1e-4
    want_top = ref.argmax(-1)
    want_top[0, 1] = 17
    assert torch.equal(top.cpu(), want_top)
    assert float(lp[0, 1]) == 0.0 and float(lp[2, T - 1]) == 0.0
