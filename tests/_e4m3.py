"""Rows that exercise the corners of the e4m3 generation mode's quantiser (kzv/quant.py; csrc/decode_fused.hip: quant_pack8_kernel)."""
import torch


def special_rows(K, gen):
    """The rows the issue names, [n, K] float32 holding bf16 values."""
    grid = torch.arange(-8, 9, dtype=torch.float32)
    rows = [torch.zeros(K)]                                                                  # all zero: scale 1
    for k in (-20, -3, 0, 5):                                                               # amax exactly 448 * 2^k: amax / s = 448
        r = torch.randn(K, generator=gen) * 50 * 2.0 ** k
        r[3] = -448.0 * 2.0 ** k
        rows.append(r)
    r = torch.randn(K, generator=gen)                                                       # amax just above 448 * 2^k: the next scale
    r[0] = 450.0
    rows.append(r)
    # rounding ties: with amax = 256 the scale is 1; (2 j + 1) / 2 steps of every binade from the subnormals (step 2^-9) up
    ties = torch.cat([(2 * torch.arange(0, 16) + 1).float() * 2.0 ** (e - 4) for e in range(-9, 8)])
    r = torch.zeros(K)
    r[:ties.numel()] = ties[:K] * torch.where(torch.arange(ties.numel()) % 2 == 0, 1.0, -1.0)[:K]
    r[K - 1] = 256.0
    rows.append(r)
    r = torch.zeros(K)                                                                      # the e4m3 subnormal range, |w / s| < 2^-6
    r[:K - 1] = (torch.rand(K - 1, generator=gen) * 2 - 1) * 2.0 ** -6
    r[:grid.numel()] = grid * 2.0 ** -10                                                    # multiples of half a subnormal step
    r[K - 1] = 300.0
    rows.append(r)
    return torch.stack(rows).to(torch.bfloat16).to(torch.float32)
