"""float64 restatement of the grouped clip + RAdamScheduleFree step (csrc/optim.hip: clip_step_groups_kernel) in terms of the oracle.

Every trainable group is an optimizer of its own, as schedulefree keeps them: ``oracle.RAdamScheduleFreeState`` built with
lr * lr_scale and weight_decay * wd_scale, stepped by ``oracle.radam_schedulefree_step`` on the group's slice.  Frozen groups
(lr_scale == 0) have no state and their slices are never touched.  The clip coefficient is ``oracle.clip_grad_norm`` over the
trainable slices (torch's clip_grad_norm_ sees only parameters that have a gradient).
"""
import numpy as np

from oracle import trocr_oracle as O


class GroupedRef:
    def __init__(self, p0, groups, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, ema_decay=None):
        self.groups = [(int(lo), int(hi), float(ls), float(ws)) for lo, hi, ls, ws in groups]
        self.y = np.asarray(p0, dtype=np.float64).copy()
        self.z = self.y.copy()
        self.v = np.zeros_like(self.y)
        self.ema = self.y.copy() if ema_decay is not None else None
        self.ema_decay = ema_decay
        self.states = [None if ls == 0.0 else O.RAdamScheduleFreeState(lr=lr * ls, beta1=beta1, beta2=beta2, eps=eps, weight_decay=weight_decay * ws)
                       for _, _, ls, ws in self.groups]
        self.last_ckp1 = []

    def step(self, g, max_norm=0.0, grad_scale=1.0):
        """One step from the fp32 gradient ``g``; returns (total norm of the scaled trainable gradient, clip coefficient)."""
        gs = np.asarray(g, dtype=np.float64) * grad_scale
        total, coef = 0.0, 1.0
        if max_norm > 0:
            total, coef = O.clip_grad_norm([gs[lo:hi] for (lo, hi, ls, _) in self.groups if ls != 0.0], max_norm)
        self.last_ckp1 = []
        for (lo, hi, ls, _), st in zip(self.groups, self.states):
            if st is None:
                continue
            y, z, v = self.y[lo:hi], self.z[lo:hi], self.v[lo:hi]          # views: updated in place
            _, ckp1 = O.radam_schedulefree_step(st, y, z, v, gs[lo:hi] * coef)
            self.last_ckp1.append(ckp1)
            if self.ema is not None:
                self.ema[lo:hi] += (1.0 - self.ema_decay) * (y - self.ema[lo:hi])
        return total, coef
