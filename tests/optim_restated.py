"""numpy restatement of the grouped, clipped Adam of csrc/optim.hip and of the state-dict index mapping of
spacap3d_amd/optim.py -- written from the contract, not from the code under test.

Update: float32, operation for operation as the kernel (no fused multiply-add); squared norms, the norm and the clip
coefficient in float64, the coefficient rounded once to float32; a non-finite total skips the update and leaves the step
count alone.
"""
import numpy as np

F = np.float32


def sqnorms(grads, group_of, num_groups):
    """float64 sums of squares per group, then the total (sum of the group sums)."""
    sq = np.zeros(num_groups + 1, dtype=np.float64)
    for g, k in zip(grads, group_of):
        g64 = np.asarray(g, dtype=np.float64).reshape(-1)
        sq[k] += float(np.sum(g64 * g64))
    sq[num_groups] = float(np.sum(sq[:num_groups]))
    return sq


def clip_coef(total_sq, grad_scale, max_norm):
    """clip_grad_norm_'s min(1, max_norm / (norm + 1e-6)) on the norm of the MEAN gradient, in float64, rounded once."""
    if max_norm is None or max_norm <= 0 or not np.isfinite(total_sq):
        return F(1.0)
    norm = float(grad_scale) * np.sqrt(np.float64(total_sq))
    return F(min(1.0, float(max_norm) / (norm + 1e-6)))


class RestatedAdam:
    def __init__(self, params, group_of, lrs, wds, betas=(0.9, 0.999), eps=1e-8, max_norm=None):
        self.p = [np.array(p, dtype=F) for p in params]
        self.m = [np.zeros_like(p) for p in self.p]
        self.v = [np.zeros_like(p) for p in self.p]
        self.group_of, self.G = list(group_of), len(lrs)
        self.lrs, self.wds = [F(x) for x in lrs], [F(x) for x in wds]
        self.b1, self.b2, self.eps = F(betas[0]), F(betas[1]), F(eps)
        self.max_norm = max_norm
        self.t, self.skipped = 0, 0
        self.norm = self.coef = None

    def step(self, grads, grad_scale=1.0):
        grads = [np.asarray(g, dtype=F) for g in grads]
        sq = sqnorms(grads, self.group_of, self.G)
        total = sq[self.G]
        with np.errstate(invalid="ignore"):
            self.norm = F(float(grad_scale) * np.sqrt(total))
        self.coef = clip_coef(total, grad_scale, self.max_norm)
        if not np.isfinite(total):
            self.skipped += 1
            return False
        self.t += 1
        one = F(1.0)
        s = F(grad_scale) * self.coef
        t = F(self.t)
        c1, c2 = one - np.power(self.b1, t, dtype=F), one - np.power(self.b2, t, dtype=F)
        rs2 = one / np.sqrt(c2, dtype=F)
        for i, g in enumerate(grads):
            k = self.group_of[i]
            step_size, wd = self.lrs[k] / c1, self.wds[k]
            p, m, v = self.p[i], self.m[i], self.v[i]
            gg = g * s + wd * p
            m[...] = self.b1 * m + (one - self.b1) * gg
            v[...] = self.b2 * v + (one - self.b2) * gg * gg
            p[...] = p - step_size * (m / (np.sqrt(v, dtype=F) * rs2 + self.eps))
        return True


# ---- the layout: padded offsets, flat <-> per parameter, torch's state indices ---------------------------------------------
def padded_offsets(numels):
    """Every tensor starts on a multiple of 4 elements (16 bytes) -> (offsets, total)."""
    offs, off = [], 0
    for n in numels:
        offs.append(off)
        off = (off + n + 3) // 4 * 4
    return offs, off


def flat_to_params(flat, offsets, shapes):
    return [np.array(flat[o:o + int(np.prod(s, dtype=np.int64))]).reshape(s) for o, s in zip(offsets, shapes)]


def params_to_flat(tensors, offsets, total):
    flat = np.zeros(total, dtype=F)
    for t, o in zip(tensors, offsets):
        flat[o:o + t.size] = np.asarray(t, dtype=F).reshape(-1)
    return flat


def state_indices(groups_of_names, names_with_state):
    """torch numbers the parameters group by group, each in the order given; only those with state appear -> {name: index}."""
    have, out, n = set(names_with_state), {}, 0
    for names in groups_of_names:
        for name in names:
            if name in have:
                out[name] = n
            n += 1
    return out
