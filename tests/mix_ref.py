"""Test helper: csrc/mixup.hip restated on the host (include/uvit.h).

`mix_batch(x, desc, boxes, erase_mode, seed, iteration)` is uvit_op_mix_batch in numpy float32 with the op's operation order: every
product and sum is IEEE float32, evaluated as the kernel writes it, so every output value that holds no Box-Muller fill is the
kernel's bit for bit.  The hash and the uniforms are exact integers; the normal of a fill is formed in float64 from them and rounded
to float32 once (numpy's float32 log / cos are not the device's either), and `mix_batch` also returns the mask of the values that
hold such a fill, for which NOISE_TOL applies.

`soft_ce(z, y, partner, lam, s)` is uvit_op_probe_ce_mix in float64 torch: the dense target of timm's mixup_target against log_softmax.
"""
import numpy as np
import torch

M32 = 0xFFFFFFFF
F64 = torch.float64
TWO_PI_F32 = float(np.float32(6.2831854820251465))

# |device n - exact n| for one fill, from the header's formula n = sqrtf(-2 logf(u1)) cosf(fl(2 pi_f u2)) with exact u1, u2 in (0, 1),
# u1 >= 2^-24 so r = sqrt(-2 ln u1) <= 5.77:
#   the angle: one rounding of a product <= 6.29, 2^-24 x 6.29 = 3.75e-7, moves the cosine by as much; cosf itself 2 ulp of a value
#   <= 1, 1.2e-7: the cosine within 5.0e-7;  r: logf 1 ulp (2^-23 relative), halved by the square root, plus sqrtf's own rounding:
#   1.2e-7 relative;  the product: one more rounding, 6e-8 relative.
#   |dn| <= 5.77 x 5.0e-7 + 5.77 x 1.8e-7 = 3.9e-6  ->  4e-6, the figure DESIGN.md section 9.16 has for the same construction.
NOISE_Z_TOL = 4e-6


def noise_tol(ref):
    """Bound of |out - restatement| at an output value that holds a fill: the device's normal against the float64 one rounded to
    float32 (NOISE_Z_TOL + 2^-24 x 5.77 = 3.5e-7), passed on by a convex combination (lam, 1 - lam in [0, 1]: no growth), whose two
    products and one sum then round differently by at most 3 x 2^-24 of the values involved (|values| <= |ref| + 12)."""
    return NOISE_Z_TOL + 3.5e-7 + 3 * 2.0 ** -24 * (np.abs(ref) + 12.0)


def hash32(x):
    """uvit_hash32 of csrc/common.h on numpy uint64 arrays (or ints) holding 32-bit values: exact."""
    x = np.asarray(x, dtype=np.uint64) & np.uint64(M32)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & np.uint64(M32)
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & np.uint64(M32)
    return x ^ (x >> np.uint64(16))


def sample_key(seed, iteration, j):
    """kj of the header: kit = h(seed ^ (iteration 0x9E3779B9 + 0x7F4A7C15)), kj = h(kit ^ (j + 1) 0x85EBCA6B)."""
    kit = int(hash32((int(seed) ^ ((int(iteration) * 0x9E3779B9 + 0x7F4A7C15) & M32)) & M32))
    return int(hash32(kit ^ (((int(j) + 1) * 0x85EBCA6B) & M32)))


def uniforms(kj, q):
    """(u1, u2) of counters q (uint64 array) under the sample key: ((h >> 9) + 0.5) 2^-23, exact in float32 and in float64."""
    k1, k2 = int(hash32(kj ^ 0x1B873593)), int(hash32(kj ^ 0xCC9E2D51))
    q = np.asarray(q, dtype=np.uint64)
    u = lambda k: ((hash32(q ^ np.uint64(k)) >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23      # noqa: E731
    return u(k1), u(k2)


def normals(kj, q):
    """n(j, q) in float64: the kernel's float32 2 pi, everything else exact to double rounding."""
    u1, u2 = uniforms(kj, q)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(TWO_PI_F32 * u2)


def erased(x, boxes, erase_mode, seed, iteration):
    """e(j) of every sample, float32 (B, 3, S, S), and the mask of the values that hold a Box-Muller fill."""
    B, _, S, _ = x.shape
    e = x.astype(np.float32).copy()
    noisy = np.zeros(x.shape, dtype=bool)
    R = 0 if boxes is None else boxes.shape[1]
    for j in range(B):
        kj = sample_key(seed, iteration, j)
        for r in range(R):
            top, left, h, w = (int(v) for v in boxes[j, r])
            if h == 0:
                continue
            win = (slice(None), slice(top, top + h), slice(left, left + w))
            if erase_mode == 0:
                e[j][win] = 0.0
                noisy[j][win] = False                           # a later box overwrites an earlier one
                continue
            if erase_mode == 1:
                fill = normals(kj, np.arange(3, dtype=np.uint64) + np.uint64(3 * r)).reshape(3, 1, 1)
                e[j][win] = np.broadcast_to(fill, (3, h, w)).astype(np.float32)
            else:
                c, y, xx = np.meshgrid(np.arange(3), np.arange(top, top + h), np.arange(left, left + w), indexing="ij")
                e[j][win] = normals(kj, ((c * S + y) * S + xx).astype(np.uint64)).astype(np.float32)
            noisy[j][win] = True
    return e, noisy


def mix_batch(x, desc, boxes, erase_mode, seed, iteration):
    """(out, noisy): uvit_op_mix_batch in float32, and the mask of the output values that hold a Box-Muller fill."""
    B, _, S, _ = x.shape
    e, en = erased(x, boxes, erase_mode, seed, iteration)
    out, noisy = np.empty_like(e), np.zeros(x.shape, dtype=bool)
    for b in range(B):
        d = desc[b]
        p, kind = int(d["partner"]), int(d["kind"])
        if kind == 0:
            out[b], noisy[b] = e[b], en[b]
        elif kind == 1:
            lam = np.float32(d["lam"])
            oml = np.float32(1.0) - lam
            out[b] = (lam * e[b]).astype(np.float32) + (oml * e[p]).astype(np.float32)
            noisy[b] = en[b] | en[p]
        else:
            out[b], noisy[b] = e[b], en[b]
            win = (slice(None), slice(int(d["yl"]), int(d["yh"])), slice(int(d["xl"]), int(d["xh"])))
            out[b][win], noisy[b][win] = e[p][win], en[p][win]
    return out, noisy


# ---- the soft-target loss ----
# uvit_op_probe_ce_mix against float64.  A row's loss is lam La + (1 - lam) Lb with La, Lb the row formula of uvit_op_probe_ce, for
# which tests/test_gpu_probe.py::test_cross_entropy derives |L - ref| <= 1e-5 (1 + |ref|): a convex combination of two such values
# (L >= 0, so the combination of the references is the reference) keeps that bound, and the two products and the sum add three
# roundings at the loss's magnitude.  dlogits = (p - t) / B: the 1e-5 / B of that test for p, and t = (1 - s) (lam [k = ya] + (1 - lam)
# [k = yb]) + s / K, a value in [0, 1] formed with four roundings.
def ce_loss_tol(ref):
    return 1e-5 * (1.0 + abs(ref)) + 3 * 2.0 ** -24 * abs(ref)


def ce_grad_tol(B):
    return (1e-5 + 4 * 2.0 ** -24) / B


def soft_target(y, partner, lam, K, s):
    """timm mixup_target: lam oh(y) + (1 - lam) oh(y[partner]), oh = off + (on - off) onehot with off = s / K, on = 1 - s + off."""
    y, partner, lam = torch.as_tensor(y), torch.as_tensor(partner).long(), torch.as_tensor(lam).to(F64).view(-1, 1)
    oh = lambda t: torch.full((t.shape[0], K), s / K, dtype=F64).scatter_add_(1, t.view(-1, 1), torch.full((t.shape[0], 1), 1.0 - s, dtype=F64))  # noqa: E731
    return lam * oh(y) + (1.0 - lam) * oh(y[partner])


def soft_ce(logits, y, partner, lam, s):
    """SoftTargetCrossEntropy on the mixed target: row losses (B,), their mean, d mean / d logits = (softmax - t) / B, float64."""
    z = torch.as_tensor(logits).to(F64)
    B, K = z.shape
    t = soft_target(y, partner, lam, K, s)
    logp = torch.log_softmax(z, dim=-1)
    rows = -(t * logp).sum(-1)
    return rows, rows.mean(), (logp.exp() - t) / B
