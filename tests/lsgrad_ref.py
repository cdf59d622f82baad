"""Float64 restatement of the LayerScale gradient taken from the weight gradient (csrc/elementwise.hip, ls_dgamma_kernel) and its
derived error bound.  No GPU: tests/test_host_lsgrad.py pins the algebra against the definition, tests/test_gpu_lsgrad.py the kernel
against this file.

With dy = rowscale * gamma * dx the gradient of the branch output y = a W^T + b, dW = dy^T a and db = sum_m dy:
    dgamma_j = sum_m rowscale_m dx_mj y_mj = (sum_k W_jk dW_jk + b_j db_j) / gamma_j
"""
import torch

F64 = torch.float64


def dgamma_from_wgrad(sets, gamma):
    """sets: [(W [C, K], dW [C, K], b [C], db [nrep, C])], one or two; gamma [C].  Returns (dgamma [C] float64 with 0 where gamma == 0,
    S [C] = the sum of the absolute values of every term of the numerator)."""
    g = gamma.to(F64)
    num, S = torch.zeros_like(g), torch.zeros_like(g)
    for W, dW, b, db in sets:
        prod = W.to(F64) * dW.to(F64)
        num += prod.sum(1) + b.to(F64) * db.to(F64).sum(0)
        S += prod.abs().sum(1) + b.to(F64).abs() * db.to(F64).abs().sum(0)
    safe = torch.where(g == 0, torch.ones_like(g), g)
    return torch.where(g == 0, torch.zeros_like(g), num / safe), S


def dgamma_bound(S, gamma, K, nrep):
    """|err_j| <= (K + nrep + 2) 2^-23 S_j / |gamma_j|.  Every one of the K products and the K + nrep additions of the numerator is one
    fp32 rounding (2^-24 relative to a partial sum that never exceeds S_j in magnitude): (2 K + nrep) 2^-24 S_j <= (K + nrep) 2^-23 S_j
    in whatever order they are summed; the quotient and the addition onto the destination are one rounding each of a value no larger
    than S_j / |gamma_j| (the tests keep the destination below that): the + 2."""
    g = gamma.to(F64).abs()
    return (K + nrep + 2) * 2.0 ** -23 * S / torch.where(g == 0, torch.ones_like(g), g)


def branch_terms(a, W, b, dx, rowscale, gamma, tokens, kept=None):
    """The definition and the quantities the step computes, in float64, for one Block branch.  a [M, K] the branch's input rows (M =
    samples * tokens, dense), dx [M, C] the residual-stream gradient, rowscale [samples] the drop-path multipliers (0 = dropped).
    kept (bool [samples], None = all): the branch runs on the COMPACT rows of the kept samples only, as the drop-path sample lists do.
    Returns (dgamma by the definition over all rows, dW, db)."""
    a, W, b, dx, gamma = (t.to(F64) for t in (a, W, b, dx, gamma))
    rs = rowscale.to(F64).repeat_interleave(tokens)[:, None]
    y = a @ W.T + b
    definition = (rs * dx * y).sum(0)
    rows = torch.arange(a.shape[0]) if kept is None else torch.nonzero(kept.repeat_interleave(tokens)).flatten()
    dy = (rs * gamma * dx)[rows]                                    # compact, like the branch's buffers
    return definition, dy.T @ a[rows], dy.sum(0)
