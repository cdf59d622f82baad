"""CPU, float64: the LayerScale gradient taken from the weight gradient equals its definition, with drop-path multipliers (some 0) and
compact rows in it; and the reference's treatment of gamma == 0."""
import pytest
import torch

import lsgrad_ref as G


def _case(seed, samples, tokens, K, C):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)      # noqa: E731
    M = samples * tokens
    gamma = torch.tensor([1e-4, 1.0, -3.0, 1e-20], dtype=torch.float64)[torch.randint(0, 4, (C,), generator=g)]
    return dict(a=r(M, K), W=r(C, K) * K ** -0.5, b=r(C), dx=r(M, C), gamma=gamma)


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("samples,tokens,K,C", [(5, 7, 24, 16), (3, 10, 64, 40)])
def test_quotient_equals_the_definition(samples, tokens, K, C, compact):
    c = _case(11 + samples, samples, tokens, K, C)
    rowscale = torch.tensor([0.0 if i % 3 == 1 else 1.25 for i in range(samples)], dtype=torch.float64)
    kept = rowscale != 0
    definition, dW, db = G.branch_terms(c["a"], c["W"], c["b"], c["dx"], rowscale, c["gamma"], tokens, kept if compact else None)
    got, _ = G.dgamma_from_wgrad([(c["W"], dW, c["b"], db[None])], c["gamma"])
    assert (rowscale == 0).any() and definition.abs().min() > 0
    assert ((got - definition).abs() <= 1e-12 * definition.abs()).all(), ((got - definition).abs() / definition.abs()).max()


def test_two_sets_share_one_gamma():
    """The two-stream model's proj / cov_proj: the definition sums both streams' rows, the quotient both (W, dW, b, db) sets."""
    c0, c1 = _case(5, 4, 6, 32, 24), _case(6, 4, 6, 32, 24)
    gamma = c0["gamma"]
    rs0, rs1 = torch.tensor([1.0, 0.0, 2.0, 1.0], dtype=torch.float64), torch.tensor([0.0, 1.5, 1.0, 0.0], dtype=torch.float64)
    d0, dW0, db0 = G.branch_terms(c0["a"], c0["W"], c0["b"], c0["dx"], rs0, gamma, 6)
    d1, dW1, db1 = G.branch_terms(c1["a"], c1["W"], c1["b"], c1["dx"], rs1, gamma, 6, rs1 != 0)
    got, _ = G.dgamma_from_wgrad([(c0["W"], dW0, c0["b"], db0[None]), (c1["W"], dW1, c1["b"], db1[None])], gamma)
    assert ((got - (d0 + d1)).abs() <= 1e-12 * (d0 + d1).abs()).all()


def test_replicas_are_summed_and_gamma_zero_gives_zero():
    c = _case(9, 2, 5, 16, 12)
    gamma = c["gamma"].clone()
    gamma[3] = 0.0
    rowscale = torch.ones(2, dtype=torch.float64)
    definition, dW, db = G.branch_terms(c["a"], c["W"], c["b"], c["dx"], rowscale, gamma, 5)
    assert dW[3].abs().max() == 0 and db[3] == 0                          # dW_j: and db_j vanish with gamma_j: 0 / 0
    parts = torch.randn(4, 12, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    parts[3] = db - parts[:3].sum(0)                                       # four replicas that sum to db
    got, S = G.dgamma_from_wgrad([(c["W"], dW, c["b"], parts)], gamma)
    keep = gamma != 0
    assert got[3] == 0 and ((got - definition).abs()[keep] <= 1e-10 * S[keep] / gamma.abs()[keep]).all()
    assert (G.dgamma_bound(S, gamma, 16, 4)[keep] > 0).all()
