"""The CPU reference of the parabolic corrector trajectories (tests/parabolic_enrichment_ref.py) checked on itself, no GPU:
its stationary limit, its zero-right-hand-side steps, and the gap figure the GPU limit test takes its tolerance from."""
import numpy as np

import parabolic_enrichment_ref as ref
from common import oracle_from_problem, problem_with_q_components

T = 0.05


def _oracle(Q=1, shape=(3, 3), kc=2):
    p = problem_with_q_components(list(shape), kc, Q)
    return oracle_from_problem(p), (0.6,) * Q if Q == 1 else tuple(np.linspace(0.3, 0.9, Q))


def test_one_huge_step_approaches_the_stationary_corrector():
    """x_1 = (A + M / dt)^-1 b -> A^-1 b: the gap falls like 1 / dt, and at dt = 1e6 T -- the step of the GPU limit test -- it
    is below the figure that test allows for it (measured here: 7.1e-7 at dt = 1e6 T on the 3 x 3 grid; LIMIT_GAP = 1e-6)."""
    o, mu = _oracle()
    marked = list(range(o.S))
    gaps = [ref.stationary_limit_gap(o, marked, mu, dt) for dt in (1e2 * T, 1e4 * T, 1e6 * T)]
    print('stationary limit gaps at dt = 1e2, 1e4, 1e6 T:', gaps)
    assert gaps[0] > gaps[1] > gaps[2]
    assert 50.0 < gaps[0] / gaps[1] < 200.0            # first order in 1 / dt
    assert gaps[2] < ref.LIMIT_GAP
    # ... while a step of the size the trajectories use is nowhere near the stationary corrector: the two problems differ
    assert ref.stationary_limit_gap(o, marked, mu, T / 4) > 0.1


def test_zero_rows_of_phi_and_linearity():
    o, mu = _oracle(Q=2)
    nt, dt = 4, T / 4
    rng = np.random.default_rng(3)
    b_K = np.stack([o.b, rng.standard_normal(o.b.shape)])
    phi = np.array([[9.0, 9.0], [0.0, 0.0], [1.0, 0.5], [0.0, 0.0], [0.3, -2.0]])
    x = ref.corrector_trajectory(o, 4, mu, dt, nt, phi, b_K)
    assert np.abs(x[0]).max() == 0.0                                         # zero right-hand side from a zero state
    assert 0.0 < np.abs(x[2]).max() < np.abs(x[1]).max()                     # a zero row later on: decay
    # linear in the source, row 0 of phi is never read
    phi2 = phi.copy()
    phi2[0] = -1.0
    phi2[1:] *= 2.0
    assert np.allclose(ref.corrector_trajectory(o, 4, mu, dt, nt, phi2, b_K), 2.0 * x, rtol=1e-12, atol=0.0)
    # K = 1 with the oracle's own load vector is the default
    one = ref.corrector_trajectory(o, 4, mu, dt, nt)
    assert np.array_equal(one, ref.corrector_trajectory(o, 4, mu, dt, nt, np.ones((nt + 1, 1)), o.b[None]))
    assert ref.corrector_trajectories(o, [4, 0], mu, dt, nt).shape == (2, o.n, nt)
