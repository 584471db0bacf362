"""CPU reference of the 3D parabolic corrector trajectories (``lrbms3_local_correction_euler``) and of the
enrichment loop built on them, on top of ``oracle.lrbms3d``: test infrastructure only, the product never imports it.

On the neighbourhood N(ii) of a marked subdomain (``enrichment3d_ref.hood_system``: the SWIPDG operator with the all-Dirichlet
outer boundary) implicit Euler with zero initial value,

    (M_N + dt A_N(mu)) x_{k+1} = M_N x_k + dt sum_j phi[k+1][j] b_j|_N,   k = 0 .. nt-1,

with M_N the rows / columns of the oracle's mass ``o.M`` and ONE sparse LU for all steps; x_k restricted to ii is kept.
Validated in tests/test_parabolic_enrichment3d_host.py: a neighbourhood that is the whole domain gives
``parabolic3d_ref.Parabolic3D.solve``.

``replay`` is the enrichment loop of tests/test_parabolic_enrichment3d_gpu.py on the CPU alone: LU trajectories, the local POD of
tests/local_pod_ref.py, ``parabolic3d_ref.ParabolicReduced3D`` on the compact bases, every subdomain marked in every round
(Doerfler marking with theta = 1.0)."""
import functools

import numpy as np
import scipy.sparse.linalg as spla

import common3d as c3
import enrichment3d_ref as eref
import local_pod_ref as pod
from parabolic3d_ref import Parabolic3D, ParabolicReduced3D

CORR_TOL = 1e-8        # the tolerance of tests/test_enrichment3d_gpu.py for the stationary correctors (iterative vs direct solve)
# One implicit Euler step of dt = 1e6 T (T = LOOP['T']) against the stationary corrector, both solved directly on the CPU: the gap is
# 1.8e-7 on interior_3x3x3 at its mu (1.8e-3 at 1e2 T, 1.8e-5 at 1e4 T: first order in 1 / dt;
# tests/test_parabolic_enrichment3d_host.py asserts it stays below LIMIT_GAP).  The GPU limit test compares the native call's one
# huge step with the native stationary correctors at CORR_TOL + LIMIT_GAP = the solver tolerance plus this gap of the two PROBLEMS.
LIMIT_GAP = 3e-7
LIMIT_GRID = 'interior_3x3x3'

# The loop of the GPU test and of its CPU replay: bases = the constant and the final state of ONE trajectory at mu0, the loop at mu.
# T is of the size of the slowest time scale of a neighbourhood of the unit cube: the three snapshots of a corrector trajectory then
# have singular values 1 : 1e-2 : 3e-4, a factor 300 above the POD threshold rtol (with T = 0.3 the third sits AT the threshold and
# the sizes of a round would hinge on round-off).
LOOP = dict(name='interior_3x3x3', T=0.03, nt=3, mu0=0.9, mu=0.15, pod_modes=2, rounds=3, rtol=1e-6)


def corrector_trajectory(o, ii, mu, dt, nt, phi=None, b_K=None):
    """[nt, n]: row k - 1 = x_k on subdomain ``ii``.  ``phi`` [nt + 1, K] (row k = time of step k; default: ones, K = 1),
    ``b_K`` [K, ndof] global load vectors (default: the oracle's own ``b``)."""
    dofs = eref.hood_dofs(o, ii)
    A = eref.hood_system(o, ii, mu)
    M = o.M.tocsr()[dofs][:, dofs]
    bK = o.b[None, dofs] if b_K is None else np.asarray(b_K).reshape(len(b_K), -1)[:, dofs]
    phi = np.ones((nt + 1, bK.shape[0])) if phi is None else np.asarray(phi, dtype=np.float64)
    assert phi.shape == (nt + 1, bK.shape[0])
    lu = spla.splu((M + dt * A).tocsc())
    k0 = o.mesh.neighborhood_of(ii).index(ii)
    x = np.zeros(len(dofs))
    out = np.zeros((nt, o.n))
    for k in range(nt):
        x = lu.solve(M @ x + dt * (phi[k + 1] @ bK))
        out[k] = x[k0 * o.n:(k0 + 1) * o.n]
    return out


def corrector_trajectories(o, marked, mu, dt, nt, phi=None, b_K=None):
    """[len(marked), n, nt], the layout of the native call (step fastest)."""
    return np.stack([corrector_trajectory(o, ii, mu, dt, nt, phi, b_K).T for ii in marked])


def stationary_limit_gap(o, marked, mu, dt):
    """max over ``marked`` of |x_1(dt) - x_stationary|_max / |x_stationary|_max: how far ONE implicit Euler step of size ``dt``
    is from the stationary corrector ``enrichment3d_ref.corrector`` (x_1 = (A + M / dt)^-1 b, so the gap is O(|A^-1 M| / dt)),
    both solved directly on the CPU."""
    gap = 0.0
    for ii in marked:
        stat = eref.corrector(o, ii, mu)
        one = corrector_trajectory(o, ii, mu, dt, 1)[0]
        gap = max(gap, float(np.abs(one - stat).max() / np.abs(stat).max()))
    return gap


def max_rel(got, ref):
    """max_k |got_k - ref_k|_max / max_k |ref_k|_max for trajectories [n, nt]: relative to the largest step."""
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def switching_source(o, nt, seed=2):
    """(b_K [2, S, n], phi [nt + 1, 2]) of the K = 2 cells: the oracle's load and a random vector of its size; the first rows of phi
    that drive a step are zero (the source starts late), row 0 -- never read -- is not."""
    rng = np.random.default_rng(seed)
    b = o.b.reshape(o.S, o.n)
    b_K = np.stack([b, rng.standard_normal(b.shape) * np.abs(b).max()])
    phi = rng.uniform(0.3, 1.0, (nt + 1, 2))
    phi[0] = 7.0
    phi[1:1 + max(1, nt // 2)] = 0.0
    return b_K, phi


# ------------------------------------------------------------------------------------------------- the enrichment loop
def local_products(o):
    """Dense local energy products [S, n, n]: the diagonal blocks of the oracle's ``P``."""
    Pt = o.P.tocsr()
    return np.stack([pod.sym(Pt[o.dofs_of(ii)][:, o.dofs_of(ii)].toarray()) for ii in range(o.S)])


def start_bases(o, U_final, P):
    """The start of the loop: per subdomain the constant and the block of ``U_final`` [S, n], P-orthonormal (Gram-Schmidt in this
    order) -> list of [n, 2]."""
    out = []
    for ii in range(o.S):
        X = np.stack([np.ones(o.n), np.asarray(U_final)[ii]], axis=1)
        out.append(_gram_schmidt(X, P[ii]))
    return out


def _gram_schmidt(X, P):
    V = np.zeros_like(X)
    for j in range(X.shape[1]):
        v = X[:, j].copy()
        for _ in range(2):
            v -= V[:, :j] @ (V[:, :j].T @ (P @ v))
        V[:, j] = v / np.sqrt(v @ (P @ v))
    return V


def trajectory_error(o, bases, u, U_fom):
    """|V u - U|_F / |U|_F over the whole trajectory: u [nt + 1, sum N_s] on the compact ``bases``, U_fom [nt + 1, S, n]."""
    off = np.concatenate([[0], np.cumsum([b.shape[1] for b in bases])])
    rec = np.stack([u[:, off[ii]:off[ii + 1]] @ bases[ii].T for ii in range(o.S)], axis=1)
    return float(np.linalg.norm(rec - U_fom) / np.linalg.norm(U_fom))


@functools.lru_cache(maxsize=None)
def replay():
    """The loop of ``LOOP`` on the CPU.  Returns a dict: ``start`` (the bases every run starts from, list of [n, 2]), ``sizes``
    [rounds + 1][S] (before the first round and after every round), ``errors`` [rounds + 1] (``trajectory_error`` of the reduced
    solution on those bases), ``margin`` (the smallest factor between a singular value of a POD call and its threshold: the sizes
    do not hinge on round-off while it is large), ``U_fom``."""
    c = LOOP
    p = c3.make_problem(c['name'])
    o = c3.oracle_of(p)
    T, nt, mu = c['T'], c['nt'], c['mu']
    P = local_products(o)
    fom = Parabolic3D(o, T, nt)
    U_fom = fom.solve(mu)
    start = start_bases(o, fom.solve(c['mu0'])[nt], P)
    traj = corrector_trajectories(o, list(range(o.S)), mu, T / nt, nt)       # the correctors depend on mu alone: one set for all rounds
    bases = [b.copy() for b in start]
    sizes, errors, margin = [], [], np.inf
    for rnd in range(c['rounds'] + 1):
        sizes.append([b.shape[1] for b in bases])
        red = ParabolicReduced3D(o, bases, T, nt)
        errors.append(trajectory_error(o, bases, red.solve(mu), U_fom))
        if rnd == c['rounds']:
            break
        for ii in range(o.S):
            nl = bases[ii].shape[1]
            V = np.concatenate([bases[ii], np.zeros((o.n, c['pod_modes']))], axis=1)
            margin = min(margin, pod.threshold_margin(traj[ii][None], V[None], [nl], P[ii][None], rtol=c['rtol']))
            Vn, _, added = pod.local_pod_one(traj[ii], V, nl, P[ii], c['pod_modes'], rtol=c['rtol'])
            bases[ii] = Vn[:, :nl + added]
    return dict(start=start, sizes=sizes, errors=errors, margin=margin, U_fom=U_fom, problem=p, oracle=o)
