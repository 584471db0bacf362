"""NumPy restatement of the single and stationary 3D / P2 solvers (pylrbms_amd/csrc/online3d.hip, lrbms3d.hip), iterate by iterate, on top of
tests/pcg_ref.py, tests/fom_batch3d_ref.py and tests/parabolic_batch3d_ref.py.  Nothing here is new arithmetic: every function
names the operator and the preconditioner of one export and hands them to ``pcg_ref.pcg_iterate``.

  lrbms3_reduced_solve            A(theta) on the 7-slot layout; D^-1: inverse self-slot blocks of A(theta) (zero diagonal -> 1)
  lrbms3_reduced_solve_batch      column m at its own theta_m; D^-1 at the mean theta of the column's group of 16 (``group_means``);
                                  with an installed preconditioner D^-1 AND A0^-1 at the build parameter
  lrbms3_fom_solve                ``BatchFomPrecond3D`` with both levels at the solve's theta; the coarse level at the parameter of
                                  the solve that built a kept inverse (lrbms3_fom_precond_keep)
  lrbms3_*_implicit_euler, step 1 operator M + dt A(theta), both levels built on it; the unknown is the correction d = u_1 - u_0 for
                                  the right-hand side (M u_0 + dt b) - (M + dt A) u_0, the ratio refers to |M u_0 + dt b|

Every builder takes the mutant switches the GPU cells must be able to tell from the product (tests/test_pcg_iterates3d_host.py
proves on the CPU that they can)."""
import numpy as np
import scipy.sparse as sp
from scipy.sparse.linalg import splu, spsolve

import fom_batch3d_ref as ref3
import parabolic_batch3d_ref as par3
import pcg_ref

SELF = par3.SELF
GROUP = 16                                # red_batch_run: columns per group


class Cell:
    """The columns of one call: operator As[j], preconditioner Ms[j] (an ``apply``) and right-hand side cols[:, j]; ``scale[j]`` =
    |cols_j| / |reference right-hand side| (1 unless the export takes its ratio against another vector: the Euler steps).
    ``pad``: a diagonal added for the direct solve only (1 on zero-padded unknowns, as D^-1 has)."""

    def __init__(self, As, Ms, cols, scale=None, pad=None):
        cols = np.asarray(cols, dtype=np.float64)
        self.cols = cols[:, None] if cols.ndim == 1 else cols
        self.m = self.cols.shape[1]
        self.As = list(As) if isinstance(As, (list, tuple)) else [As] * self.m
        self.Ms = list(Ms) if isinstance(Ms, (list, tuple)) else [Ms] * self.m
        self.scale = np.ones(self.m) if scale is None else np.asarray(scale, dtype=np.float64).reshape(self.m)
        self.pad = pad

    def iterate(self, k):
        """The ``reference(k)`` of ``check_iterates``: (X_k [n, m], ratios [m])."""
        out = [pcg_ref.pcg_iterate(lambda p, A=A: A @ p, M, self.cols[:, j], k) for j, (A, M) in enumerate(zip(self.As, self.Ms))]
        return np.stack([x for x, _ in out], axis=1), np.array([r for _, r in out]) * self.scale

    def solve(self, j=0):
        A = self.As[j] if self.pad is None else self.As[j] + self.pad
        return spsolve(sp.csc_matrix(A), self.cols[:, j])

    def other(self, Ms):
        """The same operators and right-hand sides under other preconditioners (a mutant)."""
        return Cell(self.As, Ms, self.cols, self.scale, self.pad)


def miss(X, X_ref):
    """Largest relative distance of a column of X from the same column of X_ref (zero reference columns skipped)."""
    nrm = np.linalg.norm(X_ref, axis=0)
    live = nrm > 0.0
    return float((np.linalg.norm(X - X_ref, axis=0)[live] / nrm[live]).max())


# ------------------------------------------------------------------------------------------------------------- reduced
def group_means(thetas):
    """[ng, Q]: the mean theta of every group of 16 columns, accumulated as sum_m theta_m / nm in column order (red_batch_run)."""
    thetas = np.asarray(thetas, dtype=np.float64)
    out = []
    for g in range(0, thetas.shape[0], GROUP):
        rows = thetas[g:g + GROUP]
        acc = np.zeros(thetas.shape[1])
        for row in rows:
            acc = acc + row / rows.shape[0]
        out.append(acc)
    return np.stack(out)


def self_blocks(B, theta, M_red=None, dt=1.0):
    """The self-slot blocks [S, N, N] of dt A(theta) (+ M_red)."""
    D = dt * np.einsum('q,qsij->sij', np.asarray(theta, dtype=np.float64), np.asarray(B, dtype=np.float64)[:, :, SELF])
    return D if M_red is None else D + np.asarray(M_red)


def reduced_blocks_precond(B, theta, M_red=None, dt=1.0):
    """Block-Jacobi alone: ``reduced_block_jacobi`` (k3_block_inverse, zero diagonal -> 1) of the self-slot blocks."""
    return pcg_ref.block_jacobi(pcg_ref.reduced_block_jacobi(self_blocks(B, theta, M_red, dt)))


def reduced_two_level(B, nbr, theta_blocks, theta_coarse):
    """D^-1 at ``theta_blocks`` plus R0^T A0^-1 R0 with A0 the (0, 0) entries of the blocks at ``theta_coarse``
    (lrbms3_reduced_precond_build: k3r_coarse_fill, k3b_coarse_apply): ``StepPrecond3D`` with zero mass and dt = 1."""
    S, N = np.asarray(B).shape[1], np.asarray(B).shape[-1]
    zero = np.zeros((S, N, N))
    P = par3.StepPrecond3D(B, zero, nbr, theta_blocks, 1.0, coarse=False)
    crs = par3.StepPrecond3D(B, zero, nbr, theta_coarse, 1.0, coarse=True)
    assert crs.has_coarse, 'the coarse matrix of the reference is not positive definite'
    P.cho = crs.cho
    return P.apply


def reduced_single(B, nbr, theta, rhs, block_theta=None, keep=None):
    """lrbms3_reduced_solve.  Mutant: ``block_theta`` (inverse blocks at another parameter)."""
    A = pcg_ref.reduced_operator(pcg_ref.combine_reduced(B, theta), nbr)
    M = reduced_blocks_precond(B, theta if block_theta is None else block_theta)
    pad = None if keep is None else sp.diags(1.0 - np.asarray(keep, dtype=np.float64).ravel())
    return Cell(A, M, np.asarray(rhs).reshape(-1), pad=pad)


def reduced_batch(B, nbr, thetas, cols, build_theta=None, blocks=None, coarse='build'):
    """lrbms3_reduced_solve_batch(_src), stationary: column m at thetas[m] with right-hand side cols[:, m].
    No installed preconditioner (``build_theta`` None): block-Jacobi at the group mean.  Installed: both levels at ``build_theta``.
    Mutants: ``blocks`` = 'own' (the column's theta) | 'call' (the mean over the whole call) | 'group' (the group mean under an
    installed preconditioner); ``coarse`` = None (no coarse level) | 'own' (the coarse level at the column's theta)."""
    thetas = np.asarray(thetas, dtype=np.float64)
    nmu = thetas.shape[0]
    As = [pcg_ref.reduced_operator(pcg_ref.combine_reduced(B, th), nbr) for th in thetas]
    blocks = blocks or ('group' if build_theta is None else 'build')
    means = group_means(thetas)
    at = {'own': lambda m: thetas[m], 'group': lambda m: means[m // GROUP], 'call': lambda m: thetas.mean(axis=0),
          'build': lambda m: np.asarray(build_theta, dtype=np.float64)}
    made = {}

    def precond(m):
        tb = at[blocks](m)
        tc = None if (build_theta is None or coarse is None) else at[coarse](m)
        key = (tuple(tb), None if tc is None else tuple(tc))
        if key not in made:
            made[key] = reduced_blocks_precond(B, tb) if tc is None else reduced_two_level(B, nbr, tb, tc)
        return made[key]
    return Cell(As, [precond(m) for m in range(nmu)], cols)


def reduced_euler_step(B, M_red, nbr, theta, dt, rhs, u0, mass_in_blocks=True, keep=None):
    """First step of lrbms3_reduced_implicit_euler from u0 [S, N]: the correction's system.  Mutant: inverse blocks of dt A alone."""
    S, N = np.asarray(M_red).shape[:2]
    A = par3.step_operator(B, M_red, nbr, theta, dt)
    u0 = np.asarray(u0, dtype=np.float64).reshape(S * N)
    f = par3.mass_operator(M_red) @ u0 + dt * np.asarray(rhs).reshape(S * N)
    col = f - A @ u0
    M = reduced_blocks_precond(B, theta, M_red if mass_in_blocks else None, dt)
    pad = None if keep is None else sp.diags(1.0 - np.asarray(keep, dtype=np.float64).ravel())
    return Cell(A, M, col, scale=[np.linalg.norm(col) / np.linalg.norm(f)], pad=pad)


# ---------------------------------------------------------------------------------------------------------- full order
class SparseCoarseFomPrecond3D(ref3.BatchFomPrecond3D):
    """The two-level preconditioner WITHOUT the cap of 8 192 coarse unknowns (a mutant reference on grids beyond it): the same
    R0 and Galerkin matrix, solved by a sparse LU instead of the dense Cholesky factor."""

    def __init__(self, A_blk, A_crs, S, n, Phi):
        super().__init__(A_blk, A_crs, S, n, None, coarse=0)
        self.R0 = sp.kron(sp.identity(S, format='csr'), np.asarray(Phi, dtype=np.float64).T, format='csr')
        self.lu = splu(sp.csc_matrix(self.R0 @ sp.csr_matrix(A_crs) @ self.R0.T))

    def _apply(self, r):
        return super()._apply(r) + self.R0.T @ self.lu.solve(self.R0 @ r)


def fom_precond(A_blk, A_crs, S, n, Phi, coarse=1, capped=True):
    if capped or Phi is None or coarse == 0:
        return ref3.BatchFomPrecond3D(A_blk, A_crs, S, n, Phi, coarse)
    return SparseCoarseFomPrecond3D(A_blk, A_crs, S, n, Phi)


def fom_single(Aq, S, n, Phi, theta, b, coarse=1, coarse_theta=None, capped=True):
    """lrbms3_fom_solve: ``BatchFomPrecond3D(A(theta), A(theta_coarse), ...)``, theta_coarse = theta unless a kept inverse was built
    at another parameter.  Mutants: ``coarse`` 0, ``coarse_theta``, ``capped`` False (P1 where the product falls back)."""
    A = ref3.combine(Aq, theta)
    P = fom_precond(A, A if coarse_theta is None else ref3.combine(Aq, coarse_theta), S, n, Phi, coarse, capped)
    c = Cell(A, P.apply, np.asarray(b).reshape(-1))
    c.precond = P
    return c


def oracle_mass(o):
    """The oracle's mass matrix with rows and columns in the product's order [S][n]."""
    perm = np.concatenate([np.asarray(o.dofs_of(s)) for s in range(o.S)])
    return o.M.tocsr()[perm][:, perm].tocsr()


def fom_euler_step(Aq, mass, S, n, Phi, theta, dt, b, u0, coarse=1, mass_in_blocks=True):
    """First step of lrbms3_fom_implicit_euler from u0 [S, n]: the correction's system, both levels on M + dt A(theta).
    Mutants: ``coarse`` 0, ``mass_in_blocks`` False (element blocks of dt A alone)."""
    dtA = dt * ref3.combine(Aq, theta)
    A = (sp.csr_matrix(mass) + dtA).tocsr()
    u0 = np.asarray(u0, dtype=np.float64).reshape(S * n)
    f = mass @ u0 + dt * np.asarray(b).reshape(S * n)
    col = f - A @ u0
    P = ref3.BatchFomPrecond3D(A if mass_in_blocks else dtA, A, S, n, Phi, coarse)
    c = Cell(A, P.apply, col, scale=[np.linalg.norm(col) / np.linalg.norm(f)])
    c.precond = P
    return c
