"""NumPy restatement of lrbms3_fom_solve_batch (pylrbms_amd/csrc/lrbms3d.hip) on top of tests/pcg_ref.py.

Column m of a call solves A(theta_m) x_m = sum_j phi[m][j] b_K[j] from x = 0 by PCG with ONE preconditioner per call,

    M^-1 = blockdiag_10(A(theta_bar))^-1 + R0^T (R0 A(theta_bar) R0^T)^-1 R0,

theta_bar[q] = (1 / nmu) sum_m theta[m][q] summed in column order: the inverse 10 x 10 element blocks AND the coarse level are
built at the call mean (in 2D, tests/fom_batch_ref.py, the element blocks are the column's own).  The rows of R0 are the nc <= 4
functions per subdomain of ``lrbms3_fom_coarse_space`` (``default_phi``: what ``Native3DContext.mesh_upload`` installs, P1 in
the subdomain-local coordinates).  Without a coarse level (``coarse`` 0, no functions, more than 8 192 coarse unknowns, a coarse
matrix that is not positive definite) the element blocks run alone.

The sparse operator is built from the product's layouts A_diag [Q, S, n_T, 5, 100] / A_cpl [Q, S, 6, ncf, 100]: block 0 of an
element is its own 10 x 10 block, block 1 + f the one towards ``nb_elem[e, f]`` inside the subdomain; a face on side ``side`` of
the subdomain couples through A_cpl[.., side, face_pos[e, f]] with element ``nb_out[e, f]`` of the neighbour in slot
``SIDE_TO_SLOT[side]`` (the maps of ``common3d.oracle_assembled``)."""
import numpy as np
import scipy.sparse as sp

import pcg_ref

COARSE_MAX = 8192                         # lrbms3d.hip FOM_MAX_COARSE


def default_phi(template):
    """Phi [n, 4] of ``Native3DContext.mesh_upload``: 1 and the three local coordinates, centred and scaled by the extent."""
    x = np.asarray(template.node_coordinates(), dtype=np.float64)
    ext = x.max(axis=0) - x.min(axis=0)
    return np.concatenate([np.ones((template.n, 1)), (x - 0.5 * (x.max(axis=0) + x.min(axis=0))) / ext], axis=1)


def component_operators(A_diag, A_cpl, template, nbr):
    """[A_q]: the Q sparse [S n, S n] components of the full-order operator from the product's block layouts."""
    from pylrbms_amd.grid3d import SIDE_TO_SLOT
    t = template
    A_diag, A_cpl, nbr = np.asarray(A_diag, dtype=np.float64), np.asarray(A_cpl, dtype=np.float64), np.asarray(nbr)
    Q, S = A_diag.shape[0], A_diag.shape[1]
    nT, n = t.n_T, t.n
    nb_elem, nb_out, face_pos = (np.asarray(a).reshape(nT, 4) for a in (t.nb_elem, t.nb_out, t.face_pos))
    ii, jj = np.meshgrid(np.arange(10), np.arange(10), indexing='ij')
    e = np.arange(nT)
    rows, cols, pick = [], [], []          # pick: (array 0 = A_diag / 1 = A_cpl, s, index arrays into [.., 100])

    def put(s, er, s2, ec, which, idx):
        rows.append((s * n + 10 * er[:, None, None] + ii).ravel())
        cols.append((s2 * n + 10 * ec[:, None, None] + jj).ravel())
        pick.append((which, s, idx))

    for s in range(S):
        put(s, e, s, e, 0, (e, np.zeros(nT, dtype=int)))
        for f in range(4):
            inner = nb_elem[:, f] >= 0
            put(s, e[inner], s, nb_elem[inner, f], 0, (e[inner], np.full(int(inner.sum()), 1 + f)))
            for side in range(6):
                on = nb_elem[:, f] == -(1 + side)
                s2 = int(nbr[s, SIDE_TO_SLOT[side]])
                if s2 >= 0 and on.any():
                    put(s, e[on], s2, nb_out[on, f], 1, (np.full(int(on.sum()), side), face_pos[on, f]))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    out = []
    for q in range(Q):
        src = (A_diag[q].reshape(S, nT, 5, 100), A_cpl[q].reshape(S, 6, t.ncf, 100))
        data = np.concatenate([src[which][s][idx].ravel() for which, s, idx in pick])
        out.append(sp.csr_matrix((data, (rows, cols)), shape=(S * n, S * n)))
    return out


def combine(Aq, theta):
    A = float(theta[0]) * Aq[0]
    for q in range(1, len(Aq)):
        A = A + float(theta[q]) * Aq[q]
    return A.tocsr()


def mean_theta(thetas):
    """theta_bar of a call: summed in column order, then divided by nmu."""
    thetas = np.asarray(thetas, dtype=np.float64)
    acc = np.zeros(thetas.shape[1])
    for row in thetas:
        acc = acc + row
    return acc / thetas.shape[0]


class BatchFomPrecond3D:
    """blockdiag_10(A_blk)^-1 + R0^T (R0 A_crs R0^T)^-1 R0 with R0 = I_S (x) Phi^T.  ``Phi`` None or ``coarse`` 0: blocks alone."""

    def __init__(self, A_blk, A_crs, S, n, Phi, coarse=1):
        self.S, self.n = S, n
        self.Minv = np.linalg.inv(pcg_ref.diagonal_blocks(A_blk, 10))
        self.R0 = self.A1 = self.cho = None
        nc = 0 if (Phi is None or coarse == 0) else int(np.asarray(Phi).shape[1])
        if nc > 1 and nc * S > COARSE_MAX:
            nc = 1
        if nc * S > COARSE_MAX:
            nc = 0
        if nc > 0:
            R0 = sp.kron(sp.identity(S, format='csr'), np.asarray(Phi, dtype=np.float64)[:, :nc].T, format='csr')
            self.A1 = (R0 @ sp.csr_matrix(A_crs) @ R0.T).toarray()
            self.cho = pcg_ref._coarse_factor(self.A1)
            self.R0 = R0 if self.cho is not None else None
        self.apply = pcg_ref._as2d(self._apply)

    @property
    def has_coarse(self):
        return self.cho is not None

    def _apply(self, r):
        import scipy.linalg as sla
        m = r.shape[1]
        z = np.einsum('eij,ejm->eim', self.Minv, r.reshape(-1, 10, m)).reshape(-1, m)
        if self.cho is not None:
            z = z + self.R0.T @ sla.cho_solve(self.cho, self.R0 @ r)
        return z


class BatchFom3DRef:
    """Operators, right-hand sides and preconditioners of one call: thetas [nmu, Q], phi [nmu, K], b_K [K, S, n].
    Switches for the mutant references: ``coarse`` 0 (no coarse level), ``coarse_theta`` (where the coarse level is built;
    default the call mean), ``block_theta`` (where the element blocks are inverted: default the call mean, 'own' = every column
    at its own theta, or a theta)."""

    def __init__(self, A_diag, A_cpl, template, nbr, thetas, phi, b_K, Phi='default', coarse=1, coarse_theta=None, block_theta=None,
                 Aq=None):
        self.thetas = np.asarray(thetas, dtype=np.float64)
        self.nmu = self.thetas.shape[0]
        S, n = np.asarray(A_diag).shape[1], template.n
        self.S, self.n = S, n
        Phi = default_phi(template) if isinstance(Phi, str) else Phi
        self.Aq = component_operators(A_diag, A_cpl, template, nbr) if Aq is None else Aq      # (a cell's mutants share them)
        self.As = [combine(self.Aq, th) for th in self.thetas]
        tb = mean_theta(self.thetas)
        self.A_bar = combine(self.Aq, tb)
        A_crs = self.A_bar if coarse_theta is None else combine(self.Aq, coarse_theta)
        if isinstance(block_theta, str):
            assert block_theta == 'own'
            self.Ms = [BatchFomPrecond3D(A, A_crs, S, n, Phi, coarse) for A in self.As]
        else:
            A_blk = self.A_bar if block_theta is None else combine(self.Aq, block_theta)
            self.Ms = [BatchFomPrecond3D(A_blk, A_crs, S, n, Phi, coarse)] * self.nmu
        K = np.asarray(b_K).shape[0]
        self.cols = np.einsum('mk,kn->nm', np.asarray(phi, dtype=np.float64), np.asarray(b_K, dtype=np.float64).reshape(K, -1))

    @property
    def has_coarse(self):
        return self.Ms[0].has_coarse

    def iterate(self, k):
        """The ``reference(k)`` of ``check_iterates``: (X_k [S n, nmu], ratios [nmu])."""
        out = [pcg_ref.pcg_iterate(lambda p, A=A: A @ p, M.apply, self.cols[:, j], k)
               for j, (A, M) in enumerate(zip(self.As, self.Ms))]
        return np.stack([x for x, _ in out], axis=1), np.array([r for _, r in out])

    def solve(self, j):
        from scipy.sparse.linalg import spsolve
        return spsolve(self.As[j].tocsc(), self.cols[:, j])
