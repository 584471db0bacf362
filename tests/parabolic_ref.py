"""NumPy / SciPy restatements of the side kernels of the 2D parabolic path, for tests/test_parabolic_dispatch_gpu.py.

The full-order references are built from oracle objects only (``o.l2_product``, ``o.Div[ii]``, ``o.block``,
``o.assemble_global``, ``OracleReductor.image_bases``): sparse matrices applied as matrices, nothing per element, no template
table and no slot loop of the kernels.  The reduced ones work on the arrays a call takes (B_sys [Q, S, 5, N, N], M_red [S, N, N],
the slot table ``nbr`` [S, 5]) through the sparse operator of tests/pcg_ref.py and dense solves.

Every function takes ``fault``: one of FAULTS switches it to a wrong variant a kernel could compute (a fault a function does not
have leaves it unchanged).  tests/test_parabolic_dispatch_host.py pins the right variants to oracle/parabolic.py and shows that
the cells of the GPU module tell every wrong one apart."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import pcg_ref
from oracle.lrbms import OracleReductor

FAULTS = ('drop_r_ud',              # the -2 r_ud term dropped
          'mass_not_inverse',       # M instead of M^-1
          'boundary_sign',          # the sign of a domain-boundary face not forced to +1
          'mass_every_slot',        # the mass added to every slot instead of slot 2
          'first_64',               # first 64 entries only
          'drop_last_chunk',        # the last chunk of 16 columns dropped
          'theta_q2')               # theta_q of q >= 2 ignored
CHUNK = 16                          # columns per trip of InstationaryDuneDiscretization._reconstruction_terms


def _theta(theta, fault):
    th = np.array(theta, dtype=np.float64)
    if fault == 'theta_q2':
        th[2:] = 0.0
    return th


def local_mass(o, ii):
    return sp.csr_matrix(o.block(o.l2_product, ii, ii))


# ------------------------------------------------------------------------------------------------------------ full order
def mass_inverse_norm2(o, Y, fault=None):
    """Y [S, n, L] -> y^T M^-1 y per subdomain and column [S, L], by a sparse LU of ``o.l2_product``."""
    Y = np.asarray(Y, dtype=np.float64)
    S, n, L = Y.shape
    M = sp.csc_matrix(o.l2_product)
    flat = Y.reshape(S * n, L)
    if fault == 'first_64':
        flat = flat * (np.arange(S * n) % n < 64)[:, None]
    Z = M @ flat if fault == 'mass_not_inverse' else spla.splu(M).solve(flat)
    return (flat * Z).reshape(S, n, L).sum(axis=1)


def divergence(o, ii, fault=None):
    """``o.Div[ii]`` [n, n_rt].  'boundary_sign': the column of a domain-boundary face carries the sign of the orientation rule of
    the faces inside the domain (+1 for the lexicographically positive normal, else -1) instead of +1."""
    D = sp.csr_matrix(o.Div[ii])
    if fault != 'boundary_sign':
        return D
    m = o.mesh
    faces = np.asarray(m.rt_faces[ii])
    nrm = m.face_normal[faces]
    positive = (nrm[:, 0] > 1e-12) | ((np.abs(nrm[:, 0]) <= 1e-12) & (nrm[:, 1] > 0))
    sign = np.where((m.face_kind[faces] == 2) & ~positive, -1.0, 1.0)
    return sp.csr_matrix(D @ sp.diags(sign))


def div_rows(o, Rt, mode, fault=None):
    """Rt [S, n_rt, C].  mode 0: the divergence per element [S, n_T, C] (every third row of Div Rt: its three rows of an element
    are equal); mode 1: M_ii Div_ii Rt_ii [S, n, C]."""
    Rt = np.asarray(Rt, dtype=np.float64)
    out = []
    for ii in range(o.S):
        D = divergence(o, ii, fault) @ Rt[ii]
        out.append(D[::3] if mode == 0 else local_mass(o, ii) @ D)
    return np.stack(out)


def div_pairing(o, theta, Rt_slots, G, fault=None):
    """Rt_slots [S, n_rt, 5 Q L] (columns (slot, q, l)), G [S, n, L] -> [S, L]:  G[ii]^T M_ii^-1 M_ii Div_ii Rt_ii theta."""
    th = _theta(theta, fault)
    Q = len(th)
    Rt_slots, G = np.asarray(Rt_slots, dtype=np.float64), np.asarray(G, dtype=np.float64)
    S, nrt, C = Rt_slots.shape
    L = C // (5 * Q)
    out = np.zeros((S, L))
    for ii in range(S):
        Ur = np.einsum('q,rsql->rl', th, Rt_slots[ii].reshape(nrt, 5, Q, L))
        M = local_mass(o, ii)
        MD = M @ (divergence(o, ii, fault) @ Ur)
        Z = M @ MD if fault == 'mass_not_inverse' else spla.splu(sp.csc_matrix(M)).solve(MD)
        out[ii] = np.einsum('nl,nl->l', G[ii], Z)
    return out


def reconstruction_terms_full(o, U, mu, fault=None):
    """U [L, S, n] -> [3, S, L]: r_l2(BU_R, BU_R), r_l2(F_R, F_R) and r_ud(BU_R - F_R, U_r) per subdomain and vector, with
    BU_R = M^-1 A(mu) U, F_R = M^-1 b and U_r the flux reconstruction of U on the subdomain (all sources, all components)."""
    U = np.asarray(U, dtype=np.float64)
    L, S, n = U.shape
    m = o.mesh
    th = _theta(o.theta(mu), fault)
    A = o.assemble_global(mu)
    M = sp.csc_matrix(o.l2_product)
    lu = spla.splu(M)
    apply = (lambda x: M @ x) if fault == 'mass_not_inverse' else lu.solve
    F_R = apply(o.b)
    BU_R = apply(A @ U.reshape(L, S * n).T)                                  # [S n, L]
    # the L vectors as one basis of L columns: RT[kk][i] is [n_rt, Q L], columns (q, l)
    OI, RT = OracleReductor(o, [U[:, ii, :].T for ii in range(S)]).image_bases()
    out = np.zeros((3, S, L))
    for ii in range(S):
        sl = slice(ii * n, (ii + 1) * n)
        M_ii = local_mass(o, ii)
        ur = sum(np.einsum('q,rql->rl', th, RT[kk][m.neighborhood_of(kk).index(ii)].reshape(-1, len(th), L))
                 for kk in m.neighborhood_of(ii))
        MD = M_ii @ (divergence(o, ii, fault) @ ur)                          # [n, L]
        out[0, ii] = np.einsum('nl,nl->l', BU_R[sl], M_ii @ BU_R[sl])
        out[1, ii] = F_R[sl] @ (M_ii @ F_R[sl])
        out[2, ii] = np.einsum('nl,nl->l', BU_R[sl] - F_R[sl][:, None], MD)
    if fault == 'drop_last_chunk':
        out[:, :, CHUNK * ((L - 1) // CHUNK):] = 0.0
    return out


def summed(terms, fault=None):
    """t1 - t2 - 2 t3 of a stack of the three terms (first axis)."""
    return terms[0] - terms[1] - (0.0 if fault == 'drop_r_ud' else 2.0) * terms[2]


def magnitude(terms):
    """|t1| + |t2| + 2 |t3|: what the summed output is compared relative to."""
    return np.abs(terms[0]) + np.abs(terms[1]) + 2.0 * np.abs(terms[2])


# ---------------------------------------------------------------------------------------------------------------- reduced
def _regular(M_red):
    """M_red with 1 on the diagonal of a zero-padded unknown (zero row and column)."""
    M = np.array(M_red, dtype=np.float64)
    S, N, _ = M.shape
    d = M[:, np.arange(N), np.arange(N)]
    d[d == 0.0] = 1.0
    M[:, np.arange(N), np.arange(N)] = d
    return M


def _mass_apply(M_red, fault):
    M = _regular(M_red)
    if fault == 'mass_not_inverse':
        return lambda s, y: M[s] @ y
    return lambda s, y: np.linalg.solve(M[s], y)


def reduced_operator(B, nbr, theta, fault=None):
    return pcg_ref.reduced_operator(pcg_ref.combine_reduced(B, _theta(theta, fault)), nbr)


def reduced_time_residual(B, M_red, nbr, theta, dU, fault=None):
    """dU [L, S, N] -> y^T M_red[s]^-1 y [L, S] with y = (sum_q theta_q B_q dU_l)_s, any Q."""
    dU = np.asarray(dU, dtype=np.float64)
    L, S, N = dU.shape
    A = reduced_operator(B, nbr, theta, fault)
    Minv = _mass_apply(M_red, fault)
    out = np.zeros((L, S))
    for l in range(L):
        y = (A @ dU[l].reshape(S * N)).reshape(S, N)
        for s in range(S):
            out[l, s] = y[s] @ Minv(s, y[s])
    return out


def reduced_reconstruction_terms(B, M_red, rhs, G_ud, nbr, theta, U, fault=None):
    """U [L, S, N] -> [3, L, S]: y^T M_red^-1 y, b^T M_red^-1 b and (M_red^-1 (y - b))^T G_ud ur with y = (A_red(theta) u_l)_s,
    b = rhs[s] and ur the theta-weighted coefficients of the five slots in column order (slot, q, j); G_ud [S, N, 5 Q N]."""
    U, rhs, G_ud = (np.asarray(x, dtype=np.float64) for x in (U, rhs, G_ud))
    L, S, N = U.shape
    th = _theta(theta, fault)
    Q = len(th)
    nbr = np.asarray(nbr)
    A = reduced_operator(B, nbr, theta, fault)
    Minv = _mass_apply(M_red, fault)
    out = np.zeros((3, L, S))
    for l in range(L):
        y = (A @ U[l].reshape(S * N)).reshape(S, N)
        for s in range(S):
            ur = np.zeros((5, Q, N))
            for slot in np.nonzero(nbr[s] >= 0)[0]:
                ur[slot] = th[:, None] * U[l, nbr[s, slot]][None, :]
            ur = ur.reshape(-1)
            if fault == 'first_64':
                ur[64:] = 0.0
            out[0, l, s] = y[s] @ Minv(s, y[s])
            out[1, l, s] = rhs[s] @ Minv(s, rhs[s])
            out[2, l, s] = Minv(s, y[s] - rhs[s]) @ (G_ud[s] @ ur)
    return out


def step_blocks(B, M_red, theta, dt, fault=None):
    """dt A(theta) + M_red in the fixed-slot layout [S, 5, N, N].  'mass_every_slot': M_red on all five slots; 'no_mass': on
    none."""
    Amu = dt * pcg_ref.combine_reduced(B, _theta(theta, fault))
    if fault == 'mass_every_slot':
        Amu += np.asarray(M_red)[:, None]
    elif fault != 'no_mass':
        Amu[:, 2] += np.asarray(M_red)
    return Amu


def mass_preconditioner(B, M_red, nbr, theta, dt, fault=None, coarse=1):
    """The preconditioner of the single reduced implicit Euler: the inverse diagonal blocks of M_red + dt A_ss plus the coarse
    level, as ``pcg_ref.ReducedPrecond`` (``.apply``, ``.has_coarse``)."""
    return pcg_ref.ReducedPrecond(step_blocks(B, M_red, theta, dt, fault), nbr, coarse)
