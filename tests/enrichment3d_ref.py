"""CPU reference of the 3D neighbourhood corrector problems (reference block_swipdg.py:227-316), built on
``oracle.lrbms3d.Discretization3D``.  Test infrastructure only: the product never imports it.

The corrector of subdomain ``ii`` at ``mu`` is the SWIPDG problem on N(ii) = ii and its face neighbours: every face with exactly
one side in N(ii) is a Dirichlet face seen from the inside element, the right-hand side is the L2 functional of f, the solution
is restricted to ii.  In matrix terms: ``d.system_matrix(mu)`` restricted to the DoFs of N(ii), plus, on every coupling face with
exactly one side inside, theta-weighted (Dirichlet-face block of the inside element - inner-face own / own block that the
system matrix already holds).  Both blocks are evaluated with the oracle's own face points, basis evaluation and constants;
on the plus side of a face the outward normal is minus the stored one.

Validated in tests/test_enrichment3d_host.py: (1) summed over all coupling faces and both sides the correction turns the
element-diagonal blocks of A_q into those of ``d._swipdg(fn, False, True)`` (every subdomain boundary a Dirichlet face);
(2) on a 3 x 1 x 1 strip the correctors of the end subdomains equal independent oracles on the 2 x 1 x 1 boxes; (3) a
neighbourhood that is the whole domain gives ``d.solve(mu)``."""
import numpy as np
import scipy.sparse.linalg as spla

from oracle.lrbms3d import BETA_3D, NLOC, SIGMA_BOUNDARY_P2, SIGMA_INNER_P2, _feval


def coupling_corrections(d, q):
    """(faces [F], minus [F, 10, 10], plus [F, 10, 10]) for component q: per coupling face the correction block of the element
    on its minus and on its plus side, each = Dirichlet-face block seen from that element - inner-face own / own block."""
    cache = d.__dict__.setdefault('_enrichment_corrections', {})
    if q in cache:
        return cache[q]
    m, K, fn = d.mesh, d.kappa, d.lambda_funcs[q]
    faces = np.nonzero(m.face_is_coupling)[0]
    xq, wq = d._face_points(faces, d.deg + 4)
    lm = _feval(fn, xq)
    area = m.face_area[faces]
    ww = wq[None, :] * area[:, None]
    out = []
    for side, sgn in ((m.face_minus, 1.0), (m.face_plus, -1.0)):
        E = side[faces, 0]
        nrm = sgn * m.face_normal[faces]                                   # outward from the element of this side
        ph, gr = d._face_side(E, None, xq)
        delta = np.einsum('fa,ab,fb->f', nrm, K, nrm)
        D = np.einsum('fk,ab,fkib,fa->fki', lm, K, gr, nrm)                # lambda kappa grad phi . n
        sym = ph[..., :, None] * D[..., None, :] + D[..., :, None] * ph[..., None, :]
        pp = ph[..., :, None] * ph[..., None, :]
        sig_b = lm * SIGMA_BOUNDARY_P2 * delta[:, None] / area[:, None] ** BETA_3D
        sig_i = lm * SIGMA_INNER_P2 * 0.5 * delta[:, None] / area[:, None] ** BETA_3D
        dirichlet = np.einsum('fk,fkij->fij', ww, -sym + sig_b[..., None, None] * pp)
        inner = np.einsum('fk,fkij->fij', ww, -0.5 * sym + sig_i[..., None, None] * pp)
        out.append(dirichlet - inner)
    cache[q] = (faces, out[0], out[1])
    return cache[q]


def correction_matrix(d, q, inside=None):
    """Sparse [ndof, ndof]: the correction blocks of component q on the element-diagonal.  ``inside``: boolean per subdomain --
    only faces with exactly one side inside, on the inside element; None: every coupling face, both sides."""
    m = d.mesh
    faces, cm, cp = coupling_corrections(d, q)
    Em, Ep = m.face_minus[faces, 0], m.face_plus[faces, 0]
    if inside is None:
        km = kp = np.ones(len(faces), dtype=bool)
    else:
        im, ip = inside[m.elem_subdomain[Em]], inside[m.elem_subdomain[Ep]]
        km, kp = im & ~ip, ip & ~im
    return (d._scatter(Em[km], Em[km], cm[km], d.ndof) + d._scatter(Ep[kp], Ep[kp], cp[kp], d.ndof)).tocsr()


def hood_dofs(d, ii):
    return np.concatenate([d.dofs_of(kk) for kk in d.mesh.neighborhood_of(ii)])


def hood_system(d, ii, mu):
    """The operator of the corrector problem of subdomain ii at mu on the DoFs of N(ii) (neighbourhood in ascending order)."""
    inside = np.zeros(d.S, dtype=bool)
    inside[d.mesh.neighborhood_of(ii)] = True
    A = d.system_matrix(mu)
    for t, q in zip(d.theta(mu), range(d.Q)):
        A = A + t * correction_matrix(d, q, inside)
    dofs = hood_dofs(d, ii)
    return A.tocsr()[dofs][:, dofs].tocsc()


def corrector(d, ii, mu, b=None):
    """The corrector of subdomain ii [n]: sparse LU of ``hood_system`` against the load ``b`` (default ``d.b``), restricted to ii."""
    b = d.b if b is None else np.asarray(b).ravel()
    x = spla.spsolve(hood_system(d, ii, mu), b[hood_dofs(d, ii)])
    k = d.mesh.neighborhood_of(ii).index(ii)
    return x[k * d.n:(k + 1) * d.n]


def dcorr_layout(p, d):
    """The per-face correction blocks in the product's layout D_corr [Q, S, 6, ncf, 10, 10] (zero on physical sides and on padded
    positions) for the common3d problem ``p`` with oracle ``d``."""
    from pylrbms_amd.grid3d import SIDE_TO_SLOT
    grid, t, m = p['grid'], p['grid'].template, d.mesh
    out = np.zeros((d.Q, d.S, 6, t.ncf, NLOC, NLOC))
    for q in range(d.Q):
        faces, cm, cp = coupling_corrections(d, q)
        where = {int(f): k for k, f in enumerate(faces)}
        for s in range(d.S):
            el = m.elements_of(s)
            for a in range(6):
                if grid.neighbor_slots[s, SIDE_TO_SLOT[a]] < 0:
                    continue
                for pos in range(t.ncf):
                    e, f = int(t.side_elem[a, pos]), int(t.side_face[a, pos])
                    if e < 0:
                        continue
                    fid = int(m.elem_face[el[e], f])
                    k = where[fid]
                    out[q, s, a, pos] = cm[k] if m.face_minus[fid, 0] == el[e] else cp[k]
    return out
