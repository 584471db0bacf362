"""Affine sources ``f = sum_j c_j f_j`` shared by the stationary and the parabolic 2D paths (DESIGN.md sections 5.4.1, 5.4.2).

The reference's ``discretize`` takes ``p['f'] = {'functions': [f_j], 'coefficients': [c_j]}``
(discretize_elliptic_block_swipdg.py:589-598).  One component with the literal coefficient 1 is the plain source every path
has always taken; anything else is set up here once per discretization: the load vectors ``b_K [K][S][n]``, the samples
``f_smp_K`` and the Grams ``F2 [S][K][K]``.  The coefficients are evaluated on the host (the library never evaluates an
expression): ``c_j(mu)`` on the stationary path, ``c_j(t, mu)`` on the parabolic one.
"""
import numpy as np


def source_components(p):
    """(functions, coefficients) of a source that is not one component with coefficient 1, else None."""
    f = p['f']
    if not isinstance(f, dict):
        return None
    funcs, coeffs = list(f['functions']), list(f['coefficients'])
    if len(funcs) != len(coeffs) or not funcs:
        raise ValueError("p['f'] needs as many coefficients as functions (and at least one)")
    if len(funcs) == 1 and not hasattr(coeffs[0], 'evaluate') and coeffs[0] == 1:
        return None
    return funcs, coeffs


def coefficient_parameter_type(c):
    """The parameter type a source coefficient reads ({} for a plain number); products read the union of their factors'."""
    if not hasattr(c, 'evaluate'):
        return {}
    if hasattr(c, 'factors'):
        out = {}
        for fac in c.factors:
            out.update(coefficient_parameter_type(fac))
        return out
    return dict(getattr(c, 'parameter_type', None) or {})


def check_coefficients(coeffs, parameter_type):
    """ValueError unless every coefficient's parameter type is contained in ``parameter_type`` (same names and shapes).  A
    coefficient of the time ``'_t'`` belongs to the parabolic path: NotImplementedError on the stationary one."""
    for j, c in enumerate(coeffs):
        for k, shape in coefficient_parameter_type(c).items():
            if k == '_t' and k not in parameter_type:
                raise NotImplementedError('source coefficient {} depends on the time (_t): a time-dependent source needs the '
                                          'parabolic discretize'.format(j))
            if k not in parameter_type or tuple(parameter_type[k]) != tuple(shape):
                raise ValueError("source coefficient {} reads the parameter {!r} of shape {}, which p['parameter_type'] = {} does "
                                 'not contain'.format(j, k, tuple(shape), dict(parameter_type)))


def evaluate_coefficients(coeffs, mu):
    """[K] fp64: the coefficients at the (parsed) parameter ``mu``; a plain number is a constant."""
    return np.array([c.evaluate(mu) if hasattr(c, 'evaluate') else float(c) for c in coeffs], dtype=np.float64)


def local_estimates(engine, U, theta, src, rows):
    """nc / r / df [S, len(U)] of the full-order vectors ``U`` [S, n, L] with the affine source ``src`` (``setup_sources``): every chunk
    of 16 vectors goes through the pass as a basis, the batched estimate runs with f2 = 0 and r_fd = 0, and the f terms of the
    residual indicator come from ``lrbms_project_sources`` on the same chunk and ``lrbms_reduced_source_terms`` with the
    coefficient row ``rows[l]`` of column l (``rows`` [L, K], host or device; None: no f terms).  Shared by the stationary and the
    parabolic path (DESIGN.md sections 5.4.1, 5.4.2)."""
    import torch
    eng, c = engine, engine.ctx
    zero_f2 = c.zeros(eng.S)
    out = []
    for c0 in range(0, U.shape[2], 16):
        V = U[:, :, c0:c0 + 16].contiguous()
        L = V.shape[2]
        buf = eng.project_and_estimate(V, project_system=False)
        grams = list(buf['grams'])
        grams[1] = torch.zeros_like(grams[1])                             # r_fd of the engine's own b (sum_j f_j): not used
        u = torch.eye(L, dtype=V.dtype, device=V.device).expand(eng.S, L, L).contiguous()
        eta = c.reduced_estimate_batch(np.tile(theta, (L, 1)), u, tuple(grams), zero_f2, eng.ceps, eng.hdiam)
        if rows is not None:
            D = c.div_apply(c.flux_reconstruct(eng.F, V), mode=0)
            _, r_fd_K = c.project_sources(eng.Q, src['b_K'], V, D)
            r = rows[c0:c0 + L]
            eta[1] += c.reduced_source_terms(theta, r.contiguous() if hasattr(r, 'contiguous') else np.ascontiguousarray(r), src['F2'],
                                             r_fd_K, u, eng.ceps, eng.hdiam)
        out.append(eta)
    eta = torch.cat(out, dim=2)
    return eta[0], eta[1], eta[2]


def setup_sources(engine, funcs, coeffs):
    """Load vectors b_K [K][S][n] (``lrbms_assemble_rhs`` per component) and Grams F2 [S][K][K] (``lrbms_assemble_source_gram``)
    of the K source components, sampled at the points of the engine's rules ``rhs`` / ``f2``.  Returns the source record."""
    import torch
    from pylrbms_amd.engine import sample_function, volume_record_points
    eng = engine
    sp = eng.quadrature
    xf, cl, kl = volume_record_points(eng.grid, eng.local, (sp.rhs, sp.f2))
    f_smp_K = eng.ctx.from_numpy(np.ascontiguousarray(np.stack([sample_function(fn, xf, cl, kl) for fn in funcs])))
    c = eng.ctx
    b_K, f2, ceps = c.empty(len(funcs), eng.S, eng.t.n), c.empty(eng.S), c.empty(eng.S)      # (f2, ceps of a component: not used)
    for j in range(len(funcs)):
        c.assemble_rhs(f_smp_K[j].contiguous(), eng.lhat, out=(b_K[j], f2, ceps))              # straight into its slab of b_K
    F2 = eng.ctx.assemble_source_gram(f_smp_K)
    return {'functions': funcs, 'coefficients': coeffs, 'K': len(funcs), 'f_smp_K': f_smp_K, 'b_K': b_K, 'F2': F2}
