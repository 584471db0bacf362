"""Affine sources ``f = sum_j c_j f_j`` on the 3D / P2 path: the 3D counterpart of
``pylrbms_amd.sources``, shared by the stationary and the parabolic 3D discretizations.

The 3D problem dict has no ``parameter_type``: mu is a plain number, and a source coefficient is a plain number or a plain
callable, like ``p['lambda']['coefficients']``.  A callable is called as ``c(mu)``, or as ``c(mu, t)`` on the parabolic path if
it takes two positional arguments; which of the two is decided once per coefficient, from its signature.  Coefficient objects
with an ``.evaluate`` method (functionals over a named parameter type) and sharded grids belong to the 2D path.

One component with the literal coefficient 1 is the plain source the path has always taken; anything else is set up here once
per discretization: the samples ``f_smp_K``, the load vectors ``b_K [K][S][n]``, the element integrals ``bdiv_K [K][S][n_T]``
and the Grams ``F2 [S][K][K]``.  The engine itself is built on ``sum_j f_j``.
"""
import inspect
import numbers

import numpy as np


def coefficient_arity(c, what='source coefficient'):
    """0 for a plain number, 1 for a callable ``c(mu)``, 2 for a callable ``c(mu, t)`` -- from the signature, never by trying a
    call.  Anything else is a TypeError, a callable whose signature cannot be read included.

    The rule: only positional parameters WITHOUT a default count.  A defaulted parameter is a bound constant, not an argument the
    path supplies -- the problem files write ``lambda mu, q=q: mu ** q`` to bind a loop variable -- so ``c(mu, t=0.0)`` is a
    coefficient of mu alone and never receives the time; a coefficient that reads t declares it without a default.

    ``what`` names the coefficient in the messages: the diffusion coefficients of the parabolic path go by the same rule."""
    if isinstance(c, numbers.Real) and not isinstance(c, bool):
        return 0
    if not callable(c):
        raise TypeError('a {} of the 3D path is a number or a callable, not {!r}'.format(what, type(c).__name__))
    kinds = (inspect.Parameter.POSITIONAL_ONLY, inspect.Parameter.POSITIONAL_OR_KEYWORD)
    try:
        sig = inspect.signature(c)
    except ValueError as exc:                      # some builtins and C callables carry no signature
        raise TypeError('the signature of the {} {!r} cannot be read ({}): wrap it in a function of (mu) or '
                        '(mu, t)'.format(what, c, exc))
    pos = [q for q in sig.parameters.values() if q.kind in kinds and q.default is inspect.Parameter.empty]
    if len(pos) not in (1, 2):
        raise TypeError('a {} takes (mu) or (mu, t); this one takes {} positional arguments'.format(what, len(pos)))
    return len(pos)


def check_sources3d(grid, coeffs):
    """The refusals of the 3D path, before any device work; returns the arities of the coefficients."""
    if any(hasattr(c, 'evaluate') for c in coeffs):
        raise NotImplementedError('a source coefficient with .evaluate (a functional over a named parameter type) exists on the 2D path '
                                  'only: the 3D path takes plain numbers and callables c(mu) / c(mu, t)')
    if getattr(grid, 'world_size', 1) > 1:
        raise NotImplementedError('a multi-component / parameter-dependent source on a sharded grid exists on the 2D path only: the 3D '
                                  'path takes it on one rank')
    return [coefficient_arity(c) for c in coeffs]


def sum_function(funcs):
    """x -> sum_j f_j(x): what the engine is built on."""
    funcs = list(funcs)

    def f_sum(x):
        out = np.asarray(funcs[0](x), dtype=np.float64)
        for fn in funcs[1:]:
            out = out + np.asarray(fn(x), dtype=np.float64)
        return out
    return f_sum


def evaluate_stationary(src, mu):
    """[K] fp64: the coefficients at ``mu``.  NotImplementedError if one of them reads the time."""
    if any(a == 2 for a in src['arity']):
        raise NotImplementedError('the source depends on time (a coefficient c(mu, t)): this needs the parabolic solve')
    return np.array([float(c) if a == 0 else float(c(mu)) for c, a in zip(src['coefficients'], src['arity'])], dtype=np.float64)


def table_times(dt, nt):
    """[nt + 1] fp64: t_k = k dt, the time of row k of every per-step table (the source's phi and the diffusion's theta_t): the one
    place the times come from, so the two cannot disagree on t_k."""
    return np.array([k * float(dt) for k in range(int(nt) + 1)], dtype=np.float64)


def diffusion_arities(coeffs):
    """The arities of the diffusion coefficients ``p['lambda']['coefficients']``: plain callables c(mu) or c(mu, t)."""
    ar = [coefficient_arity(c, 'diffusion coefficient') for c in coeffs]
    if 0 in ar:
        raise TypeError('a diffusion coefficient of the 3D path is a callable c(mu) or c(mu, t), not a number')
    return ar


def evaluate_table(src, mu, dt, nt):
    """[nt + 1][K] fp64: row k holds the coefficients at t_k = k dt.  Step k -> k + 1 of implicit Euler uses row k + 1, the elliptic
    part of U_k in the estimate uses row k."""
    out = np.empty((int(nt) + 1, len(src['coefficients'])), dtype=np.float64)
    for k, t in enumerate(table_times(dt, nt).tolist()):
        out[k] = [float(c) if a == 0 else float(c(mu)) if a == 1 else float(c(mu, t)) for c, a in zip(src['coefficients'], src['arity'])]
    return out


def setup_sources3d(engine, funcs, coeffs, arity):
    """The source record of K components sampled at the points ``Engine3D`` samples ``f`` at: ``f_smp_K`` [K, S, n_T, f_stride],
    ``b_K`` [K, S, n] and ``bdiv_K`` [K, S, n_T] (``lrbms3_assemble_rhs`` per component), ``F2`` [S, K, K]
    (``lrbms3_assemble_source_gram``)."""
    import torch
    from pylrbms_amd.engine3d import sample
    eng, c = engine, engine.ctx
    _, xh, _ = eng.t.record_points(eng.spec)
    org = np.stack([eng.grid.subdomain_origin(s) for s in eng.local])
    f_smp_K = c.from_numpy(np.stack([np.stack([sample(fn, xh + o) for o in org]) for fn in funcs]))
    parts = [c.assemble_rhs(f_smp_K[j].contiguous(), eng.lhat) for j in range(len(funcs))]
    b_K = torch.stack([q[0] for q in parts]).contiguous()
    bdiv_K = torch.stack([q[3] for q in parts]).contiguous()
    return {'functions': list(funcs), 'coefficients': list(coeffs), 'arity': list(arity), 'K': len(funcs), 'f_smp_K': f_smp_K,
            'b_K': b_K, 'bdiv_K': bdiv_K, 'F2': c.assemble_source_gram(f_smp_K)}


def zeroed(engine, out):
    """(out, ops) for an estimate without its f terms: r_fd, f2 and bdiv replaced by zeros (the indicator is affine in them)."""
    c = engine.ctx
    QN = int(out['G_bb'].shape[1])
    cache = engine.__dict__.setdefault('_zero_source_terms', {})          # read-only zeros, kept per engine (r_fd per QN)
    if 'ops' not in cache:
        cache['ops'] = dict(f2=c.zeros(engine.S), bdiv=c.zeros(engine.S, engine.t.n_T))
    if QN not in cache:
        cache[QN] = c.zeros(engine.S, QN)
    return dict(out, r_fd=cache[QN]), dict(engine.ops, **cache['ops'])


def source_terms(engine, Q, src, thetas, rows, r_fd_K, out, u):
    """``lrbms3_reduced_source_terms`` for the columns u [S, N, L] with ``thetas`` [L, Q] and coefficient rows ``rows`` [L, K]."""
    return engine.ctx.reduced_source_terms(Q, thetas, rows, src['F2'], r_fd_K, src['bdiv_K'], out['Rb'], u, engine.ops['ceps'],
                                           engine.hdiam)
