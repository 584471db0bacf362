"""Parabolic block SWIPDG P2 discretization in 3D on the HIP path: the 3D counterpart of
``pylrbms_amd.discretize_parabolic_block_swipdg`` (reference discretize_parabolic_block_swipdg.py:17-95, estimators.py:139-168).

``M u' + A(mu) u = f`` with the block L2 product as mass, zero initial data and implicit Euler with ``nt`` steps:

    d, data = discretize(grid_and_problem_data, T, nt)     # the elliptic 3D discretize + T, time_stepper, initial_data
    U = d.solve(mu)                                       # [S, n, nt + 1]: ONE native call (lrbms3_fom_implicit_euler)
    Us = d.solve_batch(mus)                               # a training set, 64 trajectories per native call
    d.estimate(U, mu)                                     # est, (local_eta_nc, local_eta_r, local_eta_df, time_residual, time_deriv_nc)
    reductor = ParabolicLRBMSReductor3D(d)
    reductor.extend_basis(U[:, :, idx]);  rd = reductor.reduce()
    u = rd.solve(mu);  rd.estimate(u, mu);  reductor.reconstruct(u)
    us = rd.solve_batch(mus);  rd.estimate_batch(us, mus, native=True)     # sweeps: 64 parameters per native call

Online enrichment (2D: 5.3.1) is opt-in, as on the elliptic 3D path: ``discretize(..., online_enrichment=True)``
also assembles the corrector data.  Then

    d.solve_for_local_correction_trajectories(subdomains, mu)     # [nmark, n, nt]: ONE native call (lrbms3_local_correction_euler)
    reductor.enrich_local_batch(marked, u, mu, pod_modes=2);  rd = reductor.reduce(touched=marked)
    est, parts, indicators = rd.estimate(u, mu, decompose=True)   # what AdaptiveEnrichment(..., pod_modes=) marks with

The estimate restates ``OracleParabolic.estimate`` (oracle/parabolic.py): the elliptic terms of every vector of the trajectory,
scaled by 2 sqrt(dt / 3); ``time_residual_k = sqrt(dt / 3 * sum_s y^T M_s^-1 y)`` with ``y = A(mu) (U_{k+1} - U_k)``;
``time_deriv_nc = sqrt(max(nc(dU), 0) / dt)``; ``est = |eta| + |time_residual| + |time_deriv_nc|``.

Diffusion coefficients of the time (2D: 5.4.6): a ``p['lambda']['coefficients']`` entry with the signature
``c(mu, t)`` makes the discretization time-dependent (``d._tv``).  ``d.diffusion_coefficients(mu)`` is the table theta_t [nt + 1, Q]
at the times of the source table; the step k -> k + 1 solves with row k + 1.  ``solve`` / ``solve_batch``, ``rd.solve`` /
``rd.solve_batch`` and ``rd.estimate`` / ``rd.estimate_batch`` run the three ``lrbms3_*_tv`` exports (the single calls as one
column: a single-trajectory export combines ``M + dt A`` once and has no row to change).  mu_bar / mu_hat sit at t = 0.  For
d/dt A != 0 the estimate is an indicator, not a proven bound.

Not built (``NotImplementedError``): the elliptic-reconstruction terms (the reference's branch is ``assert False``,
estimators.py:64) and sharded discretizations (``S_ext != S``); enrichment without the keyword, with diffusion coefficients of the
time (the step operator of the corrector solver is built once per call) or with non-zero initial data."""
import numpy as np

from pylrbms_amd.discretize_elliptic_block_swipdg_3d import BlockDiscretization3D, LRBMSReductor3D, ReducedDiscretization3D
from pylrbms_amd.discretize_parabolic_block_swipdg import ImplicitEulerTimeStepper
from pylrbms_amd.parameters import CubicParameterSpace
from pylrbms_amd.reductor import ExtensionError, LocalBasisSlab

_NEEDS_KEYWORD = ('online enrichment on the parabolic 3D path needs the corrector data: '
                  'discretize(grid_and_problem_data, T, nt, online_enrichment=True)')


def _parabolic_estimate(d, mu, dt, eta_loc, time_residual2, time_deriv_nc2, times=None):
    """ParabolicEstimator.estimate (estimators.py:141-168) from the local elliptic terms eta_loc [3, S, L] of the L vectors, the
    summed time residuals y^T M^-1 y [L - 1] and the nc terms of the differences [S, L - 1] (all squared quantities).  ``times``
    [L] (coefficients of the time): alpha and gamma of vector k are taken at t_k, mu_bar / mu_hat at t = 0."""
    nc, r, df = (np.asarray(x, dtype=np.float64) for x in eta_loc)
    if times is None:
        a_bar, a_hat, g_bar = d.alpha(mu, d.mu_bar), d.alpha(mu, d.mu_hat), d.gamma(mu, d.mu_bar)
    else:
        a_bar, a_hat, g_bar = (np.array([fn(mu, ref, t) for t in times], dtype=np.float64)
                               for fn, ref in ((d.alpha, d.mu_bar), (d.alpha, d.mu_hat), (d.gamma, d.mu_bar)))
    eta = (np.sqrt(g_bar) * np.linalg.norm(nc, axis=0) + (1.0 / np.sqrt(a_hat)) * np.linalg.norm(r + df, axis=0)) / np.sqrt(a_bar)
    time_residual = np.sqrt(np.asarray(time_residual2, dtype=np.float64) * (dt / 3))
    s = 2 * np.sqrt(dt / 3)
    eta, nc, r, df = eta * s, nc * s, r * s, df * s
    time_deriv_nc = np.sqrt(np.maximum(np.asarray(time_deriv_nc2, dtype=np.float64), 0.0) / dt)
    est = np.linalg.norm(eta) + np.linalg.norm(time_residual) + np.linalg.norm(time_deriv_nc)
    return est, (nc, r, df, time_residual, time_deriv_nc)


class InstationaryDiscretization3D(BlockDiscretization3D):
    """The 3D block discretization with ``T``, ``time_stepper`` (implicit Euler, ``nt`` steps), zero ``initial_data`` [S, n] and
    ``parameter_space``; built by ``discretize`` below."""

    _time_dependent_source = True

    @property
    def dt(self):
        return self.T / self.time_stepper.nt

    def source_coefficients(self, mu):
        """The host table phi [nt + 1, K] of the source f(t, mu) = sum_j c_j(mu, t) f_j: row k at t_k = k dt.  Step k -> k + 1 uses
        row k + 1; the elliptic part of U_k in the estimate uses row k.  Ones [nt + 1, 1] without an affine source."""
        nt = self.time_stepper.nt
        if self._src is None:
            return np.ones((nt + 1, 1))
        from pylrbms_amd.sources3d import evaluate_table
        return evaluate_table(self._src, mu, self.dt, nt)

    def diffusion_coefficients(self, mu):
        """The host table theta_t [nt + 1, Q] of the diffusion coefficients: row k at the time of row k of ``source_coefficients``
        (``sources3d.table_times``).  The step k -> k + 1 solves with row k + 1; in the estimate the elliptic rows of U_k use row k
        and the time residual of U_{k+1} - U_k row k + 1.  Every entry must be positive (ValueError naming q and k).  On a
        time-independent discretization every row is ``theta(mu)``."""
        from pylrbms_amd.sources3d import table_times
        nt = self.time_stepper.nt
        if not self._tv:
            return np.tile(self.theta(mu), (nt + 1, 1))
        tab = np.stack([self._theta_at(mu, t) for t in table_times(self.dt, nt).tolist()])
        bad = np.argwhere(~(tab > 0.0))
        if len(bad):
            k, q = (int(v) for v in bad[0])
            raise ValueError('diffusion coefficient q = {} is {!r} at step k = {} (t = {!r}), mu = {!r}: every theta_q(t, mu) must '
                             'be positive'.format(q, float(tab[k, q]), k, k * self.dt, mu))
        return tab

    def _estimator_coefficients(self, mu):
        """coef [nt + 1, 2] of ``lrbms3_reduced_parabolic_estimate_batch_tv``: (sqrt(gamma_bar / alpha_bar), 1 / sqrt(alpha_hat
        alpha_bar)) with mu at t_k and mu_bar / mu_hat at t = 0."""
        from pylrbms_amd.sources3d import table_times
        out = np.empty((self.time_stepper.nt + 1, 2))
        for k, t in enumerate(table_times(self.dt, self.time_stepper.nt).tolist()):
            a_bar, a_hat, g_bar = self.alpha(mu, self.mu_bar, t), self.alpha(mu, self.mu_hat, t), self.gamma(mu, self.mu_bar, t)
            out[k] = np.sqrt(g_bar / a_bar), 1.0 / np.sqrt(a_hat * a_bar)
        return out

    def solve(self, mu, rtol=1e-10, max_iter=50000, return_info=False):
        """The trajectory as a device slab U [S, n, nt + 1] (U[:, :, 0] = the initial data): all nt implicit Euler steps in one
        native call, each a warm-started two-level CG on M + dt A(mu).  ``last_solve_info`` = (total CG iterations, worst relative
        residual).  With diffusion coefficients of the time: one column of ``lrbms3_fom_implicit_euler_batch_tv``."""
        eng = self.engine
        if self._tv:
            b_K = self._src['b_K'] if self._src is not None else eng.ops['b'].reshape(1, eng.S, eng.t.n)
            phi = np.asarray(self.source_coefficients(mu), dtype=np.float64)[None]
            U, inf = eng.ctx.fom_implicit_euler_batch_tv(self.diffusion_coefficients(mu)[None], self.dt, self.time_stepper.nt,
                                                         eng.ops['A_diag'], eng.ops['A_cpl'], b_K, phi, U0=self.initial_data, rtol=rtol,
                                                         max_iter=max_iter)
            U, info = U[:, :, :, 0], (inf['iterations'], inf['relative_residual'])
        elif self._src is None:
            U, info = eng.ctx.fom_implicit_euler(self.Q, self.theta(mu), self.dt, self.time_stepper.nt, eng.ops['A_diag'],
                                                 eng.ops['A_cpl'], eng.ops['b'], U0=self.initial_data, rtol=rtol, max_iter=max_iter)
        else:
            U, info = eng.ctx.fom_implicit_euler_src(self.Q, self.theta(mu), self.dt, self.time_stepper.nt, eng.ops['A_diag'],
                                                     eng.ops['A_cpl'], self._src['b_K'], self.source_coefficients(mu),
                                                     U0=self.initial_data, rtol=rtol, max_iter=max_iter)
        self.last_solve_info = info
        U = U.permute(1, 2, 0).contiguous()
        return (U, info) if return_info else U

    def solve_for_local_correction_trajectories(self, subdomains, mu, rtol=1e-12, max_iter=20000, return_info=False):
        """The parabolic counterpart of ``solve_for_local_corrections``: on the neighbourhood of every subdomain of ``subdomains``
        (all-Dirichlet outer boundary) the implicit Euler trajectory with zero initial value, the source of ``solve(mu)`` and the
        ``nt`` steps of the time stepper, restricted to the subdomain -- all of them in ONE native call
        (``lrbms3_local_correction_euler``).  Returns the device tensor ``[len(subdomains), n, nt]`` (column k - 1 =
        step k); ``info`` / ``last_local_correction_info`` [len(subdomains), 2] = the PCG iterations summed over the steps and the
        worst final residual ratio of a step.  ``NotImplementedError`` (before any device work) without
        ``discretize(..., online_enrichment=True)``, for diffusion coefficients of the time and for non-zero initial data."""
        if not self.online_enrichment:
            raise NotImplementedError(_NEEDS_KEYWORD)
        if self._tv:
            raise NotImplementedError('solve_for_local_correction_trajectories: the diffusion coefficients depend on time (a coefficient '
                                      'c(mu, t)); the corrector solver builds its step operator M + dt A(theta) once per call and '
                                      'would have to rebuild it in every step')
        if self.initial_data is not None and bool((self.initial_data != 0).any()):
            raise NotImplementedError('solve_for_local_correction_trajectories: non-zero initial data; the corrector trajectories '
                                      'start at x_0 = 0')
        eng, nt = self.engine, self.time_stepper.nt
        marked = [eng.local.index(int(ii)) for ii in subdomains]
        b_K = self._src['b_K'] if self._src is not None else eng.ops['b'].reshape(1, eng.S, eng.t.n)
        corr, info = eng.local_corrections_euler(self.theta(mu), self.dt, nt, marked, b_K=b_K, phi=self.source_coefficients(mu),
                                                 rtol=rtol, max_iter=max_iter)
        self.last_local_correction_info = info
        return (corr, info) if return_info else corr

    def _no_stationary(self):
        if self._tv:
            raise NotImplementedError('the diffusion coefficients depend on time (a coefficient c(mu, t)): there is no stationary '
                                      'operator, this needs the parabolic solve')

    def solve_stationary(self, mu, rtol=1e-10, max_iter=50000, return_info=False):
        """The elliptic solve of the underlying discretization (the limit t -> oo).  NotImplementedError if a source coefficient
        depends on time (before the engine is read)."""
        self._no_stationary()
        if self._src is not None:
            from pylrbms_amd.sources3d import evaluate_stationary
            evaluate_stationary(self._src, mu)
        return BlockDiscretization3D.solve(self, mu, rtol=rtol, max_iter=max_iter, return_info=return_info)

    def solve_batch(self, mus, rtol=1e-10, max_iter=50000, return_info=False, as_snapshots=False):
        """Trajectories for a whole training set, 64 parameters per native ``lrbms3_fom_implicit_euler_batch`` call: panels of 16
        columns share every read of the operator blocks, one two-level preconditioner per call on ``M + dt A`` at the mean theta of
        its columns.  Returns a list with, per parameter, the tensor ``[S, n, nt + 1]`` that ``solve(mu)`` returns --
        here a VIEW of the call's panel ``[nt + 1, S, n, nmu]`` (not contiguous; ``estimate`` makes its input contiguous, other
        consumers call ``.contiguous()``).  ``as_snapshots=True``: one contiguous tensor ``[S, n, len(mus) * nt]`` instead, the steps
        1 .. nt of every parameter, parameter-major: the slab ``extend_basis(..., method='pod')`` takes (at most 128 vectors).
        ``as_snapshots='slabs'``: the list of the step slabs ``U[k]``, k = 1 .. nt, of every native call -- contiguous views
        ``[S, n, nmu_call]`` of the panels, no copy and no limit: what ``extend_basis(..., method='hapod')`` takes (sharded: the views
        ``[S, n, nt]`` of the trajectories).
        ``last_solve_info`` / ``return_info``: (CG iterations summed over the calls, worst final residual ratio).  On a sharded grid
        it is the loop of ``solve``."""
        import torch
        eng = self.engine
        mus = list(mus)
        if not mus:
            raise ValueError('solve_batch: no parameters')
        nt = self.time_stepper.nt
        slabs = isinstance(as_snapshots, str) and as_snapshots == 'slabs'
        if as_snapshots and not slabs and len(mus) * nt > 128:
            raise ValueError('solve_batch(as_snapshots=True): {} x {} vectors, the local POD takes at most 128'.format(len(mus), nt))
        trajs, panels, its, rel = [], [], 0, 0.0
        if eng.S_ext != eng.S:
            for mu in mus:
                U, info = self.solve(mu, rtol=rtol, max_iter=max_iter, return_info=True)
                trajs.append(U)
                its, rel = its + info[0], max(rel, info[1])
        else:
            if self._tv:                                   # a theta row per step: [len(mus), nt + 1, Q]
                theta, native = np.stack([self.diffusion_coefficients(mu) for mu in mus]), eng.ctx.fom_implicit_euler_batch_tv
            else:
                theta, native = np.stack([self.theta(mu) for mu in mus]), eng.ctx.fom_implicit_euler_batch
            phi = np.stack([np.asarray(self.source_coefficients(mu), dtype=np.float64) for mu in mus])     # [len(mus), nt + 1, K]
            b_K = self._src['b_K'] if self._src is not None else eng.ops['b'].reshape(1, eng.S, eng.t.n)
            for m0 in range(0, len(mus), 64):
                U, info = native(theta[m0:m0 + 64], self.dt, nt, eng.ops['A_diag'], eng.ops['A_cpl'], b_K,
                                 phi[m0:m0 + 64], U0=self.initial_data, rtol=rtol, max_iter=max_iter)
                its, rel = its + info['iterations'], max(rel, info['relative_residual'])
                trajs += [U[:, :, :, m].permute(1, 2, 0) for m in range(U.shape[3])]
                panels.append(U)
        self.last_solve_info = (its, rel)
        if slabs:
            out = [U[k] for U in panels for k in range(1, nt + 1)] if eng.S_ext == eng.S else [u[:, :, 1:] for u in trajs]
        else:
            out = torch.cat([u[:, :, 1:] for u in trajs], dim=2).contiguous() if as_snapshots else trajs
        return (out, self.last_solve_info) if return_info else out

    def solve_stationary_batch(self, mus, rtol=1e-10, max_iter=50000, return_info=False):
        """The elliptic ``solve_batch`` of the underlying discretization: one tensor [S, n, len(mus)] of stationary solutions.
        NotImplementedError if a source coefficient depends on time, as ``solve_stationary``."""
        self._no_stationary()
        mus = list(mus)
        if self._src is not None:
            from pylrbms_amd.sources3d import evaluate_stationary
            for mu in mus:
                evaluate_stationary(self._src, mu)
        eng = self.engine
        if eng.S_ext != eng.S:                       # (the elliptic loop would call this class's ``solve``)
            import torch
            if not mus:
                raise ValueError('solve_stationary_batch: no parameters')
            cols, its, rel = [], 0, 0.0
            for mu in mus:
                U, info = self.solve_stationary(mu, rtol=rtol, max_iter=max_iter, return_info=True)
                cols.append(U[:, :, None])
                its, rel = max(its, info[0]), max(rel, info[1])
            U = torch.cat(cols, dim=2).contiguous()
            return (U, (its, rel)) if return_info else U
        return BlockDiscretization3D.solve_batch(self, mus, rtol=rtol, max_iter=max_iter, return_info=return_info)

    def _elliptic_terms(self, U, mu, rows=None, thetas=None):
        """Local nc / r / df [3, S, L] of every column of U [S, n, L]: chunks of <= 64 // Q columns become a basis of the pass
        (it takes Q N <= 64) and the batched estimate with identity coefficients evaluates each column's forms.  With an affine
        source the estimate runs without its f terms and ``rows`` [L, K] (the source coefficients of every column; None: no f terms,
        the caller reads the nc row only) adds them through ``lrbms3_project_sources`` / ``lrbms3_reduced_source_terms``.
        ``thetas`` [L, Q]: a diffusion coefficient row per column (None: ``theta(mu)`` for every column)."""
        import torch
        from pylrbms_amd import sources3d
        eng, src = self.engine, self._src
        theta = self.theta(mu) if thetas is None else None
        step = max(1, 64 // self.Q)
        out = []
        for c0 in range(0, U.shape[2], step):
            V = U[:, :, c0:c0 + step].contiguous()
            L = V.shape[2]
            u = torch.eye(L, dtype=V.dtype, device=V.device).expand(eng.S_ext, L, L).contiguous()
            th = np.tile(theta, (L, 1)) if thetas is None else np.ascontiguousarray(thetas[c0:c0 + L], dtype=np.float64)
            if src is None:
                buf = eng.project_and_estimate(V)
                out.append(eng.ctx.reduced_estimate_batch(self.Q, th, u, buf, eng.ops, eng.hdiam))
                continue
            work = eng.alloc_work(L)
            buf = eng.project_and_estimate(V, work=work)
            buf0, ops0 = sources3d.zeroed(eng, buf)
            eta = eng.ctx.reduced_estimate_batch(self.Q, th, u, buf0, ops0, eng.hdiam)
            if rows is not None:
                _, r_fd_K = eng.ctx.project_sources(self.Q, src['b_K'], src['bdiv_K'], V, work)
                eta[1] += sources3d.source_terms(eng, self.Q, src, th, np.ascontiguousarray(rows[c0:c0 + L]), r_fd_K, buf, u)
            out.append(eta)
        return torch.cat(out, dim=2).cpu().numpy()

    def estimate(self, U, mu, decompose=False):
        """est, (local_eta_nc [S, nt+1], local_eta_r, local_eta_df, time_residual [nt], time_deriv_nc [S, nt]) of a trajectory
        U [S, n, nt + 1] (``decompose`` is accepted for the API shape: the parts are always returned).  With diffusion
        coefficients of the time this is the verification path of the ``_tv`` estimate: the same kernels per step, the elliptic
        rows of U_k at row k of ``diffusion_coefficients``, A(row k + 1) (U_{k+1} - U_k) in the time residual, alpha and gamma per
        row."""
        eng = self.engine
        U = (U if isinstance(U, eng.ctx.torch.Tensor) else eng.ctx.from_numpy(np.asarray(U))).contiguous()
        dU = (U[:, :, 1:] - U[:, :, :-1]).contiguous()
        if self._tv:
            import torch
            from pylrbms_amd.sources3d import table_times
            nt = self.time_stepper.nt
            if U.shape[2] != nt + 1:
                raise ValueError('with diffusion coefficients of the time the estimate takes the whole trajectory [S, n, nt + 1]')
            th = self.diffusion_coefficients(mu)
            eta_loc = self._elliptic_terms(U, mu, rows=self.source_coefficients(mu) if self._src is not None else None, thetas=th)
            Y = torch.cat([eng.ctx.fom_apply(self.Q, th[k + 1], eng.ops['A_diag'], eng.ops['A_cpl'], dU[:, :, k:k + 1].contiguous())
                           for k in range(nt)], dim=2).contiguous()
            tr2 = eng.ctx.mass_inverse_norm2(Y).sum(dim=0).cpu().numpy()
            tdnc2 = self._elliptic_terms(dU, mu, thetas=th[1:])[0]          # (the nc form reads no theta)
            return _parabolic_estimate(self, mu, self.dt, eta_loc, tr2, tdnc2, times=table_times(self.dt, nt).tolist())
        if self._src is not None and U.shape[2] != self.time_stepper.nt + 1:
            raise ValueError('with a time-dependent source the estimate takes the whole trajectory [S, n, nt + 1]')
        eta_loc = self._elliptic_terms(U, mu, rows=self.source_coefficients(mu) if self._src is not None else None)
        Y = eng.ctx.fom_apply(self.Q, self.theta(mu), eng.ops['A_diag'], eng.ops['A_cpl'], dU)
        tr2 = eng.ctx.mass_inverse_norm2(Y).sum(dim=0).cpu().numpy()
        tdnc2 = self._elliptic_terms(dU, mu)[0]
        return _parabolic_estimate(self, mu, self.dt, eta_loc, tr2, tdnc2)


class InstationaryReducedDiscretization3D(ReducedDiscretization3D):
    """``rd`` of the parabolic path: the reduced elliptic model plus the projected mass ``M_red`` [S, N, N]."""

    def __init__(self, reductor, out, M_red, rhs_red_K=None, r_fd_K=None):
        super().__init__(reductor, out, rhs_red_K, r_fd_K)
        self.M_red = M_red
        self.T, self.time_stepper = reductor.d.T, reductor.d.time_stepper

    @property
    def dt(self):
        return self.T / self.time_stepper.nt

    def _tv_limits(self, what, estimate=False):
        """The ``_tv`` exports are batched kernels: a reduced model outside their limits is refused, never handed to a single export
        that would silently use one coefficient row."""
        if self.N > 32:
            raise NotImplementedError('{} with diffusion coefficients of the time runs the batched kernels: N = {} > 32 is outside '
                                      'their limit'.format(what, self.N))
        if estimate and self.d.Q * self.N > 64:
            raise NotImplementedError('{} with diffusion coefficients of the time runs the batched estimate: Q N = {} > 64 is outside '
                                      'its limit'.format(what, self.d.Q * self.N))

    def _solve_batch_tv(self, chunk, rtol, max_iter):
        d = self.d
        theta_t = np.stack([d.diffusion_coefficients(mu) for mu in chunk])          # [nmu, nt + 1, Q]
        if self.rhs_red_K is None:
            return d.engine.ctx.reduced_implicit_euler_batch_tv(d.Q, theta_t, self.dt, self.time_stepper.nt, self.out['B_sys'], self.M_red,
                                                                self.out['rhs_red'], rtol=rtol, max_iter=max_iter)
        phi = np.stack([np.asarray(d.source_coefficients(mu), dtype=np.float64) for mu in chunk])
        return d.engine.ctx.reduced_implicit_euler_batch_tv(d.Q, theta_t, self.dt, self.time_stepper.nt, self.out['B_sys'], self.M_red,
                                                            self.rhs_red_K, phi=phi, rtol=rtol, max_iter=max_iter)

    def solve(self, mu, rtol=1e-12, max_iter=20000, return_info=False):
        """Reduced implicit Euler from zero: u [nt + 1, S, N] (one native call; with diffusion coefficients of the time one column of
        ``lrbms3_reduced_implicit_euler_batch_tv``)."""
        d = self.d
        if d._tv:
            self._tv_limits('rd.solve')
            U, info = self._solve_batch_tv([mu], rtol, max_iter)
            u = U[:, :, :, 0].contiguous()
        elif self.rhs_red_K is None:
            u, info = d.engine.ctx.reduced_implicit_euler(d.Q, d.theta(mu), self.dt, self.time_stepper.nt, self.out['B_sys'], self.M_red,
                                                          self.out['rhs_red'], rtol=rtol, max_iter=max_iter)
        else:
            u, info = d.engine.ctx.reduced_implicit_euler_src(d.Q, d.theta(mu), self.dt, self.time_stepper.nt, self.out['B_sys'],
                                                              self.M_red, self.rhs_red_K, d.source_coefficients(mu), rtol=rtol,
                                                              max_iter=max_iter)
        self.last_solve_info = info
        return (u, info) if return_info else u

    def solve_batch(self, mus, rtol=1e-12, max_iter=20000, return_info=False):
        """Parameter sweep over the parabolic reduced model: one ``lrbms3_reduced_implicit_euler_batch(_src)`` call per 64
        parameters -> [len(mus), nt + 1, S, N]; entry m is what ``solve(mus[m])`` returns (the estimator stays per trajectory).
        info: (largest per-call iteration count, worst relative residual).  N > 32: one ``solve`` per parameter."""
        import torch
        d, nt, out = self.d, self.time_stepper.nt, []
        info = (0, 0.0)
        if d._tv:
            self._tv_limits('rd.solve_batch')
            for b0 in range(0, len(mus), 64):
                U, inf = self._solve_batch_tv(mus[b0:b0 + 64], rtol, max_iter)
                out.append(U.permute(3, 0, 1, 2))
                info = (max(info[0], inf[0]), max(info[1], inf[1]))
        elif self.N > 32:                     # the batched kernels take N <= 32
            for mu in mus:
                u, inf = self.solve(mu, rtol=rtol, max_iter=max_iter, return_info=True)
                out.append(u[None])
                info = (max(info[0], inf[0]), max(info[1], inf[1]))
        else:
            ctx = d.engine.ctx
            for b0 in range(0, len(mus), 64):          # 64 per native call: four groups of 16 on four streams
                chunk = mus[b0:b0 + 64]
                th = np.stack([d.theta(mu) for mu in chunk])
                if self.rhs_red_K is None:
                    U, inf = ctx.reduced_implicit_euler_batch(d.Q, th, self.dt, nt, self.out['B_sys'], self.M_red, self.out['rhs_red'],
                                                              rtol=rtol, max_iter=max_iter)
                else:
                    phi = np.stack([np.asarray(d.source_coefficients(mu), dtype=np.float64) for mu in chunk])     # [nmu, nt + 1, K]
                    U, inf = ctx.reduced_implicit_euler_batch_src(d.Q, th, self.dt, nt, self.out['B_sys'], self.M_red, self.rhs_red_K,
                                                                  phi, rtol=rtol, max_iter=max_iter)
                out.append(U.permute(3, 0, 1, 2))
                info = (max(info[0], inf[0]), max(info[1], inf[1]))
        U = torch.cat(out, dim=0).contiguous()
        self.last_solve_info = info
        return (U, info) if return_info else U

    def local_indicators(self, parts, mu):
        """Per-subdomain indicators [S] of a parabolic estimate, from its ``parts`` (2D: ``InstationaryReducedDiscretization
        .local_indicators``): per step ``2 / alpha_bar (gamma_bar nc^2 + (r + df)^2 / alpha_hat)`` on that step's columns, summed
        over the steps, plus ``sum_k time_deriv_nc[s, k]^2``.  The time-stepping residual is a global ``M^-1`` norm and has no local
        share: a marking heuristic, not a bound."""
        d = self.d
        nc, r, df, _, time_deriv_nc = parts
        a_bar, a_hat, g_bar = d.alpha(mu, d.mu_bar), d.alpha(mu, d.mu_hat), d.gamma(mu, d.mu_bar)
        elliptic = (2. / a_bar) * (g_bar * nc ** 2 + (1. / a_hat) * (r + df) ** 2)        # [S, nt + 1]
        return elliptic.sum(axis=1) + (time_deriv_nc ** 2).sum(axis=1)

    def estimate(self, u, mu, decompose=False):
        """The five parts of ``InstationaryDiscretization3D.estimate`` for reduced coefficients u [nt + 1, S, N]: the elliptic terms
        from the batched reduced estimate (one parameter column per time step), the nc row of the same call on the differences, the
        time residual with M_red^-1.  With diffusion coefficients of the time: one column of the ``_tv`` export.
        ``decompose=True``: a third entry ``indicators [S]`` (``local_indicators``), what ``AdaptiveEnrichment`` marks with."""
        if decompose:
            if self.d._tv:
                raise NotImplementedError('estimate(decompose=True): the diffusion coefficients depend on time (a coefficient c(mu, t)); '
                                          'alpha / gamma of the local indicators would change from step to step')
            est, parts = self.estimate(u, mu)
            return est, parts, self.local_indicators(parts, mu)
        d = self.d
        if d._tv:
            return self.estimate_batch(u[None], [mu], decompose=decompose, native=True)[0]
        eng, Q, theta = d.engine, d.Q, d.theta(mu)
        u = u.contiguous()
        du = (u[1:] - u[:-1]).contiguous()
        L = u.shape[0]
        out, ops = (self.out, eng.ops) if self.rhs_red_K is None else self._zeroed()
        th, uc = np.tile(theta, (L, 1)), u.permute(1, 2, 0).contiguous()
        eta_loc = eng.ctx.reduced_estimate_batch(Q, th, uc, out, ops, eng.hdiam)
        if self.rhs_red_K is not None:        # the f terms of all nt + 1 columns in one launch, column k with row k of the table
            from pylrbms_amd.sources3d import source_terms
            if L != self.time_stepper.nt + 1:
                raise ValueError('with a time-dependent source the estimate takes the whole trajectory [nt + 1, S, N]')
            eta_loc[1] += source_terms(eng, Q, d._src, th, d.source_coefficients(mu), self.r_fd_K, self.out, uc)
        eta_loc = eta_loc.cpu().numpy()
        tdnc2 = eng.ctx.reduced_estimate_batch(Q, np.tile(theta, (L - 1, 1)), du.permute(1, 2, 0).contiguous(), out, ops,
                                               eng.hdiam)[0].cpu().numpy()
        tr2 = eng.ctx.reduced_time_residual(Q, theta, self.out['B_sys'], self.M_red, du).sum(dim=1).cpu().numpy()
        return _parabolic_estimate(d, mu, self.dt, eta_loc, tr2, tdnc2)

    def estimate_batch(self, U, mus, decompose=False, native=False):
        """The estimates of the trajectories U [len(mus), nt + 1, S, N] (as ``solve_batch`` returns them): a list with, per
        parameter, the tuple ``estimate(U[m], mus[m])`` returns.

        ``native=False`` (the default) IS the loop of ``estimate``, bit for bit; nothing is routed to the batched export.
        ``native=True``: one ``lrbms3_reduced_parabolic_estimate_batch`` call per 64 parameters -- the chunk is
        permuted into the panel [nt + 1, S, N, nmu] once, the source coefficients come from ``d.source_coefficients``, one
        device-to-host copy per output, NumPy parts as ``estimate`` returns them.  It agrees with the loop to round-off, not in
        the bits: the time residual runs on the matrix-core panel matvec and the norms are summed on the device.  With N > 32
        or Q N > 64 (the limits of the batched kernels) ``native=True`` runs the loop, as ``solve_batch`` does for N > 32.

        With diffusion coefficients of the time both values of ``native`` run ``lrbms3_reduced_parabolic_estimate_batch_tv`` on whole
        trajectories; outside the limits of the batched kernels that is a NotImplementedError."""
        assert len(U) == len(mus), 'estimate_batch: one trajectory per parameter'
        d = self.d
        mus = list(mus)
        tv = d._tv
        if tv:
            self._tv_limits('rd.estimate', estimate=True)
            if not mus:
                return []
            if U.shape[1] != self.time_stepper.nt + 1:
                raise ValueError('with diffusion coefficients of the time the estimate takes the whole trajectory [nt + 1, S, N]')
        elif not native or self.N > 32 or d.Q * self.N > 64 or not mus:
            return [self.estimate(U[m], mu, decompose=decompose) for m, mu in enumerate(mus)]
        eng, nt = d.engine, self.time_stepper.nt
        src = self.rhs_red_K is not None
        if U.shape[1] != nt + 1:
            if src:
                raise ValueError('with a time-dependent source the estimate takes the whole trajectory [nt + 1, S, N]')
            nt = int(U.shape[1]) - 1           # (a part of a trajectory: the estimate of its steps, as ``estimate`` does)
            if nt < 1:
                raise ValueError('estimate_batch: a trajectory has at least two vectors')
        out, ops = self._zeroed() if src else (self.out, eng.ops)
        res = []
        for b0 in range(0, len(mus), 64):
            chunk = mus[b0:b0 + 64]
            if tv:                                 # a row per step: theta_t [nmu, nt + 1, Q], coef [nmu, nt + 1, 2]
                th = np.stack([d.diffusion_coefficients(mu) for mu in chunk])
                coef = np.stack([d._estimator_coefficients(mu) for mu in chunk])
                native_call = eng.ctx.reduced_parabolic_estimate_batch_tv
            else:
                th = np.stack([d.theta(mu) for mu in chunk])
                coef = np.empty((len(chunk), 2))
                for m, mu in enumerate(chunk):
                    a_bar, a_hat, g_bar = d.alpha(mu, d.mu_bar), d.alpha(mu, d.mu_hat), d.gamma(mu, d.mu_bar)
                    coef[m] = np.sqrt(g_bar / a_bar), 1.0 / np.sqrt(a_hat * a_bar)
                native_call = eng.ctx.reduced_parabolic_estimate_batch
            panel = U[b0:b0 + 64].permute(1, 2, 3, 0).contiguous()
            kw = {}
            if src:
                kw = dict(phi=np.stack([np.asarray(d.source_coefficients(mu), dtype=np.float64) for mu in chunk]), F2=d._src['F2'],
                          r_fd_K=self.r_fd_K, bdiv_K=d._src['bdiv_K'])
            r = native_call(d.Q, th, coef, self.dt, nt, panel, self.out['B_sys'], self.M_red, out, ops, eng.hdiam, **kw)
            h = {k: v.cpu().numpy() for k, v in r.items()}
            for m in range(len(chunk)):
                nc, rr, df = (np.ascontiguousarray(h['eta_loc'][i, :, :, m].T) for i in range(3))      # [S, nt + 1]
                res.append((float(h['est'][m]), (nc, rr, df, np.ascontiguousarray(h['time_residual'][:, m]),
                                                 np.ascontiguousarray(h['time_deriv_nc'][:, :, m].T))))
        return res


class ParabolicLRBMSReductor3D(LRBMSReductor3D):
    """``ParabolicLRBMSReductor`` (2D: pylrbms_amd.reductor) for the 3D path.  ``extend_basis`` takes a trajectory [S, n, L]: its
    vectors are Gram-Schmidt-ed into the local bases one after the other, a vector that is numerically in the span of a local basis
    is skipped for that subdomain, ``ExtensionError`` if nothing was added anywhere; ``reduce()`` returns the instationary reduced
    model; ``reconstruct(u)`` maps u [nt + 1, S, N] to [S, n, nt + 1].

    Online enrichment is opt-in.  On a discretization made with ``online_enrichment=True`` the constructor returns
    an ``EnrichingParabolicLRBMSReductor3D``, whose ``reduce(touched=None)`` has the incremental form ``AdaptiveEnrichment`` probes
    the signature for; this class keeps ``reduce()``, the whole re-reduction, and its ``enrich_local(_batch)`` name the keyword."""

    extend_basis = LocalBasisSlab._extend_basis_trajectory

    def __new__(cls, d=None, *args, **kwargs):
        if cls is ParabolicLRBMSReductor3D and getattr(d, 'online_enrichment', False):
            cls = EnrichingParabolicLRBMSReductor3D                  # (a subclass: __init__ runs on it with the same arguments)
        return super().__new__(cls)

    def enrich_local(self, subdomain, U, mu=None, pod_modes=1, rtol=1e-6):
        """``enrich_local_batch`` for the one subdomain; ``ExtensionError`` if its basis did not grow."""
        d = getattr(self, 'd', None)
        if d is None or not d.online_enrichment:
            raise NotImplementedError(_NEEDS_KEYWORD)
        if not self.enrich_local_batch([subdomain], U, mu, pod_modes=pod_modes, rtol=rtol):
            raise ExtensionError('the local corrector trajectory is (numerically) in the span of the local basis')

    def enrich_local_batch(self, subdomains, U, mu=None, pod_modes=1, rtol=1e-6):
        """Online enrichment of the parabolic reduced model (the semantics of the 2D reductor, 5.3.1): the corrector
        trajectories of the marked subdomains (``d.solve_for_local_correction_trajectories``, one native call) are scattered into a
        zero slab [S, n, nt] and compressed by ``lrbms3_local_pod`` against the current bases in the local energy product: at most
        ``pod_modes`` new vectors per marked subdomain, those with a singular value above ``rtol`` times the largest snapshot norm;
        an unmarked subdomain keeps its bits.  The slab grows only when its free columns do not suffice, and then to an even width
        as ``reserve`` pads (the wide-load form of the pass takes even N; at most 64 // Q); a call that gains nothing leaves the
        width as it was, so the next ``reduce(touched=)`` stays incremental.  ``U`` is accepted and unused.  Returns the subdomains
        whose basis grew (they are marked dirty for ``reduce(touched=)``); adding nothing is not an error here."""
        d = getattr(self, 'd', None)
        if d is None or not d.online_enrichment:
            raise NotImplementedError(_NEEDS_KEYWORD)
        subdomains = [int(ii) for ii in subdomains]
        if not subdomains:
            return []
        if int(pod_modes) < 1:
            raise ValueError('enrich_local_batch: pod_modes must be >= 1')
        if not rtol >= self.POD_MIN_RTOL:
            raise ValueError('enrich_local_batch: rtol < 1e-7: the Gram matrix squares the singular values, below that they are noise')
        self._pod_product()                                          # (a reductor without such a product refuses here)
        eng = d.engine
        corr = d.solve_for_local_correction_trajectories(subdomains, mu)           # [nmark, n, nt]
        rows_host = np.array([eng.local.index(ii) for ii in subdomains], dtype=np.int64)
        width0 = self.basis_size()
        gained = self._extend_marked_pod(rows_host, corr, pod_modes, rtol)
        if self.basis_size() != width0:
            self.reserve(self.basis_size())                          # the slab grew: to an even width
        return [ii for ii, i in zip(subdomains, rows_host) if gained[i] > 0]

    def reduce(self):
        rd = LRBMSReductor3D.reduce(self)
        return self._with_mass(rd)

    def _with_mass(self, rd):
        """The instationary model of the elliptic one: the mass is projected for the whole slab (one workgroup per subdomain)."""
        M_red = self.d.engine.ctx.project_mass(self._V.contiguous())
        return InstationaryReducedDiscretization3D(self, rd.out, M_red, rd.rhs_red_K, rd.r_fd_K)

    def reconstruct(self, u):
        return self._torch.einsum('snj,ksj->snk', self._V, u).contiguous()


class EnrichingParabolicLRBMSReductor3D(ParabolicLRBMSReductor3D):
    """The parabolic 3D reductor of a discretization made with ``online_enrichment=True`` (what ``ParabolicLRBMSReductor3D(d)`` returns
    there): ``reduce`` takes ``touched``."""

    def reduce(self, touched=None):
        """``touched``: as ``LRBMSReductor3D.reduce`` -- only the changed subdomains and their neighbours are projected again, into
        the arrays of the previous model; the mass is projected for the whole slab either way."""
        return self._with_mass(LRBMSReductor3D.reduce(self, touched=touched))


def discretize(grid_and_problem_data, T, nt, device_index=0, elliptic_reconstruction=False, online_enrichment=False):
    """``(d, data)`` of the parabolic 3D path: the elliptic 3D ``discretize`` plus ``T``, implicit Euler with ``nt`` steps, zero
    initial data and the parameter space.  ``online_enrichment=True`` also assembles the corrector data (``D_corr``, as the
    elliptic 3D ``discretize``) that ``solve_for_local_correction_trajectories`` and ``enrich_local(_batch)`` need."""
    if elliptic_reconstruction:
        raise NotImplementedError('elliptic_reconstruction: the reference never evaluates it (estimators.py:64 is assert False); '
                                  'the 3D parabolic path does not build it')
    grid = grid_and_problem_data['grid']
    if getattr(grid, 'world_size', 1) > 1:
        raise NotImplementedError('the 3D parabolic path needs all subdomains on one rank (sharded discretization: S_ext != S)')
    d = InstationaryDiscretization3D(grid_and_problem_data, device_index=device_index, online_enrichment=online_enrichment)
    eng = d.engine
    if eng.S_ext != eng.S:
        raise NotImplementedError('the 3D parabolic path needs all subdomains on one rank (sharded discretization: S_ext != S)')
    if not (float(T) > 0.0) or int(nt) < 1:
        raise ValueError('T > 0 and nt >= 1 required')
    d.T = float(T)
    d.time_stepper = ImplicitEulerTimeStepper(nt=nt, solver_options='operator')
    d.initial_data = eng.ctx.zeros(eng.S, eng.t.n)
    pr = d.parameter_range if d.parameter_range is not None else (0.1, 1.0)
    d.parameter_space = CubicParameterSpace({'mu': ()}, pr[0], pr[1])
    d.name = 'parabolic_block_swipdg_3d'
    data = {'grid': d.grid, 'engine': eng, 'operators': eng.ops}
    return d, data
