"""``discretize`` of the parabolic block-SWIPDG LRBMS discretization
(reference python/dune/pylrbms/discretize_parabolic_block_swipdg.py:17-95; SURVEY.md section 8f "next" #3).

``M u' + A(mu) u = f`` with the block L2 product as mass (:49-59), zero initial data (:82) and pyMOR's implicit Euler
with ``nt`` steps (:87).  The reference's version does not run at HEAD; repaired call sites:

* ``discretize_ell(grid_and_problem_data)`` (:44) -> the three-argument elliptic ``discretize``;
* ``ParabolicEstimator(...)`` with 8 arguments (:76-77) -> the 12-argument constructor of estimators.py:28-30 (grid and
  ``mpi_comm`` taken from the elliptic estimator);
* the estimator's ``elliptic_reconstruction=True`` hits ``assert False`` (estimators.py:64) -> flag, default off.

``solve(mu)`` is ONE native call for the whole trajectory (``lrbms_fom_implicit_euler``): the theta-weighted block
operator plus the mass is combined once, every step is a warm-started CG on it.  On a sharded discretization the solves
run on the gathered operator, and so does the time residual of the parabolic estimate (its elliptic-reconstruction
variant needs all subdomains on one rank).  ``solve_batch(mus)`` runs the trajectories of a training set 64 parameters per
native call (``lrbms_fom_implicit_euler_batch``); the elliptic batch stays reachable as
``solve_stationary_batch``.

Time-dependent affine sources (the reference's artificial-channels problem, python/scripts/parabolic.py):
``p['f'] = {'functions': [f_0 .. f_{K-1}], 'coefficients': [phi_0 .. phi_{K-1}]}`` with coefficients that may read ``mu`` and
``'_t'``.  The host evaluates ``phi [nt + 1][K]`` once per ``mu`` (``d.source_coefficients(mu)``: row 0 at t = 0, row k at the time
of step k accumulated as pyMOR's implicit Euler does, ``t += dt``); the load vectors ``b_K [K][S][n]`` and the Grams
``F2 [S][K][K]`` are assembled once.  ``solve`` -> ``lrbms_fom_implicit_euler_src``; the estimate evaluates the elliptic part of
``U_k`` with ``f(t_k, mu)`` (row k): ``lrbms_reduced_estimate_batch`` with f2 = 0, r_fd = 0 plus ``lrbms_project_sources`` /
``lrbms_reduced_source_terms``.  A single component with coefficient 1 takes the path above unchanged.
Single rank only; the elliptic reconstruction is not available with such a source.

Time-dependent diffusion coefficients: a ``lambda`` coefficient whose ``parameter_type`` names ``'_t'`` makes
the discretization time-dependent (``'_t'`` does not join ``d.parameter_type``).  ``d.diffusion_coefficients(mu)`` is the table
``theta_t [nt + 1][Q]`` at the times of ``source_coefficients``; the step k -> k + 1 solves with row k + 1, as pyMOR's implicit Euler
assembles ``M + dt A(mu)`` at ``mu['_t'] = t_{k+1}``.  ``solve`` / ``solve_batch`` run ``lrbms_fom_implicit_euler_batch_tv`` (the batched
kernels take theta per column as launch arguments: a row per step rebuilds no operator); the estimate freezes the coefficient per
step.  Single rank, no elliptic reconstruction, no stationary solves; ``mu_bar`` / ``mu_hat`` without a ``'_t'`` sit at ``_t = 0``.
"""
import numpy as np

from pylrbms_amd.discretize_elliptic_block_swipdg import DuneDiscretization, OperatorHandle
from pylrbms_amd.discretize_elliptic_block_swipdg import discretize as discretize_ell
from pylrbms_amd.estimators import ParabolicEstimator
from pylrbms_amd.parameters import CubicParameterSpace
from pylrbms_amd.sources import coefficient_parameter_type, local_estimates, setup_sources, source_components
from pylrbms_amd.vectorarrays import BlockVectorArray


class ImplicitEulerTimeStepper:
    """Stand-in for ``pymor.algorithms.timestepping.ImplicitEulerTimeStepper``: only ``nt`` is read on this path."""

    def __init__(self, nt, solver_options='operator'):
        self.nt = int(nt)
        self.solver_options = solver_options


class InstationaryDuneDiscretization(DuneDiscretization):
    """Reference :17-40.  Built from the elliptic discretization by ``discretize`` below."""

    def _solve_options(self, inverse_options):
        opts = inverse_options if isinstance(inverse_options, dict) else {}
        return min(float(opts.get('precision', 1e-12)), 1e-10), max(int(opts.get('max_iter', 20000)), 20000)

    _src = None       # the time-dependent source (``_setup_sources``), None: one component with coefficient 1
    _tv = False       # a lambda coefficient reads '_t': theta_q(t, mu), a coefficient row per step

    def _time_rows(self, mu):
        """``mu`` at the times of the ``nt + 1`` rows of the coefficient tables: row 0 at t = 0, row k at the time of step k,
        accumulated like pyMOR's ``implicit_euler`` (``t += dt``, then ``mu['_t'] = t``).  The ONE loop behind
        ``source_coefficients`` and ``diffusion_coefficients``: phi and theta cannot disagree on t_k."""
        from pylrbms_amd.parameters import Parameter
        mu = self.parse_parameter(mu)
        nt = self.time_stepper.nt
        dt = self.T / nt
        rows = []
        t = 0.0
        for k in range(nt + 1):
            if k > 0:
                t += dt
            rows.append(Parameter(dict(mu, _t=np.array(t))))
        return rows

    def source_coefficients(self, mu):
        """``phi [nt + 1][K]`` (fp64, host) of the time-dependent source at ``mu``: row 0 at t = 0, row k at the time of step k
        (``_time_rows``).  A plain number as coefficient is a constant."""
        if self._src is None:
            return np.ones((self.time_stepper.nt + 1, 1))
        coeffs = self._src['coefficients']
        return np.array([[c.evaluate(mu_t) if hasattr(c, 'evaluate') else float(c) for c in coeffs] for mu_t in self._time_rows(mu)])

    def diffusion_coefficients(self, mu):
        """``theta_t [nt + 1][Q]`` (fp64, host): row k holds theta_q(t_k, mu) at the times of ``source_coefficients``; on a
        discretization without a time-dependent coefficient every row is ``theta(mu)``.  ValueError unless every entry is positive."""
        if not self._tv:
            return np.tile(self.theta(mu), (self.time_stepper.nt + 1, 1))
        th = np.array([[c.evaluate(mu_t) for c in self.lambda_coeffs] for mu_t in self._time_rows(mu)])
        bad = np.argwhere(~(th > 0))
        if len(bad):
            k, q = (int(v) for v in bad[0])
            raise ValueError('diffusion coefficient q = {} at step k = {}: theta_q(t_k, mu) = {} is not positive'.format(q, k, th[k, q]))
        return th

    def theta(self, mu):
        if self._tv and '_t' not in self.parse_parameter(mu):
            raise NotImplementedError("theta(mu): the diffusion coefficients depend on time, mu needs a '_t' "
                                      '(diffusion_coefficients(mu) is the table of all steps)')
        return DuneDiscretization.theta(self, mu)

    def _estimator_coefficients(self, mu):
        """``coef [nt + 1][2]``: sqrt(gamma_bar / alpha_bar) and 1 / sqrt(alpha_hat alpha_bar) of the elliptic eta at every row of
        ``_time_rows`` (the second argument of ``lrbms_reduced_parabolic_estimate_batch_tv``)."""
        est = self.estimator
        coef = np.empty((self.time_stepper.nt + 1, 2))
        for k, mu_t in enumerate(self._time_rows(mu)):
            alpha_bar = est.alpha(est.lambda_coeffs, mu_t, est.mu_bar)
            gamma_bar = est.gamma(est.lambda_coeffs, mu_t, est.mu_bar)
            alpha_hat = est.alpha(est.lambda_coeffs, mu_t, est.mu_hat)
            coef[k] = np.sqrt(gamma_bar) / np.sqrt(alpha_bar), (1. / np.sqrt(alpha_hat)) / np.sqrt(alpha_bar)
        return coef

    def _phi_device(self, mu):
        return self.engine.ctx.from_numpy(np.ascontiguousarray(self.source_coefficients(mu)))

    def solve(self, mu, inverse_options=None):
        """``_solve`` (:28-40): ``nt + 1`` vectors, the first one the (zero) initial data."""
        import torch
        eng = self.engine
        rtol, max_iter = self._solve_options(inverse_options)
        dt = self.T / self.time_stepper.nt
        U0 = self.initial_data.tensor[:, :, 0] if self.initial_data is not None else None
        if self._tv:                                                       # one column of the batched export
            U = self.solve_batch([mu], inverse_options=inverse_options)[0]
            return BlockVectorArray(U.tensor.contiguous(), self.solution_space)
        if self._src is not None:
            U, info = eng.ctx.fom_implicit_euler_src(self.theta(mu), dt, self.time_stepper.nt, eng.A_diag, eng.A_cpl,
                                                     self._src['b_K'], self._phi_device(mu), U0=U0, rtol=rtol, max_iter=max_iter)
            self.last_solve_info = info
            return BlockVectorArray(U.permute(1, 2, 0), self.solution_space)
        if eng.S_ext != eng.S:
            # sharded: like the stationary solve, on the gathered block operator (DuneDiscretization._global_fom); the
            # initial data of the reference is zero (:82), a non-zero one would have to be gathered as well
            if U0 is not None and bool((U0 != 0).any()):
                raise NotImplementedError('non-zero initial data on a sharded discretization')
            ctx, A_diag_all, A_cpl_all, b_all = self._global_fom()
            U, info = ctx.fom_implicit_euler(self.theta(mu), dt, self.time_stepper.nt, A_diag_all, A_cpl_all, b_all, rtol=rtol,
                                             max_iter=max_iter)
            U = U[:, torch.as_tensor(eng.local, device=U.device)]
        else:
            U, info = eng.ctx.fom_implicit_euler(self.theta(mu), dt, self.time_stepper.nt, eng.A_diag, eng.A_cpl, eng.b, U0=U0,
                                                 rtol=rtol, max_iter=max_iter)
        self.last_solve_info = info
        return BlockVectorArray(U.permute(1, 2, 0), self.solution_space)

    def solve_batch(self, mus, inverse_options=None, as_snapshots=False):
        """Trajectories for a whole training set, 64 parameters per native ``lrbms_fom_implicit_euler_batch`` call (panels of 16
        columns that share every read of the operator blocks; one coarse level per call at the mean theta).  Returns a list with,
        per parameter, the ``BlockVectorArray`` ``[S, n, nt + 1]`` that ``solve(mu)`` returns -- views of the call's panel
        ``[nt + 1, S, n, nmu]``, as ``rd.solve_batch`` hands out its trajectories.  ``as_snapshots=True``: one ``BlockVectorArray`` of
        ``len(mus) * nt`` vectors instead, the steps 1 .. nt of every parameter, parameter-major: the layout
        ``extend_basis(..., method='pod')`` takes (at most 128 vectors).  ``as_snapshots='slabs'``: the list of the step slabs
        ``U[k]``, k = 1 .. nt, of every native call instead -- contiguous views ``[S, n, nmu_call]`` of the panels, no copy and no limit:
        what ``extend_basis(..., method='hapod')`` takes (sharded: the views ``[S, n, nt]`` of the trajectories).
        ``precision`` / ``max_iter`` as in ``solve``.
        ``last_solve_info``: the CG iterations summed over the calls and the worst final residual ratio.  On a sharded grid it is
        the loop of ``solve``."""
        import torch
        eng = self.engine
        mus = list(mus)
        if not mus:
            raise ValueError('solve_batch: no parameters')
        nt = self.time_stepper.nt
        slabs = isinstance(as_snapshots, str) and as_snapshots == 'slabs'
        if as_snapshots and not slabs and len(mus) * nt > 128:
            raise ValueError('solve_batch(as_snapshots=True): {} x {} vectors, the local POD takes at most 128'.format(len(mus), nt))
        its, rel = 0, 0.0
        panels = []
        if eng.S_ext != eng.S:
            trajs = []
            for mu in mus:
                trajs.append(self.solve(mu, inverse_options=inverse_options))
                its += self.last_solve_info['iterations']
                rel = max(rel, self.last_solve_info['relative_residual'])
        else:
            rtol, max_iter = self._solve_options(inverse_options)
            if self._tv:
                theta = np.stack([self.diffusion_coefficients(mu) for mu in mus])   # [len(mus), nt + 1, Q]
                native = eng.ctx.fom_implicit_euler_batch_tv
            else:
                theta = np.stack([self.theta(mu) for mu in mus])
                native = eng.ctx.fom_implicit_euler_batch
            phi = np.stack([self.source_coefficients(mu) for mu in mus])                # [len(mus), nt + 1, K]
            b_K = self._src['b_K'] if self._src is not None else eng.b.reshape(1, eng.S, eng.t.n)
            U0 = self.initial_data.tensor[:, :, 0] if self.initial_data is not None else None
            trajs = []
            for m0 in range(0, len(mus), 64):
                U, info = native(theta[m0:m0 + 64], self.T / nt, nt, eng.A_diag, eng.A_cpl, b_K, phi[m0:m0 + 64], U0=U0, rtol=rtol,
                                 max_iter=max_iter)
                its, rel = its + info['iterations'], max(rel, info['relative_residual'])
                trajs += [BlockVectorArray.view_of(U[:, :, :, m].permute(1, 2, 0), self.solution_space) for m in range(U.shape[3])]
                panels.append(U)
        self.last_solve_info = {'iterations': its, 'relative_residual': rel}
        if slabs:
            if eng.S_ext != eng.S:
                return [u.tensor[:, :, 1:] for u in trajs]
            return [U[k] for U in panels for k in range(1, nt + 1)]
        if not as_snapshots:
            return trajs
        return BlockVectorArray(torch.cat([u.tensor[:, :, 1:] for u in trajs], dim=2).contiguous(), self.solution_space)

    def solve_stationary(self, mu, inverse_options=None):
        """The elliptic solve of the underlying discretization (the limit ``t -> oo``)."""
        if self._tv:
            raise NotImplementedError('solve_stationary: the diffusion coefficients depend on time (theta_q(t, mu))')
        if self._src is not None:
            raise NotImplementedError('solve_stationary: the source depends on time (f = sum_j phi_j(t, mu) f_j)')
        return DuneDiscretization.solve(self, mu, inverse_options=inverse_options)

    def solve_stationary_batch(self, mus, inverse_options=None):
        """The elliptic ``solve_batch`` of the underlying discretization: one array of ``len(mus)`` stationary solutions."""
        if self._tv:
            raise NotImplementedError('solve_stationary_batch: the diffusion coefficients depend on time (theta_q(t, mu))')
        if self._src is not None:
            raise NotImplementedError('solve_stationary_batch: the source depends on time (f = sum_j phi_j(t, mu) f_j)')
        if self.engine.S_ext != self.engine.S:                       # (the elliptic loop would call this class's ``solve``)
            import torch
            mus = list(mus)
            if not mus:
                raise ValueError('solve_stationary_batch: no parameters')
            cols, its, rel = [], 0, 0.0
            for mu in mus:
                cols.append(self.solve_stationary(mu, inverse_options=inverse_options).tensor)
                its = max(its, self.last_solve_info['iterations'])
                rel = max(rel, self.last_solve_info['relative_residual'])
            self.last_solve_info = {'iterations': its, 'relative_residual': rel}
            return BlockVectorArray(torch.cat(cols, dim=2).contiguous(), self.solution_space)
        return DuneDiscretization.solve_batch(self, mus, inverse_options=inverse_options)

    def _refuse_local_corrections(self, what):
        """What the parabolic enrichment does not cover, refused before anything runs."""
        import torch
        eng = self.engine
        if self._tv:
            raise NotImplementedError(what + ': the diffusion coefficients depend on time (theta_q(t, mu)); the corrector kernel '
                                      'builds its step operator M + dt A(theta) once and would have to rebuild it in every step')
        if eng.S_ext != eng.S:
            raise NotImplementedError(what + ': a sharded discretization (S_ext != S); the neighbourhood problems need the operator '
                                      'blocks and load vectors of the halo subdomains on this rank')
        if getattr(self.estimator, 'elliptic_reconstruction', False):
            raise NotImplementedError(what + ': elliptic_reconstruction=True; the indicators that mark subdomains do not carry the '
                                      'reconstruction terms')
        if self.initial_data is not None and bool(torch.count_nonzero(self.initial_data.tensor)):
            raise NotImplementedError(what + ': non-zero initial data; the corrector trajectories start at x_0 = 0')

    def solve_for_local_correction_trajectories(self, subdomains, mu=None, inverse_options=None):
        """The parabolic counterpart of ``solve_for_local_corrections``: on the neighbourhood of every subdomain of ``subdomains``
        (all-Dirichlet outer boundary) the implicit Euler trajectory with zero initial value, the source of ``solve(mu)`` and the
        ``nt`` steps of the time stepper, restricted to the subdomain -- all of them in ONE launch
        (``lrbms_local_correction_euler``: one workgroup per neighbourhood runs every step).  Returns the device tensor
        ``[len(subdomains), n, nt]`` (column k - 1 = step k); ``last_local_correction_info`` [len(subdomains), 2] = the PCG iterations
        summed over the steps and the worst final residual ratio of a step.  ``NotImplementedError`` for time-dependent diffusion
        coefficients, non-zero initial data, a sharded discretization and ``elliptic_reconstruction=True``."""
        self._refuse_local_corrections('solve_for_local_correction_trajectories')
        eng = self.engine
        rtol, max_iter = self._solve_options(inverse_options)
        mu = self.parse_parameter(mu)
        nt = self.time_stepper.nt
        marked = [eng.local.index(int(ii)) for ii in subdomains]
        b_K = self._src['b_K'] if self._src is not None else None
        corr, info = eng.local_corrections_euler(self.theta(mu), self.T / nt, nt, marked, self._phi_device(mu), b_K=b_K, rtol=rtol,
                                                 max_iter=max_iter)
        self.last_local_correction_info = info
        return corr

    def _source_rows(self, mu, L):
        """The phi rows of the columns of an array of ``L`` vectors: the trajectory's rows if ``L == nt + 1``; otherwise None
        (no source: the time-derivative term reads only the nonconformity of U_{k+1} - U_k, which does not involve f)."""
        if self._src is None or L != self.time_stepper.nt + 1:
            return None
        return self._phi_device(mu)

    def _local_estimates(self, U, mu):
        """With a time-dependent source: the indicators of U_k for f(t_k, mu) = sum_j phi[k][j] f_j.  The source-free part is
        the batched estimate with f2 = 0 and r_fd = 0; the f terms of the residual indicator come from
        ``lrbms_project_sources`` on the same chunk (identity coefficients) and ``lrbms_reduced_source_terms``."""
        if self._src is None:
            return DuneDiscretization._local_estimates(self, U, mu)
        return local_estimates(self.engine, U.tensor, self.theta(mu), self._src, self._source_rows(mu, len(U)))

    def _time_residual_norm2(self, dU, mu):
        """``R = operator.apply(dU, mu); l2_product.apply_inverse(R).pairwise_dot(R)`` (estimators.py:146-148): [len(dU)]."""
        eng = self.engine
        if eng.S_ext != eng.S:
            # sharded: the residual norm is a sum over ALL subdomains; like the solves it is taken on the gathered block
            # operator (every rank gathers the difference vectors and evaluates the same global sum)
            from pylrbms_amd.parallel import gather_subdomain_rows
            ctx, A_d, A_c, _ = self._global_fom()
            dU_all = gather_subdomain_rows(dU.tensor.contiguous(), self._owned_subdomains(), eng.grid.num_subdomains,
                                           getattr(self.mpi_comm, 'group', None)).contiguous()
            R = ctx.fom_apply(self.theta(mu), A_d, A_c, dU_all)
            return ctx.mass_inverse_norm2(R).sum(dim=0).cpu().numpy()
        R = eng.ctx.fom_apply(self.theta(mu), eng.A_diag, eng.A_cpl, dU.tensor.contiguous())
        return eng.ctx.mass_inverse_norm2(R).sum(dim=0).cpu().numpy()

    def estimate(self, U, mu=None, decompose=False):
        if not self._tv:
            return DuneDiscretization.estimate(self, U, mu, decompose=decompose)
        return self._estimate_tv(U, mu)

    def _estimate_tv(self, U, mu):
        """The parabolic estimate of a full-order trajectory with the coefficient frozen per step (the verification path of
        ``lrbms_reduced_parabolic_estimate_batch_tv``): the elliptic indicators of U_k at row k of
        ``diffusion_coefficients`` / ``source_coefficients``, the time residual of U_{k+1} - U_k with A(theta_t[k + 1])
        (``lrbms_fom_apply`` per step), the nonconformity of the differences as before (it reads no theta)."""
        import torch
        eng, est = self.engine, self.estimator
        nt = self.time_stepper.nt
        dt = self.T / nt
        assert len(U) == nt + 1, 'estimate: a trajectory of nt + 1 vectors'
        th, rows, coef = self.diffusion_coefficients(mu), self._time_rows(mu), self._estimator_coefficients(mu)
        phi = self._phi_device(mu) if self._src is not None else None
        cols = []
        for k in range(nt + 1):
            if self._src is not None:
                cols.append(local_estimates(eng, U.tensor[:, :, k:k + 1].contiguous(), th[k], self._src, phi[k:k + 1]))
            else:
                cols.append(DuneDiscretization._local_estimates(self, U[k:k + 1], rows[k]))
        nc, r, df = (torch.cat([c[i] for c in cols], dim=1) for i in range(3))       # [S, nt + 1]
        if est.sqrt_local:
            nc, r, df = (x.abs().sqrt() for x in (nc, r, df))
        sc = 2 * np.sqrt(dt / 3)
        eta = (coef[:, 0] * nc.norm(dim=0).cpu().numpy() + coef[:, 1] * (r + df).norm(dim=0).cpu().numpy()) * sc
        dU = U[1:] - U[:-1]
        tr = np.empty(nt)
        for k in range(nt):
            R = eng.ctx.fom_apply(th[k + 1], eng.A_diag, eng.A_cpl, dU.tensor[:, :, k:k + 1].contiguous())
            tr[k] = float(eng.ctx.mass_inverse_norm2(R).sum())
        time_residual = np.sqrt(tr * (dt / 3))
        time_deriv_nc = np.sqrt(np.maximum(self._local_estimates(dU, rows[1])[0].cpu().numpy() * (1 / dt), 0.0))
        est_value = np.linalg.norm(eta) + np.linalg.norm(time_residual) + np.sqrt(float(np.sum(time_deriv_nc ** 2)))
        return est_value, tuple(x.cpu().numpy() * sc for x in (nc, r, df)) + (time_residual, time_deriv_nc)

    def _reconstruction_terms(self, U, mu):
        """``r_l2(BU_R, BU_R) - r_l2(F_R, F_R) - 2 r_ud(BUF_R, U_r)`` per subdomain and vector (estimators.py:65-68,
        :80-83) -> [S, len(U)]:  BU = A(mu) U (``lrbms_fom_apply``), the ``r_l2`` terms are ``M^-1`` norms
        (``lrbms_mass_inverse_norm2``), and in ``r_ud(M^-1 (BU - f), U_r)`` the mass matrices cancel:
        ``(BU - f)^T Div U_r`` (``lrbms_flux_reconstruct`` -> ``lrbms_div_apply`` -> ``lrbms_div_pairing``)."""
        import torch
        eng = self.engine
        if eng.S_ext != eng.S:
            raise NotImplementedError('the elliptic-reconstruction terms need all subdomains on one rank')
        theta = self.theta(mu)
        c = eng.ctx
        t2 = c.mass_inverse_norm2(eng.b.reshape(eng.S, eng.t.n, 1).contiguous())            # [S, 1]
        out = []
        for c0 in range(0, len(U), 16):
            V = U.tensor[:, :, c0:c0 + 16].contiguous()
            BU = c.fom_apply(theta, eng.A_diag, eng.A_cpl, V)
            t1 = c.mass_inverse_norm2(BU)
            D = c.div_apply(c.flux_reconstruct(eng.F, V), mode=0)
            t3 = c.div_pairing(theta, D, (BU - eng.b.reshape(eng.S, eng.t.n, 1)).contiguous())
            out.append(t1 - t2 - 2.0 * t3)
        return torch.cat(out, dim=1)


def _source_components(p):
    """(functions, coefficients) of a source that is not one component with coefficient 1, else None
    (``pylrbms_amd.sources.source_components``)."""
    return source_components(p)


def _lambda_reads_time(p):
    """True if a coefficient of ``p['lambda']`` names ``'_t'`` in its ``parameter_type``."""
    lam = p['lambda']
    return isinstance(lam, dict) and any('_t' in coefficient_parameter_type(c) for c in lam['coefficients'])


def _at_time_zero(mu, parameter_type):
    """``mu`` as a ``Parameter`` with ``_t = 0`` unless it brings a ``'_t'`` of its own."""
    from pylrbms_amd.parameters import Parameter, parse_parameter
    mu = parse_parameter(mu, parameter_type)
    return mu if '_t' in mu else Parameter(dict(mu, _t=np.array(0.0)))


def _setup_sources(d, funcs, coeffs):
    """b_K, f_smp_K and F2 of the K source components (``pylrbms_amd.sources.setup_sources``), kept as ``d._src``."""
    d._src = setup_sources(d.engine, funcs, coeffs)


def discretize(grid_and_problem_data, T, nt, solver_options=None, mpi_comm=None, device_index=None,
               elliptic_reconstruction=False, conventions=None):
    """Reference :43-95.  Returns ``(d, d_data)``.  ``p['f']`` may be ``{'functions': [...], 'coefficients': [...]}`` with any
    number of components and coefficients of ``mu`` and ``'_t'`` (module docstring).  ``conventions``: the switches of the elliptic
    ``discretize`` (e.g. ``{'oswald_vertex_patch': True}``), handed on to it."""
    tv = _lambda_reads_time(grid_and_problem_data)
    if tv:
        grid = grid_and_problem_data['grid']
        if len(grid.subdomains_on_rank) != grid.num_subdomains:
            raise NotImplementedError('time-dependent diffusion coefficients (theta_q(t, mu)) need all subdomains on one rank')
        if elliptic_reconstruction:
            raise NotImplementedError('elliptic_reconstruction with time-dependent diffusion coefficients (theta_q(t, mu))')
        # the reference parameters of alpha / gamma and of the energy product: without a '_t' of their own they sit at _t = 0
        ptype = {k: v for k, v in grid_and_problem_data.get('parameter_type', {}).items() if k != '_t'}
        grid_and_problem_data = dict(grid_and_problem_data, parameter_type=ptype,
                                     mu_bar=_at_time_zero(grid_and_problem_data['mu_bar'], ptype),
                                     mu_hat=_at_time_zero(grid_and_problem_data['mu_hat'], ptype))
    src = _source_components(grid_and_problem_data)
    if src is not None:
        from pylrbms_amd.functions import SumFunction
        grid = grid_and_problem_data['grid']
        if len(grid.subdomains_on_rank) != grid.num_subdomains:
            raise NotImplementedError('a time-dependent / multi-component source needs all subdomains on one rank')
        if elliptic_reconstruction:
            raise NotImplementedError('elliptic_reconstruction with a time-dependent / multi-component source')
        # the elliptic discretization is built on sum_j f_j (its quadrature orders cover every component); its own b / f2
        # are not read on this path
        grid_and_problem_data = dict(grid_and_problem_data, f=SumFunction(src[0], [1.0] * len(src[0]), name='f_sum'))
    d, d_data = discretize_ell(grid_and_problem_data, solver_options, mpi_comm, device_index=device_index, conventions=conventions,
                               _time_dependent_lambda=tv)
    assert isinstance(d.parameter_space, CubicParameterSpace)              # :45
    d.__class__ = InstationaryDuneDiscretization
    d._tv = tv
    d.T = float(T)
    d.time_stepper = ImplicitEulerTimeStepper(nt=nt, solver_options='operator')   # :87
    d.initial_data = d.solution_space.zeros(1, d.engine.ctx)               # :82
    d.mass = d.products['l2']                                              # :60
    for ii in d.engine.local:                                              # :65-74
        for kind in ('r_ud', 'r_l2'):
            name = '{}_{}'.format(kind, ii)
            d.operators[name] = OperatorHandle(name, 'l2' if kind == 'r_l2' else kind, ii, d)
    e = d.estimator                                                        # :76-77
    d.estimator = ParabolicEstimator(e.grid, e.min_diffusion_evs, e.subdomain_diameters, e.local_eta_rf_squared,
                                     e.lambda_coeffs, e.mu_bar, e.mu_hat, e.flux_reconstruction,
                                     e.oswald_interpolation_error, e.mpi_comm,
                                     elliptic_reconstruction=elliptic_reconstruction)
    parameter_range = grid_and_problem_data['parameter_range'] if 'parameter_range' in grid_and_problem_data else (0.1, 1.0)
    d.parameter_space = CubicParameterSpace(d.parameter_type, parameter_range[0], parameter_range[1])   # :93
    d.name = 'parabolic_block_swipdg'
    if src is not None:
        _setup_sources(d, *src)
    return d, d_data
