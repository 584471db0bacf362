"""Block SWIPDG P2 discretization in 3D on the HIP path (BASELINE.json config 5) behind the reference's API shape.

The reference's ``discretize`` (python/dune/pylrbms/discretize_elliptic_block_swipdg.py:530-811) binds the 2D / P1 operators
only (:22-23); this module gives the 3D / P2 path the same surface for the calls on the hot path:

    d, data = discretize(grid_and_problem_data)          # :530       offline assembly (lrbms3_assemble_*)
    d.estimate(U, mu)                                     # :205-217   full-order estimate of a block DG vector
    reductor = LRBMSReductor3D(d, bases)                  # reductor.py:17-31
    rd = reductor.reduce()                                # reductor.py:33-73   one lrbms3_project_estimate pass
    u = rd.solve(mu);  rd.estimate(u, mu)                 # online (estimators.py:45-130)

``grid_and_problem_data``: the dict of ``pylrbms_amd.multiscale_problem3d.init_grid_and_problem`` (grid, lambda functions and
coefficient functionals, lambda_bar / lambda_hat, f, mu_bar / mu_hat).  ``d.solve(mu)`` generates snapshots (block-Jacobi CG).

Online enrichment (reductor.py:75-78, online_enrichment.py) is opt-in: ``discretize(..., online_enrichment=True)`` also assembles
the Dirichlet correction blocks of the neighbourhood corrector problems; ``d.solve_for_local_correction(s)``,
``reductor.enrich_local`` / ``enrich_local_batch`` and ``AdaptiveEnrichment`` then run on the 3D objects."""
import numpy as np

from pylrbms_amd._native import NativeError
from pylrbms_amd.engine3d import Engine3D
from pylrbms_amd.reductor import ExtensionError, LocalBasisSlab


class BlockSpace3D:
    """What ``AdaptiveEnrichment`` and its callbacks read of a (block) vector space: ``num_blocks`` and ``dim``."""

    def __init__(self, num_blocks, dim):
        self.num_blocks, self.dim = int(num_blocks), int(dim)


_NEEDS_KEYWORD = 'online enrichment in 3D needs the corrector data: discretize(..., online_enrichment=True)'


class BlockDiscretization3D:
    _src = None                        # the affine source record (``sources3d.setup_sources3d``); None: one component, coefficient 1
    _time_dependent_source = False     # the parabolic subclass takes coefficients c(mu, t)
    _tv = False                        # a diffusion coefficient reads the time: theta_q(t, mu), a row per step
    _theta_arity = None                # 1 / 2 per diffusion coefficient (``sources3d.coefficient_arity``); None: all c(mu)

    def __init__(self, p, device_index=0, online_enrichment=False):
        self.grid = p['grid']
        self.online_enrichment = bool(online_enrichment)
        if self.online_enrichment and getattr(self.grid, 'world_size', 1) > 1:
            raise NotImplementedError('online_enrichment=True on a sharded 3D grid: the corrector solves need all subdomains on one rank')
        lam = p['lambda']
        f = p['f']
        comp = None
        if isinstance(f, dict):
            from pylrbms_amd import sources3d
            from pylrbms_amd.sources import source_components
            comp = source_components(p)
            if comp is None:
                f = f['functions'][0]
            else:                                          # f = sum_j c_j f_j; the refusals come before any device work
                arity = sources3d.check_sources3d(self.grid, comp[1])
                if 2 in arity and not self._time_dependent_source:
                    raise NotImplementedError('a source coefficient c(mu, t) depends on time: this needs the parabolic discretize')
                f = sources3d.sum_function(comp[0])          # the engine is built on sum_j f_j, as in 2D
        self.coefficients = list(lam['coefficients'])
        from pylrbms_amd.sources3d import diffusion_arities
        self._theta_arity = diffusion_arities(self.coefficients)      # c(mu) or c(mu, t), read before any device work
        self._tv = 2 in self._theta_arity
        if self._tv and not self._time_dependent_source:
            raise NotImplementedError('a diffusion coefficient c(mu, t) depends on time: this needs the parabolic discretize')
        self.mu_bar, self.mu_hat = p['mu_bar'], p['mu_hat']
        self.engine = Engine3D(self.grid, lam['functions'], f, p['lambda_bar'], p['lambda_hat'],
                               data_degree=p.get('data_degree', 2), device_index=device_index,
                               theta_bar=list(self._theta_at(self.mu_bar, 0.0))).assemble(self.online_enrichment)
        self.Q = self.engine.Q
        self.solution_space = BlockSpace3D(self.engine.S, self.engine.S * self.engine.t.n)
        self.parameter_range = p.get('parameter_range')
        if comp is not None:
            self._src = sources3d.setup_sources3d(self.engine, comp[0], comp[1], arity)

    def source_coefficients(self, mu):
        """[K]: the coefficients c_j(mu) of the source f(mu) = sum_j c_j(mu) f_j ([1.] without an affine source)."""
        if self._src is None:
            return np.ones(1)
        from pylrbms_amd.sources3d import evaluate_stationary
        return evaluate_stationary(self._src, mu)

    def _load_vector(self, mu):
        """b(mu) [S, n]: ``lrbms3_combine_sources`` of the components' load vectors."""
        if self._src is None:
            return self.engine.ops['b']
        from pylrbms_amd.sources3d import evaluate_stationary
        return self.engine.ctx.combine_sources(evaluate_stationary(self._src, mu), self._src['b_K'])

    def _coefficient(self, q, mu, t):
        """Diffusion coefficient q at (mu, t): ``c(mu)``, or ``c(mu, t)`` where its signature takes the time."""
        c = self.coefficients[q]
        return c(mu, t) if self._theta_arity is not None and self._theta_arity[q] == 2 else c(mu)

    def _theta_at(self, mu, t):
        return np.array([float(self._coefficient(q, mu, t)) for q in range(len(self.coefficients))], dtype=np.float64)

    def theta(self, mu):
        if self._tv:
            raise NotImplementedError('the diffusion coefficients depend on time: no single row is "the" theta '
                                      '(diffusion_coefficients(mu) is the table of all steps)')
        return np.array([float(c(mu)) for c in self.coefficients], dtype=np.float64)

    def parse_parameter(self, mu):
        """``d.parse_parameter(mu)`` (online_enrichment.py:69): the 3D coefficient functionals take ``mu`` as it is."""
        return mu

    def solve_for_local_corrections(self, subdomains, mu, rtol=1e-12, max_iter=20000, return_info=False):
        """The correctors of ``subdomains`` at ``mu`` in one batched native solve: [len(subdomains), n] (device).  Each is the
        SWIPDG problem on the subdomain and its face neighbours with Dirichlet data on the outer boundary and the load b(mu),
        restricted to the subdomain (block_swipdg.py:227-316).  ``info`` [len, 2]: iterations, final relative residual."""
        if not self.online_enrichment:
            raise NotImplementedError(_NEEDS_KEYWORD)
        eng = self.engine
        marked = [eng.local.index(int(ii)) for ii in subdomains]
        corr, info = eng.local_corrections(self.theta(mu), marked, rtol=rtol, max_iter=max_iter, b=self._load_vector(mu))
        return (corr, info) if return_info else corr

    def solve_for_local_correction(self, subdomain, Us, mu, rtol=1e-12, max_iter=20000):
        """``d.solve_for_local_correction(subdomain, Us, mu)`` (block_swipdg.py:227-316) -> [n] (device).  ``Us`` feeds only the
        Dirichlet lift the reference has commented out: accepted and unused."""
        return self.solve_for_local_corrections([subdomain], mu, rtol=rtol, max_iter=max_iter)[0]

    def shape_functions(self, subdomain, order=0):
        """``d.shape_functions(subdomain, order)`` (discretize_elliptic_block_swipdg.py:190-203 in 2D): the constant (order 0)
        and, for order 1, the three coordinate functions relative to the subdomain centre, as P2 nodal vectors [n, 1 or 4]
        (device).  The reductor starts every local basis with them (reductor.py:29-31)."""
        if order not in (0, 1):
            raise NotImplementedError('shape functions of order 0 and 1')
        eng = self.engine
        x = np.asarray(eng.t.node_coordinates(), dtype=np.float64)
        cols = [np.ones(eng.t.n)]
        if order == 1:
            centre = 0.5 * (x.max(axis=0) + x.min(axis=0))
            cols += [x[:, a] - centre[a] for a in range(3)]
        return eng.ctx.from_numpy(np.stack(cols, axis=1))

    def alpha(self, mu, mu2, t=0.0):
        """min_q theta_q(mu) / theta_q(mu2) as written in the reference: the loop returns in its first pass
        (estimators.py:114-121), i.e. the first component only.  With coefficients of the time, ``mu`` is taken at ``t`` and the
        reference parameter ``mu2`` (mu_bar / mu_hat) at t = 0."""
        return self._coefficient(0, mu, t) / self._coefficient(0, mu2, 0.0)

    def gamma(self, mu, mu2, t=0.0):
        return max(self._coefficient(q, mu, t) / self._coefficient(q, mu2, 0.0) for q in range(len(self.coefficients)))

    def combine(self, eta_loc, mu, decompose=False):
        """EstimatorBase._estimate_elliptic (estimators.py:99-112) from the local terms [3, S]."""
        nc, r, df = (np.asarray(x, dtype=np.float64) for x in eta_loc)
        a_bar, a_hat, g_bar = self.alpha(mu, self.mu_bar), self.alpha(mu, self.mu_hat), self.gamma(mu, self.mu_bar)
        if getattr(self.grid, 'world_size', 1) > 1:
            # sharded: eta_loc holds this rank's subdomains only; the two mpi_norm of estimators.py:100-101 as one all-reduce of the
            # sums of squares (parallel.global_norms, as in 2D) -- on the device, RCCL has no host collectives
            import torch
            from pylrbms_amd.parallel import global_norms
            dev = self.engine.ctx.device
            norms = global_norms(torch.as_tensor(nc, device=dev), torch.as_tensor(r + df, device=dev), getattr(self, 'group', None))
            n_nc, n_rdf = float(norms[0]), float(norms[1])
        else:
            n_nc, n_rdf = np.linalg.norm(nc), np.linalg.norm(r + df)
        eta = (1.0 / np.sqrt(a_bar)) * (np.sqrt(g_bar) * n_nc + (1.0 / np.sqrt(a_hat)) * n_rdf)
        if not decompose:
            return eta
        return eta, (nc, r, df), (2.0 / a_bar) * (g_bar * nc ** 2 + (1.0 / a_hat) * (r + df) ** 2)

    def solve(self, mu, rtol=1e-10, max_iter=50000, return_info=False):
        """``d.solve(mu)`` (:219-225): the full-order solution as a block DG vector [S, n] -- CG on the never-assembled block
        operator with a two-level preconditioner (10 x 10 element blocks + P1 per subdomain; ``lrbms3_fom_solve``); snapshot
        generation.  Sharded (one tile of subdomains per rank): as in 2D every rank gathers the block operator once (1.6 GB at
        config 5, against 288 GB of HBM) and solves redundantly through a second context that holds the GLOBAL neighbour table;
        it keeps its own rows."""
        eng = self.engine
        if eng.S_ext == eng.S:
            if not getattr(self, '_fom_kept', False):       # one dense coarse factorisation for all snapshots of this discretization
                eng.ctx.fom_precond_keep(True)
                self._fom_kept = True
            U, info = eng.ctx.fom_solve(self.Q, self.theta(mu), eng.ops['A_diag'], eng.ops['A_cpl'], self._load_vector(mu), rtol=rtol,
                                        max_iter=max_iter)
            return (U, info) if return_info else U
        import torch
        ctx, A_d, A_c, b = self._global_fom()
        U, info = ctx.fom_solve(self.Q, self.theta(mu), A_d, A_c, b, rtol=rtol, max_iter=max_iter)
        U = U[torch.as_tensor(eng.local, device=U.device)].contiguous()
        return (U, info) if return_info else U

    def solve_batch(self, mus, rtol=1e-10, max_iter=50000, return_info=False):
        """Snapshots for a whole training set: one tensor [S, n, len(mus)] (the slab layout ``extend_basis(..., method='pod')``
        takes), 64 parameters per native ``lrbms3_fom_solve_batch`` call: panels of 16 columns share every read of the operator
        blocks, one two-level preconditioner per call at the mean theta of its columns.  ``info``: (largest
        iteration count of a panel, worst final residual ratio).  On a sharded grid it is the loop of ``solve``."""
        import torch
        eng = self.engine
        mus = list(mus)
        if not mus:
            raise ValueError('solve_batch: no parameters')
        cols, its, rel = [], 0, 0.0
        if eng.S_ext != eng.S:
            for mu in mus:
                U, info = self.solve(mu, rtol=rtol, max_iter=max_iter, return_info=True)
                cols.append(U[:, :, None])
                its, rel = max(its, info[0]), max(rel, info[1])
        else:
            theta = np.stack([self.theta(mu) for mu in mus])
            # (the stationary coefficients [K] also on the parabolic subclass, whose table is [nt + 1, K]: ``solve_stationary_batch``)
            phi = np.stack([BlockDiscretization3D.source_coefficients(self, mu) for mu in mus])
            b_K = self._src['b_K'] if self._src is not None else eng.ops['b'].reshape(1, eng.S, eng.t.n)
            for m0 in range(0, len(mus), 64):
                X, info = eng.ctx.fom_solve_batch(theta[m0:m0 + 64], eng.ops['A_diag'], eng.ops['A_cpl'], phi[m0:m0 + 64], b_K,
                                                  rtol=rtol, max_iter=max_iter)
                cols.append(X)
                its, rel = max(its, info['iterations']), max(rel, info['relative_residual'])
        U = cols[0] if len(cols) == 1 else torch.cat(cols, dim=2).contiguous()
        return (U, (its, rel)) if return_info else U

    def _global_fom(self):
        """(context, A_diag [Q, S_total, n_T, 5, 100], A_cpl [Q, S_total, 6, ncf, 100], b [S_total, n]) in global subdomain order."""
        if getattr(self, '_fom_global', None) is None:
            from pylrbms_amd._native3d import Native3DContext
            from pylrbms_amd.parallel import gather_subdomain_rows
            eng, g = self.engine, self.grid
            owned = [list(g._partition(r, g.world_size)) for r in range(g.world_size)]
            total = g.num_subdomains
            group = getattr(self, 'group', None)
            A_d = gather_subdomain_rows(eng.ops['A_diag'].permute(1, 0, 2, 3, 4).contiguous(), owned, total, group)
            A_c = gather_subdomain_rows(eng.ops['A_cpl'].permute(1, 0, 2, 3, 4).contiguous(), owned, total, group)
            b = gather_subdomain_rows(eng.ops['b'], owned, total, group)
            ctx = Native3DContext(eng.ctx.device.index)
            nbr = np.asarray(g.neighbor_slots, dtype=np.int32).reshape(total, 7)
            ctx.mesh_upload(eng.t, eng.spec, eng.t.tables(eng.spec), nbr, g.phys_mask, total, total)
            ctx.fom_precond_keep(True)
            self._fom_global = (ctx, A_d.permute(1, 0, 2, 3, 4).contiguous(), A_c.permute(1, 0, 2, 3, 4).contiguous(), b.contiguous())
        return self._fom_global

    def apply(self, U, mu):
        """A(mu) U for a block DG array U [S, n, M] (BlockOperator.apply, :500-507)."""
        eng = self.engine
        return eng.ctx.fom_apply(self.Q, self.theta(mu), eng.ops['A_diag'], eng.ops['A_cpl'], U)

    def estimate(self, U, mu, decompose=False):
        """Full-order estimate of the block DG vector U [S, n] (:205-217): the pass with U as a one-column basis, u = 1."""
        eng = self.engine
        V = (U if isinstance(U, eng.ctx.torch.Tensor) else eng.ctx.from_numpy(np.asarray(U))).reshape(eng.S_ext, eng.t.n, 1).contiguous()
        ones = eng.ctx.zeros(eng.S_ext, 1) + 1.0
        if self._src is None:
            out = eng.project_and_estimate(V)
            return self.combine(eng.reduced_estimate(self.theta(mu), ones, out).cpu().numpy(), mu, decompose)
        # affine source: the estimate without its f terms, plus the f terms at c(mu) (the residual indicator is affine in them)
        from pylrbms_amd import sources3d
        theta, phi = self.theta(mu), self.source_coefficients(mu)
        work = eng.alloc_work(1)
        out = eng.project_and_estimate(V, work=work)
        out0, ops0 = sources3d.zeroed(eng, out)
        eta = eng.ctx.reduced_estimate(self.Q, theta, ones, out0, ops0, eng.hdiam)
        _, r_fd_K = eng.ctx.project_sources(self.Q, self._src['b_K'], self._src['bdiv_K'], V, work)
        eta[1] += sources3d.source_terms(eng, self.Q, self._src, theta[None], phi[None], r_fd_K, out, ones[:, :, None].contiguous())[:, 0]
        return self.combine(eta.cpu().numpy(), mu, decompose)


class ReducedDiscretization3D:
    """``rd``: the 7-slot block-sparse reduced system and the projected estimator operators (factored layout), in HBM."""

    def __init__(self, reductor, out, rhs_red_K=None, r_fd_K=None):
        """``rhs_red_K`` [K, S, N], ``r_fd_K`` [K, S, QN]: the projections of an affine source's components
        (``lrbms3_project_sources``); ``out['rhs_red']`` and ``out['r_fd']`` -- those of sum_j f_j -- are then None."""
        self.reductor, self.d, self.out = reductor, reductor.d, out
        self.rhs_red_K, self.r_fd_K = rhs_red_K, r_fd_K
        self.N = out['B_sys'].shape[-1]
        self.solution_space = BlockSpace3D(self.d.engine.S, sum(reductor.local_sizes()))

    @property
    def operators(self):
        """Dense blocks of the projected estimator operators (reference: ``rd.operators``), built on request from the factors."""
        from pylrbms_amd.engine3d import expand_factored
        if self.rhs_red_K is not None:
            raise NotImplementedError('dense operators of a reduced model with an affine source (rhs_red and r_fd are per component)')
        return expand_factored(self.d.engine, self.out, self.d.Q, self.N)

    def _phi(self, mu):
        """[K]: the stationary source coefficients c(mu) (NotImplementedError if one of them depends on time)."""
        from pylrbms_amd.sources3d import evaluate_stationary
        return evaluate_stationary(self.d._src, mu)

    def _zeroed(self):
        if getattr(self, '_zero', None) is None:
            from pylrbms_amd.sources3d import zeroed
            self._zero = zeroed(self.d.engine, self.out)
        return self._zero

    def solve(self, mu, rtol=1e-12, max_iter=20000, return_info=False):
        """``rd.solve(mu)`` (online_adaptive_lrbms.py:141).  N <= 32: the batched solver with one parameter -- it has the
        two-level preconditioner of this reduced model and the matrix-core panel matvec; larger N: the single-parameter
        block-Jacobi PCG."""
        if self.N <= 32:
            U, info = self.solve_batch([mu], rtol=rtol, max_iter=max_iter, return_info=True)
            return (U[0], info) if return_info else U[0]
        eng = self.d.engine
        if self.rhs_red_K is None:
            u, info = eng.reduced_solve(self.d.theta(mu), self.out, rtol=rtol, max_iter=max_iter)
        else:                                  # rhs_red(mu) by lrbms3_combine_sources, then the single-parameter solve
            rhs = eng.ctx.combine_sources(self._phi(mu), self.rhs_red_K)
            u, info = eng.ctx.reduced_solve(self.d.Q, self.d.theta(mu), self.out['B_sys'], rhs, rtol=rtol, max_iter=max_iter)
        return (u, info) if return_info else u

    def solve_batch(self, mus, rtol=1e-12, max_iter=20000, return_info=False):
        """Reduced solutions for a list of parameters, <= 64 per native call: [len(mus), S, N]."""
        import torch
        eng, out = self.d.engine, []
        info = (0, 0.0)
        if self.N > 32:                       # the batched kernels take N <= 32: one native solve per parameter
            for mu in mus:
                u, inf = self.solve(mu, rtol=rtol, max_iter=max_iter, return_info=True)
                out.append(u[None])
                info = (max(info[0], inf[0]), max(info[1], inf[1]))
            U = torch.cat(out, dim=0).contiguous()
            return (U, info) if return_info else U
        # two-level preconditioner: inverse diagonal blocks + coarse level on the first local basis vectors, the coarse inverse built
        # once per reduced model at the middle of the parameter range (mu_bar without one); any SPD preconditioner is admissible
        if getattr(self, '_pc', None) is None:
            pr = self.d.parameter_range
            mu_ref = 0.5 * (pr[0] + pr[1]) if pr is not None else self.d.mu_bar
            try:
                self._pc = eng.ctx.reduced_precond_build(self.d.Q, self.d.theta(mu_ref), self.out['B_sys'])
            except NativeError as exc:         # first basis vectors that do not give an SPD coarse matrix (e.g. a zero vector):
                if 'not positive definite' not in str(exc):      # block-Jacobi alone; anything else (HIP errors, bad arguments) is raised
                    raise
                self._pc = False
        eng.ctx.reduced_precond_use(self._pc if self._pc is not False else None)
        try:
            for b0 in range(0, len(mus), 64):          # 64 per native call: four groups of 16 on four streams
                th = np.stack([self.d.theta(mu) for mu in mus[b0:b0 + 64]])
                if self.rhs_red_K is None:
                    ub, inf = eng.ctx.reduced_solve_batch(self.d.Q, th, self.out['B_sys'], self.out['rhs_red'], rtol=rtol, max_iter=max_iter)
                else:
                    ph = np.stack([self._phi(mu) for mu in mus[b0:b0 + 64]])
                    ub, inf = eng.ctx.reduced_solve_batch_src(self.d.Q, th, ph, self.out['B_sys'], self.rhs_red_K, rtol=rtol,
                                                              max_iter=max_iter)
                out.append(ub.permute(2, 0, 1))
                info = (max(info[0], inf[0]), max(info[1], inf[1]))
        finally:
            eng.ctx.reduced_precond_use(None)
        U = torch.cat(out, dim=0).contiguous()
        return (U, info) if return_info else U

    def estimate_batch(self, U, mus, decompose=False):
        """Estimates of the reduced solutions U [len(mus), S, N] (as ``solve_batch`` returns them): list of eta; with ``decompose``
        list of (eta, (nc, r, df), local indicators) as ``estimate`` returns them."""
        eng = self.d.engine
        th = np.stack([self.d.theta(mu) for mu in mus])
        u = U.permute(1, 2, 0).contiguous()
        if self.rhs_red_K is None:
            eta = eng.ctx.reduced_estimate_batch(self.d.Q, th, u, self.out, eng.ops, eng.hdiam)
        else:                                  # the f terms of all columns in one launch, each with its own theta and c(mu)
            from pylrbms_amd.sources3d import source_terms
            out0, ops0 = self._zeroed()
            eta = eng.ctx.reduced_estimate_batch(self.d.Q, th, u, out0, ops0, eng.hdiam)
            ph = np.stack([self._phi(mu) for mu in mus])
            eta[1] += source_terms(eng, self.d.Q, self.d._src, th, ph, self.r_fd_K, self.out, u)
        eta = eta.cpu().numpy()
        return [self.d.combine(eta[:, :, m], mu, decompose) for m, mu in enumerate(mus)]

    def estimate(self, u, mu, decompose=False):
        eng = self.d.engine
        if self.rhs_red_K is None:
            eta_loc = eng.reduced_estimate(self.d.theta(mu), u.contiguous(), self.out)
        else:
            from pylrbms_amd.sources3d import source_terms
            out0, ops0 = self._zeroed()
            theta = self.d.theta(mu)
            eta_loc = eng.ctx.reduced_estimate(self.d.Q, theta, u.contiguous(), out0, ops0, eng.hdiam)
            eta_loc[1] += source_terms(eng, self.d.Q, self.d._src, theta[None], self._phi(mu)[None], self.r_fd_K,
                                       self.out, u[:, :, None].contiguous())[:, 0]
        return self.d.combine(eta_loc.cpu().numpy(), mu, decompose)


ExtensionError3D = ExtensionError      # a vector handed to ``extend_basis`` is (numerically) in the span of a local basis


class LRBMSReductor3D(LocalBasisSlab):
    """``LRBMSReductor`` (reference reductor.py:17-78) for the 3D path: the same constructor and methods, local bases as ONE
    device slab [S, n, N_max] (ragged bases: zero columns behind the ``local_sizes()[s]`` vectors of a subdomain).

        LRBMSReductor3D(d, bases=None, products=None, order=None)
            bases      ready-made local bases: a slab [S or S_ext, n, N] / list of [n, N_s] arrays (reductor.py:22-27), or None
            products   {'domain_i': ...} of the reference is the local energy product of every subdomain (reductor.py:19,
                       online_adaptive_lrbms.py:107); here it is ``d.engine.ops['P_diag']`` (lrbms3_assemble_energy_product) and
                       the argument only switches it: None / anything = the energy product, 'euclidean' = plain dot products
            order      0 / 1: start every local basis with the shape functions of that order (reductor.py:29-31); with neither
                       ``bases`` nor ``order`` given: order 0, the reference's default (reductor.py:23-24) -- every local basis then
                       starts with the constant, which the coarse level of the reduced solver's preconditioner builds on.
                       Order 1 deviates from the reference (block_swipdg.py:195: uncentred x0, x1, x0*x1, a 2D list whose
                       projection call is undefined at HEAD): here the constant plus the three coordinates relative to the
                       subdomain centre, the 3D counterpart of "all polynomials of degree <= 1"
        extend_basis(U)            restrict a block DG function [S, n(, L)] to every subdomain, Gram-Schmidt it into the bases
        extend_basis_local(ii, U)  the same for ONE subdomain (reductor.py:31,78)
        reduce()                   one pass of the hot path (reductor.py:33-73)
        reconstruct(u), reconstruct_local(u, ii)

        enrich_local(ii, U, mu), enrich_local_batch(subdomains, U, mu)
                                   corrector solve(s) on the neighbourhood(s), then extend the basis / bases (reductor.py:75-78);
                                   need ``discretize(..., online_enrichment=True)``

    Gram-Schmidt runs on the device: the product is applied by ``lrbms3_energy_product_apply``, the rest are batched products."""

    def __init__(self, d, bases=None, products=None, order=None):
        import torch
        self.d, self._torch = d, torch
        eng = d.engine
        self.euclidean = products == 'euclidean'
        if order is None and bases is None:
            order = 0                                                    # reductor.py:23-24
        if bases is not None:
            if isinstance(bases, (list, tuple)):
                blocks = [b if isinstance(b, torch.Tensor) else eng.ctx.from_numpy(np.asarray(b)) for b in bases]
                nmax = max(int(b.shape[1]) for b in blocks)
                self._nloc = np.array([int(b.shape[1]) for b in blocks], dtype=np.int64)
                V = torch.stack([torch.nn.functional.pad(b, (0, nmax - int(b.shape[1]))) for b in blocks])
            else:
                V = bases if isinstance(bases, torch.Tensor) else eng.ctx.from_numpy(np.asarray(bases))
                self._nloc = np.full(V.shape[0], int(V.shape[2]), dtype=np.int64)
            assert V.shape[0] in (eng.S, eng.S_ext) and V.shape[1] == eng.t.n
            self._V = V.contiguous()
        if order is not None:
            if self._V is not None and self._V.shape[0] != eng.S:
                raise NotImplementedError('order= with ready-made bases that already carry their halo')
            sf = d.shape_functions(0, order)                            # the same template for every subdomain
            self._gram_schmidt_extend(sf[None].expand(eng.S, -1, -1).contiguous())

    # ------------------------------------------------------------------ bases
    @property
    def bases(self):
        """The basis slab [S (or S_ext), n, N_max] (device); columns >= local_sizes()[s] of subdomain s are zero."""
        return self._V

    def _product_apply(self, X):
        eng = self.d.engine
        if self.euclidean:
            return X
        return eng.ctx.energy_product_apply(eng.ops['P_diag'], X.contiguous())

    def _pod_product(self):
        if self.euclidean:
            raise NotImplementedError("extend_basis(method='pod') works in the local energy product (products='euclidean' was asked for)")
        return self.d.engine.ops['P_diag']

    def _pod_max_width(self):
        return max(min(self.POD_MAX_WIDTH, 64 // self.d.Q), self.basis_size())      # the limit of the pass, as reserve()

    def _pod_mark_dirty(self, idx):
        self._dirty = getattr(self, '_dirty', set()) | {int(i) for i in idx}

    def gram(self):
        """V^T P V per subdomain [S, N_max, N_max]: the identity on the filled columns after Gram-Schmidt (what the 2D pass returns
        as E_red)."""
        V = self._V[:self.d.engine.S].contiguous()
        return self._torch.einsum('snk,snl->skl', V, self._product_apply(V))

    def _append_columns(self, v, ok):
        if self._V is not None and self._V.shape[0] != self.d.engine.S:
            raise NotImplementedError('extending bases that carry their halo: extend the local slab and exchange afterwards')
        ok_host = super()._append_columns(v, ok)
        # _dirty: local indices of the subdomains whose basis changed since the last reduce()
        self._dirty = getattr(self, '_dirty', set()) | {int(i) for i in np.where(ok_host)[0]}
        return ok_host

    def reserve(self, width):
        """Room for local bases of up to ``width`` vectors: pads the slab with zero columns, to an even width (the wide-load form
        of the pass takes even N) and at most 64 // Q, the limit of the pass.  Zero columns are the ragged-basis convention of this
        path and change no result (``local_sizes()`` keeps counting real vectors); later extensions then fill existing columns,
        the slab keeps its width and ``reduce(touched=...)`` can update the previous model in place."""
        width = min(int(width) + (int(width) & 1), 64 // self.d.Q)
        if self._V is not None and width > self._V.shape[2]:
            self._V = self._torch.nn.functional.pad(self._V, (0, width - self._V.shape[2])).contiguous()
        return self.basis_size()

    def _as_slab(self, U):
        eng = self.d.engine
        U = U if isinstance(U, self._torch.Tensor) else eng.ctx.from_numpy(np.asarray(U))
        if U.dim() == 2:
            U = U[:, :, None]
        assert tuple(U.shape[:2]) == (eng.S, eng.t.n), 'a block DG function [S, n] or [S, n, L]'
        return U.contiguous()

    def extend_basis_local(self, subdomain, U):
        """Extend the basis of ONE subdomain by the vector(s) ``U`` [n] / [n, L] (reductor.py:31,78)."""
        eng = self.d.engine
        i = eng.local.index(int(subdomain))
        U = U if isinstance(U, self._torch.Tensor) else eng.ctx.from_numpy(np.asarray(U))
        U = U[:, None] if U.dim() == 1 else U
        mask = self._torch.zeros(eng.S, dtype=self._torch.bool, device=U.device)
        mask[i] = True
        for k in range(U.shape[1]):
            full = eng.ctx.zeros(eng.S, eng.t.n, 1)
            full[i, :, 0] = U[:, k]
            v, ok = self._orthonormalize(full)
            if not bool(ok[i]):
                raise ExtensionError('local vector is (numerically) in the span of the local basis')
            self._append_columns(v, ok & mask)

    def enrich_local(self, subdomain, U, mu=None):
        """Reference reductor.py:75-78: corrector solve on the neighbourhood of ``subdomain`` at ``mu``, then extend its basis;
        ``ExtensionError3D`` if the corrector is (numerically) in the span of the basis.  ``U`` feeds only the commented-out
        Dirichlet lift (reductor.py:76)."""
        self.extend_basis_local(subdomain, self.d.solve_for_local_correction(subdomain, None, mu))

    def enrich_local_batch(self, subdomains, U, mu=None):
        """The loop of online_enrichment.py:49-50 as ONE batched corrector solve and one masked Gram-Schmidt step.  Returns the
        subdomains whose basis grew (a corrector already in the span of its basis is skipped)."""
        subdomains = [int(ii) for ii in subdomains]
        if not subdomains:
            if not self.d.online_enrichment:
                raise NotImplementedError(_NEEDS_KEYWORD)
            return []
        corr = self.d.solve_for_local_corrections(subdomains, mu)
        ok = self._extend_marked([self.d.engine.local.index(ii) for ii in subdomains], corr[:, :, None])
        return [ii for ii, flag in zip(subdomains, ok) if flag]

    # ------------------------------------------------------------------ reduce / reconstruct
    def reduce(self, touched=None):
        """``reductor.reduce()`` (reductor.py:33-73): one pass of the hot path.  ``touched``: global ids of the subdomains whose local
        bases changed since the previous ``reduce()`` (the marking of online_enrichment.py:38-47): only their own arrays and the
        side arrays of them and of their face neighbours are projected again (``lrbms3_pass_set_subset``), into the
        arrays of the previous reduced model, which the returned model shares (the previous one is superseded, as in the
        reference's loop, online_enrichment.py:52).  The whole pass runs when ``touched`` is None, when there is no previous model
        of the same width, and on a sharded grid.  ``last_reduce_info``: {'incremental', 'own', 'side'}."""
        eng = self.d.engine
        if self._V is None or self._V.shape[2] == 0:
            raise RuntimeError('no basis')
        V = self._V
        if V.shape[0] != eng.S_ext:
            raise NotImplementedError('sharded discretization: hand in bases [S_ext, n, N] with the halo filled (HaloExchange)')
        V = V.contiguous()
        N = int(V.shape[2])
        dirty = getattr(self, '_dirty', set())
        self._dirty = set()
        last = getattr(self, '_last_reduce', None)
        subset = None
        if touched is not None and last is not None and last['N'] == N and eng.S_ext == eng.S:
            from pylrbms_amd.grid3d import side_targets
            subset = sorted({eng.ext_pos[int(g)] for g in touched} | dirty)
            self.last_reduce_info = {'incremental': True, 'own': len(subset), 'side': len(side_targets(eng.nbr, subset))}
        else:
            last = self._last_reduce = {'N': N, 'out': eng.alloc_outputs(N), 'work': eng.alloc_work(N), 'src': None}
            self.last_reduce_info = {'incremental': False, 'own': eng.S, 'side': eng.S}
        return ReducedDiscretization3D(self, *self._project(V, last, subset))

    def _project(self, V, buf, subset=None):
        """(out, rhs_red_K, r_fd_K) of one pass into the kept buffers ``buf`` (restricted to ``subset`` if given); with an affine
        source also ``lrbms3_project_sources`` on the pass's flux image, and the model's view of the outputs drops the projections
        of sum_j f_j (``rhs_red``, ``r_fd``): nothing may use them on such a model."""
        eng, src = self.d.engine, self.d._src
        out = dict(eng.project_and_estimate(V, buf['out'], buf['work'], subset=subset))
        if src is None:
            return out, None, None
        buf['src'] = eng.project_sources(src['b_K'], src['bdiv_K'], V, buf['work'], out=buf['src'], subset=subset)
        out['rhs_red'] = out['r_fd'] = None
        return out, buf['src'][0], buf['src'][1]

    def reconstruct(self, u):
        return self._torch.einsum('snj,sj->sn', self._V, u)

    def reconstruct_local(self, u, subdomain):
        """The block of ``reconstruct(u)`` on ONE subdomain [n] (reductor.py:76)."""
        i = self.d.engine.ext.index(int(subdomain))
        return self._V[i] @ u[i]


def discretize(grid_and_problem_data, device_index=0, online_enrichment=False):
    """``online_enrichment=True`` also assembles the corrector data (``D_corr``: as large as the coupling blocks, 157 MB at config 5)
    that ``solve_for_local_correction(s)``, ``enrich_local`` and ``enrich_local_batch`` need; without it they raise
    ``NotImplementedError``.  Not available on a sharded grid."""
    d = BlockDiscretization3D(grid_and_problem_data, device_index=device_index, online_enrichment=online_enrichment)
    eng = d.engine
    data = {'grid': d.grid, 'engine': eng, 'operators': eng.ops}
    return d, data
