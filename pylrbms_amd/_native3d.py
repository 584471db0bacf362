"""ctypes binding of the 3D / P2 entry points of liblrbms_hip.so (C ABI: include/lrbms3d_hip.h).  No CPU fallback."""
import ctypes

import numpy as np

from pylrbms_amd import _native
from pylrbms_amd._native import NativeError, c_dbl, c_i32, c_i64, c_vp, _P_DBL, _P_I32

_INT_FIELDS = ('n_T', 'n_rt', 'ncf', 'nvs', 'n_nodes', 'nb', 'nbel', 'nsel', 'nbd', 'nA', 'nB', 'nC', 'nFs', 'nFf', 'o_fs', 'o_ff', 'o_c',
               'lam_stride', 'hat_stride', 'f_stride')
_I32_TABLES = ('elem_type', 'up_face', 'order', 'nb_elem', 'nb_out', 'face_pos', 'tsign', 'elem_rt', 'rt_e0', 'rt_f0', 'rt_e1', 'rt_f1', 'side_elem',
               'side_face', 'side_elem_out', 'side_face_out', 'dof_node', 'node_ptr', 'node_dofs', 'node_mask', 'node_count',
               'side_nodes', 'sn_ptr', 'sn_dofs', 'dof_bslot', 'bn_ptr', 'bn_slots', 'bnodes', 'bnode_sides', 'bel_elem', 'bel_bnode', 'sel_elem', 'sel_sf')
_DBL_TABLES = ('divc', 'TV', 'TE', 'TAA', 'TFo', 'TFn', 'TFb', 'TPo', 'TPn', 'TPb', 'TC', 'TCb', 'TPH', 'TM', 'TB', 'TAB', 'WB', 'WC')


class MeshDesc3D(ctypes.Structure):
    _fields_ = ([(k, c_i32) for k in _INT_FIELDS] + [('volume', c_dbl), ('kmin', c_dbl)] +
                [(k, _P_I32) for k in _I32_TABLES] + [(k, _P_DBL) for k in _DBL_TABLES])


SIGNATURES3 = {
    'lrbms3_ctx_create': (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(c_vp)]),
    'lrbms3_ctx_destroy': (ctypes.c_int, [c_vp]),
    'lrbms3_last_error': (ctypes.c_char_p, [c_vp]),
    'lrbms3_ctx_set_option': (ctypes.c_int, [c_vp, c_i32, c_i32]),
    'lrbms3_mesh_upload': (ctypes.c_int, [c_vp, ctypes.POINTER(MeshDesc3D), c_i32, c_i32, _P_I32, _P_I32]),
    'lrbms3_assemble_system': (ctypes.c_int, [c_vp, c_i32, c_vp, c_vp, c_vp, c_vp]),
    'lrbms3_assemble_rhs': (ctypes.c_int, [c_vp] + [c_vp] * 7),
    'lrbms3_assemble_products': (ctypes.c_int, [c_vp, c_i32] + [c_vp] * 8),
    'lrbms3_assemble_flux': (ctypes.c_int, [c_vp, c_i32, c_vp, c_vp, c_vp]),
    'lrbms3_assemble_energy_product': (ctypes.c_int, [c_vp, c_i32, _P_DBL, c_vp, c_vp, c_vp]),
    'lrbms3_energy_product_apply': (ctypes.c_int, [c_vp, c_i32, c_vp, c_vp, c_vp, c_vp]),
    'lrbms3_work_size': (c_i64, [c_vp, c_i32, c_i32]),
    'lrbms3_project_estimate': (ctypes.c_int, [c_vp, c_i32, c_i32] + [c_vp] * 26),
    'lrbms3_project_estimate_phase': (ctypes.c_int, [c_vp, c_i32, c_i32, c_i32] + [c_vp] * 26),
    'lrbms3_pass_set_subset': (ctypes.c_int, [c_vp, _P_I32, c_i32]),
    'lrbms3_kernel_timing': (ctypes.c_int, [c_vp, c_i32]),
    'lrbms3_kernel_timing_read': (ctypes.c_int, [c_vp, ctypes.c_char_p, c_i64, _P_DBL, c_i32, _P_I32]),
    'lrbms3_reduced_estimate': (ctypes.c_int, [c_vp, c_i32, c_i32, _P_DBL] + [c_vp] * 18 + [c_dbl, c_vp, c_vp]),
    'lrbms3_reduced_estimate_batch': (ctypes.c_int, [c_vp, c_i32, c_i32, c_i32, _P_DBL] + [c_vp] * 18 + [c_dbl, c_vp, c_vp]),
    'lrbms3_reduced_solve_work_size': (c_i64, [c_vp, c_i32]),
    'lrbms3_reduced_solve': (ctypes.c_int, [c_vp, c_i32, c_i32, _P_DBL, c_vp, c_vp, c_vp, c_vp, c_dbl, c_i32, _P_DBL, c_vp]),
    'lrbms3_reduced_solve_batch_work_size': (c_i64, [c_vp, c_i32, c_i32]),
    'lrbms3_reduced_solve_batch': (ctypes.c_int, [c_vp, c_i32, c_i32, c_i32, _P_DBL, c_vp, c_vp, c_vp, c_vp, c_dbl, c_i32, _P_DBL, c_vp]),
    'lrbms3_fom_coarse_space': (ctypes.c_int, [c_vp, c_i32, _P_DBL]),
    'lrbms3_fom_precond_keep': (ctypes.c_int, [c_vp, c_i32]),
    'lrbms3_reduced_precond_size': (c_i64, [c_vp, c_i32]),
    'lrbms3_reduced_precond_work_size': (c_i64, [c_vp, c_i32]),
    'lrbms3_reduced_precond_build': (ctypes.c_int, [c_vp, c_i32, c_i32, _P_DBL, c_vp, c_vp, c_vp, c_vp]),
    'lrbms3_reduced_precond_use': (ctypes.c_int, [c_vp, c_i32, c_vp]),
    'lrbms3_fom_solve_work_size': (c_i64, [c_vp]),
    'lrbms3_fom_solve': (ctypes.c_int, [c_vp, c_i32, _P_DBL, c_vp, c_vp, c_vp, c_vp, c_vp, c_dbl, c_i32, _P_DBL, c_vp]),
    # batched snapshots
    'lrbms3_fom_solve_batch_work_size': (c_i64, [c_vp, c_i32]),
    'lrbms3_fom_solve_batch': (ctypes.c_int, [c_vp, c_i32, c_i32, _P_DBL, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_dbl, c_i32,
                                              _P_DBL, c_vp]),
    'lrbms3_fom_solve_batch_panel_info': (ctypes.c_int, [c_vp, _P_DBL]),
    'lrbms3_fom_apply': (ctypes.c_int, [c_vp, c_i32, c_i32, _P_DBL, c_vp, c_vp, c_vp, c_vp, c_vp]),
    'lrbms3_mass_inverse_norm2': (ctypes.c_int, [c_vp, c_i32, c_vp, c_vp, c_vp]),
    'lrbms3_project_mass': (ctypes.c_int, [c_vp, c_i32, c_vp, c_vp, c_vp]),
    'lrbms3_fom_implicit_euler_work_size': (c_i64, [c_vp]),
    'lrbms3_fom_implicit_euler': (ctypes.c_int, [c_vp, c_i32, _P_DBL, c_dbl, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_dbl, c_i32,
                                                 _P_DBL, c_vp]),
    # batched full-order trajectories
    'lrbms3_fom_implicit_euler_batch_work_size': (c_i64, [c_vp, c_i32]),
    'lrbms3_fom_implicit_euler_batch': (ctypes.c_int, [c_vp, c_i32, c_i32, c_i32, _P_DBL, c_dbl, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                                       c_dbl, c_i32, _P_DBL, c_vp]),
    'lrbms3_fom_implicit_euler_batch_panel_info': (ctypes.c_int, [c_vp, _P_DBL]),
    'lrbms3_reduced_implicit_euler_work_size': (c_i64, [c_vp, c_i32]),
    'lrbms3_reduced_implicit_euler': (ctypes.c_int, [c_vp, c_i32, c_i32, _P_DBL, c_dbl, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_dbl,
                                                     c_i32, _P_DBL, c_vp]),
    'lrbms3_reduced_time_residual_work_size': (c_i64, [c_vp, c_i32]),
    'lrbms3_reduced_time_residual': (ctypes.c_int, [c_vp, c_i32, c_i32, c_i32, _P_DBL, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    # affine sources
    'lrbms3_assemble_source_gram': (ctypes.c_int, [c_vp, c_i32, c_vp, c_vp, c_vp]),
    'lrbms3_project_sources': (ctypes.c_int, [c_vp, c_i32, c_i32, c_i32] + [c_vp] * 7),
    'lrbms3_reduced_source_terms': (ctypes.c_int, [c_vp, c_i32, c_i32, c_i32, c_i32] + [c_vp] * 8 + [c_dbl, c_vp, c_vp]),
    'lrbms3_reduced_solve_batch_src': (ctypes.c_int, [c_vp, c_i32, c_i32, c_i32, c_i32, _P_DBL, _P_DBL, c_vp, c_vp, c_vp, c_vp, c_dbl, c_i32,
                                                      _P_DBL, c_vp]),
    'lrbms3_combine_sources': (ctypes.c_int, [c_vp, c_i32, c_i64, _P_DBL, c_vp, c_vp, c_vp]),
    'lrbms3_fom_implicit_euler_src': (ctypes.c_int, [c_vp, c_i32, c_i32, _P_DBL, c_dbl, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_dbl,
                                                     c_i32, _P_DBL, c_vp]),
    'lrbms3_reduced_implicit_euler_src': (ctypes.c_int, [c_vp, c_i32, c_i32, c_i32, _P_DBL, c_dbl, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp,
                                                         c_vp, c_dbl, c_i32, _P_DBL, c_vp]),
    # batched reduced trajectories
    'lrbms3_reduced_implicit_euler_batch_work_size': (c_i64, [c_vp, c_i32, c_i32]),
    'lrbms3_reduced_implicit_euler_batch': (ctypes.c_int, [c_vp, c_i32, c_i32, c_i32, _P_DBL, c_dbl, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp,
                                                           c_dbl, c_i32, _P_DBL, c_vp]),
    'lrbms3_reduced_implicit_euler_batch_src': (ctypes.c_int, [c_vp, c_i32, c_i32, c_i32, c_i32, _P_DBL, c_dbl, c_i32, c_vp, c_vp, c_vp,
                                                               c_vp, c_vp, c_vp, c_dbl, c_i32, _P_DBL, c_vp]),
    # batched parabolic estimates
    'lrbms3_reduced_parabolic_estimate_batch_work_size': (c_i64, [c_vp, c_i32, c_i32, c_i32]),
    'lrbms3_reduced_parabolic_estimate_batch': (ctypes.c_int, [c_vp] + [c_i32] * 5 + [c_dbl, _P_DBL, _P_DBL] + [c_vp] * 20 + [c_dbl] +
                                                [c_vp] * 11),
    # time-dependent diffusion coefficients on the three batched parabolic exports
    'lrbms3_fom_implicit_euler_batch_tv': (ctypes.c_int, [c_vp, c_i32, c_i32, c_i32, _P_DBL, c_dbl, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                                          c_dbl, c_i32, _P_DBL, c_vp]),
    'lrbms3_reduced_implicit_euler_batch_tv': (ctypes.c_int, [c_vp, c_i32, c_i32, c_i32, c_i32, _P_DBL, c_dbl, c_i32, c_vp, c_vp, c_vp,
                                                              c_vp, c_vp, c_vp, c_dbl, c_i32, _P_DBL, c_vp]),
    'lrbms3_reduced_parabolic_estimate_batch_tv_work_size': (c_i64, [c_vp, c_i32, c_i32, c_i32]),
    'lrbms3_reduced_parabolic_estimate_batch_tv': (ctypes.c_int, [c_vp] + [c_i32] * 5 + [c_dbl, _P_DBL, _P_DBL] + [c_vp] * 20 + [c_dbl] +
                                                   [c_vp] * 11),
    # online enrichment
    'lrbms3_assemble_dirichlet_correction': (ctypes.c_int, [c_vp, c_i32, c_vp, c_vp, c_vp]),
    'lrbms3_local_correction_work_size': (c_i64, [c_vp, c_i32]),
    'lrbms3_local_correction_solve': (ctypes.c_int, [c_vp, c_i32, _P_DBL, c_i32, _P_I32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_dbl, c_i32,
                                                     _P_DBL, c_vp]),
    # corrector trajectories
    'lrbms3_local_correction_euler_work_size': (c_i64, [c_vp, c_i32, c_i32]),
    'lrbms3_local_correction_euler': (ctypes.c_int, [c_vp, c_i32, c_i32, _P_DBL, c_dbl, c_i32, c_i32, _P_I32, c_vp, c_vp, c_vp, c_vp, c_vp,
                                                     c_vp, c_vp, c_dbl, c_i32, _P_DBL, c_vp]),
    # local POD basis extension
    'lrbms3_local_pod_work_size': (c_i64, [c_vp, c_i32, c_i32]),
    'lrbms3_local_pod': (ctypes.c_int, [c_vp, c_i32, c_i32, c_i32, c_dbl, c_dbl] + [c_vp] * 9),
    'lrbms3_local_pod_stream_state_size': (c_i64, [c_vp, c_i32, c_i32]),
    'lrbms3_local_pod_stream_work_size': (c_i64, [c_vp, c_i32, c_i32, c_i32]),
    'lrbms3_local_pod_stream_begin': (ctypes.c_int, [c_vp, c_i32, c_i32, c_vp, c_vp]),
    'lrbms3_local_pod_stream_push': (ctypes.c_int, [c_vp, c_i32, c_i32, c_i32, c_i32] + [c_vp] * 7),
    'lrbms3_local_pod_stream_finish': (ctypes.c_int, [c_vp, c_i32, c_i32, c_i32, c_i32, c_dbl, c_dbl] + [c_vp] * 10),
}

_bound = None


def load_library(path=None):
    global _bound
    if _bound is not None and path is None:
        return _bound
    lib = _native.load_library(path)
    for name, (restype, argtypes) in SIGNATURES3.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    _bound = lib
    return lib


class Native3DContext(_native.ContextBase):
    """One lrbms3_ctx per (process, device); tensors are contiguous float64 CUDA tensors, shapes checked on the host."""

    PREFIX = 'lrbms3_'
    TIMING_CAP = 4096
    _load = staticmethod(load_library)
    OPTIONS = {'ksplit': 1, 'serial': 2, 'waves': 3, 'estimate_valu': 4, 'solve_valu': 5, 'fom_coarse': 6, 'pod_rotate_valu': 7}

    # ------------------------------------------------------------------ mesh
    def mesh_upload(self, template, spec, tables, nbr, phys, S, S_ext):
        t = template
        self.t, self.spec, self.S, self.S_ext = t, spec, int(S), int(S_ext)
        d = MeshDesc3D()
        vals = dict(n_T=t.n_T, n_rt=t.n_rt, ncf=t.ncf, nvs=t.nvs, n_nodes=t.n_nodes, nb=t.nb, nbel=len(t.bel_elem),
                    nsel=len(t.sel_elem), nbd=t.nbd, nA=spec.nA, nB=spec.nB, nC=spec.nC, nFs=spec.nFs, nFf=spec.nFf, o_fs=spec.o_fs,
                    o_ff=spec.o_ff, o_c=spec.o_c, lam_stride=spec.lam_stride, hat_stride=spec.hat_stride, f_stride=spec.f_stride)
        for k, v in vals.items():
            setattr(d, k, int(v))
        d.volume = float(t.volume)
        d.kmin = float(np.linalg.eigvalsh(0.5 * (t.kappa + t.kappa.T)).min())
        keep = {}
        for k in _I32_TABLES:
            keep[k] = np.ascontiguousarray(getattr(t, k), dtype=np.int32).reshape(-1)
            if keep[k].size == 0:
                keep[k] = np.zeros(1, dtype=np.int32)
            setattr(d, k, keep[k].ctypes.data_as(_P_I32))
        for k in _DBL_TABLES:
            src = t.divc if k == 'divc' else tables[k]
            keep[k] = np.ascontiguousarray(src, dtype=np.float64).reshape(-1)
            setattr(d, k, keep[k].ctypes.data_as(_P_DBL))
        nb = np.ascontiguousarray(nbr, dtype=np.int32)
        ph = np.ascontiguousarray(phys, dtype=np.int32)
        assert nb.shape == (S, 7) and ph.shape == (S_ext,)
        rc = self.lib.lrbms3_mesh_upload(self.handle, ctypes.byref(d), S, S_ext, nb.ctypes.data_as(_P_I32), ph.ctypes.data_as(_P_I32))
        self._check(rc, 'lrbms3_mesh_upload')
        self.n_T, self.n, self.n_rt, self.ncf, self.nbf, self.nvs, self.nb, self.n_nodes = (t.n_T, t.n, t.n_rt, t.ncf, t.nbf, t.nvs,
                                                                                              t.nb, t.n_nodes)
        # coarse space of the full-order solver's preconditioner: P1 per subdomain in the local coordinates, centred and scaled
        x = np.asarray(t.node_coordinates(), dtype=np.float64)
        ext = x.max(axis=0) - x.min(axis=0)
        self.fom_coarse_space(np.concatenate([np.ones((t.n, 1)), (x - 0.5 * (x.max(axis=0) + x.min(axis=0))) / ext], axis=1))

    def fom_precond_keep(self, keep=True):
        """The next ``fom_solve`` leaves its coarse inverse in the context, the following ones reuse it for every parameter
        (``False``: drop it, one factorisation per solve again)."""
        self._check(self.lib.lrbms3_fom_precond_keep(self.handle, 1 if keep else 0), 'lrbms3_fom_precond_keep')

    def fom_coarse_space(self, Phi):
        """Phi [n, nc] (nc <= 4) values of the coarse functions of ``fom_solve``'s two-level preconditioner at the local DoFs,
        the same for every subdomain; ``None`` switches the coarse level off."""
        if Phi is None:
            self._check(self.lib.lrbms3_fom_coarse_space(self.handle, 0, None), 'lrbms3_fom_coarse_space')
            return
        Phi = np.ascontiguousarray(Phi, dtype=np.float64)
        assert Phi.ndim == 2 and Phi.shape[0] == self.t.n and 1 <= Phi.shape[1] <= 4
        self._check(self.lib.lrbms3_fom_coarse_space(self.handle, int(Phi.shape[1]), Phi.ctypes.data_as(_P_DBL)), 'lrbms3_fom_coarse_space')

    # ------------------------------------------------------------------ assembly
    def assemble_system(self, lam):
        Q, sp = lam.shape[0], self.spec
        A_diag, A_cpl = self.empty(Q, self.S, self.n_T, 5, 100), self.empty(Q, self.S, 6, self.ncf, 100)
        rc = self.lib.lrbms3_assemble_system(self.handle, Q, self._ptr(lam, (Q, self.S_ext, self.n_T, sp.lam_stride), 'lam'),
                                             c_vp(A_diag.data_ptr()), c_vp(A_cpl.data_ptr()), self._stream())
        self._check(rc, 'lrbms3_assemble_system')
        return A_diag, A_cpl

    def assemble_rhs(self, f_smp, lhat):
        sp = self.spec
        b, f2, ceps, bdiv = self.empty(self.S, self.n), self.empty(self.S), self.empty(self.S), self.empty(self.S, self.n_T)
        rc = self.lib.lrbms3_assemble_rhs(self.handle, self._ptr(f_smp, (self.S, self.n_T, sp.f_stride), 'f_smp'),
                                          self._ptr(lhat, (self.S, self.n_T, sp.hat_stride), 'lhat'), c_vp(b.data_ptr()),
                                          c_vp(f2.data_ptr()), c_vp(ceps.data_ptr()), c_vp(bdiv.data_ptr()), self._stream())
        self._check(rc, 'lrbms3_assemble_rhs')
        return b, f2, ceps, bdiv

    def assemble_products(self, lam, lbar, lhat):
        Q, sp = lam.shape[0], self.spec
        ebar, Aaa = self.empty(self.S, self.n_T, 100), self.empty(Q, Q, self.S, self.n_T, 100)
        Aab, Bbb = self.empty(Q, self.S, self.n_T, 40), self.empty(self.S, self.n_T, 16)
        rc = self.lib.lrbms3_assemble_products(self.handle, Q, self._ptr(lam, (Q, self.S_ext, self.n_T, sp.lam_stride), 'lam'),
                                               self._ptr(lbar, (self.S, self.n_T, sp.nB), 'lbar'),
                                               self._ptr(lhat, (self.S, self.n_T, sp.hat_stride), 'lhat'), c_vp(ebar.data_ptr()),
                                               c_vp(Aaa.data_ptr()), c_vp(Aab.data_ptr()), c_vp(Bbb.data_ptr()), self._stream())
        self._check(rc, 'lrbms3_assemble_products')
        return ebar, Aaa, Aab, Bbb

    def assemble_flux(self, lam):
        Q, sp = lam.shape[0], self.spec
        Cf = self.empty(Q, self.S_ext, self.n_T, 4, 10)
        rc = self.lib.lrbms3_assemble_flux(self.handle, Q, self._ptr(lam, (Q, self.S_ext, self.n_T, sp.lam_stride), 'lam'),
                                           c_vp(Cf.data_ptr()), self._stream())
        self._check(rc, 'lrbms3_assemble_flux')
        return Cf

    def assemble_energy_product(self, theta_bar, lam):
        """P_diag [S, n_T, 5, 100]: the local energy product at mu_bar (block-ELL, local to every subdomain)."""
        Q, sp = lam.shape[0], self.spec
        th = np.ascontiguousarray(theta_bar, dtype=np.float64)
        assert th.shape == (Q,)
        P = self.empty(self.S, self.n_T, 5, 100)
        rc = self.lib.lrbms3_assemble_energy_product(self.handle, Q, th.ctypes.data_as(_P_DBL),
                                                     self._ptr(lam, (Q, self.S_ext, self.n_T, sp.lam_stride), 'lam'),
                                                     c_vp(P.data_ptr()), self._stream())
        self._check(rc, 'lrbms3_assemble_energy_product')
        return P

    def energy_product_apply(self, P_diag, X):
        """P X for X [S, n, M] (M vectors per subdomain)."""
        M = X.shape[2]
        Y = self.empty(self.S, self.n, M)
        rc = self.lib.lrbms3_energy_product_apply(self.handle, M, self._ptr(P_diag, (self.S, self.n_T, 5, 100), 'P_diag'),
                                                  self._ptr(X, (self.S, self.n, M), 'X'), c_vp(Y.data_ptr()), self._stream())
        self._check(rc, 'lrbms3_energy_product_apply')
        return Y

    def local_pod(self, P_diag, U, V, nloc, modes, rtol=1e-6, atol=0.0, work=None):
        """``lrbms3_local_pod``: at most ``modes`` POD modes of the snapshots ``U`` [S, n, L] per subdomain, in the local energy
        product ``P_diag``, into the free columns of ``V``; arguments and result as ``ContextBase._local_pod``."""
        return self._local_pod(self._ptr(P_diag, (self.S, self.n_T, 5, 100), 'P_diag'), U, V, nloc, modes, rtol, atol, work)

    def _pod_product_ptr(self, P_diag):
        return self._ptr(P_diag, (self.S, self.n_T, 5, 100), 'P_diag')

    # ------------------------------------------------------------------ pass
    OUT_NAMES = ('B_sys', 'rhs_red', 'G_nc', 'G_bb', 'G_rdd', 'G_ab', 'G_aa', 'r_fd', 'Rb', 'Yb', 'Dp', 'Xab', 'As', 'Cn')

    def out_shapes(self, Q, N):
        S, QN = self.S, Q * N
        return dict(B_sys=(Q, S, 7, N, N), rhs_red=(S, N), G_nc=(S, N, N), G_bb=(S, QN, QN), G_rdd=(S, QN, QN), G_ab=(Q, S, N, QN),
                    G_aa=(Q, Q, S, N, N), r_fd=(S, QN), Rb=(S, self.nbf, QN), Yb=(S, self.nbf, QN), Dp=(S, self.nbf, QN),
                    Xab=(Q, S, self.nbf, N), As=(S, 6, self.nvs, N), Cn=(S, self.nb, N))

    def work_size(self, Q, N):
        return int(self.lib.lrbms3_work_size(self.handle, Q, N))

    def project_estimate(self, Q, V, ops, work, out, phase=0):
        N = V.shape[2]
        S, nT = self.S, self.n_T
        shp = self.out_shapes(Q, N)
        args = [self._ptr(V, (self.S_ext, self.n, N), 'V'), self._ptr(ops['A_diag'], (Q, S, nT, 5, 100), 'A_diag'),
                self._ptr(ops['A_cpl'], (Q, S, 6, self.ncf, 100), 'A_cpl'), self._ptr(ops['b'], (S, self.n), 'b'),
                self._ptr(ops['ebar'], (S, nT, 100), 'ebar'), self._ptr(ops['Aaa'], (Q, Q, S, nT, 100), 'Aaa'),
                self._ptr(ops['Aab'], (Q, S, nT, 40), 'Aab'), self._ptr(ops['Bbb'], (S, nT, 16), 'Bbb'),
                self._ptr(ops['bdiv'], (S, nT), 'bdiv'), self._ptr(ops['Cf'], (Q, self.S_ext, nT, 4, 10), 'Cf')]
        if work.numel() < self.work_size(Q, N):
            raise NativeError('work buffer too small')
        args.append(c_vp(work.data_ptr()))
        args += [self._ptr(out[k], shp[k], k) for k in self.OUT_NAMES]
        rc = self.lib.lrbms3_project_estimate_phase(self.handle, int(phase), Q, N, *args, self._stream())
        self._check(rc, 'lrbms3_project_estimate_phase')
        return out

    def pass_set_subset(self, changed):
        """Restrict the following ``project_estimate`` / ``project_sources`` calls to the subdomains ``changed`` (strictly ascending
        indices in the S_ext ordering) and the face neighbours their side arrays reach; ``None`` or empty: all -- incremental
        re-projection after online enrichment (include/lrbms3d_hip.h: lrbms3_pass_set_subset)."""
        if changed is None or len(changed) == 0:
            self._check(self.lib.lrbms3_pass_set_subset(self.handle, None, 0), 'lrbms3_pass_set_subset')
            return
        arr = np.ascontiguousarray(changed, dtype=np.int32).reshape(-1)
        self._check(self.lib.lrbms3_pass_set_subset(self.handle, arr.ctypes.data_as(_P_I32), int(arr.size)), 'lrbms3_pass_set_subset')

    # ------------------------------------------------------------------ online
    def reduced_estimate(self, Q, theta, u, out, ops, hdiam):
        N = u.shape[1]
        S = self.S
        shp = self.out_shapes(Q, N)
        th = np.ascontiguousarray(theta, dtype=np.float64)
        assert th.shape == (Q,)
        eta = self.empty(3, S)
        names = ('G_nc', 'G_bb', 'G_rdd', 'G_ab', 'G_aa', 'r_fd', 'Rb', 'Yb', 'Dp', 'Xab', 'As', 'Cn')
        args = [self._ptr(u, (self.S_ext, N), 'u')] + [self._ptr(out[k], shp[k], k) for k in names]
        args += [self._ptr(ops['ebar'], (S, self.n_T, 100), 'ebar'), self._ptr(ops['Bbb'], (S, self.n_T, 16), 'Bbb'),
                 self._ptr(ops['bdiv'], (S, self.n_T), 'bdiv'), self._ptr(ops['f2'], (S,), 'f2'), self._ptr(ops['ceps'], (S,), 'ceps')]
        rc = self.lib.lrbms3_reduced_estimate(self.handle, Q, N, th.ctypes.data_as(_P_DBL), *args, float(hdiam), c_vp(eta.data_ptr()),
                                              self._stream())
        self._check(rc, 'lrbms3_reduced_estimate')
        return eta

    def reduced_estimate_batch(self, Q, thetas, u, out, ops, hdiam):
        """thetas [nmu, Q], u [S_ext, N, nmu] (parameter fastest) -> eta_loc [3, S, nmu]."""
        N, nmu, S = u.shape[1], u.shape[2], self.S
        shp = self.out_shapes(Q, N)
        th = np.ascontiguousarray(thetas, dtype=np.float64)
        assert th.shape == (nmu, Q)
        eta = self.empty(3, S, nmu)
        names = ('G_nc', 'G_bb', 'G_rdd', 'G_ab', 'G_aa', 'r_fd', 'Rb', 'Yb', 'Dp', 'Xab', 'As', 'Cn')
        args = [self._ptr(u, (self.S_ext, N, nmu), 'u')] + [self._ptr(out[k], shp[k], k) for k in names]
        args += [self._ptr(ops['ebar'], (S, self.n_T, 100), 'ebar'), self._ptr(ops['Bbb'], (S, self.n_T, 16), 'Bbb'),
                 self._ptr(ops['bdiv'], (S, self.n_T), 'bdiv'), self._ptr(ops['f2'], (S,), 'f2'), self._ptr(ops['ceps'], (S,), 'ceps')]
        rc = self.lib.lrbms3_reduced_estimate_batch(self.handle, Q, N, nmu, th.ctypes.data_as(_P_DBL), *args, float(hdiam),
                                                    c_vp(eta.data_ptr()), self._stream())
        self._check(rc, 'lrbms3_reduced_estimate_batch')
        return eta

    def reduced_solve(self, Q, theta, B_sys, rhs_red, rtol=1e-13, max_iter=5000, work=None):
        N = rhs_red.shape[1]
        S = self.S
        th = np.ascontiguousarray(theta, dtype=np.float64)
        if work is None:
            work = self.empty(int(self.lib.lrbms3_reduced_solve_work_size(self.handle, N)))
        u = self.empty(S, N)
        info = (c_dbl * 2)()
        rc = self.lib.lrbms3_reduced_solve(self.handle, Q, N, th.ctypes.data_as(_P_DBL), self._ptr(B_sys, (Q, S, 7, N, N), 'B_sys'),
                                           self._ptr(rhs_red, (S, N), 'rhs_red'), c_vp(work.data_ptr()), c_vp(u.data_ptr()),
                                           float(rtol), int(max_iter), info, self._stream())
        self._check(rc, 'lrbms3_reduced_solve')
        return u, (int(info[0]), float(info[1]))

    def reduced_solve_batch(self, Q, thetas, B_sys, rhs_red, rtol=1e-13, max_iter=5000, work=None):
        """thetas [nmu, Q] (nmu <= 64: up to four groups of 16 on four streams) -> u [S, N, nmu] (parameter fastest),
        (iterations, worst relative residual)."""
        N, S = rhs_red.shape[1], self.S
        th = np.ascontiguousarray(thetas, dtype=np.float64)
        nmu = th.shape[0]
        assert th.shape == (nmu, Q)
        if work is None:
            work = self.empty(int(self.lib.lrbms3_reduced_solve_batch_work_size(self.handle, N, nmu)))
        u = self.empty(S, N, nmu)
        info = (c_dbl * 2)()
        rc = self.lib.lrbms3_reduced_solve_batch(self.handle, Q, N, nmu, th.ctypes.data_as(_P_DBL),
                                                 self._ptr(B_sys, (Q, S, 7, N, N), 'B_sys'), self._ptr(rhs_red, (S, N), 'rhs_red'),
                                                 c_vp(work.data_ptr()), c_vp(u.data_ptr()), float(rtol), int(max_iter), info,
                                                 self._stream())
        self._check(rc, 'lrbms3_reduced_solve_batch')
        return u, (int(info[0]), float(info[1]))

    def reduced_precond_build(self, Q, theta, B_sys):
        """Two-level preconditioner of the batched reduced solve at the reference parameter ``theta``: one device buffer,
        the coarse inverse [S, S] followed by the inverse diagonal blocks [S, N, N]."""
        N, S = B_sys.shape[-1], self.S
        th = np.ascontiguousarray(theta, dtype=np.float64)
        assert th.shape == (Q,)
        work = self.empty(int(self.lib.lrbms3_reduced_precond_work_size(self.handle, N)))
        pc = self.empty(int(self.lib.lrbms3_reduced_precond_size(self.handle, N)))        # [S, S] coarse inverse | [S, N, N] inverse blocks
        rc = self.lib.lrbms3_reduced_precond_build(self.handle, Q, N, th.ctypes.data_as(_P_DBL), self._ptr(B_sys, (Q, S, 7, N, N), 'B_sys'),
                                                   c_vp(work.data_ptr()), c_vp(pc.data_ptr()), self._stream())
        self._check(rc, 'lrbms3_reduced_precond_build')
        self.torch.cuda.current_stream().synchronize()          # `work` goes out of scope
        pc._lrbms_N = N
        return pc

    def reduced_precond_use(self, pc):
        """Subsequent ``reduced_solve_batch`` calls use ``pc`` (``None``: inverse diagonal blocks alone).  The context keeps a reference."""
        self._pc_keep = pc
        rc = self.lib.lrbms3_reduced_precond_use(self.handle, int(pc._lrbms_N) if pc is not None else 0,
                                                 c_vp(pc.data_ptr()) if pc is not None else None)
        self._check(rc, 'lrbms3_reduced_precond_use')

    def fom_solve(self, Q, theta, A_diag, A_cpl, b, rtol=1e-10, max_iter=50000, work=None):
        th = np.ascontiguousarray(theta, dtype=np.float64)
        if work is None:
            work = self.empty(int(self.lib.lrbms3_fom_solve_work_size(self.handle)))
        x = self.empty(self.S, self.n)
        info = (c_dbl * 2)()
        rc = self.lib.lrbms3_fom_solve(self.handle, Q, th.ctypes.data_as(_P_DBL),
                                       self._ptr(A_diag, (Q, self.S, self.n_T, 5, 100), 'A_diag'),
                                       self._ptr(A_cpl, (Q, self.S, 6, self.ncf, 100), 'A_cpl'), self._ptr(b, (self.S, self.n), 'b'),
                                       c_vp(work.data_ptr()), c_vp(x.data_ptr()), float(rtol), int(max_iter), info, self._stream())
        self._check(rc, 'lrbms3_fom_solve')
        return x, (int(info[0]), float(info[1]))

    def fom_solve_batch(self, thetas, A_diag, A_cpl, phi, b_K, rtol=1e-10, max_iter=50000, work=None):
        """Column m: A(thetas[m]) x_m = sum_j phi[m][j] b_K[j] for nmu <= 64 parameters in one call (``lrbms3_fom_solve_batch``:
        panels of 16 columns on the matrix cores, one two-level preconditioner at the mean theta) -> (X [S, n, nmu], info).
        thetas [nmu, Q] host; phi [nmu, K] host or device; b_K [K, S, n].  ``info``: ``iterations`` (largest panel count),
        ``relative_residual`` (worst final |r| / |b_m|), ``panel_iterations``."""
        Q, S = int(A_diag.shape[0]), self.S
        th = np.ascontiguousarray(thetas, dtype=np.float64)
        nmu = th.shape[0]
        assert th.shape == (nmu, Q)
        K = int(b_K.shape[0])
        ph = self._dev2(phi, (nmu, K), 'phi')
        size = int(self.lib.lrbms3_fom_solve_batch_work_size(self.handle, nmu))
        if size < 0:
            raise NativeError('lrbms3_fom_solve_batch: nmu = {} is not in 1..64'.format(nmu))
        if work is None:
            work = self.empty(size)
        elif work.numel() < size:
            raise NativeError('work buffer too small')
        X = self.empty(S, self.n, nmu)
        info = (c_dbl * 2)()
        rc = self.lib.lrbms3_fom_solve_batch(self.handle, Q, nmu, th.ctypes.data_as(_P_DBL),
                                             self._ptr(A_diag, (Q, S, self.n_T, 5, 100), 'A_diag'),
                                             self._ptr(A_cpl, (Q, S, 6, self.ncf, 100), 'A_cpl'), K, c_vp(ph.data_ptr()),
                                             self._ptr(b_K, (K, S, self.n), 'b_K'), c_vp(work.data_ptr()), c_vp(X.data_ptr()),
                                             float(rtol), int(max_iter), info, self._stream())
        panels = (c_dbl * 8)()
        self.lib.lrbms3_fom_solve_batch_panel_info(self.handle, panels)
        self._check(rc, 'lrbms3_fom_solve_batch')
        return X, {'iterations': int(info[0]), 'relative_residual': float(info[1]),
                   'panel_iterations': [int(v) for v in list(panels)[0:2 * ((nmu + 15) // 16):2]]}

    def fom_apply(self, Q, theta, A_diag, A_cpl, x):
        M = x.shape[2]
        th = np.ascontiguousarray(theta, dtype=np.float64)
        y = self.empty(self.S, self.n, M)
        rc = self.lib.lrbms3_fom_apply(self.handle, Q, M, th.ctypes.data_as(_P_DBL),
                                       self._ptr(A_diag, (Q, self.S, self.n_T, 5, 100), 'A_diag'),
                                       self._ptr(A_cpl, (Q, self.S, 6, self.ncf, 100), 'A_cpl'),
                                       self._ptr(x, (self.S_ext, self.n, M), 'x'), c_vp(y.data_ptr()), self._stream())
        self._check(rc, 'lrbms3_fom_apply')
        return y

    # ------------------------------------------------------------------ parabolic
    def mass_inverse_norm2(self, Y):
        """Y [S, n, L] -> [S, L]: y^T M_s^-1 y per subdomain and vector (block L2 product inverted element by element)."""
        if Y.dim() != 3:
            raise NativeError('Y: expected [S, n, L]')
        L = int(Y.shape[2])
        out = self.empty(self.S, L)
        rc = self.lib.lrbms3_mass_inverse_norm2(self.handle, L, self._ptr(Y, (self.S, self.n, L), 'Y'), c_vp(out.data_ptr()),
                                                self._stream())
        self._check(rc, 'lrbms3_mass_inverse_norm2')
        return out

    def project_mass(self, V):
        """V [S_ext, n, N] -> M_red [S, N, N] = V_s^T M_s V_s (N <= 64)."""
        if V.dim() != 3:
            raise NativeError('V: expected [S_ext, n, N]')
        N = int(V.shape[2])
        M_red = self.empty(self.S, N, N)
        rc = self.lib.lrbms3_project_mass(self.handle, N, self._ptr(V, (self.S_ext, self.n, N), 'V'), c_vp(M_red.data_ptr()),
                                          self._stream())
        self._check(rc, 'lrbms3_project_mass')
        return M_red

    def fom_implicit_euler(self, Q, theta, dt, nt, A_diag, A_cpl, b, U0=None, rtol=1e-10, max_iter=50000, work=None):
        """(M + dt A(mu)) u_{k+1} = M u_k + dt b for k < nt in one native call -> U [nt + 1, S, n] (U[0] = U0, default zero),
        (total CG iterations, worst final relative residual)."""
        th = np.ascontiguousarray(theta, dtype=np.float64)
        assert th.shape == (Q,)
        nt = int(nt)
        if work is None:
            size = int(self.lib.lrbms3_fom_implicit_euler_work_size(self.handle))
            if size < 0:
                raise NativeError('lrbms3_fom_implicit_euler_work_size: mesh not uploaded')
            work = self.empty(size)
        U = self.empty(max(nt, 0) + 1, self.S, self.n)
        if U0 is None:
            U[0].zero_()
        else:
            U[0].copy_(U0.reshape(self.S, self.n))
        info = (c_dbl * 2)()
        rc = self.lib.lrbms3_fom_implicit_euler(self.handle, Q, th.ctypes.data_as(_P_DBL), float(dt), nt,
                                                self._ptr(A_diag, (Q, self.S, self.n_T, 5, 100), 'A_diag'),
                                                self._ptr(A_cpl, (Q, self.S, 6, self.ncf, 100), 'A_cpl'),
                                                self._ptr(b, (self.S, self.n), 'b'), c_vp(work.data_ptr()), c_vp(U.data_ptr()),
                                                float(rtol), int(max_iter), info, self._stream())
        self._check(rc, 'lrbms3_fom_implicit_euler')
        return U, (int(info[0]), float(info[1]))

    def fom_implicit_euler_batch(self, thetas, dt, nt, A_diag, A_cpl, b_K, phi, U0=None, rtol=1e-10, max_iter=50000, work=None):
        """Column m: (M + dt A(thetas[m])) u_{k+1} = M u_k + dt sum_j phi[m, k + 1, j] b_K[j], nt steps, for nmu <= 64 parameters in
        one call (``lrbms3_fom_implicit_euler_batch``: panels of 16 columns on the matrix cores, one two-level preconditioner at the
        mean theta) -> (U [nt + 1, S, n, nmu], info).  thetas [nmu, Q] host; phi [nmu, nt + 1, K] host or device; b_K [K, S, n];
        U0 None (zeros), [S, n] (every column) or [S, n, nmu].  ``info``: ``iterations`` (summed over panels and steps),
        ``relative_residual`` (worst final ratio), ``panel_iterations``."""
        return self._fom_implicit_euler_batch('lrbms3_fom_implicit_euler_batch', thetas, dt, nt, A_diag, A_cpl, b_K, phi, U0, rtol,
                                              max_iter, work)

    def fom_implicit_euler_batch_tv(self, theta_t, dt, nt, A_diag, A_cpl, b_K, phi, U0=None, rtol=1e-10, max_iter=50000, work=None):
        """``fom_implicit_euler_batch`` with a coefficient row per step (``lrbms3_fom_implicit_euler_batch_tv``):
        theta_t [nmu, nt + 1, Q] host, the step k -> k + 1 of column m solves with theta_t[m, k + 1]."""
        return self._fom_implicit_euler_batch('lrbms3_fom_implicit_euler_batch_tv', theta_t, dt, nt, A_diag, A_cpl, b_K, phi, U0, rtol,
                                              max_iter, work)

    def _fom_implicit_euler_batch(self, export, thetas, dt, nt, A_diag, A_cpl, b_K, phi, U0, rtol, max_iter, work):
        Q, S, K, nt = int(A_diag.shape[0]), self.S, int(b_K.shape[0]), int(nt)
        th = np.ascontiguousarray(thetas, dtype=np.float64)
        nmu = th.shape[0]
        assert th.shape == ((nmu, nt + 1, Q) if export.endswith('_tv') else (nmu, Q))
        ph = self._dev2(phi, (nmu, nt + 1, K), 'phi')
        size = int(self.lib.lrbms3_fom_implicit_euler_batch_work_size(self.handle, nmu))
        if size < 0:
            raise NativeError('{}: nmu = {} is not in 1..64'.format(export, nmu))
        if work is None:
            work = self.empty(size)
        elif work.numel() < size:
            raise NativeError('work buffer too small')
        U = self.empty(max(nt, 0) + 1, S, self.n, nmu)
        if U0 is None:
            U[0].zero_()
        else:
            U[0].copy_(U0.reshape(S, self.n, -1))                # [S, n, 1] broadcasts over the columns
        info = (c_dbl * 2)()
        rc = getattr(self.lib, export)(self.handle, Q, K, nmu, th.ctypes.data_as(_P_DBL), float(dt), nt,
                                       self._ptr(A_diag, (Q, S, self.n_T, 5, 100), 'A_diag'),
                                       self._ptr(A_cpl, (Q, S, 6, self.ncf, 100), 'A_cpl'), self._ptr(b_K, (K, S, self.n), 'b_K'),
                                       c_vp(ph.data_ptr()), c_vp(work.data_ptr()), c_vp(U.data_ptr()), float(rtol), int(max_iter), info,
                                       self._stream())
        panels = (c_dbl * 8)()
        self.lib.lrbms3_fom_implicit_euler_batch_panel_info(self.handle, panels)
        self._check(rc, export)
        return U, {'iterations': int(info[0]), 'relative_residual': float(info[1]),
                   'panel_iterations': [int(v) for v in list(panels)[0:2 * ((nmu + 15) // 16):2]]}

    def reduced_implicit_euler(self, Q, theta, dt, nt, B_sys, M_red, rhs_red, U0=None, rtol=1e-12, max_iter=20000, work=None):
        """(M_red + dt sum_q theta_q B_sys_q) u_{k+1} = M_red u_k + dt rhs_red -> U [nt + 1, S, N] (U[0] = U0, default zero),
        (total CG iterations, worst final relative residual)."""
        N, S = int(rhs_red.shape[1]), self.S
        th = np.ascontiguousarray(theta, dtype=np.float64)
        assert th.shape == (Q,)
        nt = int(nt)
        if work is None:
            work = self.empty(int(self.lib.lrbms3_reduced_implicit_euler_work_size(self.handle, N)))
        U = self.empty(max(nt, 0) + 1, S, N)
        if U0 is None:
            U[0].zero_()
        else:
            U[0].copy_(U0.reshape(S, N))
        info = (c_dbl * 2)()
        rc = self.lib.lrbms3_reduced_implicit_euler(self.handle, Q, N, th.ctypes.data_as(_P_DBL), float(dt), nt,
                                                    self._ptr(B_sys, (Q, S, 7, N, N), 'B_sys'), self._ptr(M_red, (S, N, N), 'M_red'),
                                                    self._ptr(rhs_red, (S, N), 'rhs_red'), c_vp(work.data_ptr()),
                                                    c_vp(U.data_ptr()), float(rtol), int(max_iter), info, self._stream())
        self._check(rc, 'lrbms3_reduced_implicit_euler')
        return U, (int(info[0]), float(info[1]))

    def reduced_time_residual(self, Q, theta, B_sys, M_red, dU, work=None):
        """dU [L, S, N] -> [L, S]: y^T M_red[s]^-1 y with y = (sum_q theta_q B_sys_q dU_l)_s."""
        if dU.dim() != 3:
            raise NativeError('dU: expected [L, S, N]')
        L, S, N = int(dU.shape[0]), self.S, int(dU.shape[2])
        th = np.ascontiguousarray(theta, dtype=np.float64)
        assert th.shape == (Q,)
        if work is None:
            work = self.empty(int(self.lib.lrbms3_reduced_time_residual_work_size(self.handle, N)))
        out = self.empty(L, S)
        rc = self.lib.lrbms3_reduced_time_residual(self.handle, Q, N, L, th.ctypes.data_as(_P_DBL),
                                                   self._ptr(B_sys, (Q, S, 7, N, N), 'B_sys'), self._ptr(M_red, (S, N, N), 'M_red'),
                                                   self._ptr(dU, (L, S, N), 'dU'), c_vp(work.data_ptr()), c_vp(out.data_ptr()),
                                                   self._stream())
        self._check(rc, 'lrbms3_reduced_time_residual')
        return out

    # ------------------------------------------------------------------ affine sources
    def _dev2(self, a, shape, name):
        """A host or device table as a contiguous device tensor of the given shape."""
        a = a if isinstance(a, self.torch.Tensor) else self.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))
        a = a.contiguous()
        self._ptr(a, shape, name)
        return a

    def assemble_source_gram(self, f_smp_K):
        """f_smp_K [K, S, n_T, f_stride] -> F2 [S, K, K] = (f_j, f_l)_{L2(Omega_s)}."""
        K = int(f_smp_K.shape[0])
        F2 = self.empty(self.S, K, K)
        rc = self.lib.lrbms3_assemble_source_gram(self.handle, K, self._ptr(f_smp_K, (K, self.S, self.n_T, self.spec.f_stride), 'f_smp_K'),
                                                  c_vp(F2.data_ptr()), self._stream())
        self._check(rc, 'lrbms3_assemble_source_gram')
        return F2

    def project_sources(self, Q, b_K, bdiv_K, V, work, out=None):
        """rhs_red_K [K, S, N] = V_s^T b_K[j, s] and r_fd_K [K, S, QN] = sum_e bdiv_K[j, s, e] div(R_self)_e; ``work`` is the work
        buffer of a finished ``project_estimate`` pass on the same ``V`` (its flux image R_self lies at offset 0).  ``out``: the
        two arrays to write into (a restricted pass, ``pass_set_subset``, writes the rows of its own list only)."""
        K, N, S = int(b_K.shape[0]), int(V.shape[2]), self.S
        if work.numel() < S * self.n_rt * Q * N:
            raise NativeError('work: not the work buffer of a pass with this Q and N')
        rhs_K, rfd_K = out if out is not None else (self.empty(K, S, N), self.empty(K, S, Q * N))
        self._ptr(rhs_K, (K, S, N), 'rhs_red_K'), self._ptr(rfd_K, (K, S, Q * N), 'r_fd_K')
        rc = self.lib.lrbms3_project_sources(self.handle, Q, N, K, self._ptr(b_K, (K, S, self.n), 'b_K'),
                                             self._ptr(bdiv_K, (K, S, self.n_T), 'bdiv_K'), self._ptr(V, (self.S_ext, self.n, N), 'V'),
                                             c_vp(work.data_ptr()), c_vp(rhs_K.data_ptr()), c_vp(rfd_K.data_ptr()), self._stream())
        self._check(rc, 'lrbms3_project_sources')
        return rhs_K, rfd_K

    def reduced_source_terms(self, Q, thetas, phi, F2, r_fd_K, bdiv_K, Rb, u, ceps, hdiam):
        """The f terms of the residual indicator for the L columns u [S, N, L] with their own thetas [L, Q] and phi [L, K] (host
        or device): [S, L], to be added to the r row of ``reduced_estimate_batch`` run with f2 = 0, r_fd = 0 and bdiv = 0."""
        S, N, L, K = self.S, int(u.shape[1]), int(u.shape[2]), int(F2.shape[1])
        th, ph = self._dev2(thetas, (L, Q), 'theta'), self._dev2(phi, (L, K), 'phi')
        out = self.empty(S, L)
        rc = self.lib.lrbms3_reduced_source_terms(self.handle, Q, N, K, L, c_vp(th.data_ptr()), c_vp(ph.data_ptr()),
                                                  self._ptr(F2, (S, K, K), 'F2'), self._ptr(r_fd_K, (K, S, Q * N), 'r_fd_K'),
                                                  self._ptr(bdiv_K, (K, S, self.n_T), 'bdiv_K'), self._ptr(Rb, (S, self.nbf, Q * N), 'Rb'),
                                                  self._ptr(u, (S, N, L), 'u'), self._ptr(ceps, (S,), 'ceps'), float(hdiam),
                                                  c_vp(out.data_ptr()), self._stream())
        self._check(rc, 'lrbms3_reduced_source_terms')
        return out

    def reduced_solve_batch_src(self, Q, thetas, phi, B_sys, rhs_red_K, rtol=1e-13, max_iter=5000, work=None):
        """``reduced_solve_batch`` where column m solves against sum_j phi[m, j] rhs_red_K[j]: thetas [nmu, Q], phi [nmu, K] (host)
        -> u [S, N, nmu], (iterations, worst relative residual)."""
        K, N, S = int(rhs_red_K.shape[0]), int(rhs_red_K.shape[2]), self.S
        th = np.ascontiguousarray(thetas, dtype=np.float64)
        nmu = th.shape[0]
        ph = np.ascontiguousarray(phi, dtype=np.float64)
        assert th.shape == (nmu, Q) and ph.shape == (nmu, K)
        if work is None:
            work = self.empty(int(self.lib.lrbms3_reduced_solve_batch_work_size(self.handle, N, nmu)))
        u = self.empty(S, N, nmu)
        info = (c_dbl * 2)()
        rc = self.lib.lrbms3_reduced_solve_batch_src(self.handle, Q, N, K, nmu, th.ctypes.data_as(_P_DBL), ph.ctypes.data_as(_P_DBL),
                                                     self._ptr(B_sys, (Q, S, 7, N, N), 'B_sys'),
                                                     self._ptr(rhs_red_K, (K, S, N), 'rhs_red_K'), c_vp(work.data_ptr()),
                                                     c_vp(u.data_ptr()), float(rtol), int(max_iter), info, self._stream())
        self._check(rc, 'lrbms3_reduced_solve_batch_src')
        return u, (int(info[0]), float(info[1]))

    def combine_sources(self, phi, x_K):
        """sum_j phi[j] x_K[j] for x_K [K, ...] (device), phi [K] (host): a tensor of shape x_K.shape[1:]."""
        K = int(x_K.shape[0])
        ph = np.ascontiguousarray(phi, dtype=np.float64)
        assert ph.shape == (K,)
        self._ptr(x_K, tuple(x_K.shape), 'x_K')
        y = self.empty(*x_K.shape[1:])
        rc = self.lib.lrbms3_combine_sources(self.handle, K, int(y.numel()), ph.ctypes.data_as(_P_DBL), c_vp(x_K.data_ptr()),
                                             c_vp(y.data_ptr()), self._stream())
        self._check(rc, 'lrbms3_combine_sources')
        return y

    def fom_implicit_euler_src(self, Q, theta, dt, nt, A_diag, A_cpl, b_K, phi, U0=None, rtol=1e-10, max_iter=50000, work=None):
        """``fom_implicit_euler`` with the step right-hand side M u_k + dt sum_j phi[k + 1, j] b_K[j]; phi [nt + 1, K] (host or
        device) -> U [nt + 1, S, n], (total CG iterations, worst final relative residual)."""
        th = np.ascontiguousarray(theta, dtype=np.float64)
        assert th.shape == (Q,)
        nt, K = int(nt), int(b_K.shape[0])
        ph = self._dev2(phi, (max(nt, 0) + 1, K), 'phi')
        if work is None:
            work = self.empty(int(self.lib.lrbms3_fom_implicit_euler_work_size(self.handle)))
        U = self.empty(max(nt, 0) + 1, self.S, self.n)
        if U0 is None:
            U[0].zero_()
        else:
            U[0].copy_(U0.reshape(self.S, self.n))
        info = (c_dbl * 2)()
        rc = self.lib.lrbms3_fom_implicit_euler_src(self.handle, Q, K, th.ctypes.data_as(_P_DBL), float(dt), nt,
                                                    self._ptr(A_diag, (Q, self.S, self.n_T, 5, 100), 'A_diag'),
                                                    self._ptr(A_cpl, (Q, self.S, 6, self.ncf, 100), 'A_cpl'),
                                                    self._ptr(b_K, (K, self.S, self.n), 'b_K'), c_vp(ph.data_ptr()),
                                                    c_vp(work.data_ptr()), c_vp(U.data_ptr()), float(rtol), int(max_iter), info,
                                                    self._stream())
        self._check(rc, 'lrbms3_fom_implicit_euler_src')
        return U, (int(info[0]), float(info[1]))

    def reduced_implicit_euler_src(self, Q, theta, dt, nt, B_sys, M_red, rhs_red_K, phi, U0=None, rtol=1e-12, max_iter=20000, work=None):
        """``reduced_implicit_euler`` with M_red u_k + dt sum_j phi[k + 1, j] rhs_red_K[j]; phi [nt + 1, K] (host or device)
        -> U [nt + 1, S, N], (total CG iterations, worst final relative residual)."""
        K, N, S = int(rhs_red_K.shape[0]), int(rhs_red_K.shape[2]), self.S
        th = np.ascontiguousarray(theta, dtype=np.float64)
        assert th.shape == (Q,)
        nt = int(nt)
        ph = self._dev2(phi, (max(nt, 0) + 1, K), 'phi')
        if work is None:
            work = self.empty(int(self.lib.lrbms3_reduced_implicit_euler_work_size(self.handle, N)))
        U = self.empty(max(nt, 0) + 1, S, N)
        if U0 is None:
            U[0].zero_()
        else:
            U[0].copy_(U0.reshape(S, N))
        info = (c_dbl * 2)()
        rc = self.lib.lrbms3_reduced_implicit_euler_src(self.handle, Q, N, K, th.ctypes.data_as(_P_DBL), float(dt), nt,
                                                        self._ptr(B_sys, (Q, S, 7, N, N), 'B_sys'), self._ptr(M_red, (S, N, N), 'M_red'),
                                                        self._ptr(rhs_red_K, (K, S, N), 'rhs_red_K'), c_vp(ph.data_ptr()),
                                                        c_vp(work.data_ptr()), c_vp(U.data_ptr()), float(rtol), int(max_iter), info,
                                                        self._stream())
        self._check(rc, 'lrbms3_reduced_implicit_euler_src')
        return U, (int(info[0]), float(info[1]))

    # ------------------------------------------------------------------ batched reduced trajectories
    def _batch_trajectory_buffers(self, name, N, nmu, nt, U0, work):
        """work and U [nt + 1, S, N, nmu] (U[0] = U0: [S, N] for every column, or [S, N, nmu]; default zero) of the batched
        reduced implicit Euler exports."""
        need = int(self.lib.lrbms3_reduced_implicit_euler_batch_work_size(self.handle, N, nmu))
        if need < 0:
            raise NativeError('{}: bad N / nmu'.format(name))
        if work is None:
            work = self.empty(need)
        if work.numel() < need:
            raise NativeError('{}: work too small'.format(name))
        U = self.zeros(max(int(nt), 0) + 1, self.S, N, nmu)
        if U0 is not None:
            U[0] = U0.reshape(self.S, N, -1)          # [S, N, 1] broadcasts over the columns
        return work, U

    def reduced_implicit_euler_batch(self, Q, thetas, dt, nt, B_sys, M_red, rhs_red, U0=None, rtol=1e-12, max_iter=20000, work=None):
        """nmu <= 64 reduced trajectories in one call: thetas [nmu, Q] -> U [nt + 1, S, N, nmu] (parameter fastest), (iterations
        of the slowest group summed over the steps, worst final relative residual); column m is what ``reduced_implicit_euler``
        returns at thetas[m].  ``max_iter`` caps the iterations of one step."""
        N, S = int(rhs_red.shape[1]), self.S
        th = np.ascontiguousarray(thetas, dtype=np.float64)
        nmu = th.shape[0]
        assert th.shape == (nmu, Q)
        work, U = self._batch_trajectory_buffers('reduced_implicit_euler_batch', N, nmu, nt, U0, work)
        info = (c_dbl * 2)()
        rc = self.lib.lrbms3_reduced_implicit_euler_batch(self.handle, Q, N, nmu, th.ctypes.data_as(_P_DBL), float(dt), int(nt),
                                                          self._ptr(B_sys, (Q, S, 7, N, N), 'B_sys'), self._ptr(M_red, (S, N, N), 'M_red'),
                                                          self._ptr(rhs_red, (S, N), 'rhs_red'), c_vp(work.data_ptr()),
                                                          c_vp(U.data_ptr()), float(rtol), int(max_iter), info, self._stream())
        self._check(rc, 'lrbms3_reduced_implicit_euler_batch')
        return U, (int(info[0]), float(info[1]))

    def reduced_implicit_euler_batch_src(self, Q, thetas, dt, nt, B_sys, M_red, rhs_red_K, phi, U0=None, rtol=1e-12, max_iter=20000,
                                         work=None):
        """``reduced_implicit_euler_batch`` with the step right-hand side M_red u_k + dt sum_j phi[m, k + 1, j] rhs_red_K[j] in
        column m; phi [nmu, nt + 1, K] (host or device)."""
        K, N, S = int(rhs_red_K.shape[0]), int(rhs_red_K.shape[2]), self.S
        th = np.ascontiguousarray(thetas, dtype=np.float64)
        nmu = th.shape[0]
        assert th.shape == (nmu, Q)
        ph = self._dev2(phi, (nmu, max(int(nt), 0) + 1, K), 'phi')
        work, U = self._batch_trajectory_buffers('reduced_implicit_euler_batch_src', N, nmu, nt, U0, work)
        info = (c_dbl * 2)()
        rc = self.lib.lrbms3_reduced_implicit_euler_batch_src(self.handle, Q, N, K, nmu, th.ctypes.data_as(_P_DBL), float(dt), int(nt),
                                                              self._ptr(B_sys, (Q, S, 7, N, N), 'B_sys'),
                                                              self._ptr(M_red, (S, N, N), 'M_red'),
                                                              self._ptr(rhs_red_K, (K, S, N), 'rhs_red_K'), c_vp(ph.data_ptr()),
                                                              c_vp(work.data_ptr()), c_vp(U.data_ptr()), float(rtol), int(max_iter), info,
                                                              self._stream())
        self._check(rc, 'lrbms3_reduced_implicit_euler_batch_src')
        return U, (int(info[0]), float(info[1]))

    def reduced_implicit_euler_batch_tv(self, Q, theta_t, dt, nt, B_sys, M_red, rhs_red, phi=None, U0=None, rtol=1e-12, max_iter=20000,
                                        work=None):
        """``reduced_implicit_euler_batch`` (phi None, rhs_red [S, N]) or ``reduced_implicit_euler_batch_src`` (phi [nmu, nt + 1, K],
        rhs_red [K, S, N]) with a coefficient row per step (``lrbms3_reduced_implicit_euler_batch_tv``): theta_t
        [nmu, nt + 1, Q] host, the step k -> k + 1 of column m solves with theta_t[m, k + 1]."""
        S, nt = self.S, int(nt)
        K = 0 if phi is None else int(rhs_red.shape[0])
        N = int(rhs_red.shape[-1])
        th = np.ascontiguousarray(theta_t, dtype=np.float64)
        nmu = th.shape[0]
        assert th.shape == (nmu, nt + 1, Q), 'theta_t must be [nmu, nt + 1, Q]'
        ph = c_vp(None) if phi is None else c_vp(self._dev2(phi, (nmu, nt + 1, K), 'phi').data_ptr())
        work, U = self._batch_trajectory_buffers('reduced_implicit_euler_batch_tv', N, nmu, nt, U0, work)
        info = (c_dbl * 2)()
        rc = self.lib.lrbms3_reduced_implicit_euler_batch_tv(self.handle, Q, N, K, nmu, th.ctypes.data_as(_P_DBL), float(dt), nt,
                                                             self._ptr(B_sys, (Q, S, 7, N, N), 'B_sys'),
                                                             self._ptr(M_red, (S, N, N), 'M_red'),
                                                             self._ptr(rhs_red, (K, S, N) if K else (S, N), 'rhs_red'), ph,
                                                             c_vp(work.data_ptr()), c_vp(U.data_ptr()), float(rtol), int(max_iter), info,
                                                             self._stream())
        self._check(rc, 'lrbms3_reduced_implicit_euler_batch_tv')
        return U, (int(info[0]), float(info[1]))

    # ------------------------------------------------------------------ batched parabolic estimates
    def reduced_parabolic_estimate_batch(self, Q, thetas, coef, dt, nt, U, B_sys, M_red, out, ops, hdiam, phi=None, F2=None, r_fd_K=None,
                                         bdiv_K=None, work=None):
        """The parabolic estimate of the nmu <= 64 trajectories of the panel U [nt + 1, S, N, nmu] in one call
        (``lrbms3_reduced_parabolic_estimate_batch``): thetas [nmu, Q], coef [nmu, 2] (host); ``out`` / ``ops`` as for
        ``reduced_estimate_batch``; with a time-dependent source phi [nmu, nt + 1, K] (host or device), F2 [S, K, K], r_fd_K
        [K, S, QN], bdiv_K [K, S, n_T] and ``out`` / ``ops`` with zeroed r_fd / f2 / bdiv.  Returns a dict of device tensors:
        eta_loc [3, nt + 1, S, nmu], time_deriv_nc [nt, S, nmu], time_residual [nt, nmu], eta [nt + 1, nmu], est [nmu]."""
        return self._reduced_parabolic_estimate_batch('lrbms3_reduced_parabolic_estimate_batch', Q, thetas, coef, dt, nt, U, B_sys, M_red, out,
                                                      ops, hdiam, phi, F2, r_fd_K, bdiv_K, work)

    def reduced_parabolic_estimate_batch_tv(self, Q, theta_t, coef, dt, nt, U, B_sys, M_red, out, ops, hdiam, phi=None, F2=None,
                                            r_fd_K=None, bdiv_K=None, work=None):
        """``reduced_parabolic_estimate_batch`` with a coefficient row per step (``lrbms3_reduced_parabolic_estimate_batch_tv``,
        DESIGN.md 9.18): theta_t [nmu, nt + 1, Q], coef [nmu, nt + 1, 2] (host).  The elliptic rows of U[k], the source terms and
        the scaling of eta[k] use row k, the time residual of U[k + 1] - U[k] row k + 1."""
        return self._reduced_parabolic_estimate_batch('lrbms3_reduced_parabolic_estimate_batch_tv', Q, theta_t, coef, dt, nt, U, B_sys, M_red,
                                                      out, ops, hdiam, phi, F2, r_fd_K, bdiv_K, work)

    def _reduced_parabolic_estimate_batch(self, export, Q, thetas, coef, dt, nt, U, B_sys, M_red, out, ops, hdiam, phi, F2, r_fd_K, bdiv_K,
                                          work):
        S, N, nt = self.S, int(B_sys.shape[-1]), int(nt)
        th = np.ascontiguousarray(thetas, dtype=np.float64)
        nmu = th.shape[0]
        cf = np.ascontiguousarray(coef, dtype=np.float64)
        if export.endswith('_tv'):
            assert th.shape == (nmu, nt + 1, Q) and cf.shape == (nmu, nt + 1, 2), 'theta_t must be [nmu, nt + 1, Q], coef [nmu, nt + 1, 2]'
        else:
            assert th.shape == (nmu, Q) and cf.shape == (nmu, 2), 'thetas must be [nmu, Q], coef [nmu, 2]'
        shp = self.out_shapes(Q, N)
        names = ('G_nc', 'G_bb', 'G_rdd', 'G_ab', 'G_aa', 'r_fd', 'Rb', 'Yb', 'Dp', 'Xab', 'As', 'Cn')
        args = [self._ptr(U, (max(nt, 0) + 1, S, N, nmu), 'U'), self._ptr(B_sys, (Q, S, 7, N, N), 'B_sys'),
                self._ptr(M_red, (S, N, N), 'M_red')] + [self._ptr(out[k], shp[k], k) for k in names]
        args += [self._ptr(ops['ebar'], (S, self.n_T, 100), 'ebar'), self._ptr(ops['Bbb'], (S, self.n_T, 16), 'Bbb'),
                 self._ptr(ops['bdiv'], (S, self.n_T), 'bdiv'), self._ptr(ops['f2'], (S,), 'f2'), self._ptr(ops['ceps'], (S,), 'ceps')]
        K, src = 0, [c_vp(None)] * 4
        if phi is not None:
            K = int(F2.shape[1])
            ph = self._dev2(phi, (nmu, max(nt, 0) + 1, K), 'phi')
            src = [c_vp(ph.data_ptr()), self._ptr(F2, (S, K, K), 'F2'), self._ptr(r_fd_K, (K, S, Q * N), 'r_fd_K'),
                   self._ptr(bdiv_K, (K, S, self.n_T), 'bdiv_K')]
        need = int(getattr(self.lib, export + '_work_size')(self.handle, N, nmu, nt))
        if need < 0:
            raise NativeError('{}: bad N / nmu / nt'.format(export[7:]))
        if work is None:
            work = self.empty(need)
        if work.numel() < need:
            raise NativeError('{}: work too small'.format(export[7:]))
        res = {'eta_loc': self.empty(3, nt + 1, S, nmu), 'time_deriv_nc': self.empty(nt, S, nmu), 'time_residual': self.empty(nt, nmu),
               'eta': self.empty(nt + 1, nmu), 'est': self.empty(nmu)}
        rc = getattr(self.lib, export)(
            self.handle, Q, N, K, nmu, nt, float(dt), th.ctypes.data_as(_P_DBL), cf.ctypes.data_as(_P_DBL), *args, float(hdiam), *src,
            c_vp(work.data_ptr()), *[c_vp(res[k].data_ptr()) for k in ('eta_loc', 'time_deriv_nc', 'time_residual', 'eta', 'est')],
            self._stream())
        self._check(rc, export)
        return res

    # ------------------------------------------------------------------ online enrichment
    def assemble_dirichlet_correction(self, lam):
        """D_corr [Q, S, 6, ncf, 100]: per coupling face, Dirichlet-face block minus the inner-face own / own block in A_diag."""
        Q, sp = lam.shape[0], self.spec
        D_corr = self.empty(Q, self.S, 6, self.ncf, 100)
        rc = self.lib.lrbms3_assemble_dirichlet_correction(self.handle, Q, self._ptr(lam, (Q, self.S_ext, self.n_T, sp.lam_stride), 'lam'),
                                                           c_vp(D_corr.data_ptr()), self._stream())
        self._check(rc, 'lrbms3_assemble_dirichlet_correction')
        return D_corr

    def local_correction_work_size(self, nmark):
        return int(self.lib.lrbms3_local_correction_work_size(self.handle, int(nmark)))

    def local_correction_solve(self, Q, theta, marked, A_diag, A_cpl, D_corr, b, rtol=1e-10, max_iter=20000, work=None):
        """The corrector problems of the subdomains ``marked`` in one native call -> corr [nmark, n], info [nmark, 2] (host:
        iterations, final relative residual)."""
        th = np.ascontiguousarray(theta, dtype=np.float64)
        mk = np.ascontiguousarray(marked, dtype=np.int32).reshape(-1)
        nmark = int(mk.size)
        assert th.shape == (Q,) and nmark >= 1
        if work is None:
            work = self.empty(self.local_correction_work_size(nmark))
        elif work.numel() < self.local_correction_work_size(nmark):
            raise NativeError('work buffer too small')
        corr = self.empty(nmark, self.n)
        info = np.zeros((nmark, 2))
        rc = self.lib.lrbms3_local_correction_solve(self.handle, Q, th.ctypes.data_as(_P_DBL), nmark, mk.ctypes.data_as(_P_I32),
                                                    self._ptr(A_diag, (Q, self.S, self.n_T, 5, 100), 'A_diag'),
                                                    self._ptr(A_cpl, (Q, self.S, 6, self.ncf, 100), 'A_cpl'),
                                                    self._ptr(D_corr, (Q, self.S, 6, self.ncf, 100), 'D_corr'),
                                                    self._ptr(b, (self.S, self.n), 'b'), c_vp(work.data_ptr()), c_vp(corr.data_ptr()),
                                                    float(rtol), int(max_iter), info.ctypes.data_as(_P_DBL), self._stream())
        self._check(rc, 'lrbms3_local_correction_solve')
        return corr, info

    def local_correction_euler_work_size(self, nmark, nt):
        return int(self.lib.lrbms3_local_correction_euler_work_size(self.handle, int(nmark), int(nt)))

    def local_correction_euler(self, Q, theta, dt, nt, marked, A_diag, A_cpl, D_corr, b_K, phi, rtol=1e-10, max_iter=20000, work=None):
        """The corrector trajectories of the parabolic enrichment (``lrbms3_local_correction_euler``): b_K [K, S, n],
        phi [nt + 1, K] (host or device) -> corr [nmark, n, nt] (step fastest: column k - 1 = x_k), info [nmark, 2] (host:
        iterations summed over the steps, worst final residual ratio of a step)."""
        th = np.ascontiguousarray(theta, dtype=np.float64)
        mk = np.ascontiguousarray(marked, dtype=np.int32).reshape(-1)
        nmark, nt, K = int(mk.size), int(nt), int(b_K.shape[0])
        assert th.shape == (Q,) and nmark >= 1 and nt >= 1
        ph = self._dev2(phi, (nt + 1, K), 'phi')
        need = self.local_correction_euler_work_size(nmark, nt)
        if work is None:
            work = self.empty(need)
        elif work.numel() < need:
            raise NativeError('work buffer too small')
        corr = self.empty(nmark, self.n, nt)
        info = np.zeros((nmark, 2))
        rc = self.lib.lrbms3_local_correction_euler(self.handle, Q, K, th.ctypes.data_as(_P_DBL), float(dt), nt, nmark,
                                                    mk.ctypes.data_as(_P_I32),
                                                    self._ptr(A_diag, (Q, self.S, self.n_T, 5, 100), 'A_diag'),
                                                    self._ptr(A_cpl, (Q, self.S, 6, self.ncf, 100), 'A_cpl'),
                                                    self._ptr(D_corr, (Q, self.S, 6, self.ncf, 100), 'D_corr'),
                                                    self._ptr(b_K, (K, self.S, self.n), 'b_K'), c_vp(ph.data_ptr()),
                                                    c_vp(work.data_ptr()), c_vp(corr.data_ptr()), float(rtol), int(max_iter),
                                                    info.ctypes.data_as(_P_DBL), self._stream())
        self._check(rc, 'lrbms3_local_correction_euler')
        return corr, info
