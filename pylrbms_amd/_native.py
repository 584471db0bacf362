"""ctypes binding of liblrbms_hip.so (C ABI: include/lrbms_hip.h).

There is NO CPU fallback: if the shared library is missing or a call fails this module raises.  PyTorch is only the
device-array container (allocation, stream handle); every number is produced by the HIP kernels.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'liblrbms_hip.so')

c_i32, c_i64, c_dbl, c_vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_double, ctypes.c_void_p
_P_I32 = ctypes.POINTER(c_i32)
_P_DBL = ctypes.POINTER(c_dbl)


class MeshDesc(ctypes.Structure):
    _fields_ = ([(k, c_i32) for k in ('kx', 'ky', 'n_T', 'n_rt', 'n_vertices', 'ncf')] +
                [('hx', c_dbl), ('hy', c_dbl), ('kappa', c_dbl * 4)] +
                [(k, _P_I32) for k in ('nb_elem', 'nb_face', 'nb_elem_out', 'nb_face_out', 'elem_side_pos', 'elem_rt',
                                       'face_sign', 'dof_vertex', 'vdof_ptr', 'vdof_idx', 'rt_e0', 'rt_f0', 'rt_e1',
                                       'rt_f1', 'rt_side', 'side_elem', 'side_elem_out', 'side_count')] +
                [('ntouch', c_i32), ('touch_elem', _P_I32), ('touch_count', _P_I32)] +
                [(k, _P_DBL) for k in ('grad', 'area', 'normal', 'face_len', 'points')])


# name -> (restype, argtypes); exactly the symbols include/lrbms_hip.h declares
SIGNATURES = {
    'lrbms_version': (ctypes.c_char_p, []),
    'lrbms_ctx_create': (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(c_vp)]),
    'lrbms_ctx_destroy': (ctypes.c_int, [c_vp]),
    'lrbms_last_error': (ctypes.c_char_p, [c_vp]),
    'lrbms_ctx_aux_stream': (c_vp, [c_vp, c_i32]),
    'lrbms_ctx_set_option': (ctypes.c_int, [c_vp, c_i32, c_i32]),
    'lrbms_set_quadrature': (ctypes.c_int, [c_vp, c_vp]),
    'lrbms_fused_set_subset': (ctypes.c_int, [c_vp, _P_I32, c_i32]),
    'lrbms_set_diagonal_neighbours': (ctypes.c_int, [c_vp, _P_I32]),
    'lrbms_kernel_timing': (ctypes.c_int, [c_vp, c_i32]),
    'lrbms_kernel_timing_read': (ctypes.c_int, [c_vp, ctypes.c_char_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_double), c_i32,
                                                ctypes.POINTER(c_i32)]),
    'lrbms_mesh_upload': (ctypes.c_int, [c_vp, ctypes.POINTER(MeshDesc), c_i32, c_i32, _P_I32]),
    'lrbms_assemble_swipdg': (ctypes.c_int, [c_vp, c_i32, c_vp, c_vp, c_vp, c_vp]),
    'lrbms_assemble_rhs': (ctypes.c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    'lrbms_assemble_products': (ctypes.c_int, [c_vp, c_i32, _P_DBL, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    'lrbms_assemble_flux': (ctypes.c_int, [c_vp, c_i32, c_vp, c_vp, c_vp]),
    'lrbms_oswald_apply': (ctypes.c_int, [c_vp, c_i32, c_vp, c_vp, c_vp]),
    'lrbms_flux_reconstruct': (ctypes.c_int, [c_vp, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp]),
    'lrbms_project_system': (ctypes.c_int, [c_vp, c_i32, c_i32] + [c_vp] * 11),
    'lrbms_estimator_work_size': (c_i64, [c_vp, c_i32, c_i32]),
    'lrbms_estimator_grams': (ctypes.c_int, [c_vp, c_i32, c_i32] + [c_vp] * 16),
    'lrbms_fused_supported': (ctypes.c_int, [c_vp, c_i32, c_i32]),
    'lrbms_fused_mfma_per_subdomain': (c_i64, [c_vp, c_i32, c_i32]),
    'lrbms_fused_fnc_ld': (c_i32, [c_vp, c_i32]),
    'lrbms_fused_factored_supported': (ctypes.c_int, [c_vp, c_i32, c_i32]),
    'lrbms_fused_work_size': (c_i64, [c_vp, c_i32, c_i32]),
    'lrbms_project_estimate_fused': (ctypes.c_int, [c_vp, c_i32, c_i32] + [c_vp] * 22),
    'lrbms_project_estimate_fused_phase': (ctypes.c_int, [c_vp, c_i32, c_i32, c_i32] + [c_vp] * 22),
    'lrbms_fside_size': (c_i64, [c_vp, c_i32, c_i32]),
    'lrbms_fnc_size': (c_i64, [c_vp, c_i32]),
    'lrbms_project_estimate_fused_factored': (ctypes.c_int, [c_vp, c_i32, c_i32, c_i32] + [c_vp] * 24),
    'lrbms_reduced_estimate_factored': (ctypes.c_int, [c_vp, c_i32, c_i32, _P_DBL] + [c_vp] * 11 + [c_dbl, c_vp, c_vp]),
    'lrbms_reduced_estimate_batch_factored': (ctypes.c_int, [c_vp, c_i32, c_i32, c_i32, _P_DBL] + [c_vp] * 11 + [c_dbl, c_vp, c_vp]),
    'lrbms_reduced_estimate': (ctypes.c_int, [c_vp, c_i32, c_i32, _P_DBL] + [c_vp] * 9 + [c_dbl, c_vp, c_vp]),
    'lrbms_reduced_estimate_batch': (ctypes.c_int, [c_vp, c_i32, c_i32, c_i32, _P_DBL] + [c_vp] * 9 + [c_dbl, c_vp, c_vp]),
    'lrbms_reduced_solve_work_size': (c_i64, [c_vp, c_i32]),
    'lrbms_reduced_solve': (ctypes.c_int, [c_vp, c_i32, c_i32, _P_DBL, c_vp, c_vp, c_vp, c_vp, c_dbl, c_i32, _P_DBL, c_vp]),
    'lrbms_reduced_solve_batch_work_size': (c_i64, [c_vp, c_i32, c_i32]),
    'lrbms_reduced_solve_batch': (ctypes.c_int, [c_vp, c_i32, c_i32, c_i32, _P_DBL, c_vp, c_vp, c_vp, c_vp, c_dbl, c_i32, _P_DBL,
                                                 c_vp]),
    'lrbms_reduced_precond_size': (c_i64, [c_vp, c_i32]),
    'lrbms_reduced_precond_build': (ctypes.c_int, [c_vp, c_i32, c_i32, _P_DBL, c_vp, c_vp, c_vp, c_vp]),
    'lrbms_reduced_precond_use': (ctypes.c_int, [c_vp, c_i32, c_vp]),
    'lrbms_fom_solve_work_size': (c_i64, [c_vp]),
    'lrbms_fom_solve': (ctypes.c_int, [c_vp, c_i32, _P_DBL, c_vp, c_vp, c_vp, c_vp, c_vp, c_dbl, c_i32, _P_DBL, c_vp]),
    'lrbms_fom_solve_batch_work_size': (c_i64, [c_vp, c_i32]),
    'lrbms_fom_solve_batch': (ctypes.c_int, [c_vp, c_i32, c_i32, _P_DBL, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_dbl, c_i32,
                                             _P_DBL, c_vp]),
    'lrbms_fom_solve_batch_panel_info': (ctypes.c_int, [c_vp, _P_DBL]),
    'lrbms_fom_implicit_euler': (ctypes.c_int, [c_vp, c_i32, _P_DBL, c_dbl, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_dbl, c_i32, _P_DBL,
                                                c_vp]),
    'lrbms_fom_implicit_euler_batch_work_size': (c_i64, [c_vp, c_i32]),
    'lrbms_fom_implicit_euler_batch': (ctypes.c_int, [c_vp, c_i32, c_i32, c_i32, _P_DBL, c_dbl, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                                      c_dbl, c_i32, _P_DBL, c_vp]),
    'lrbms_fom_implicit_euler_batch_panel_info': (ctypes.c_int, [c_vp, _P_DBL]),
    'lrbms_mass_inverse_norm2': (ctypes.c_int, [c_vp, c_i32, c_vp, c_vp, c_vp]),
    'lrbms_div_apply': (ctypes.c_int, [c_vp, c_i32, c_i32, c_vp, c_vp, c_vp]),
    'lrbms_div_pairing': (ctypes.c_int, [c_vp, c_i32, c_i32, _P_DBL, c_vp, c_vp, c_vp, c_vp]),
    'lrbms_reduced_reconstruction_terms': (ctypes.c_int, [c_vp, c_i32, c_i32, c_i32, _P_DBL] + [c_vp] * 8),
    'lrbms_reduced_implicit_euler': (ctypes.c_int, [c_vp, c_i32, c_i32, _P_DBL, c_dbl, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_dbl,
                                                    c_i32, _P_DBL, c_vp]),
    'lrbms_reduced_time_residual_work_size': (c_i64, [c_vp, c_i32]),
    'lrbms_reduced_time_residual': (ctypes.c_int, [c_vp, c_i32, c_i32, c_i32, _P_DBL, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    'lrbms_assemble_source_gram': (ctypes.c_int, [c_vp, c_i32, c_vp, c_vp, c_vp]),
    'lrbms_assembled_arrays': (c_i32, [c_vp, c_i32, ctypes.POINTER(c_vp), c_i32]),
    'lrbms_fom_implicit_euler_src': (ctypes.c_int, [c_vp, c_i32, c_i32, _P_DBL, c_dbl, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                                    c_dbl, c_i32, _P_DBL, c_vp]),
    'lrbms_reduced_implicit_euler_src': (ctypes.c_int, [c_vp, c_i32, c_i32, c_i32, _P_DBL, c_dbl, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp,
                                                        c_vp, c_dbl, c_i32, _P_DBL, c_vp]),
    'lrbms_project_sources': (ctypes.c_int, [c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    'lrbms_reduced_source_terms': (ctypes.c_int, [c_vp, c_i32, c_i32, c_i32, c_i32, _P_DBL, c_vp, c_vp, c_vp, c_vp, c_vp, c_dbl,
                                                  c_vp, c_vp]),
    'lrbms_reduced_solve_batch_src': (ctypes.c_int, [c_vp, c_i32, c_i32, c_i32, c_i32, _P_DBL, _P_DBL, c_vp, c_vp, c_vp, c_vp, c_dbl,
                                                     c_i32, _P_DBL, c_vp]),
    'lrbms_reduced_implicit_euler_batch_work_size': (c_i64, [c_vp, c_i32, c_i32]),
    'lrbms_reduced_implicit_euler_batch': (ctypes.c_int, [c_vp, c_i32, c_i32, c_i32, _P_DBL, c_dbl, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp,
                                                          c_dbl, c_i32, _P_DBL, c_vp]),
    'lrbms_reduced_implicit_euler_batch_src': (ctypes.c_int, [c_vp, c_i32, c_i32, c_i32, c_i32, _P_DBL, c_dbl, c_i32, c_vp, c_vp, c_vp,
                                                              c_vp, c_vp, c_vp, c_dbl, c_i32, _P_DBL, c_vp]),
    'lrbms_reduced_parabolic_estimate_batch_work_size': (c_i64, [c_vp, c_i32, c_i32, c_i32]),
    'lrbms_reduced_parabolic_estimate_batch': (ctypes.c_int, [c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_dbl, _P_DBL, _P_DBL, c_i32]
                                               + [c_vp] * 13 + [c_dbl] + [c_vp] * 10),
    # time-dependent diffusion coefficients: theta_t [nmu][nt+1][Q]
    'lrbms_fom_implicit_euler_batch_tv': (ctypes.c_int, [c_vp, c_i32, c_i32, c_i32, _P_DBL, c_dbl, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp,
                                                         c_vp, c_dbl, c_i32, _P_DBL, c_vp]),
    'lrbms_reduced_implicit_euler_batch_tv_work_size': (c_i64, [c_vp, c_i32, c_i32, c_i32]),
    'lrbms_reduced_implicit_euler_batch_tv': (ctypes.c_int, [c_vp, c_i32, c_i32, c_i32, c_i32, _P_DBL, c_dbl, c_i32, c_vp, c_vp, c_vp,
                                                             c_vp, c_vp, c_vp, c_dbl, c_i32, _P_DBL, c_vp]),
    'lrbms_reduced_parabolic_estimate_batch_tv_work_size': (c_i64, [c_vp, c_i32, c_i32, c_i32]),
    'lrbms_reduced_parabolic_estimate_batch_tv': (ctypes.c_int, [c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_dbl, _P_DBL, _P_DBL, c_i32]
                                                  + [c_vp] * 13 + [c_dbl] + [c_vp] * 10),
    'lrbms_combine_sources': (ctypes.c_int, [c_vp, c_i32, c_i64, _P_DBL, c_vp, c_vp, c_vp]),
    'lrbms_assemble_dirichlet_correction': (ctypes.c_int, [c_vp, c_i32, c_vp, c_vp, c_vp]),
    'lrbms_local_correction_work_size': (c_i64, [c_vp, c_i32]),
    'lrbms_local_correction_solve': (ctypes.c_int, [c_vp, c_i32, _P_DBL, c_i32, _P_I32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_dbl,
                                                    c_i32, _P_DBL, c_vp]),
    'lrbms_local_correction_euler_work_size': (c_i64, [c_vp, c_i32]),
    'lrbms_local_correction_euler': (ctypes.c_int, [c_vp, c_i32, c_i32, _P_DBL, c_dbl, c_i32, c_i32, _P_I32, c_vp, c_vp, c_vp, c_vp,
                                                    c_vp, c_vp, c_vp, c_dbl, c_i32, _P_DBL, c_vp]),
    'lrbms_blockell_apply': (ctypes.c_int, [c_vp, c_i32, c_vp, c_vp, c_vp, c_vp]),
    'lrbms_fom_apply': (ctypes.c_int, [c_vp, c_i32, c_i32, _P_DBL, c_vp, c_vp, c_vp, c_vp, c_vp]),
    'lrbms_gemm_tn': (ctypes.c_int, [c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_i64, c_i32, c_vp, c_i64, c_i32, c_vp,
                                     c_i64, c_i32, c_vp, c_dbl, c_vp]),
    # local POD basis extension
    'lrbms_local_pod_work_size': (c_i64, [c_vp, c_i32, c_i32]),
    'lrbms_local_pod': (ctypes.c_int, [c_vp, c_i32, c_i32, c_i32, c_dbl, c_dbl] + [c_vp] * 9),
    'lrbms_local_pod_stream_state_size': (c_i64, [c_vp, c_i32, c_i32]),
    'lrbms_local_pod_stream_work_size': (c_i64, [c_vp, c_i32, c_i32, c_i32]),
    'lrbms_local_pod_stream_begin': (ctypes.c_int, [c_vp, c_i32, c_i32, c_vp, c_vp]),
    'lrbms_local_pod_stream_push': (ctypes.c_int, [c_vp, c_i32, c_i32, c_i32, c_i32] + [c_vp] * 7),
    'lrbms_local_pod_stream_finish': (ctypes.c_int, [c_vp, c_i32, c_i32, c_i32, c_i32, c_dbl, c_dbl] + [c_vp] * 10),
    'lrbms_pod_gram': (ctypes.c_int, [c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp]),
    'lrbms_pod_eigh_work_size': (c_i64, [c_vp, c_i32, c_i32]),
    'lrbms_pod_eigh': (ctypes.c_int, [c_vp, c_i32, c_i32, c_i32] + [c_vp] * 7),
}

_lib = None


class NativeError(RuntimeError):
    pass


def load_library(path=None):
    """Load liblrbms_hip.so and bind every declared symbol; raises if the library or a symbol is missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or os.environ.get('LRBMS_HIP_LIB') or LIB_PATH     # LRBMS_HIP_LIB: A/B builds of tools/build_variant.sh
    # torch bundles its own libamdhip64: import it FIRST so that our NEEDED libamdhip64.so.7 resolves to the copy
    # torch uses (two HIP runtimes in one process do not share devices, streams or allocations)
    import torch  # noqa: F401
    if not os.path.exists(path):
        raise NativeError('{} is missing: run `python __graft_entry__.py` (or pylrbms_amd/_build.py) to build the HIP '
                          'extension; there is no CPU fallback'.format(path))
    lib = ctypes.CDLL(path)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)         # AttributeError if the symbol is not exported
        fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


def _i32p(a):
    return a.ctypes.data_as(_P_I32)


def _dblp(a):
    return a.ctypes.data_as(_P_DBL)


class ContextBase:
    """What the 2D and the 3D contexts share: the C context behind ``handle``, its error reporting, tensor checks, options and
    kernel timing.  A subclass names its symbol prefix (``PREFIX``: ``lrbms_`` / ``lrbms3_``), its option table and its loader."""

    PREFIX = None                       # 'lrbms_' / 'lrbms3_'
    OPTIONS = {}                        # name -> LRBMS_OPT_* / LRBMS3_OPT_* of the C header
    TIMING_CAP = None                   # kernel_timing_read: timed kernels returned per read
    _load = None                        # staticmethod: the loader that binds the C symbols of the subclass

    def __init__(self, device_index=0):
        import torch
        self.torch = torch
        if not torch.cuda.is_available():
            raise NativeError('no HIP device visible: the LRBMS hot path has no CPU fallback')
        self.lib = self._load()
        self.device = torch.device('cuda', device_index)
        handle = c_vp()
        rc = self._fn('ctx_create')(device_index, ctypes.byref(handle))
        if rc != 0:
            raise NativeError('{}ctx_create failed with code {}'.format(self.PREFIX, rc))
        self.handle = handle
        self._pid = os.getpid()

    def _fn(self, name):
        return getattr(self.lib, self.PREFIX + name)

    def close(self):
        if getattr(self, 'handle', None):
            # a fork()ed child (e.g. a multiprocessing manager started after the GPU was initialised) inherits this
            # object but not the device context behind it: freeing the parent's allocations from there aborts the process
            if getattr(self, '_pid', None) == os.getpid():
                self._fn('ctx_destroy')(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ helpers
    def _check(self, rc, what):
        if rc != 0:
            msg = self._fn('last_error')(self.handle)
            raise NativeError('{} failed ({}): {}'.format(what, rc, msg.decode() if msg else ''))

    def _stream(self):
        return c_vp(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _ptr(self, t, shape, name):
        torch = self.torch
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.device != self.device:
            raise NativeError('{}: expected a float64 tensor on {}'.format(name, self.device))
        if tuple(t.shape) != tuple(shape):
            raise NativeError('{}: expected shape {}, got {}'.format(name, tuple(shape), tuple(t.shape)))
        if not t.is_contiguous():
            raise NativeError('{}: tensor must be contiguous'.format(name))
        return c_vp(t.data_ptr())

    def empty(self, *shape):
        return self.torch.empty(*shape, dtype=self.torch.float64, device=self.device)

    def zeros(self, *shape):
        return self.torch.zeros(*shape, dtype=self.torch.float64, device=self.device)

    def from_numpy(self, a):
        return self.torch.from_numpy(np.array(a, dtype=np.float64, order='C', copy=True)).to(self.device)

    def _local_pod(self, P_ptr, U, V, nloc, modes, rtol, atol, work=None):
        """``lrbms_local_pod`` / ``lrbms3_local_pod`` on the current stream.  ``U`` [S, n, L], ``V`` [S or S_ext, n, Nw] (its free
        columns are filled in place; rows past S are a halo the call leaves alone), ``nloc`` int32 device tensor [S] (in / out),
        ``work``: at least ``local_pod_work_size(L, Nw)`` doubles (default: allocated here).  Returns the device tensors ``sv`` [S, L] and
        ``ai`` int32 [2, S] (row 0 ``added``, row 1 ``info``); nothing is copied to the host here."""
        torch = self.torch
        S, n = self.S, self.n
        L, Nw = int(U.shape[2]), int(V.shape[2])
        if V.shape[0] < S:
            raise NativeError('V: expected at least {} subdomain rows, got {}'.format(S, V.shape[0]))
        if nloc.dtype != torch.int32 or nloc.device != self.device or tuple(nloc.shape) != (S,) or not nloc.is_contiguous():
            raise NativeError('nloc: expected a contiguous int32 tensor [{}] on {}'.format(S, self.device))
        u_ptr, v_ptr = self._ptr(U, (S, n, L), 'U'), self._ptr(V, (V.shape[0], n, Nw), 'V')
        size = self.local_pod_work_size(L, Nw)
        if work is None:
            work = self.empty(size) if size > 0 else None      # (a refused shape: the call below says why)
        elif work.dtype != torch.float64 or work.device != self.device or not work.is_contiguous() or work.numel() < max(size, 1):
            raise NativeError('work: expected a contiguous float64 tensor of at least {} elements on {}'.format(size, self.device))
        sv = self.empty(S, L)
        ai = torch.empty(2, S, dtype=torch.int32, device=self.device)
        rc = self._fn('local_pod')(self.handle, L, Nw, int(modes), float(rtol), float(atol), P_ptr, u_ptr, v_ptr, c_vp(nloc.data_ptr()),
                                   c_vp(sv.data_ptr()), c_vp(ai[0].data_ptr()), c_vp(ai[1].data_ptr()),
                                   c_vp(work.data_ptr()) if work is not None else None, self._stream())
        self._check(rc, self.PREFIX + 'local_pod')
        return sv, ai

    def local_pod_work_size(self, L, Nw):
        """Doubles of ``work`` for ``local_pod`` (the formula of the C header), -1 for a shape the call refuses."""
        return int(self._fn('local_pod_work_size')(self.handle, int(L), int(Nw)))

    def _pod_product_ptr(self, P_diag):
        """The checked pointer of the local product in the layout of the subclass."""
        raise NotImplementedError

    def local_pod_stream(self, P_diag, V, nloc, keep=64, cmax=64):
        """A streamed local POD (``lrbms_local_pod_stream_*`` / ``lrbms3_local_pod_stream_*``, incremental HAPOD) against the
        basis slab ``V`` [S or S_ext, n, Nw] with ``nloc`` (int32 device tensor [S]): a ``LocalPodStream``, begun.  ``V`` and ``nloc``
        must not change until its ``finish``."""
        return LocalPodStream(self, P_diag, V, nloc, keep, cmax)

    def set_option(self, name, value):
        """Set one entry of ``OPTIONS``: a convention the reference tree leaves open or the launch policy of the library
        (LRBMS_OPT_* / LRBMS3_OPT_* of the C headers); the library reads no environment variable."""
        if name not in self.OPTIONS:
            raise NativeError('unknown option {!r}; known: {}'.format(name, sorted(self.OPTIONS)))
        self._check(self._fn('ctx_set_option')(self.handle, self.OPTIONS[name], int(value)), self.PREFIX + 'ctx_set_option')

    def kernel_timing(self, enable):
        """Bracket every kernel of the pass by HIP events on its own stream (measurement only)."""
        self._check(self._fn('kernel_timing')(self.handle, 1 if enable else 0), self.PREFIX + 'kernel_timing')

    def kernel_timing_read(self, cap=None):
        """[(kernel name, milliseconds)] of the passes since the last read, at most ``cap`` of them (synchronises the device)."""
        cap = self.TIMING_CAP if cap is None else int(cap)
        names = ctypes.create_string_buffer(64 * cap)
        ms = (c_dbl * cap)()
        count = c_i32(0)
        self._check(self._fn('kernel_timing_read')(self.handle, names, 64 * cap, ms, cap, ctypes.byref(count)),
                    self.PREFIX + 'kernel_timing_read')
        nm = names.value.decode().split('\n') if count.value else []
        return [(nm[i], ms[i]) for i in range(count.value)]


class LocalPodStream:
    """One ``begin .. push .. finish`` of the streamed local POD on a context.  ``state`` and ``work`` are allocated once, here;
    every call runs on the current stream and copies nothing to the host."""

    def __init__(self, ctx, P_diag, V, nloc, keep=64, cmax=64):
        torch = ctx.torch
        self.ctx, self.keep, self.cmax = ctx, int(keep), int(cmax)
        S, n = ctx.S, ctx.n
        if V.dim() != 3 or V.shape[0] < S:
            raise NativeError('V: expected [at least {} subdomain rows, n, Nw], got {}'.format(S, tuple(V.shape)))
        if nloc.dtype != torch.int32 or nloc.device != ctx.device or tuple(nloc.shape) != (S,) or not nloc.is_contiguous():
            raise NativeError('nloc: expected a contiguous int32 tensor [{}] on {}'.format(S, ctx.device))
        self.Nw = int(V.shape[2])
        self._P, self._P_ptr = P_diag, ctx._pod_product_ptr(P_diag)
        self._V, self._v_ptr = V, ctx._ptr(V, (V.shape[0], n, self.Nw), 'V')
        self._nloc = nloc
        self.columns = self.nodes = 0
        ssize = int(ctx._fn('local_pod_stream_state_size')(ctx.handle, self.keep, self.cmax))
        wsize = int(ctx._fn('local_pod_stream_work_size')(ctx.handle, self.keep, self.cmax, self.Nw))
        self.state = ctx.empty(ssize) if ssize > 0 else None        # (a refused shape: begin / push say why)
        self.work = ctx.empty(wsize) if wsize > 0 else None
        self.begin()

    def _p(self, t):
        return c_vp(t.data_ptr()) if t is not None else None

    def begin(self):
        """Reset the state: no carried modes, nothing lost."""
        ctx = self.ctx
        rc = ctx._fn('local_pod_stream_begin')(ctx.handle, self.keep, self.cmax, self._p(self.state), ctx._stream())
        ctx._check(rc, ctx.PREFIX + 'local_pod_stream_begin')
        self.columns = self.nodes = 0

    def push(self, U):
        """Push the snapshots ``U`` [S, n, C]; more than ``cmax`` columns go piece by piece (one ``.contiguous()`` per piece)."""
        ctx = self.ctx
        if U.dim() != 3 or U.shape[2] < 1:
            raise NativeError('U: expected [S, n, C >= 1], got {}'.format(tuple(U.shape)))
        for c0 in range(0, int(U.shape[2]), max(self.cmax, 1)):
            Uc = U[:, :, c0:c0 + max(self.cmax, 1)].contiguous()
            C = int(Uc.shape[2])
            rc = ctx._fn('local_pod_stream_push')(ctx.handle, self.keep, self.cmax, C, self.Nw, self._P_ptr,
                                                  ctx._ptr(Uc, (ctx.S, ctx.n, C), 'U'), self._v_ptr, self._p(self._nloc),
                                                  self._p(self.state), self._p(self.work), ctx._stream())
            ctx._check(rc, ctx.PREFIX + 'local_pod_stream_push')
            self.columns += C
            self.nodes += 1

    def finish(self, modes, rtol=1e-6, atol=0.0):
        """At most ``modes`` modes of everything pushed into the free columns of ``V`` (``nloc`` += added).  Returns the device
        tensors ``sv`` [S, keep], ``ai`` int32 [2, S] (row 0 ``added``, row 1 ``info``) and ``lost`` [S]."""
        ctx = self.ctx
        torch = ctx.torch
        sv = ctx.empty(ctx.S, max(self.keep, 1))
        ai = torch.empty(2, ctx.S, dtype=torch.int32, device=ctx.device)
        lost = ctx.empty(ctx.S)
        rc = ctx._fn('local_pod_stream_finish')(ctx.handle, self.keep, self.cmax, self.Nw, int(modes), float(rtol), float(atol),
                                                self._P_ptr, self._v_ptr, self._p(self._nloc), self._p(self.state), self._p(sv),
                                                self._p(ai[0]), self._p(ai[1]), self._p(lost), self._p(self.work), ctx._stream())
        ctx._check(rc, ctx.PREFIX + 'local_pod_stream_finish')
        return sv, ai, lost


class NativeContext(ContextBase):
    """One lrbms_ctx per (process, device).  Tensor arguments must be contiguous float64 CUDA tensors on that device;
    shapes are checked here, on the host, before any kernel may dereference them."""

    PREFIX = 'lrbms_'
    TIMING_CAP = 256
    _load = staticmethod(load_library)
    OPTIONS = {'oswald_zero_on_subdomain_boundary': 1, 'accumulate_coupling_across_q': 2, 'oswald_vertex_patch': 9, 'prep_lds': 10,
               # launch policy (no numerical convention): the library reads no environment variable
               'streams': 3, 'f1_ksplit': 4, 'f1_form': 5, 'coarse': 6, 'solve_valu': 7, 'estimate_valu': 8,
               'f2_form': 11,      # f2_form: 0 Gram form (column-pair producers), 1 product form k_f2, 2 Gram form with one-column producers
               'side_tables': 12,  # 1: basis-independent tables of the pass kept between passes; 0: rebuilt in every pass (arrays modified in place)
               'thin_merge': 13,   # 1: k_thin3; 0: k_thin_ncf, k_thin_rt, k_coupling one after the other in the factored layout (cross-check)
               'pod_rotate_valu': 14}   # 1: the rotation of local_pod_stream.push through k_pod_xt (cross-check of k_pod_stream_rotate)
    S = S_ext = None
    _keep = None

    # ------------------------------------------------------------------ mesh
    def mesh_upload(self, template, kappa, nbr, S, S_ext):
        t = template
        self.t, self.S, self.S_ext = t, int(S), int(S_ext)
        self.n_T, self.n, self.n_rt, self.ncf = t.n_T, t.n, t.n_rt, t.ncf
        self.nvs = max(t.nvx, t.nvy)
        arrs = {}
        d = MeshDesc()
        d.kx, d.ky, d.n_T, d.n_rt, d.n_vertices, d.ncf = t.kx, t.ky, t.n_T, t.n_rt, t.n_vertices, t.ncf
        d.hx, d.hy = t.hx, t.hy
        d.ntouch = t.ntouch
        kap = np.asarray(kappa, dtype=np.float64).reshape(4)
        for i in range(4):
            d.kappa[i] = kap[i]
        for k in ('nb_elem', 'nb_face', 'nb_elem_out', 'nb_face_out', 'elem_side_pos', 'elem_rt', 'face_sign',
                  'dof_vertex', 'vdof_ptr', 'vdof_idx', 'rt_e0', 'rt_f0', 'rt_e1', 'rt_f1', 'rt_side', 'side_elem',
                  'side_elem_out', 'side_count', 'touch_elem', 'touch_count'):
            arrs[k] = np.ascontiguousarray(getattr(t, k), dtype=np.int32)
            setattr(d, k, _i32p(arrs[k]))
        for k in ('grad', 'area', 'normal', 'face_len', 'points'):
            arrs[k] = np.ascontiguousarray(getattr(t, k), dtype=np.float64)
            setattr(d, k, _dblp(arrs[k]))
        nb = np.ascontiguousarray(nbr, dtype=np.int32)
        assert nb.shape == (S, 5)
        rc = self.lib.lrbms_mesh_upload(self.handle, ctypes.byref(d), S, S_ext, _i32p(nb))
        self._keep = (arrs, nb)
        self._check(rc, 'lrbms_mesh_upload')
        self._pins = {}                 # (the upload has emptied the context's register of assembled arrays)

    # ------------------------------------------------------------------ assembly
    def set_quadrature(self, spec):
        """Upload the rules of a ``pylrbms_amd.quadrature.QuadratureSpec`` (must precede the assembly calls; after a mesh
        upload).  Keeps the native struct: its o_* / *_stride fields are the sample record layout the host fills."""
        from pylrbms_amd.quadrature import native_quadrature
        self.quad = native_quadrature(spec)
        self.quad_spec = spec
        self._check(self.lib.lrbms_set_quadrature(self.handle, ctypes.byref(self.quad)), 'lrbms_set_quadrature')

    def _quad(self):
        if getattr(self, 'quad', None) is None:
            raise NativeError('set_quadrature() must run before the assembly calls')
        return self.quad

    def assemble_swipdg(self, lam):
        Q, qd = lam.shape[0], self._quad()
        A_diag = self.empty(Q, self.S, self.n_T, 4, 9)
        A_cpl = self.empty(Q, self.S, 4, self.ncf, 9)
        rc = self.lib.lrbms_assemble_swipdg(self.handle, Q, self._ptr(lam, (Q, self.S_ext, self.n_T, qd.lam_stride), 'lam'),
                                            c_vp(A_diag.data_ptr()), c_vp(A_cpl.data_ptr()), self._stream())
        self._check(rc, 'lrbms_assemble_swipdg')
        return A_diag, A_cpl

    def _out(self, out, shapes):
        """The output tensors of an assembly export: fresh ones, or ``out`` (written in place) after a shape check."""
        if out is None:
            return tuple(self.empty(*shape) for shape in shapes)
        assert len(out) == len(shapes)
        for x, shape in zip(out, shapes):
            self._ptr(x, shape, 'out')
        return tuple(out)

    def _pin_assembled(self, written):
        """Hold a reference to the arrays an assembly export has just written (``written``: kind of ``lrbms_assembled_arrays`` ->
        tensor) and let go of every array the context's register has dropped: pins and register hold the same addresses."""
        pins = self.__dict__.setdefault('_pins', {})
        for kind, x in written.items():
            pins[(kind, x.data_ptr())] = x
        cap = 64
        buf = (c_vp * cap)()
        live = set()
        for kind in range(4):
            n = self.lib.lrbms_assembled_arrays(self.handle, kind, buf, cap)
            if n < 0 or n > cap:
                raise NativeError('lrbms_assembled_arrays: {}'.format(n))
            live.update((kind, int(buf[i] or 0)) for i in range(n))
        for key in [k for k in pins if k not in live]:
            del pins[key]

    def assemble_rhs(self, f_smp, lhat, out=None):
        """``out``: (b, f2, ceps) of an earlier call, re-assembled in place.  The context keeps tables derived from the
        assembled arrays between fused passes (option ``side_tables``) and registers their addresses; the binding holds a
        reference to exactly the registered arrays (``_pin_assembled``), so that a registered address cannot pass to another
        tensor.  Arrays modified by other means than these calls need ``side_tables`` 0."""
        qd = self._quad()
        b, f2, ceps = self._out(out, [(self.S, self.n), (self.S,), (self.S,)])
        rc = self.lib.lrbms_assemble_rhs(self.handle, self._ptr(f_smp, (self.S, self.n_T, qd.f_stride), 'f_smp'),
                                         self._ptr(lhat, (self.S, self.n_T, qd.lhat_stride), 'lhat'), c_vp(b.data_ptr()),
                                         c_vp(f2.data_ptr()), c_vp(ceps.data_ptr()), self._stream())
        self._check(rc, 'lrbms_assemble_rhs')
        self._pin_assembled({2: b})
        return b, f2, ceps

    def assemble_products(self, theta_bar, lam, lam_df, lbar, lhat, out=None):
        Q, qd = lam.shape[0], self._quad()
        th = np.ascontiguousarray(theta_bar, dtype=np.float64)
        assert th.shape == (Q,)
        P_diag, ebar, caa, Aab, Bbb = self._out(out, [(self.S, self.n_T, 4, 9), (self.S, self.n_T), (Q, Q, self.S, self.n_T),
                                                      (Q, self.S, self.n_T, 3, 3), (self.S, self.n_T, 3, 3)])
        rc = self.lib.lrbms_assemble_products(
            self.handle, Q, _dblp(th), self._ptr(lam, (Q, self.S_ext, self.n_T, qd.lam_stride), 'lam'),
            self._ptr(lam_df, (Q, self.S, self.n_T, qd.lamdf_stride), 'lam_df'),
            self._ptr(lbar, (self.S, self.n_T, qd.lbar_stride), 'lbar'), self._ptr(lhat, (self.S, self.n_T, qd.lhat_stride), 'lhat'),
            c_vp(P_diag.data_ptr()), c_vp(ebar.data_ptr()), c_vp(caa.data_ptr()), c_vp(Aab.data_ptr()),
            c_vp(Bbb.data_ptr()), self._stream())
        self._check(rc, 'lrbms_assemble_products')
        self._pin_assembled({0: Bbb, 1: Aab, 3: ebar})
        return P_diag, ebar, caa, Aab, Bbb

    def assemble_flux(self, lam):
        Q, qd = lam.shape[0], self._quad()
        F = self.empty(Q, self.S, self.n_rt, 6)
        rc = self.lib.lrbms_assemble_flux(self.handle, Q, self._ptr(lam, (Q, self.S_ext, self.n_T, qd.lam_stride), 'lam'),
                                          c_vp(F.data_ptr()), self._stream())
        self._check(rc, 'lrbms_assemble_flux')
        return F

    # ------------------------------------------------------------------ project + estimate-offline
    def oswald_apply(self, V, out=None):
        N = V.shape[2]
        Wt = out if out is not None else self.empty(self.S, self.n, 5 * N)
        rc = self.lib.lrbms_oswald_apply(self.handle, N, self._ptr(V, (self.S_ext, self.n, N), 'V'),
                                         self._ptr(Wt, (self.S, self.n, 5 * N), 'Wt'), self._stream())
        self._check(rc, 'lrbms_oswald_apply')
        return Wt

    def flux_reconstruct(self, F, V, out=None):
        Q, N = F.shape[0], V.shape[2]
        Rt = out if out is not None else self.empty(self.S, self.n_rt, 5 * Q * N)
        rc = self.lib.lrbms_flux_reconstruct(self.handle, Q, N, self._ptr(F, (Q, self.S, self.n_rt, 6), 'F'),
                                             self._ptr(V, (self.S_ext, self.n, N), 'V'),
                                             self._ptr(Rt, (self.S, self.n_rt, 5 * Q * N), 'Rt'), self._stream())
        self._check(rc, 'lrbms_flux_reconstruct')
        return Rt

    def project_system(self, V, A_diag, A_cpl, P_diag, b, work=None, out=None):
        Q, N, S = A_diag.shape[0], V.shape[2], self.S
        if work is None:
            work = self.empty(Q * S * self.n * N)
        if work.numel() < Q * S * self.n * N:
            raise NativeError('project_system: work too small')
        if out is None:
            out = (self.empty(Q, S, 5, N, N), self.empty(S, N), self.empty(S, N, N), self.empty(S, N, N))
        B_sys, rhs_red, E_red, M_red = out
        rc = self.lib.lrbms_project_system(
            self.handle, Q, N, self._ptr(V, (self.S_ext, self.n, N), 'V'),
            self._ptr(A_diag, (Q, S, self.n_T, 4, 9), 'A_diag'), self._ptr(A_cpl, (Q, S, 4, self.ncf, 9), 'A_cpl'),
            self._ptr(P_diag, (S, self.n_T, 4, 9), 'P_diag'), self._ptr(b, (S, self.n), 'b'), c_vp(work.data_ptr()),
            self._ptr(B_sys, (Q, S, 5, N, N), 'B_sys'), self._ptr(rhs_red, (S, N), 'rhs_red'),
            self._ptr(E_red, (S, N, N), 'E_red'), self._ptr(M_red, (S, N, N), 'M_red'), self._stream())
        self._check(rc, 'lrbms_project_system')
        return B_sys, rhs_red, E_red, M_red

    def estimator_work_size(self, Q, N):
        sz = self.lib.lrbms_estimator_work_size(self.handle, Q, N)
        if sz < 0:
            raise NativeError('lrbms_estimator_work_size failed')
        return int(sz)

    def estimator_grams(self, V, Wt, Rt, ebar, caa, Aab, Bbb, b, work=None, out=None):
        Q, N, S = caa.shape[0], V.shape[2], self.S
        W, C = 5 * N, 5 * Q * N
        need = self.estimator_work_size(Q, N)
        if work is None:
            work = self.empty(need)
        if work.numel() < need:
            raise NativeError('estimator_grams: work too small')
        if out is None:
            out = (self.empty(S, W, W), self.empty(S, C), self.empty(S, 9, Q * N, Q * N), self.empty(S, 9, Q * N, Q * N),
                   self.empty(Q, S, N, C), self.empty(Q, Q, S, N, N))
        G_nc, r_fd, G_rdd, G_bb, G_ab, G_aa = out
        rc = self.lib.lrbms_estimator_grams(
            self.handle, Q, N, self._ptr(V, (self.S_ext, self.n, N), 'V'), self._ptr(Wt, (S, self.n, W), 'Wt'),
            self._ptr(Rt, (S, self.n_rt, C), 'Rt'), self._ptr(ebar, (S, self.n_T), 'ebar'),
            self._ptr(caa, (Q, Q, S, self.n_T), 'caa'), self._ptr(Aab, (Q, S, self.n_T, 3, 3), 'Aab'),
            self._ptr(Bbb, (S, self.n_T, 3, 3), 'Bbb'), self._ptr(b, (S, self.n), 'b'), c_vp(work.data_ptr()),
            self._ptr(G_nc, (S, W, W), 'G_nc'), self._ptr(r_fd, (S, C), 'r_fd'), self._ptr(G_rdd, (S, 9, Q * N, Q * N), 'G_rdd'),
            self._ptr(G_bb, (S, 9, Q * N, Q * N), 'G_bb'), self._ptr(G_ab, (Q, S, N, C), 'G_ab'),
            self._ptr(G_aa, (Q, Q, S, N, N), 'G_aa'), self._stream())
        self._check(rc, 'lrbms_estimator_grams')
        return G_nc, r_fd, G_rdd, G_bb, G_ab, G_aa

    def fused_supported(self, Q, N, factored=False):
        """Whether the fused pass runs this (template, Q, N) with the dense (default) or the factored output layout."""
        fn = self.lib.lrbms_fused_factored_supported if factored else self.lib.lrbms_fused_supported
        return bool(fn(self.handle, Q, N))

    def fused_work_size(self, Q, N):
        sz = self.lib.lrbms_fused_work_size(self.handle, Q, N)
        if sz < 0:
            raise NativeError('lrbms_fused_work_size failed')
        return int(sz)

    def fside_ld(self, Q, N):
        return 4 * Q * N + 4

    def fnc_ld(self, N):
        """Row length of F_nc [S, 4, nvs, .]: A_a | C_a | M_a0 .. M_a3 (| A_diag with the vertex-patch option) (include/lrbms_hip.h)."""
        return int(self.lib.lrbms_fused_fnc_ld(self.handle, int(N)))

    def _gram_ptrs(self, grams, Q, N):
        """Pointers of the projected estimator operators in either layout: 6 tensors = dense (G_rdd / G_bb block-compact
        [S, 9, QN, QN], G_ab [Q, S, N, 5QN]); 8 tensors = factored (self parts [S, N, N] / [S, QN, QN] / [Q, S, N, QN] +
        F_side [S, 4, ncf, 4QN + 4] + F_nc [S, 4, nvs, 2N + 4nvs], include/lrbms_hip.h).  Returns (pointer list, factored flag)."""
        S, W, C, QN = self.S, 5 * N, 5 * Q * N, Q * N
        if len(grams) == 8:
            G_nc, r_fd, G_rdd, G_bb, G_ab, G_aa, Fs, Fn = grams
            return [self._ptr(G_nc, (S, N, N), 'G_nc_self'), self._ptr(r_fd, (S, C), 'r_fd'), self._ptr(G_rdd, (S, QN, QN), 'G_rdd_self'),
                    self._ptr(G_bb, (S, QN, QN), 'G_bb_self'), self._ptr(G_ab, (Q, S, N, QN), 'G_ab_self'),
                    self._ptr(G_aa, (Q, Q, S, N, N), 'G_aa'), self._ptr(Fs, (S, 4, self.ncf, self.fside_ld(Q, N)), 'F_side'),
                    self._ptr(Fn, (S, 4, self.nvs, self.fnc_ld(N)), 'F_nc')], True
        G_nc, r_fd, G_rdd, G_bb, G_ab, G_aa = grams
        return [self._ptr(G_nc, (S, W, W), 'G_nc'), self._ptr(r_fd, (S, C), 'r_fd'), self._ptr(G_rdd, (S, 9, QN, QN), 'G_rdd'),
                self._ptr(G_bb, (S, 9, QN, QN), 'G_bb'), self._ptr(G_ab, (Q, S, N, C), 'G_ab'),
                self._ptr(G_aa, (Q, Q, S, N, N), 'G_aa')], False

    def project_estimate_fused(self, V, F, A_diag, A_cpl, P_diag, b, ebar, caa, Aab, Bbb, work, sys_out, gram_out, phase=0):
        """phase 0: the whole pass; 1 / 2: its halo-independent / halo-dependent halves (lrbms_project_estimate_fused_phase)."""
        Q, N, S = A_diag.shape[0], V.shape[2], self.S
        W, C = 5 * N, 5 * Q * N
        if work.numel() < self.fused_work_size(Q, N):
            raise NativeError('project_estimate_fused: work too small')
        B_sys, rhs_red, E_red, M_red = sys_out
        gptrs, factored = self._gram_ptrs(gram_out, Q, N)
        fn = self.lib.lrbms_project_estimate_fused_factored if factored else self.lib.lrbms_project_estimate_fused_phase
        rc = fn(
            self.handle, int(phase), Q, N, self._ptr(V, (self.S_ext, self.n, N), 'V'), self._ptr(F, (Q, S, self.n_rt, 6), 'F'),
            self._ptr(A_diag, (Q, S, self.n_T, 4, 9), 'A_diag'), self._ptr(A_cpl, (Q, S, 4, self.ncf, 9), 'A_cpl'),
            self._ptr(P_diag, (S, self.n_T, 4, 9), 'P_diag'), self._ptr(b, (S, self.n), 'b'),
            self._ptr(ebar, (S, self.n_T), 'ebar'), self._ptr(caa, (Q, Q, S, self.n_T), 'caa'),
            self._ptr(Aab, (Q, S, self.n_T, 3, 3), 'Aab'), self._ptr(Bbb, (S, self.n_T, 3, 3), 'Bbb'),
            c_vp(work.data_ptr()), self._ptr(B_sys, (Q, S, 5, N, N), 'B_sys'), self._ptr(rhs_red, (S, N), 'rhs_red'),
            self._ptr(E_red, (S, N, N), 'E_red'), self._ptr(M_red, (S, N, N), 'M_red'), *gptrs, self._stream())
        self._check(rc, 'lrbms_project_estimate_fused_phase')

    def bind_project_estimate_fused(self, V, F, A_diag, A_cpl, P_diag, b, ebar, caa, Aab, Bbb, work, sys_out, gram_out):
        """The same call with the argument checks and the pointer marshalling done ONCE: returns ``run(phase=0)``.  A
        sharded step makes three library calls on ~0.2 ms of device work; checking 23 tensors per call made the host
        the slower side.  The closure keeps the tensors alive; it must not outlive a change of their storage."""
        Q, N, S = A_diag.shape[0], V.shape[2], self.S
        W, C = 5 * N, 5 * Q * N
        if work.numel() < self.fused_work_size(Q, N):
            raise NativeError('project_estimate_fused: work too small')
        B_sys, rhs_red, E_red, M_red = sys_out
        gptrs, factored = self._gram_ptrs(gram_out, Q, N)
        ptrs = (self._ptr(V, (self.S_ext, self.n, N), 'V'), self._ptr(F, (Q, S, self.n_rt, 6), 'F'),
                self._ptr(A_diag, (Q, S, self.n_T, 4, 9), 'A_diag'), self._ptr(A_cpl, (Q, S, 4, self.ncf, 9), 'A_cpl'),
                self._ptr(P_diag, (S, self.n_T, 4, 9), 'P_diag'), self._ptr(b, (S, self.n), 'b'),
                self._ptr(ebar, (S, self.n_T), 'ebar'), self._ptr(caa, (Q, Q, S, self.n_T), 'caa'),
                self._ptr(Aab, (Q, S, self.n_T, 3, 3), 'Aab'), self._ptr(Bbb, (S, self.n_T, 3, 3), 'Bbb'),
                c_vp(work.data_ptr()), self._ptr(B_sys, (Q, S, 5, N, N), 'B_sys'), self._ptr(rhs_red, (S, N), 'rhs_red'),
                self._ptr(E_red, (S, N, N), 'E_red'), self._ptr(M_red, (S, N, N), 'M_red')) + tuple(gptrs)
        keep = (V, F, A_diag, A_cpl, P_diag, b, ebar, caa, Aab, Bbb, work, sys_out, gram_out)
        fn = self.lib.lrbms_project_estimate_fused_factored if factored else self.lib.lrbms_project_estimate_fused_phase
        handle, cur, dev = self.handle, self.torch.cuda.current_stream, self.device

        def run(phase=0, stream=None, _keep=keep):      # stream: a raw HIP stream handle (default: torch's current stream)
            rc = fn(handle, phase, Q, N, *ptrs, c_vp(cur(dev).cuda_stream if stream is None else stream))
            if rc != 0:
                self._check(rc, 'lrbms_project_estimate_fused_phase')
        return run

    # ------------------------------------------------------------------ online
    def reduced_estimate(self, theta, u, grams, f2, ceps, hdiam):
        Q, S, N = grams[4].shape[0], self.S, grams[4].shape[2]
        th = np.ascontiguousarray(theta, dtype=np.float64)
        assert th.shape == (Q,)
        eta = self.empty(3, S)
        gptrs, factored = self._gram_ptrs(grams, Q, N)
        fn = self.lib.lrbms_reduced_estimate_factored if factored else self.lib.lrbms_reduced_estimate
        rc = fn(self.handle, Q, N, _dblp(th), self._ptr(u, (self.S_ext, N), 'u'), *gptrs, self._ptr(f2, (S,), 'f2'),
                self._ptr(ceps, (S,), 'ceps'), float(hdiam), c_vp(eta.data_ptr()), self._stream())
        self._check(rc, 'lrbms_reduced_estimate')
        return eta

    def reduced_estimate_batch(self, thetas, u, grams, f2, ceps, hdiam):
        """thetas [nmu, Q], u [S_ext, N, nmu] -> eta_loc [3, S, nmu]."""
        Q, S, N = grams[4].shape[0], self.S, grams[4].shape[2]
        th = np.ascontiguousarray(thetas, dtype=np.float64)
        nmu = th.shape[0]
        assert th.shape == (nmu, Q)
        eta = self.empty(3, S, nmu)
        gptrs, factored = self._gram_ptrs(grams, Q, N)
        fn = self.lib.lrbms_reduced_estimate_batch_factored if factored else self.lib.lrbms_reduced_estimate_batch
        rc = fn(self.handle, Q, N, nmu, _dblp(th), self._ptr(u, (self.S_ext, N, nmu), 'u'), *gptrs, self._ptr(f2, (S,), 'f2'),
                self._ptr(ceps, (S,), 'ceps'), float(hdiam), c_vp(eta.data_ptr()), self._stream())
        self._check(rc, 'lrbms_reduced_estimate_batch')
        return eta

    def reduced_solve(self, theta, B_sys, rhs_red, rtol=1e-13, max_iter=20000, work=None):
        Q, S, N = B_sys.shape[0], self.S, B_sys.shape[3]
        th = np.ascontiguousarray(theta, dtype=np.float64)
        assert th.shape == (Q,)
        need = int(self.lib.lrbms_reduced_solve_work_size(self.handle, N))
        if work is None:
            work = self.empty(need)
        if work.numel() < need:
            raise NativeError('reduced_solve: work too small')
        u = self.empty(S, N)
        info = np.zeros(2)
        rc = self.lib.lrbms_reduced_solve(self.handle, Q, N, _dblp(th), self._ptr(B_sys, (Q, S, 5, N, N), 'B_sys'),
                                          self._ptr(rhs_red, (S, N), 'rhs_red'), c_vp(work.data_ptr()),
                                          c_vp(u.data_ptr()), float(rtol), int(max_iter), _dblp(info), self._stream())
        self._check(rc, 'lrbms_reduced_solve')
        return u, {'iterations': int(info[0]), 'relative_residual': float(info[1])}

    def reduced_solve_batch(self, thetas, B_sys, rhs_red, rtol=1e-13, max_iter=20000, work=None):
        """thetas [nmu, Q] -> u [S, N, nmu] (mu fastest), info."""
        Q, S, N = B_sys.shape[0], self.S, B_sys.shape[3]
        th = np.ascontiguousarray(thetas, dtype=np.float64)
        nmu = th.shape[0]
        assert th.shape == (nmu, Q)
        need = int(self.lib.lrbms_reduced_solve_batch_work_size(self.handle, N, nmu))
        if work is None:
            work = self.empty(need)
        if work.numel() < need:
            raise NativeError('reduced_solve_batch: work too small')
        u = self.empty(S, N, nmu)
        info = np.zeros(2)
        rc = self.lib.lrbms_reduced_solve_batch(self.handle, Q, N, nmu, _dblp(th), self._ptr(B_sys, (Q, S, 5, N, N), 'B_sys'),
                                                self._ptr(rhs_red, (S, N), 'rhs_red'), c_vp(work.data_ptr()),
                                                c_vp(u.data_ptr()), float(rtol), int(max_iter), _dblp(info), self._stream())
        self._check(rc, 'lrbms_reduced_solve_batch')
        return u, {'iterations': int(info[0]), 'relative_residual': float(info[1])}

    def reduced_solve_batches(self, thetas, B_sys, rhs_red, per_call=64, rtol=1e-13, max_iter=20000, concat=True):
        """Parameter sweep: thetas [nmu, Q] for any nmu -> u [S, N, nmu] (``concat=False``: the list of per-call arrays
        [S, N, <= per_call], no copy), info.  ``lrbms_reduced_solve_batch`` takes up to 64 parameters per call and runs them as
        (<= 4) groups of 16 on the caller's stream and the library's side streams itself -- no host threads, one caller per
        context (include/lrbms_hip.h: a ctx is not re-entrant)."""
        torch = self.torch
        th = np.ascontiguousarray(thetas, dtype=np.float64)
        per_call = max(1, min(int(per_call), 64))
        work = self.empty(int(self.lib.lrbms_reduced_solve_batch_work_size(self.handle, int(B_sys.shape[3]), min(per_call, th.shape[0]))))
        res = [self.reduced_solve_batch(th[b0:b0 + per_call], B_sys, rhs_red, rtol=rtol, max_iter=max_iter, work=work)
               for b0 in range(0, th.shape[0], per_call)]
        if concat:
            u = torch.cat([r[0] for r in res], dim=2) if len(res) > 1 else res[0][0]
        else:
            u = [r[0] for r in res]
        return u, {'iterations': max(r[1]['iterations'] for r in res), 'relative_residual': max(r[1]['relative_residual'] for r in res)}

    def reduced_precond_build(self, theta, B_sys):
        """Two-level preconditioner of the reduced solves at the reference parameter ``theta`` -> device buffer."""
        Q, S, N = B_sys.shape[0], self.S, B_sys.shape[3]
        th = np.ascontiguousarray(theta, dtype=np.float64)
        assert th.shape == (Q,)
        work = self.empty(int(self.lib.lrbms_reduced_solve_work_size(self.handle, N)))
        pc = self.empty(int(self.lib.lrbms_reduced_precond_size(self.handle, N)))
        rc = self.lib.lrbms_reduced_precond_build(self.handle, Q, N, _dblp(th), self._ptr(B_sys, (Q, S, 5, N, N), 'B_sys'),
                                                  c_vp(work.data_ptr()), c_vp(pc.data_ptr()), self._stream())
        self._check(rc, 'lrbms_reduced_precond_build')
        pc._lrbms_N = N
        return pc

    def reduced_precond_use(self, pc):
        """Subsequent reduced solves use ``pc`` (``None``: per-call preconditioners).  The context keeps a reference."""
        self._pc_in_use = pc
        rc = self.lib.lrbms_reduced_precond_use(self.handle, int(pc._lrbms_N) if pc is not None else 0,
                                                c_vp(pc.data_ptr()) if pc is not None else None)
        self._check(rc, 'lrbms_reduced_precond_use')

    def set_diagonal_neighbours(self, nbr_diag):
        """[S, 4] int32: index into the S_ext slabs of the diagonal neighbour at corner SW, SE, NW, NE of every local subdomain
        (or -1) -- read by the Oswald vertex patch (include/lrbms_hip.h: lrbms_set_diagonal_neighbours)."""
        arr = np.ascontiguousarray(np.asarray(nbr_diag, dtype=np.int32))
        self._check(self.lib.lrbms_set_diagonal_neighbours(self.handle, arr.ctypes.data_as(_P_I32)), 'lrbms_set_diagonal_neighbours')

    def fused_set_subset(self, subset):
        """Restrict the following fused passes to the local subdomains ``subset`` (strictly ascending local indices; ``None`` or
        empty: all) -- incremental re-projection after online enrichment (include/lrbms_hip.h: lrbms_fused_set_subset)."""
        if subset is None or len(subset) == 0:
            self._check(self.lib.lrbms_fused_set_subset(self.handle, None, 0), 'lrbms_fused_set_subset')
            return
        arr = np.ascontiguousarray(np.asarray(subset, dtype=np.int32))
        self._check(self.lib.lrbms_fused_set_subset(self.handle, arr.ctypes.data_as(_P_I32), int(arr.size)), 'lrbms_fused_set_subset')

    def fused_mfma_per_subdomain(self, Q, N):
        """fp64 MFMA instructions the dense projection kernel executes per subdomain (bench.py's roofline)."""
        return int(self.lib.lrbms_fused_mfma_per_subdomain(self.handle, int(Q), int(N)))

    def aux_stream(self, i=0):
        """The i-th library-owned stream as a ``torch.cuda.ExternalStream`` (cached)."""
        cache = self.__dict__.setdefault('_aux_streams', {})
        if i not in cache:
            ptr = self.lib.lrbms_ctx_aux_stream(self.handle, int(i))
            if not ptr:
                raise NativeError('lrbms_ctx_aux_stream({}) returned NULL'.format(i))
            cache[i] = self.torch.cuda.ExternalStream(int(ptr), device=self.device)
        return cache[i]

    # ------------------------------------------------------------------ snapshot generation
    def fom_solve(self, theta, A_diag, A_cpl, b, rtol=1e-12, max_iter=100000):
        """A(mu) x = b for the full-order block operator -> (x [S, n], info)."""
        Q, S = A_diag.shape[0], self.S
        th = np.ascontiguousarray(theta, dtype=np.float64)
        assert th.shape == (Q,)
        work = self.empty(int(self.lib.lrbms_fom_solve_work_size(self.handle)))
        x = self.empty(S, self.n)
        info = np.zeros(2)
        rc = self.lib.lrbms_fom_solve(self.handle, Q, _dblp(th), self._ptr(A_diag, (Q, S, self.n_T, 4, 9), 'A_diag'),
                                      self._ptr(A_cpl, (Q, S, 4, self.ncf, 9), 'A_cpl'), self._ptr(b, (S, self.n), 'b'),
                                      c_vp(work.data_ptr()), c_vp(x.data_ptr()), float(rtol), int(max_iter), _dblp(info),
                                      self._stream())
        self._check(rc, 'lrbms_fom_solve')
        return x, {'iterations': int(info[0]), 'relative_residual': float(info[1])}

    def fom_solve_batch(self, theta, A_diag, A_cpl, phi, b_K, rtol=1e-12, max_iter=100000):
        """Column m: A(theta[m]) x_m = sum_j phi[m][j] b_K[j] for nmu <= 64 parameters in one call (panels of 16 columns, one
        coarse level at the mean theta) -> (X [S, n, nmu], info).  theta [nmu, Q] host; phi [nmu, K] host or device; b_K [K, S, n]."""
        Q, S = A_diag.shape[0], self.S
        th = np.ascontiguousarray(theta, dtype=np.float64)
        nmu = th.shape[0]
        assert th.shape == (nmu, Q)
        if not self.torch.is_tensor(phi):
            phi = self.from_numpy(np.ascontiguousarray(phi, dtype=np.float64))
        K = phi.shape[1]
        size = int(self.lib.lrbms_fom_solve_batch_work_size(self.handle, nmu))
        if size < 0:
            raise NativeError('lrbms_fom_solve_batch: nmu = {} is not in 1..64'.format(nmu))
        work = self.empty(size)
        X = self.empty(S, self.n, nmu)
        info = np.zeros(2)
        rc = self.lib.lrbms_fom_solve_batch(self.handle, Q, nmu, _dblp(th), self._ptr(A_diag, (Q, S, self.n_T, 4, 9), 'A_diag'),
                                            self._ptr(A_cpl, (Q, S, 4, self.ncf, 9), 'A_cpl'), K, self._ptr(phi, (nmu, K), 'phi'),
                                            self._ptr(b_K, (K, S, self.n), 'b_K'), c_vp(work.data_ptr()), c_vp(X.data_ptr()),
                                            float(rtol), int(max_iter), _dblp(info), self._stream())
        panels = np.zeros(8)
        self.lib.lrbms_fom_solve_batch_panel_info(self.handle, _dblp(panels))
        self._check(rc, 'lrbms_fom_solve_batch')
        return X, {'iterations': int(info[0]), 'relative_residual': float(info[1]),
                   'panel_iterations': [int(v) for v in panels[0:2 * ((nmu + 15) // 16):2]]}

    # ------------------------------------------------------------------ parabolic path
    def fom_implicit_euler(self, theta, dt, nt, A_diag, A_cpl, b, U0=None, rtol=1e-12, max_iter=100000):
        """(M + dt A(mu)) u_{k+1} = M u_k + dt b, nt steps -> (U [nt + 1, S, n], info); U0 [S, n] (default 0)."""
        Q, S = A_diag.shape[0], self.S
        th = np.ascontiguousarray(theta, dtype=np.float64)
        assert th.shape == (Q,)
        work = self.empty(int(self.lib.lrbms_fom_solve_work_size(self.handle)))
        U = self.zeros(int(nt) + 1, S, self.n)
        if U0 is not None:
            U[0] = U0.reshape(S, self.n)
        info = np.zeros(2)
        rc = self.lib.lrbms_fom_implicit_euler(self.handle, Q, _dblp(th), float(dt), int(nt),
                                               self._ptr(A_diag, (Q, S, self.n_T, 4, 9), 'A_diag'),
                                               self._ptr(A_cpl, (Q, S, 4, self.ncf, 9), 'A_cpl'), self._ptr(b, (S, self.n), 'b'),
                                               c_vp(work.data_ptr()), c_vp(U.data_ptr()), float(rtol), int(max_iter), _dblp(info),
                                               self._stream())
        self._check(rc, 'lrbms_fom_implicit_euler')
        return U, {'iterations': int(info[0]), 'relative_residual': float(info[1])}

    def fom_implicit_euler_batch(self, thetas, dt, nt, A_diag, A_cpl, b_K, phi, U0=None, rtol=1e-12, max_iter=100000):
        """Column m: (M + dt A(thetas[m])) u_{k+1} = M u_k + dt sum_j phi[m, k + 1, j] b_K[j], nt steps, for nmu <= 64 parameters in
        one call (panels of 16 columns, one coarse level at the mean theta) -> (U [nt + 1, S, n, nmu], info).  thetas [nmu, Q] host;
        phi [nmu, nt + 1, K] host or device; b_K [K, S, n]; U0 [S, n] (every column) or [S, n, nmu] (default 0)."""
        Q, S, K, nt = A_diag.shape[0], self.S, b_K.shape[0], int(nt)
        th = np.ascontiguousarray(thetas, dtype=np.float64)
        nmu = th.shape[0]
        assert th.shape == (nmu, Q)
        if not self.torch.is_tensor(phi):
            phi = self.from_numpy(np.ascontiguousarray(phi, dtype=np.float64))
        phi = phi.contiguous()
        size = int(self.lib.lrbms_fom_implicit_euler_batch_work_size(self.handle, nmu))
        if size < 0:
            raise NativeError('lrbms_fom_implicit_euler_batch: nmu = {} is not in 1..64'.format(nmu))
        work = self.empty(size)
        U = self.zeros(nt + 1, S, self.n, nmu)
        if U0 is not None:
            U[0] = U0.reshape(S, self.n, -1)                     # [S, n, 1] broadcasts over the columns
        info = np.zeros(2)
        rc = self.lib.lrbms_fom_implicit_euler_batch(self.handle, Q, K, nmu, _dblp(th), float(dt), nt,
                                                     self._ptr(A_diag, (Q, S, self.n_T, 4, 9), 'A_diag'),
                                                     self._ptr(A_cpl, (Q, S, 4, self.ncf, 9), 'A_cpl'),
                                                     self._ptr(b_K, (K, S, self.n), 'b_K'), self._ptr(phi, (nmu, nt + 1, K), 'phi'),
                                                     c_vp(work.data_ptr()), c_vp(U.data_ptr()), float(rtol), int(max_iter), _dblp(info),
                                                     self._stream())
        panels = np.zeros(8)
        self.lib.lrbms_fom_implicit_euler_batch_panel_info(self.handle, _dblp(panels))
        self._check(rc, 'lrbms_fom_implicit_euler_batch')
        return U, {'iterations': int(info[0]), 'relative_residual': float(info[1]),
                   'panel_iterations': [int(v) for v in panels[0:2 * ((nmu + 15) // 16):2]]}

    def mass_inverse_norm2(self, Y):
        """Y [S, n, L] -> [S, L]: y^T M^-1 y per subdomain and column."""
        S, L = self.S, Y.shape[2]
        out = self.empty(S, L)
        rc = self.lib.lrbms_mass_inverse_norm2(self.handle, L, self._ptr(Y, (S, self.n, L), 'Y'), c_vp(out.data_ptr()),
                                               self._stream())
        self._check(rc, 'lrbms_mass_inverse_norm2')
        return out

    def div_apply(self, Rt, mode=0):
        """Rt [S, n_rt, C] -> mode 0: div per element [S, n_T, C]; mode 1: M Div Rt [S, n, C]."""
        S, C = self.S, Rt.shape[2]
        out = self.empty(S, self.n_T if mode == 0 else self.n, C)
        rc = self.lib.lrbms_div_apply(self.handle, C, int(mode), self._ptr(Rt, (S, self.n_rt, C), 'Rt'), c_vp(out.data_ptr()),
                                      self._stream())
        self._check(rc, 'lrbms_div_apply')
        return out

    def div_pairing(self, theta, D, G):
        """D [S, n_T, 5 Q L] (div_apply mode 0), G [S, n, L] -> [S, L]: g^T Div U_r."""
        th = np.ascontiguousarray(theta, dtype=np.float64)
        Q, S, L = len(th), self.S, G.shape[2]
        out = self.empty(S, L)
        rc = self.lib.lrbms_div_pairing(self.handle, Q, L, _dblp(th), self._ptr(D, (S, self.n_T, 5 * Q * L), 'D'),
                                        self._ptr(G, (S, self.n, L), 'G'), c_vp(out.data_ptr()), self._stream())
        self._check(rc, 'lrbms_div_pairing')
        return out

    def reduced_reconstruction_terms(self, theta, B_sys, M_red, rhs_red, G_ud, U):
        """U [L, S, N] -> [L, S]: the elliptic-reconstruction terms of the reduced estimate."""
        Q, S, N, L = B_sys.shape[0], self.S, B_sys.shape[3], U.shape[0]
        th = np.ascontiguousarray(theta, dtype=np.float64)
        work = self.empty(int(self.lib.lrbms_reduced_time_residual_work_size(self.handle, N)))
        out = self.empty(L, S)
        rc = self.lib.lrbms_reduced_reconstruction_terms(
            self.handle, Q, N, L, _dblp(th), self._ptr(B_sys, (Q, S, 5, N, N), 'B_sys'), self._ptr(M_red, (S, N, N), 'M_red'),
            self._ptr(rhs_red, (S, N), 'rhs_red'), self._ptr(G_ud, (S, N, 5 * Q * N), 'G_ud'), self._ptr(U, (L, S, N), 'U'),
            c_vp(work.data_ptr()), c_vp(out.data_ptr()), self._stream())
        self._check(rc, 'lrbms_reduced_reconstruction_terms')
        return out

    def reduced_implicit_euler(self, theta, dt, nt, B_sys, M_red, rhs_red, U0=None, rtol=1e-13, max_iter=20000):
        """(M_red + dt A_red(mu)) u_{k+1} = M_red u_k + dt rhs_red -> (U [nt + 1, S, N], info)."""
        Q, S, N = B_sys.shape[0], self.S, B_sys.shape[3]
        th = np.ascontiguousarray(theta, dtype=np.float64)
        assert th.shape == (Q,)
        work = self.empty(int(self.lib.lrbms_reduced_solve_work_size(self.handle, N)))
        U = self.zeros(int(nt) + 1, S, N)
        if U0 is not None:
            U[0] = U0.reshape(S, N)
        info = np.zeros(2)
        rc = self.lib.lrbms_reduced_implicit_euler(self.handle, Q, N, _dblp(th), float(dt), int(nt),
                                                   self._ptr(B_sys, (Q, S, 5, N, N), 'B_sys'), self._ptr(M_red, (S, N, N), 'M_red'),
                                                   self._ptr(rhs_red, (S, N), 'rhs_red'), c_vp(work.data_ptr()),
                                                   c_vp(U.data_ptr()), float(rtol), int(max_iter), _dblp(info), self._stream())
        self._check(rc, 'lrbms_reduced_implicit_euler')
        return U, {'iterations': int(info[0]), 'relative_residual': float(info[1])}

    def reduced_time_residual(self, theta, B_sys, M_red, dU):
        """dU [L, S, N] -> [L, S]: y^T M_red^-1 y with y = A_red(mu) dU_l."""
        Q, S, N, L = B_sys.shape[0], self.S, B_sys.shape[3], dU.shape[0]
        th = np.ascontiguousarray(theta, dtype=np.float64)
        assert th.shape == (Q,)
        work = self.empty(int(self.lib.lrbms_reduced_time_residual_work_size(self.handle, N)))
        out = self.empty(L, S)
        rc = self.lib.lrbms_reduced_time_residual(self.handle, Q, N, L, _dblp(th), self._ptr(B_sys, (Q, S, 5, N, N), 'B_sys'),
                                                  self._ptr(M_red, (S, N, N), 'M_red'), self._ptr(dU, (L, S, N), 'dU'),
                                                  c_vp(work.data_ptr()), c_vp(out.data_ptr()), self._stream())
        self._check(rc, 'lrbms_reduced_time_residual')
        return out

    # ------------------------------------------------------------------ time-dependent affine sources (parabolic path)
    def assemble_source_gram(self, f_smp_K):
        """f_smp_K [K, S, n_T, f_stride] -> F2 [S, K, K] = (f_j, f_l)_{L2(Omega_s)}."""
        K, qd = f_smp_K.shape[0], self._quad()
        F2 = self.empty(self.S, K, K)
        rc = self.lib.lrbms_assemble_source_gram(self.handle, K, self._ptr(f_smp_K, (K, self.S, self.n_T, qd.f_stride), 'f_smp_K'),
                                                 c_vp(F2.data_ptr()), self._stream())
        self._check(rc, 'lrbms_assemble_source_gram')
        return F2

    def _phi(self, phi, rows=None):
        phi = phi if hasattr(phi, 'data_ptr') else self.from_numpy(np.ascontiguousarray(np.asarray(phi, dtype=np.float64)))
        assert phi.dim() == 2 and (rows is None or phi.shape[0] == rows), 'phi must be [{}, K]'.format(rows)
        phi = phi.contiguous()
        self._ptr(phi, tuple(phi.shape), 'phi')
        return phi

    def fom_implicit_euler_src(self, theta, dt, nt, A_diag, A_cpl, b_K, phi, U0=None, rtol=1e-12, max_iter=100000):
        """(M + dt A(mu)) u_{k+1} = M u_k + dt sum_j phi[k+1, j] b_K[j] -> (U [nt + 1, S, n], info); phi [nt + 1, K]."""
        Q, S, K = A_diag.shape[0], self.S, b_K.shape[0]
        th = np.ascontiguousarray(theta, dtype=np.float64)
        assert th.shape == (Q,)
        ph = self._phi(phi, int(nt) + 1)
        assert ph.shape[1] == K
        work = self.empty(int(self.lib.lrbms_fom_solve_work_size(self.handle)))
        U = self.zeros(int(nt) + 1, S, self.n)
        if U0 is not None:
            U[0] = U0.reshape(S, self.n)
        info = np.zeros(2)
        rc = self.lib.lrbms_fom_implicit_euler_src(self.handle, Q, K, _dblp(th), float(dt), int(nt),
                                                   self._ptr(A_diag, (Q, S, self.n_T, 4, 9), 'A_diag'),
                                                   self._ptr(A_cpl, (Q, S, 4, self.ncf, 9), 'A_cpl'),
                                                   self._ptr(b_K, (K, S, self.n), 'b_K'), c_vp(ph.data_ptr()),
                                                   c_vp(work.data_ptr()), c_vp(U.data_ptr()), float(rtol), int(max_iter), _dblp(info),
                                                   self._stream())
        self._check(rc, 'lrbms_fom_implicit_euler_src')
        return U, {'iterations': int(info[0]), 'relative_residual': float(info[1])}

    def reduced_implicit_euler_src(self, theta, dt, nt, B_sys, M_red, rhs_red_K, phi, U0=None, rtol=1e-13, max_iter=20000):
        """(M_red + dt A_red(mu)) u_{k+1} = M_red u_k + dt sum_j phi[k+1, j] rhs_red_K[j] -> (U [nt + 1, S, N], info)."""
        Q, S, N, K = B_sys.shape[0], self.S, B_sys.shape[3], rhs_red_K.shape[0]
        th = np.ascontiguousarray(theta, dtype=np.float64)
        assert th.shape == (Q,)
        ph = self._phi(phi, int(nt) + 1)
        assert ph.shape[1] == K
        work = self.empty(int(self.lib.lrbms_reduced_solve_work_size(self.handle, N)))
        U = self.zeros(int(nt) + 1, S, N)
        if U0 is not None:
            U[0] = U0.reshape(S, N)
        info = np.zeros(2)
        rc = self.lib.lrbms_reduced_implicit_euler_src(self.handle, Q, N, K, _dblp(th), float(dt), int(nt),
                                                       self._ptr(B_sys, (Q, S, 5, N, N), 'B_sys'), self._ptr(M_red, (S, N, N), 'M_red'),
                                                       self._ptr(rhs_red_K, (K, S, N), 'rhs_red_K'), c_vp(ph.data_ptr()),
                                                       c_vp(work.data_ptr()), c_vp(U.data_ptr()), float(rtol), int(max_iter),
                                                       _dblp(info), self._stream())
        self._check(rc, 'lrbms_reduced_implicit_euler_src')
        return U, {'iterations': int(info[0]), 'relative_residual': float(info[1])}

    def _batch_trajectory_buffers(self, name, N, nmu, nt, U0, work):
        """work and U [nt + 1, S, N, nmu] (U[0] = U0: [S, N] for every column, or [S, N, nmu]; default zero) of the batched
        reduced implicit Euler exports."""
        need = int(self.lib.lrbms_reduced_implicit_euler_batch_work_size(self.handle, N, nmu))
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

    def reduced_implicit_euler_batch(self, thetas, dt, nt, B_sys, M_red, rhs_red, U0=None, rtol=1e-13, max_iter=20000, work=None):
        """nmu <= 64 reduced trajectories in one call: thetas [nmu, Q] -> (U [nt + 1, S, N, nmu] (parameter fastest), info);
        column m is what ``reduced_implicit_euler`` returns at thetas[m].  ``max_iter`` caps the iterations of one step."""
        Q, S, N = B_sys.shape[0], self.S, B_sys.shape[3]
        th = np.ascontiguousarray(thetas, dtype=np.float64)
        nmu = th.shape[0]
        assert th.shape == (nmu, Q)
        work, U = self._batch_trajectory_buffers('reduced_implicit_euler_batch', N, nmu, nt, U0, work)
        info = np.zeros(2)
        rc = self.lib.lrbms_reduced_implicit_euler_batch(self.handle, Q, N, nmu, _dblp(th), float(dt), int(nt),
                                                         self._ptr(B_sys, (Q, S, 5, N, N), 'B_sys'), self._ptr(M_red, (S, N, N), 'M_red'),
                                                         self._ptr(rhs_red, (S, N), 'rhs_red'), c_vp(work.data_ptr()),
                                                         c_vp(U.data_ptr()), float(rtol), int(max_iter), _dblp(info), self._stream())
        self._check(rc, 'lrbms_reduced_implicit_euler_batch')
        return U, {'iterations': int(info[0]), 'relative_residual': float(info[1])}

    def reduced_implicit_euler_batch_src(self, thetas, dt, nt, B_sys, M_red, rhs_red_K, phi, U0=None, rtol=1e-13, max_iter=20000,
                                         work=None):
        """``reduced_implicit_euler_batch`` with the step right-hand side M_red u_k + dt sum_j phi[m, k+1, j] rhs_red_K[j] in
        column m; phi [nmu, nt + 1, K] (host or device)."""
        Q, S, N, K = B_sys.shape[0], self.S, B_sys.shape[3], rhs_red_K.shape[0]
        th = np.ascontiguousarray(thetas, dtype=np.float64)
        nmu = th.shape[0]
        assert th.shape == (nmu, Q)
        ph = phi if hasattr(phi, 'data_ptr') else self.from_numpy(np.ascontiguousarray(np.asarray(phi, dtype=np.float64)))
        assert tuple(ph.shape) == (nmu, max(int(nt), 0) + 1, K), 'phi must be [nmu, nt + 1, K]'
        ph = ph.contiguous()
        work, U = self._batch_trajectory_buffers('reduced_implicit_euler_batch_src', N, nmu, nt, U0, work)
        info = np.zeros(2)
        rc = self.lib.lrbms_reduced_implicit_euler_batch_src(self.handle, Q, N, K, nmu, _dblp(th), float(dt), int(nt),
                                                             self._ptr(B_sys, (Q, S, 5, N, N), 'B_sys'),
                                                             self._ptr(M_red, (S, N, N), 'M_red'),
                                                             self._ptr(rhs_red_K, (K, S, N), 'rhs_red_K'),
                                                             self._ptr(ph, tuple(ph.shape), 'phi'), c_vp(work.data_ptr()),
                                                             c_vp(U.data_ptr()), float(rtol), int(max_iter), _dblp(info), self._stream())
        self._check(rc, 'lrbms_reduced_implicit_euler_batch_src')
        return U, {'iterations': int(info[0]), 'relative_residual': float(info[1])}

    def reduced_parabolic_estimate_batch(self, thetas, coef, dt, nt, U, B_sys, M_red, grams, f2, ceps, hdiam, sqrt_local=False,
                                         phi=None, F2=None, r_fd_K=None, work=None):
        """The parabolic estimate of the nmu <= 64 trajectories of the panel U [nt + 1, S, N, nmu] in one call
        (``lrbms_reduced_parabolic_estimate_batch``): thetas [nmu, Q], coef [nmu, 2] (host), grams in either layout (6 tensors dense,
        8 factored); with a time-dependent source phi [nmu, nt + 1, K], F2 [S, K, K], r_fd_K [K, S, 5 Q N].  Returns a dict of device
        tensors: eta_loc [3, nt + 1, S, nmu], time_deriv_nc [nt, S, nmu], time_residual [nt, nmu], eta [nt + 1, nmu], est [nmu]."""
        Q, S, N = B_sys.shape[0], self.S, B_sys.shape[3]
        th = np.ascontiguousarray(thetas, dtype=np.float64)
        nmu, nt = th.shape[0], int(nt)
        assert th.shape == (nmu, Q)
        cf = np.ascontiguousarray(coef, dtype=np.float64)
        assert cf.shape == (nmu, 2), 'coef must be [nmu, 2]'
        gptrs, factored = self._gram_ptrs(grams, Q, N)
        if not factored:
            gptrs = gptrs + [c_vp(None), c_vp(None)]
        K = 0
        src = [c_vp(None)] * 3
        if phi is not None:
            K = int(F2.shape[1])
            ph = phi if hasattr(phi, 'data_ptr') else self.from_numpy(np.ascontiguousarray(np.asarray(phi, dtype=np.float64)))
            assert tuple(ph.shape) == (nmu, max(nt, 0) + 1, K), 'phi must be [nmu, nt + 1, K]'
            ph = ph.contiguous()
            src = [self._ptr(ph, tuple(ph.shape), 'phi'), self._ptr(F2, (S, K, K), 'F2'),
                   self._ptr(r_fd_K, (K, S, 5 * Q * N), 'r_fd_K')]
        u_ptr = self._ptr(U, (max(nt, 0) + 1, S, N, nmu), 'U')
        need = int(self.lib.lrbms_reduced_parabolic_estimate_batch_work_size(self.handle, N, max(nmu, 1), max(nt, 1)))
        if need < 0:
            raise NativeError('reduced_parabolic_estimate_batch: bad N / nmu / nt')
        if work is None:
            work = self.empty(need)
        if work.numel() < need:
            raise NativeError('reduced_parabolic_estimate_batch: work too small')
        out = {'eta_loc': self.empty(3, max(nt, 0) + 1, S, nmu), 'time_deriv_nc': self.empty(max(nt, 0), S, nmu),
               'time_residual': self.empty(max(nt, 0), nmu), 'eta': self.empty(max(nt, 0) + 1, nmu), 'est': self.empty(nmu)}
        rc = self.lib.lrbms_reduced_parabolic_estimate_batch(
            self.handle, Q, N, K, nmu, nt, float(dt), _dblp(th), _dblp(cf), int(bool(sqrt_local)), u_ptr,
            self._ptr(B_sys, (Q, S, 5, N, N), 'B_sys'), self._ptr(M_red, (S, N, N), 'M_red'), *gptrs, self._ptr(f2, (S,), 'f2'),
            self._ptr(ceps, (S,), 'ceps'), float(hdiam), *src, c_vp(work.data_ptr()), c_vp(out['eta_loc'].data_ptr()),
            c_vp(out['time_deriv_nc'].data_ptr()), c_vp(out['time_residual'].data_ptr()), c_vp(out['eta'].data_ptr()),
            c_vp(out['est'].data_ptr()), self._stream())
        self._check(rc, 'lrbms_reduced_parabolic_estimate_batch')
        return out

    # ---- time-dependent diffusion coefficients: theta_t [nmu, nt + 1, Q] on the host
    def _theta_t(self, theta_t, Q, nt):
        th = np.ascontiguousarray(theta_t, dtype=np.float64)
        assert th.ndim == 3 and th.shape[1:] == (max(int(nt), 0) + 1, Q), 'theta_t must be [nmu, nt + 1, Q]'
        return th, th.shape[0]

    def _phi_table(self, phi, nmu, nt, K):
        ph = phi if hasattr(phi, 'data_ptr') else self.from_numpy(np.ascontiguousarray(np.asarray(phi, dtype=np.float64)))
        assert tuple(ph.shape) == (nmu, max(int(nt), 0) + 1, K), 'phi must be [nmu, nt + 1, K]'
        return ph.contiguous()

    def fom_implicit_euler_batch_tv(self, theta_t, dt, nt, A_diag, A_cpl, b_K, phi, U0=None, rtol=1e-12, max_iter=100000):
        """``fom_implicit_euler_batch`` with a coefficient row per step: the step k -> k + 1 of column m solves with
        M + dt A(theta_t[m, k + 1]).  theta_t [nmu, nt + 1, Q] host."""
        Q, S, K, nt = A_diag.shape[0], self.S, b_K.shape[0], int(nt)
        th, nmu = self._theta_t(theta_t, Q, nt)
        phi = self._phi_table(phi, nmu, nt, K)
        size = int(self.lib.lrbms_fom_implicit_euler_batch_work_size(self.handle, nmu))
        if size < 0:
            raise NativeError('lrbms_fom_implicit_euler_batch_tv: nmu = {} is not in 1..64'.format(nmu))
        work = self.empty(size)
        U = self.zeros(nt + 1, S, self.n, nmu)
        if U0 is not None:
            U[0] = U0.reshape(S, self.n, -1)
        info = np.zeros(2)
        rc = self.lib.lrbms_fom_implicit_euler_batch_tv(self.handle, Q, K, nmu, _dblp(th), float(dt), nt,
                                                        self._ptr(A_diag, (Q, S, self.n_T, 4, 9), 'A_diag'),
                                                        self._ptr(A_cpl, (Q, S, 4, self.ncf, 9), 'A_cpl'),
                                                        self._ptr(b_K, (K, S, self.n), 'b_K'), self._ptr(phi, (nmu, nt + 1, K), 'phi'),
                                                        c_vp(work.data_ptr()), c_vp(U.data_ptr()), float(rtol), int(max_iter),
                                                        _dblp(info), self._stream())
        panels = np.zeros(8)
        self.lib.lrbms_fom_implicit_euler_batch_panel_info(self.handle, _dblp(panels))
        self._check(rc, 'lrbms_fom_implicit_euler_batch_tv')
        return U, {'iterations': int(info[0]), 'relative_residual': float(info[1]),
                   'panel_iterations': [int(v) for v in panels[0:2 * ((nmu + 15) // 16):2]]}

    def reduced_implicit_euler_batch_tv(self, theta_t, dt, nt, B_sys, M_red, rhs_red, phi=None, U0=None, rtol=1e-13, max_iter=20000,
                                        work=None):
        """``reduced_implicit_euler_batch`` (phi None, rhs_red [S, N]) / ``_src`` (rhs_red [K, S, N], phi [nmu, nt + 1, K]) with a
        coefficient row per step: theta_t [nmu, nt + 1, Q] host, the step k -> k + 1 runs with row k + 1."""
        Q, S, N = B_sys.shape[0], self.S, B_sys.shape[3]
        th, nmu = self._theta_t(theta_t, Q, nt)
        K = 0 if phi is None else int(rhs_red.shape[0])
        ph = None if phi is None else self._phi_table(phi, nmu, nt, K)
        need = int(self.lib.lrbms_reduced_implicit_euler_batch_tv_work_size(self.handle, N, nmu, max(int(nt), 1)))
        if need < 0:
            raise NativeError('reduced_implicit_euler_batch_tv: bad N / nmu')
        if work is None:
            work = self.empty(need)
        if work.numel() < need:
            raise NativeError('reduced_implicit_euler_batch_tv: work too small')
        U = self.zeros(max(int(nt), 0) + 1, S, N, nmu)
        if U0 is not None:
            U[0] = U0.reshape(S, N, -1)
        info = np.zeros(2)
        rc = self.lib.lrbms_reduced_implicit_euler_batch_tv(
            self.handle, Q, N, K, nmu, _dblp(th), float(dt), int(nt), self._ptr(B_sys, (Q, S, 5, N, N), 'B_sys'),
            self._ptr(M_red, (S, N, N), 'M_red'), self._ptr(rhs_red, (K, S, N) if K else (S, N), 'rhs_red'),
            c_vp(None) if ph is None else self._ptr(ph, tuple(ph.shape), 'phi'), c_vp(work.data_ptr()), c_vp(U.data_ptr()), float(rtol),
            int(max_iter), _dblp(info), self._stream())
        self._check(rc, 'lrbms_reduced_implicit_euler_batch_tv')
        return U, {'iterations': int(info[0]), 'relative_residual': float(info[1])}

    def reduced_parabolic_estimate_batch_tv(self, theta_t, coef, dt, nt, U, B_sys, M_red, grams, f2, ceps, hdiam, sqrt_local=False,
                                            phi=None, F2=None, r_fd_K=None, work=None):
        """``reduced_parabolic_estimate_batch`` with theta_t [nmu, nt + 1, Q] and coef [nmu, nt + 1, 2] (host): the elliptic rows of
        U_k use row k, the time residual of U_{k+1} - U_k row k + 1.  Same outputs."""
        Q, S, N = B_sys.shape[0], self.S, B_sys.shape[3]
        nt = int(nt)
        th, nmu = self._theta_t(theta_t, Q, nt)
        cf = np.ascontiguousarray(coef, dtype=np.float64)
        assert cf.shape == (nmu, max(nt, 0) + 1, 2), 'coef must be [nmu, nt + 1, 2]'
        gptrs, factored = self._gram_ptrs(grams, Q, N)
        if not factored:
            gptrs = gptrs + [c_vp(None), c_vp(None)]
        K = 0
        src = [c_vp(None)] * 3
        if phi is not None:
            K = int(F2.shape[1])
            ph = self._phi_table(phi, nmu, nt, K)
            src = [self._ptr(ph, tuple(ph.shape), 'phi'), self._ptr(F2, (S, K, K), 'F2'),
                   self._ptr(r_fd_K, (K, S, 5 * Q * N), 'r_fd_K')]
        u_ptr = self._ptr(U, (max(nt, 0) + 1, S, N, nmu), 'U')
        need = int(self.lib.lrbms_reduced_parabolic_estimate_batch_tv_work_size(self.handle, N, max(nmu, 1), max(nt, 1)))
        if need < 0:
            raise NativeError('reduced_parabolic_estimate_batch_tv: bad N / nmu / nt')
        if work is None:
            work = self.empty(need)
        if work.numel() < need:
            raise NativeError('reduced_parabolic_estimate_batch_tv: work too small')
        out = {'eta_loc': self.empty(3, max(nt, 0) + 1, S, nmu), 'time_deriv_nc': self.empty(max(nt, 0), S, nmu),
               'time_residual': self.empty(max(nt, 0), nmu), 'eta': self.empty(max(nt, 0) + 1, nmu), 'est': self.empty(nmu)}
        rc = self.lib.lrbms_reduced_parabolic_estimate_batch_tv(
            self.handle, Q, N, K, nmu, nt, float(dt), _dblp(th), _dblp(cf), int(bool(sqrt_local)), u_ptr,
            self._ptr(B_sys, (Q, S, 5, N, N), 'B_sys'), self._ptr(M_red, (S, N, N), 'M_red'), *gptrs, self._ptr(f2, (S,), 'f2'),
            self._ptr(ceps, (S,), 'ceps'), float(hdiam), *src, c_vp(work.data_ptr()), c_vp(out['eta_loc'].data_ptr()),
            c_vp(out['time_deriv_nc'].data_ptr()), c_vp(out['time_residual'].data_ptr()), c_vp(out['eta'].data_ptr()),
            c_vp(out['est'].data_ptr()), self._stream())
        self._check(rc, 'lrbms_reduced_parabolic_estimate_batch_tv')
        return out

    def project_sources(self, Q, b_K, V, D, out=None):
        """b_K [K, S, n], V [S(_ext), n, N], D [S, n_T, 5 Q N] -> (rhs_red_K [K, S, N], r_fd_K [K, S, 5 Q N])."""
        K, S, N = b_K.shape[0], self.S, V.shape[2]
        C = 5 * Q * N
        rhs_K, rfd_K = out if out is not None else (self.empty(K, S, N), self.empty(K, S, C))
        rc = self.lib.lrbms_project_sources(self.handle, Q, N, K, self._ptr(b_K, (K, S, self.n), 'b_K'),
                                            self._ptr(V, (V.shape[0], self.n, N), 'V'), self._ptr(D, (S, self.n_T, C), 'D'),
                                            self._ptr(rhs_K, (K, S, N), 'rhs_red_K'), self._ptr(rfd_K, (K, S, C), 'r_fd_K'),
                                            self._stream())
        self._check(rc, 'lrbms_project_sources')
        return rhs_K, rfd_K

    def reduced_source_terms(self, theta, phi, F2, r_fd_K, u, ceps, hdiam):
        """u [S, N, L] (column fastest), phi [L, K] -> [S, L]: the source part of the scaled residual indicator."""
        th = np.ascontiguousarray(theta, dtype=np.float64)
        Q, S, N, L, K = len(th), self.S, u.shape[1], u.shape[2], F2.shape[1]
        ph = self._phi(phi, L)
        assert ph.shape[1] == K
        out = self.empty(S, L)
        rc = self.lib.lrbms_reduced_source_terms(self.handle, Q, N, K, L, _dblp(th), c_vp(ph.data_ptr()),
                                                 self._ptr(F2, (S, K, K), 'F2'), self._ptr(r_fd_K, (K, S, 5 * Q * N), 'r_fd_K'),
                                                 self._ptr(u, (S, N, L), 'u'), self._ptr(ceps, (S,), 'ceps'), float(hdiam),
                                                 c_vp(out.data_ptr()), self._stream())
        self._check(rc, 'lrbms_reduced_source_terms')
        return out

    # ------------------------------------------------------------------ parameter-dependent affine sources (stationary path)
    def combine_sources(self, phi, x_K, out=None):
        """phi [K] (host), x_K [K, ...] (device) -> y [...] = sum_j phi[j] x_K[j] (``lrbms_combine_sources``)."""
        ph = np.ascontiguousarray(phi, dtype=np.float64).reshape(-1)
        K = int(x_K.shape[0])
        assert ph.shape == (K,), 'phi must have K = {} entries'.format(K)
        M = int(x_K[0].numel())
        x = self._ptr(x_K, (K,) + tuple(x_K.shape[1:]), 'x_K')
        y = out if out is not None else self.empty(*x_K.shape[1:])
        rc = self.lib.lrbms_combine_sources(self.handle, K, M, _dblp(ph), x, self._ptr(y, tuple(x_K.shape[1:]), 'y'), self._stream())
        self._check(rc, 'lrbms_combine_sources')
        return y

    def reduced_solve_batch_src(self, thetas, phis, B_sys, rhs_red_K, rtol=1e-13, max_iter=20000, work=None):
        """thetas [nmu, Q], phis [nmu, K] (host), rhs_red_K [K, S, N] -> u [S, N, nmu] (mu fastest), info: column m solves
        against sum_j phis[m, j] rhs_red_K[j]."""
        Q, S, N, K = B_sys.shape[0], self.S, B_sys.shape[3], rhs_red_K.shape[0]
        th = np.ascontiguousarray(thetas, dtype=np.float64)
        ph = np.ascontiguousarray(phis, dtype=np.float64)
        nmu = th.shape[0]
        assert th.shape == (nmu, Q) and ph.shape == (nmu, K)
        need = int(self.lib.lrbms_reduced_solve_batch_work_size(self.handle, N, nmu))
        if work is None:
            work = self.empty(need)
        if work.numel() < need:
            raise NativeError('reduced_solve_batch_src: work too small')
        u = self.empty(S, N, nmu)
        info = np.zeros(2)
        rc = self.lib.lrbms_reduced_solve_batch_src(self.handle, Q, N, K, nmu, _dblp(th), _dblp(ph),
                                                    self._ptr(B_sys, (Q, S, 5, N, N), 'B_sys'),
                                                    self._ptr(rhs_red_K, (K, S, N), 'rhs_red_K'), c_vp(work.data_ptr()),
                                                    c_vp(u.data_ptr()), float(rtol), int(max_iter), _dblp(info), self._stream())
        self._check(rc, 'lrbms_reduced_solve_batch_src')
        return u, {'iterations': int(info[0]), 'relative_residual': float(info[1])}

    def reduced_solve_batches_src(self, thetas, phis, B_sys, rhs_red_K, per_call=64, rtol=1e-13, max_iter=20000, concat=True):
        """``reduced_solve_batches`` with a right-hand side of its own per parameter (phis [nmu, K])."""
        torch = self.torch
        th = np.ascontiguousarray(thetas, dtype=np.float64)
        ph = np.ascontiguousarray(phis, dtype=np.float64)
        per_call = max(1, min(int(per_call), 64))
        work = self.empty(int(self.lib.lrbms_reduced_solve_batch_work_size(self.handle, int(B_sys.shape[3]), min(per_call, th.shape[0]))))
        res = [self.reduced_solve_batch_src(th[b0:b0 + per_call], ph[b0:b0 + per_call], B_sys, rhs_red_K, rtol=rtol,
                                            max_iter=max_iter, work=work)
               for b0 in range(0, th.shape[0], per_call)]
        if concat:
            u = torch.cat([r[0] for r in res], dim=2) if len(res) > 1 else res[0][0]
        else:
            u = [r[0] for r in res]
        return u, {'iterations': max(r[1]['iterations'] for r in res), 'relative_residual': max(r[1]['relative_residual'] for r in res)}

    # ------------------------------------------------------------------ online enrichment
    def assemble_dirichlet_correction(self, lam):
        Q = lam.shape[0]
        D = self.empty(Q, self.S, 4, self.ncf, 9)
        rc = self.lib.lrbms_assemble_dirichlet_correction(self.handle, Q, self._ptr(lam, (Q, self.S_ext, self.n_T, self._quad().lam_stride), 'lam'),
                                                          c_vp(D.data_ptr()), self._stream())
        self._check(rc, 'lrbms_assemble_dirichlet_correction')
        return D

    def _hood_args(self, theta, marked, A_diag, A_cpl, D_corr):
        """What both corrector exports marshal alike: theta [Q] and marked [nmark] as host arrays, the three operator pointers after
        their shape checks, work and the host array info.  (Sizes the library refuses still reach it: the refusal is the library's.)"""
        Q, S = A_diag.shape[0], self.S
        th = np.ascontiguousarray(theta, dtype=np.float64)
        assert th.shape == (Q,)
        mk = np.ascontiguousarray(marked, dtype=np.int32)
        nmark = int(mk.shape[0])
        ops = (self._ptr(A_diag, (Q, S, self.n_T, 4, 9), 'A_diag'), self._ptr(A_cpl, (Q, S, 4, self.ncf, 9), 'A_cpl'),
               self._ptr(D_corr, (Q, S, 4, self.ncf, 9), 'D_corr'))
        work = self.empty(max(int(self.lib.lrbms_local_correction_work_size(self.handle, nmark)), 1))
        return th, mk, ops, work, np.zeros((max(nmark, 1), 2))

    def local_correction_solve(self, theta, marked, A_diag, A_cpl, D_corr, b, rtol=1e-12, max_iter=20000):
        """marked: subdomain indices -> (corr [nmark, n], info [nmark, 2] = iterations, relative residual)."""
        th, mk, ops, work, info = self._hood_args(theta, marked, A_diag, A_cpl, D_corr)
        corr = self.empty(len(mk), self.n)
        rc = self.lib.lrbms_local_correction_solve(
            self.handle, len(th), _dblp(th), len(mk), mk.ctypes.data_as(_P_I32), *ops, self._ptr(b, (self.S, self.n), 'b'),
            c_vp(work.data_ptr()), c_vp(corr.data_ptr()), float(rtol), int(max_iter), _dblp(info), self._stream())
        self._check(rc, 'lrbms_local_correction_solve')
        return corr, info

    def local_correction_euler(self, theta, dt, nt, marked, A_diag, A_cpl, D_corr, b_K, phi, rtol=1e-10, max_iter=20000):
        """The corrector trajectories of the parabolic enrichment (``lrbms_local_correction_euler``): b_K [K, S, n], phi
        [nt + 1, K] (device) -> (corr [nmark, n, nt], step fastest: column k - 1 = x_k; info [nmark, 2] = iterations summed over the
        steps, worst final residual ratio of a step)."""
        K, nt = b_K.shape[0], int(nt)
        if phi.dim() != 2 or phi.shape[1] != K or phi.shape[0] < nt + 1:
            raise NativeError('phi: expected [nt + 1 = {}, K = {}], got {}'.format(nt + 1, K, tuple(phi.shape)))
        th, mk, ops, work, info = self._hood_args(theta, marked, A_diag, A_cpl, D_corr)
        corr = self.empty(max(len(mk), 1), self.n, max(nt, 1))
        rc = self.lib.lrbms_local_correction_euler(
            self.handle, len(th), K, _dblp(th), float(dt), nt, len(mk), mk.ctypes.data_as(_P_I32), *ops,
            self._ptr(b_K, (K, self.S, self.n), 'b_K'), self._ptr(phi, tuple(phi.shape), 'phi'), c_vp(work.data_ptr()),
            c_vp(corr.data_ptr()), float(rtol), int(max_iter), _dblp(info), self._stream())
        self._check(rc, 'lrbms_local_correction_euler')
        return corr, info

    # ------------------------------------------------------------------ helpers
    def blockell_apply(self, A, x):
        M = x.shape[2]
        y = self.empty(self.S, self.n, M)
        rc = self.lib.lrbms_blockell_apply(self.handle, M, self._ptr(A, (self.S, self.n_T, 4, 9), 'A'),
                                           self._ptr(x, (self.S, self.n, M), 'x'), c_vp(y.data_ptr()), self._stream())
        self._check(rc, 'lrbms_blockell_apply')
        return y

    def fom_apply(self, theta, A_diag, A_cpl, x, out=None):
        Q, M = A_diag.shape[0], x.shape[2]
        th = np.ascontiguousarray(theta, dtype=np.float64)
        assert th.shape == (Q,)
        y = out if out is not None else self.empty(self.S, self.n, M)
        rc = self.lib.lrbms_fom_apply(self.handle, Q, M, _dblp(th), self._ptr(A_diag, (Q, self.S, self.n_T, 4, 9), 'A_diag'),
                                      self._ptr(A_cpl, (Q, self.S, 4, self.ncf, 9), 'A_cpl'),
                                      self._ptr(x, (self.S_ext, self.n, M), 'x'), self._ptr(y, (self.S, self.n, M), 'y'),
                                      self._stream())
        self._check(rc, 'lrbms_fom_apply')
        return y

    def gemm_tn(self, X, Y, rowscale=None, alpha=1.0):
        """G[b] = alpha X[b]^T diag(rowscale) Y[b] for X [B, K, Mx], Y [B, K, My]."""
        B, K, Mx = X.shape
        My = Y.shape[2]
        assert Y.shape[:2] == (B, K)
        G = self.empty(B, Mx, My)
        rs = c_vp(rowscale.data_ptr()) if rowscale is not None else c_vp(None)
        rc = self.lib.lrbms_gemm_tn(self.handle, B, K, Mx, My, self._ptr(X, (B, K, Mx), 'X'), K * Mx, Mx,
                                    self._ptr(Y, (B, K, My), 'Y'), K * My, My, c_vp(G.data_ptr()), Mx * My, My, rs,
                                    float(alpha), self._stream())
        self._check(rc, 'lrbms_gemm_tn')
        return G

    # ------------------------------------------------------------------ local POD basis extension
    def local_pod(self, P_diag, U, V, nloc, modes, rtol=1e-6, atol=0.0, work=None):
        """``lrbms_local_pod``: at most ``modes`` POD modes of the snapshots ``U`` [S, n, L] per subdomain, in the block-ELL
        product ``P_diag``, into the free columns of ``V``; see ``ContextBase._local_pod`` for the arguments and the result."""
        return self._local_pod(self._ptr(P_diag, (self.S, self.n_T, 4, 9), 'P_diag'), U, V, nloc, modes, rtol, atol, work)

    def _pod_product_ptr(self, P_diag):
        return self._ptr(P_diag, (self.S, self.n_T, 4, 9), 'P_diag')

    def pod_gram(self, X, Y):
        """sym(X[b]^T Y[b]) for X, Y [B, K, L] (``lrbms_pod_gram``: upper-triangle MFMA tiles, mirrored)."""
        B, K, L = X.shape
        G = self.empty(B, L, L)
        rc = self.lib.lrbms_pod_gram(self.handle, B, K, L, self._ptr(X, (B, K, L), 'X'), self._ptr(Y, (B, K, L), 'Y'),
                                     c_vp(G.data_ptr()), self._stream())
        self._check(rc, 'lrbms_pod_gram')
        return G

    def pod_eigh(self, G, mode=0, kcount=None):
        """``lrbms_pod_eigh`` on G [B, L, L]: (lam [B, L] descending, Z [B, L, L], info int32 [B]).  mode 0: row j of Z[b] is the
        eigenvector of lam[b, j]; mode 1: Z = G^{-1/2} over the ``kcount[b]`` (int32 device tensor; None: all) largest eigenpairs."""
        torch = self.torch
        B, L = int(G.shape[0]), int(G.shape[1])
        lam, Z = self.empty(B, L), self.empty(B, L, L)
        info = torch.empty(B, dtype=torch.int32, device=self.device)
        size = int(self.lib.lrbms_pod_eigh_work_size(self.handle, B, L))
        work = self.empty(size) if size > 0 else None
        if kcount is not None:
            assert kcount.dtype == torch.int32 and tuple(kcount.shape) == (B,) and kcount.device == self.device
        rc = self.lib.lrbms_pod_eigh(self.handle, B, L, int(mode), self._ptr(G, (B, L, L), 'G'),
                                     c_vp(kcount.data_ptr()) if kcount is not None else None, c_vp(lam.data_ptr()), c_vp(Z.data_ptr()),
                                     c_vp(info.data_ptr()), c_vp(work.data_ptr()) if work is not None else None, self._stream())
        self._check(rc, 'lrbms_pod_eigh')
        return lam, Z, info
