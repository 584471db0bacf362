"""``LRBMSReductor`` (reference python/dune/pylrbms/reductor.py:17-78) on the HIP hot path.

``reduce()`` is the timed region of the benchmark: Oswald image bases (reductor.py:40-43), flux-reconstruction image
bases (:51-60) and the Galerkin projection of the system and of every estimator operator (:70, the fork's
``project_system``) run as HIP kernels over all local subdomains at once; the reduced operators stay block-sparse
(S x 5 blocks) instead of the reference's dense ``unblock``-ed ``(sum N)^2`` matrices.

``extend_basis`` restates the fork's ``GenericRBSystemReductor.extend_basis`` (absent from the tree; SURVEY.md
section 8a row B1): per subdomain Gram-Schmidt against the local basis w.r.t. the supplied product (the local energy
product, online_adaptive_lrbms.py:105-108), with re-orthogonalisation; products are applied with ``lrbms_blockell_apply``.
The local bases live in one HBM slab ``[S][n][N_max]``; a subdomain with fewer than ``N_max`` vectors (after online
enrichment of only the marked subdomains, reductor.py:75-78) has zero columns behind its ``nloc[s]`` vectors.  Zero
columns project to exactly zero rows / columns of every reduced operator, the reduced solve puts 1 on those diagonal
entries (``k_block_inverse``), so the padded unknowns stay 0 and every kernel keeps its uniform shape.
A global ``extend_basis`` is all-or-nothing and raises ``ExtensionError`` if any block of the snapshot is numerically
in the span of its basis.  ``extend_basis(U, method='pod', pod_modes=k)`` compresses instead: the leading POD modes of up to 128
snapshots per subdomain in the same product, deflated against the local basis (``lrbms_local_pod``, one native call batched over
the subdomains; ``LocalBasisSlab.extend_basis_pod``).  ``method='hapod'`` takes a training set of any size, e.g. the
list ``d.solve_batch(mus, as_snapshots='slabs')``: the items are pushed one after the other through ``lrbms_local_pod_stream_*``
(incremental HAPOD per subdomain) and ``pod_modes`` counts modes of the whole set (``extend_basis_hapod``).

Incremental re-projection (``reduce(touched=...)``): the reference re-reduces everything after a round of local enrichment
(online_enrichment.py:49-58 after reductor.py:75-78).  The projected operators of a target subdomain depend on the bases of
its neighbourhood only, so ``reduce(touched=marked)`` re-runs the fused pass over ``marked + neighbours(marked)`` and writes
their rows into the buffers of the previous reduced model -- as long as the slab width is unchanged (``reserve(width)`` pads the
slab with zero columns ahead of an enrichment loop: an enriched subdomain then fills one of its own zero columns and nobody
else pays for it).  The rows written are bit-identical to those of a whole pass.
"""
import numpy as np

from pylrbms_amd.vectorarrays import BlockVectorArray, BlockVectorSpace, ReducedVectorArray


class ExtensionError(Exception):
    """pymor.core.exceptions.ExtensionError (caught at online_adaptive_lrbms.py:116-119)."""


class LocalBasisSlab:
    """The local bases of a reductor as ONE device slab ``_V`` [S, n, N_max] with ``_nloc[s]`` vectors in subdomain s (zero
    columns behind them), extended by Gram-Schmidt in a local product.  Shared by the 2D and the 3D reductors; a subclass supplies
    the product (``_product_apply``) and the conversion of a snapshot to a slab [S, n, L] (``_as_slab``).  Rows past S of a
    ready-made slab are a halo: they take no part in the Gram-Schmidt."""

    _V = None                           # [S, n, N_max] device tensor
    _nloc = None                        # [S] host int array: number of basis vectors per local subdomain

    def _product_apply(self, X):
        raise NotImplementedError

    def _as_slab(self, U):
        raise NotImplementedError

    def basis_size(self):
        """N_max: the width of the basis slab (== every local basis size while the bases are uniform)."""
        return 0 if self._V is None else int(self._V.shape[2])

    def local_sizes(self):
        """``[len(rb) for rb in reductor.bases]`` of online_enrichment.py:80."""
        return [] if self._nloc is None else [int(v) for v in self._nloc[:self.d.engine.S]]

    def _orthonormalize(self, v, atol=1e-13, rtol=1e-10):
        """Gram-Schmidt (one re-orthogonalisation) of the single-column slab ``v`` [S, n, 1] against the local bases in
        the product.  Returns the normalised slab and the per-subdomain mask of blocks that were NOT
        (numerically) in the span of their basis."""
        import torch
        V = self._V[:self.d.engine.S] if self._V is not None and self._V.shape[2] > 0 else None
        v = v.clone()
        norm0 = torch.sqrt(torch.clamp((v * self._product_apply(v)).sum(dim=(1, 2)), min=0.0))
        for _ in range(2):
            if V is not None:
                coef = torch.einsum('snk,snl->skl', V, self._product_apply(v))     # zero-padded columns give 0
                v = v - torch.einsum('snk,skl->snl', V, coef)
        norm = torch.sqrt(torch.clamp((v * self._product_apply(v)).sum(dim=(1, 2)), min=0.0))
        ok = (norm > atol) & (norm > rtol * norm0)
        v = torch.where(ok[:, None, None], v / torch.where(ok, norm, torch.ones_like(norm))[:, None, None],
                        torch.zeros_like(v))
        return v, ok

    def _append_columns(self, v, ok):
        """Write block s of ``v`` behind the ``nloc[s]`` vectors of subdomain s for every s with ``ok[s]``; returns ``ok`` on
        the host."""
        import torch
        eng = self.d.engine
        ok_host = ok.cpu().numpy().astype(bool)
        if self._V is None:
            self._V = eng.ctx.zeros(eng.S, eng.t.n, 0)
            self._nloc = np.zeros(eng.S, dtype=np.int64)
        idx = np.where(ok_host)[0]
        if len(idx) == 0:
            return ok_host
        if int(self._nloc[idx].max()) + 1 > self._V.shape[2]:
            self._V = torch.cat([self._V, eng.ctx.zeros(eng.S, eng.t.n, 1)], dim=2).contiguous()
        rows = torch.as_tensor(idx, device=self._V.device)
        cols = torch.as_tensor(self._nloc[idx], device=self._V.device)
        self._V[rows, :, cols] = v[rows, :, 0]
        self._nloc[idx] += 1
        return ok_host

    def _extend_marked(self, marked, vecs):
        """Extend the bases of the local subdomains ``marked`` by the blocks ``vecs`` [len(marked), n, 1]; returns the
        per-entry success flags (a block in the span of its basis is skipped)."""
        import torch
        eng = self.d.engine
        full = eng.ctx.zeros(eng.S, eng.t.n, 1)
        rows = torch.as_tensor(np.asarray(marked, dtype=np.int64), device=full.device)
        full[rows] = vecs
        v, ok = self._orthonormalize(full)
        mask = torch.zeros(eng.S, dtype=torch.bool, device=full.device)
        mask[rows] = True
        ok_host = self._append_columns(v, ok & mask)
        return [bool(ok_host[i]) for i in marked]

    def _gram_schmidt_extend(self, U):
        """Extend EVERY local basis by the columns of U [S, n, L], one after the other (all-or-nothing per column)."""
        for k in range(U.shape[2]):
            v, ok = self._orthonormalize(U[:, :, k:k + 1])
            if not bool(ok.all()):
                raise ExtensionError('snapshot block is (numerically) in the span of its local basis')
            self._append_columns(v, ok)

    def extend_basis(self, U, method='gram_schmidt', pod_modes=None):
        """Restrict a global snapshot to every subdomain and extend all local bases (the fork's ``extend_basis``;
        online_adaptive_lrbms.py:117-121); all-or-nothing: ``ExtensionError`` if a block is in the span of its basis.
        ``method='pod'`` (pyMOR's ``extend_basis(U, method='pod', pod_modes=k)``): ``extend_basis_pod(U, modes=pod_modes)``;
        ``method='hapod'``: ``extend_basis_hapod(U, modes=pod_modes)``, the streamed POD of a training set of any size."""
        if method == 'pod':
            return self.extend_basis_pod(U, modes=pod_modes)
        if method == 'hapod':
            return self.extend_basis_hapod(U, modes=pod_modes)
        if method != 'gram_schmidt':
            raise ValueError("extend_basis: method is 'gram_schmidt', 'pod' or 'hapod', not {!r}".format(method))
        self._gram_schmidt_extend(self._as_slab(U))

    # ------------------------------------------------------------------ POD extension
    POD_MAX_COLUMNS = 128               # snapshots per native call (lrbms_local_pod: L <= 128)
    POD_MAX_WIDTH = 64                  # slab width the native call takes (and the fused pass: N <= 64)
    POD_MIN_RTOL = 1e-7                 # below it the Gram route resolves nothing (include/lrbms_hip.h)

    def _pod_product(self):
        """The local product in the form the context's ``local_pod`` takes."""
        raise NotImplementedError

    def _pod_width(self, width):
        """The slab width that holds ``width`` vectors (a subclass rounds as its ``reserve`` does)."""
        return width

    def _pod_max_width(self):
        """The widest slab a POD extension pads to (a subclass lowers it to what its pass takes)."""
        return self.POD_MAX_WIDTH

    def _pod_mark_dirty(self, idx):
        """Record the local subdomains ``idx`` as changed since the last ``reduce()`` (``_dirty`` of the subclass)."""

    def _pod_slab(self, U):
        """``U`` as one slab [S, n, L]: a trajectory / block array, a ready-made slab, or a list of those, stacked along the
        column axis in the order given."""
        import torch
        if isinstance(U, (list, tuple)):
            if not U:
                raise ValueError('extend_basis_pod: no snapshots')
            return torch.cat([self._pod_slab(u) for u in U], dim=2).contiguous()
        if isinstance(U, torch.Tensor) and U.dim() == 3:
            return U.contiguous()
        return self._as_slab(U).contiguous()

    def _pod_call(self, Uc, k, rtol, atol):
        """One ``local_pod`` call on the chunk ``Uc`` [S, n, L <= 128] with at most ``k`` new vectors per subdomain: pads the slab to
        the width the call may need, runs it, adds the counts to ``_nloc`` and marks the grown subdomains dirty.  Returns
        ``(sv, added, info)``; the device-to-host copy of the counts is the one synchronisation."""
        import torch
        eng = self.d.engine
        S = eng.S
        need = self._pod_width(min(int(self._nloc[:S].max()) + k, self._pod_max_width()))
        if need > self._V.shape[2]:
            self._V = torch.nn.functional.pad(self._V, (0, need - self._V.shape[2])).contiguous()
        nloc = torch.as_tensor(np.ascontiguousarray(self._nloc[:S], dtype=np.int32)).to(self._V.device)
        sv, ai = eng.ctx.local_pod(self._pod_product(), Uc, self._V, nloc, k, rtol, atol)
        added, info = ai.cpu().numpy().astype(np.int64)
        self._nloc[:S] += added
        self._pod_mark_dirty(np.where(added > 0)[0])
        return sv, added, info

    def _pod_cut_back(self, width0):
        """Cut the slab back to what was filled, but never below ``width0``, its width before the POD calls."""
        top = int(self._nloc.max())
        keep = width0 if top <= width0 else self._pod_width(top)     # (nothing past the old width: the slab is as it was)
        if self._V.shape[2] > keep:                                  # columns past every nloc[s] are zero
            self._V = self._V[:, :, :keep].contiguous()

    def _extend_marked_pod(self, rows_host, corr, pod_modes, rtol):
        """The POD step of the parabolic reductors' ``enrich_local_batch`` (2D and 3D): the corrector trajectories ``corr``
        [len(rows_host), n, nt] of the local subdomains ``rows_host`` are scattered into a zero slab [S, n, nt] and compressed by
        the local POD against the current bases, at most ``pod_modes`` new vectors per marked subdomain; chunks of 128 columns, each
        against the basis the previous one has grown, a later chunk with only the subdomains that have room left.  Returns the
        number of vectors gained per local subdomain [S]."""
        import torch
        eng = self.d.engine
        rows = torch.as_tensor(rows_host, device=corr.device)
        slab = eng.ctx.zeros(eng.S, eng.t.n, corr.shape[2])
        slab[rows] = corr
        if self._V is None:
            self._V = eng.ctx.zeros(eng.S, eng.t.n, 0)
            self._nloc = np.zeros(eng.S, dtype=np.int64)
        width0 = self.basis_size()
        gained = np.zeros(eng.S, dtype=np.int64)
        room = np.zeros(eng.S, dtype=np.int64)
        room[rows_host] = int(pod_modes)
        failed = None
        for c0 in range(0, slab.shape[2], self.POD_MAX_COLUMNS):
            room_c = room.copy()                                                      # the room at the start of this chunk
            for k in sorted(set(int(v) for v in room_c[room_c > 0]), reverse=True):   # (the first chunk: one call, k = pod_modes)
                Uc = slab[:, :, c0:c0 + self.POD_MAX_COLUMNS].clone()
                Uc[torch.as_tensor(np.where(room_c != k)[0], device=Uc.device)] = 0.0
                _, added, info = self._pod_call(Uc, min(k, Uc.shape[2]), rtol, 0.0)
                gained += added
                room -= added
                if info.any():
                    failed = np.where(info != 0)[0]
                    break
            if failed is not None:
                break
        self._pod_cut_back(width0)
        if failed is not None:
            raise RuntimeError('enrich_local_batch: the eigen-solver reported info != 0 on local subdomains {}'.format(failed.tolist()))
        return gained

    def extend_basis_pod(self, U, modes=None, rtol=1e-6, atol=0.0):
        """POD extension of every local basis, the batched method of snapshots per subdomain (``lrbms_local_pod`` /
        ``lrbms3_local_pod``): the snapshots are deflated against the local basis in the local product and at most ``modes`` of
        their leading POD modes, those with a singular value above ``max(atol, rtol * max_j |u_j|)``, are appended,
        product-orthonormal among themselves and to the basis.  Snapshots in the span of a basis add nothing there.

        ``U``: a trajectory, a slab [S, n, L], or a list of those (stacked along the column axis).  More than 128 columns run as
        consecutive calls of at most 128 columns, in order, each against the basis the previous one has grown, with ``modes`` as
        the cap of every call: a HIERARCHICAL compression, not one global POD of all columns.  ``modes=None``: as many as pass
        the threshold and fit.  The slab is padded to the width the call may need (at most 64; 3D: 64 // Q, the limit of the pass, as
        ``reserve``) and cut back to what was filled.

        Purely local: no communication, so it works on a sharded discretization as it is; halo rows of a slab that carries
        them are not touched.  One device-to-host copy of the added counts per native call is the only synchronisation.
        Returns ``(sv, added)`` as NumPy arrays: the singular values of the deflated snapshots [S, L], descending per call
        (the calls side by side), and the number of vectors added per subdomain.  ``ExtensionError`` if nothing was added."""
        eng = self.d.engine
        S = eng.S
        U = self._pod_slab(U)
        if U.dim() != 3 or U.shape[0] != S or U.shape[1] != eng.t.n or U.shape[2] < 1:
            raise ValueError('extend_basis_pod: snapshots [S = {}, n = {}, L >= 1] expected, got {}'.format(S, eng.t.n, tuple(U.shape)))
        if modes is not None and int(modes) < 1:
            raise ValueError('extend_basis_pod: modes must be >= 1')
        if not rtol >= self.POD_MIN_RTOL:
            raise ValueError('extend_basis_pod: rtol < 1e-7: the Gram matrix squares the singular values, below that they are noise')
        if not atol >= 0.0:
            raise ValueError('extend_basis_pod: atol must be >= 0')
        self._pod_product()                                          # (a reductor without such a product refuses here)
        if self._V is None:
            self._V = eng.ctx.zeros(S, eng.t.n, 0)
            self._nloc = np.zeros(S, dtype=np.int64)
        width0 = self.basis_size()
        svs, total = [], np.zeros(S, dtype=np.int64)
        failed = None
        for c0 in range(0, U.shape[2], self.POD_MAX_COLUMNS):
            Uc = U[:, :, c0:c0 + self.POD_MAX_COLUMNS].contiguous()
            k = Uc.shape[2] if modes is None else min(int(modes), Uc.shape[2])
            sv, added, info = self._pod_call(Uc, k, rtol, atol)
            total += added
            svs.append(sv)
            if info.any():
                failed = np.where(info != 0)[0]
                break
        self._pod_cut_back(width0)
        if failed is not None:
            raise RuntimeError('extend_basis_pod: the eigen-solver reported info != 0 on local subdomains {}'.format(failed.tolist()))
        if total.sum() == 0:
            raise ExtensionError('no snapshot block extends its local basis')
        return np.concatenate([sv.cpu().numpy() for sv in svs], axis=1), total

    # ------------------------------------------------------------------ streamed POD extension (HAPOD)
    last_pod_info = None                # {'columns', 'nodes', 'lost'} of the last extend_basis_hapod

    def _hapod_items(self, U):
        """The slabs [S, n, C] of ``U`` in the order given: a trajectory / block array, a ready-made slab, or a list / iterator of
        those.  Nothing is stacked."""
        import collections.abc
        import torch
        if isinstance(U, torch.Tensor) and U.dim() == 3:
            yield U
        elif isinstance(U, (list, tuple, collections.abc.Iterator)):
            for u in U:
                yield from self._hapod_items(u)
        else:
            yield self._as_slab(U)

    def extend_basis_hapod(self, U, modes=None, rtol=1e-6, atol=0.0, keep=64):
        """POD extension of every local basis by a training set of ANY size (``lrbms_local_pod_stream_*``, the incremental
        hierarchical approximate POD of Himpe, Leibner and Rave 2018, per subdomain): the items of ``U`` -- a trajectory, a block
        array or a slab [S, n, C], or a list or iterator of those, e.g. ``d.solve_batch(mus, as_snapshots='slabs')`` -- are pushed
        one after the other in the order given, in pieces of at most ``128 - keep`` columns, and never concatenated; per subdomain
        at most ``keep`` scaled modes are carried from piece to piece.  At the end at most ``modes`` modes of the WHOLE set, those
        above ``max(atol, rtol * max_j |u_j|)``, are appended as ``extend_basis_pod`` appends them (``modes=None``: as many as pass
        and fit).  While no piece has more than ``keep`` directions above the Gram route's noise floor the result is the POD of all
        columns whatever the chunking; in any case the squared projection error of the deflated set is at most
        ``last_pod_info['lost']`` per subdomain.

        Slab padding and cut-back, reserved columns, ``_dirty``, ``ExtensionError`` and the ``RuntimeError`` on ``info`` are those of
        ``extend_basis_pod``.  Purely local (works on a sharded discretization as it is).  One device-to-host copy at the end is
        the only synchronisation, however many columns were pushed.  Returns ``(sv, added)`` as NumPy arrays: the singular values
        of the carried panel [S, keep], descending, and the number of vectors added per subdomain; ``last_pod_info`` =
        ``{'columns', 'nodes', 'lost'}`` (columns pushed, native pushes, ``lost`` [S])."""
        import torch
        eng = self.d.engine
        S = eng.S
        keep = int(keep)
        if not 1 <= keep <= self.POD_MAX_WIDTH:
            raise ValueError('extend_basis_hapod: keep must be in [1, 64]')
        if modes is not None and int(modes) < 1:
            raise ValueError('extend_basis_hapod: modes must be >= 1')
        if not rtol >= self.POD_MIN_RTOL:
            raise ValueError('extend_basis_hapod: rtol < 1e-7: the Gram matrix squares the singular values, below that they are noise')
        if not atol >= 0.0:
            raise ValueError('extend_basis_hapod: atol must be >= 0')
        P = self._pod_product()
        items = self._hapod_items(U)
        first = next(items, None)
        if first is None:
            raise ValueError('extend_basis_hapod: no snapshots')
        if self._V is None:
            self._V = eng.ctx.zeros(S, eng.t.n, 0)
            self._nloc = np.zeros(S, dtype=np.int64)
        width0 = self.basis_size()
        k = keep if modes is None else min(int(modes), keep)
        need = self._pod_width(min(int(self._nloc[:S].max()) + k, self._pod_max_width()))
        if need > self._V.shape[2]:
            self._V = torch.nn.functional.pad(self._V, (0, need - self._V.shape[2])).contiguous()

        def cut_back():
            top = int(self._nloc.max())
            width = width0 if top <= width0 else self._pod_width(top)   # (nothing past the old width: the slab is as it was)
            if self._V.shape[2] > width:                                # columns past every nloc[s] are zero
                self._V = self._V[:, :, :width].contiguous()

        try:
            nloc = torch.as_tensor(np.ascontiguousarray(self._nloc[:S], dtype=np.int32)).to(self._V.device)
            stream = eng.ctx.local_pod_stream(P, self._V, nloc, keep=keep, cmax=self.POD_MAX_COLUMNS - keep)
            item = first
            while item is not None:
                if item.dim() != 3 or item.shape[0] != S or item.shape[1] != eng.t.n or item.shape[2] < 1:
                    raise ValueError('extend_basis_hapod: snapshots [S = {}, n = {}, C >= 1] expected, got {}'.format(
                        S, eng.t.n, tuple(item.shape)))
                stream.push(item)
                item = next(items, None)
            sv, ai, lost = stream.finish(k, rtol, atol)
            host = torch.cat([ai.to(sv.dtype).t(), lost[:, None], sv], dim=1).cpu().numpy()      # the one synchronisation
            added, info = host[:, 0].astype(np.int64), host[:, 1].astype(np.int64)
            self._nloc[:S] += added
            self._pod_mark_dirty(np.where(added > 0)[0])
            self.last_pod_info = {'columns': int(stream.columns), 'nodes': int(stream.nodes), 'lost': host[:, 2].copy()}
        finally:
            cut_back()
        if info.any():
            raise RuntimeError('extend_basis_hapod: the eigen-solver reported info != 0 on local subdomains {}'.format(
                np.where(info != 0)[0].tolist()))
        if added.sum() == 0:
            raise ExtensionError('no snapshot block extends its local basis')
        return host[:, 3:].copy(), added

    def _extend_basis_trajectory(self, U, max_vectors=None, method='gram_schmidt', pod_modes=None):
        """``extend_basis`` of the parabolic reductors: the vectors of a trajectory are Gram-Schmidt-ed into the local bases one
        after the other, a vector that is numerically in the span of a local basis is skipped for that subdomain (pyMOR
        ``gram_schmidt`` semantics), at most until the slab is ``max_vectors`` wide; ``ExtensionError`` if nothing was added.
        ``method='pod'``: the leading ``pod_modes`` POD modes of the whole trajectory instead of its first vectors
        (``extend_basis_pod``; with ``max_vectors`` no local basis grows past it); ``method='hapod'``: the same through
        ``extend_basis_hapod``, for any number of snapshots (``U`` may be the list of ``solve_batch(mus, as_snapshots='slabs')``)."""
        if method in ('pod', 'hapod'):
            if max_vectors is not None:
                room = int(max_vectors) - (0 if self._nloc is None else int(self._nloc[:self.d.engine.S].max()))
                if room < 1:
                    raise ExtensionError('no snapshot block extends its local basis')
                pod_modes = room if pod_modes is None else min(int(pod_modes), room)
            if method == 'hapod':
                return self.extend_basis_hapod(U, modes=pod_modes)
            return self.extend_basis_pod(U, modes=pod_modes)
        if method != 'gram_schmidt':
            raise ValueError("extend_basis: method is 'gram_schmidt', 'pod' or 'hapod', not {!r}".format(method))
        U = self._as_slab(U)
        added = 0
        for k in range(U.shape[2]):
            if max_vectors is not None and self.basis_size() >= max_vectors:
                break
            v, ok = self._orthonormalize(U[:, :, k:k + 1])
            added += int(self._append_columns(v, ok).sum())
        if added == 0:
            raise ExtensionError('no snapshot block extends its local basis')


class ReducedDiscretization:
    """``rd``: block-sparse reduced system + projected estimator operators, resident in HBM.

    With a parameter-dependent affine source (``d._affine_f``) ``rhs_red_K [K, S, N]`` and ``r_fd_K [K, S, 5 Q N]`` hold the
    projected components (``LRBMSReductor.reduce``); what the pass projected from ``sum_j f_j`` belongs to no parameter, so such a
    model exposes ``rhs_red = None`` and ``operators['r_fd'] = None``."""

    rhs_red_K = r_fd_K = None

    def __init__(self, reductor, buffers, N):
        import torch
        self.reductor, self.d, self.N = reductor, reductor.d, N
        eng = self.d.engine
        self.B_sys, self.rhs_red, self.E_red, self.M_red = buffers['sys']      # owned by this reduced model (no copies:
        self.grams = tuple(buffers['grams'])                                    # the reductor allocates fresh outputs)
        self.estimator = self.d.estimator
        self.parameter_space = self.d.parameter_space

        class _Space:
            dim = int(sum(reductor.local_sizes())) if eng.S == eng.grid.num_subdomains else eng.grid.num_subdomains * N
        self.solution_space = _Space
        self.operator = type('Op', (), {'source': _Space, 'range': _Space})
        self._operators = None
        self.products = {'l2': self.M_red}
        self._torch = torch

    @property
    def operators(self):
        """The projected estimator operators as block arrays (reference: ``rd.operators``, projected at reductor.py:70).
        The kernels keep the blocks that involve a neighbour slot in factored form (``self.grams``, 8 tensors); the dense
        block-compact arrays are built on first access only -- the estimate never needs them."""
        if self._operators is None:
            from pylrbms_amd.engine import expand_factored_grams
            g = expand_factored_grams(self.grams)
            self._operators = {'nc': g[0], 'r_fd': None if self._affine() else g[1], 'r_dd': g[2], 'df_bb': g[3], 'df_ab': g[4],
                               'df_aa': g[5], 'local_energy_dg_product': self.E_red}
        return self._operators

    def parse_parameter(self, mu):
        return self.d.parse_parameter(mu)

    def _reference_theta(self):
        """theta at the middle of the parameter range (the reference parameter of the prebuilt preconditioner)."""
        ps = self.parameter_space
        mid = 0.5 * (ps.minimum + ps.maximum)
        mu = {k: np.full(shape, mid) for k, shape in ps.parameter_type.items()}
        return self.d.theta(mu)

    def _solve_with_preconditioner(self, ctx, B_sys, fn):
        """Run ``fn()`` (reduced solves on ``ctx``) with this model's two-level preconditioner, built once at the middle
        of the parameter range (``lrbms_reduced_precond_build``; any SPD preconditioner is admissible)."""
        cache = self.__dict__.setdefault('_pc', {})
        if id(ctx) not in cache:
            cache[id(ctx)] = ctx.reduced_precond_build(self._reference_theta(), B_sys)
        ctx.reduced_precond_use(cache[id(ctx)])
        try:
            return fn()
        finally:
            ctx.reduced_precond_use(None)

    def _affine(self):
        """The stationary path's affine source is projected into this model (parabolic models keep their own reading)."""
        return self.rhs_red_K is not None and getattr(self.d, '_affine_f', None) is not None

    def solve(self, mu, inverse_options=None):
        """``rd.solve(mu)`` (online_adaptive_lrbms.py:141): (sum_q theta_q A_q^red) u = b^red.  The reference does a
        dense LU of the unblocked matrix; here PCG on the block-sparse system (``lrbms_reduced_solve``) with the inverse
        diagonal blocks plus a coarse level on the first local basis vectors as preconditioner.  With an affine source
        b^red(mu) = sum_j theta^f_j(mu) rhs_red_K[j] (``lrbms_combine_sources``)."""
        eng = self.d.engine
        theta = self.d.theta(mu)
        if self._affine():
            rhs = eng.ctx.combine_sources(self.d.f_coefficients(mu), self.rhs_red_K)
            u, info = self._solve_with_preconditioner(eng.ctx, self.B_sys, lambda: eng.reduced_solve(theta, self.B_sys, rhs))
            self.last_solve_info = info
            return ReducedVectorArray(u.reshape(eng.S, self.N, 1))
        if eng.S_ext != eng.S:
            ctx, B_all, rhs_all = self._global_online()
            u, info = self._solve_with_preconditioner(ctx, B_all, lambda: ctx.reduced_solve(theta, B_all, rhs_all))
            self.last_solve_info = info
            u = u[self._torch.as_tensor(eng.local, device=u.device)]
            return ReducedVectorArray(u.reshape(eng.S, self.N, 1))
        u, info = self._solve_with_preconditioner(eng.ctx, self.B_sys, lambda: eng.reduced_solve(theta, self.B_sys, self.rhs_red))
        self.last_solve_info = info
        return ReducedVectorArray(u.reshape(eng.S, self.N, 1))

    def solve_batch(self, mus):
        """Parameter sweep: ``len(mus)`` reduced solutions, <= 64 per ``lrbms_reduced_solve_batch`` call (the library runs them as
        groups of 16 on its own streams); returns one ``ReducedVectorArray`` with ``len(mus)`` vectors."""
        eng = self.d.engine
        thetas = np.array([self.d.theta(mu) for mu in mus])
        if self._affine():                                   # a right-hand side of its own per parameter (single rank)
            phis = np.array([self.d.f_coefficients(mu) for mu in mus])
            u = self._solve_with_preconditioner(
                eng.ctx, self.B_sys, lambda: eng.ctx.reduced_solve_batches_src(thetas, phis, self.B_sys, self.rhs_red_K)[0])
            return ReducedVectorArray(u)
        # sharded: on the gathered reduced system, like solve(); every rank keeps the rows of its own subdomains
        ctx, B_sys, rhs = self._global_online() if eng.S_ext != eng.S else (eng.ctx, self.B_sys, self.rhs_red)

        def run():
            return ctx.reduced_solve_batches(thetas, B_sys, rhs)[0]
        u = self._solve_with_preconditioner(ctx, B_sys, run)
        if eng.S_ext != eng.S:
            u = u[self._torch.as_tensor(eng.local, device=u.device)]
        return ReducedVectorArray(u)

    def _global_online(self):
        """Sharded discretization: the reduced system is small (S x 5 blocks of N x N per affine component), so every rank
        gathers all of it once (one all-gather each for B_sys and rhs_red) and solves redundantly on its own GPU through
        a second library context that holds the GLOBAL neighbour table.  Returns (context, B_sys, rhs_red) in global order."""
        if getattr(self, '_online', None) is None:
            from pylrbms_amd._native import NativeContext
            from pylrbms_amd.grid import DDSubdomainsGrid
            from pylrbms_amd.parallel import gather_subdomain_rows
            eng = self.d.engine
            g = eng.grid
            group = getattr(self.d.mpi_comm, 'group', None)
            owned = [list(DDSubdomainsGrid(g.lower_left, g.upper_right, g.K, g.P, rank=r, world_size=g.world_size).subdomains_on_rank)
                     for r in range(g.world_size)]
            total = g.num_subdomains
            B = gather_subdomain_rows(self.B_sys.permute(1, 0, 2, 3, 4).contiguous(), owned, total, group)
            rhs = gather_subdomain_rows(self.rhs_red, owned, total, group)
            ctx = NativeContext(eng.ctx.device.index)
            nbr = np.asarray(g.neighbor_slots, dtype=np.int32).reshape(total, 5)
            ctx.mesh_upload(eng.t, eng.kappa, nbr, total, total)
            self._online = (ctx, B.permute(1, 0, 2, 3, 4).contiguous(), rhs.contiguous())
        return self._online

    def _local_estimates(self, U, mu):
        if self._affine():
            return self._local_estimates_affine(U, mu)
        torch = self._torch
        eng = self.d.engine
        theta = self.d.theta(mu)
        u_all = U.tensor                                                   # [S, N, len(U)]
        if eng.S_ext != eng.S:
            # halo coefficients: every rank contributes its rows to a global [S_total, N, len] table (one all-reduce),
            # then picks the rows of its ext ordering
            import torch.distributed as dist
            table = torch.zeros(eng.grid.num_subdomains, self.N, u_all.shape[2], dtype=u_all.dtype, device=u_all.device)
            table[torch.as_tensor(eng.local, device=u_all.device)] = u_all
            dist.all_reduce(table, group=getattr(self.d.mpi_comm, 'group', None))
            u_all = table[torch.as_tensor(eng.ext, device=u_all.device)]
        cols = []
        for c0 in range(0, u_all.shape[2], 16):                            # the batched estimate takes <= 16 vectors
            u = u_all[:, :, c0:c0 + 16].contiguous()
            L = u.shape[2]
            if L == 1:
                cols.append(eng.reduced_estimate(theta, u[:, :, 0].contiguous(), self.grams)[:, :, None])
            else:
                cols.append(eng.ctx.reduced_estimate_batch(np.tile(theta, (L, 1)), u, self.grams, eng.f2, eng.ceps, eng.hdiam))
        eta = torch.cat(cols, dim=2)
        return eta[0], eta[1], eta[2]

    def _local_estimates_affine(self, U, mu):
        """With an affine source: the batched estimate with f2 = 0 and r_fd = 0 plus ``lrbms_reduced_source_terms`` on r_fd_K and
        F2 with the row theta^f(mu) for every column (the reduced counterpart of DuneDiscretization._local_estimates_affine)."""
        torch = self._torch
        eng = self.d.engine
        theta = self.d.theta(mu)
        phi = self.d.f_coefficients(mu)
        u_all = U.tensor                                                   # [S, N, len(U)]
        zero_f2 = eng.ctx.zeros(eng.S)
        grams = list(self.grams)
        grams[1] = torch.zeros_like(grams[1])
        grams = tuple(grams)
        cols = []
        for c0 in range(0, u_all.shape[2], 16):
            u = u_all[:, :, c0:c0 + 16].contiguous()
            L = u.shape[2]
            eta = eng.ctx.reduced_estimate_batch(np.tile(theta, (L, 1)), u, grams, zero_f2, eng.ceps, eng.hdiam)
            eta[1] += eng.ctx.reduced_source_terms(theta, np.tile(phi, (L, 1)), self.d._affine_f['F2'], self.r_fd_K, u, eng.ceps,
                                                   eng.hdiam)
            cols.append(eta)
        eta = torch.cat(cols, dim=2)
        return eta[0], eta[1], eta[2]

    def estimate(self, U, mu=None, decompose=False):
        """``rd.estimate(u, mu=, decompose=)``: same code path as the full-order estimate (estimators.py:45-112) with
        the reduced operators (reduced OI = identity, reduced FR = theta-weighted identities, reductor.py:44-66)."""
        return self.estimator.estimate(U, self.parse_parameter(mu), self, decompose=decompose)


    def estimate_batch(self, U, mus, decompose=False):
        """``estimate`` for a parameter sweep: ``U`` holds one solution per parameter -- the array ``solve_batch(mus)`` returns
        (``len(mus)`` vectors), a tensor ``[len(mus), S, N]`` or a list of single-vector arrays --, 64 parameters per
        ``lrbms_reduced_estimate_batch`` call (plus ``lrbms_reduced_source_terms`` with an affine source).  Returns the list of what
        ``estimate(U_m, mu_m, decompose=decompose)`` returns."""
        torch = self._torch
        eng = self.d.engine
        mus = [self.parse_parameter(mu) for mu in mus]
        if isinstance(U, (list, tuple)):
            u_all = torch.cat([(u.tensor if hasattr(u, 'tensor') else u.reshape(eng.S, self.N, 1)) for u in U], dim=2)
        elif hasattr(U, 'tensor'):
            u_all = U.tensor                                               # [S, N, len(mus)]
        else:
            u_all = U.permute(1, 2, 0)                                     # [len(mus), S, N]
        assert tuple(u_all.shape) == (eng.S, self.N, len(mus)), 'estimate_batch: one solution per parameter'
        if eng.S_ext != eng.S:
            return [self.estimate(ReducedVectorArray(u_all[:, :, m:m + 1].contiguous()), mu, decompose=decompose)
                    for m, mu in enumerate(mus)]
        est = self.estimator
        affine = self._affine()
        grams = list(self.grams)
        f2 = eng.f2
        if affine:
            grams[1] = torch.zeros_like(grams[1])
            f2 = eng.ctx.zeros(eng.S)
        cols = []
        for b0 in range(0, len(mus), 64):
            chunk = mus[b0:b0 + 64]
            u = u_all[:, :, b0:b0 + len(chunk)].contiguous()
            thetas = np.array([self.d.theta(mu) for mu in chunk])
            eta = eng.ctx.reduced_estimate_batch(thetas, u, tuple(grams), f2, eng.ceps, eng.hdiam)
            if affine:                                                     # the source rows: theta enters, so one call per parameter
                for m, mu in enumerate(chunk):
                    eta[1, :, m:m + 1] += eng.ctx.reduced_source_terms(thetas[m], self.d.f_coefficients(mu)[None], self.d._affine_f['F2'],
                                                                       self.r_fd_K, u[:, :, m:m + 1].contiguous(), eng.ceps, eng.hdiam)
            cols.append(eta)
        eta = torch.cat(cols, dim=2)                                       # [3, S, len(mus)]
        if est.sqrt_local:
            eta = eta.abs().sqrt()
        sq = torch.stack([(eta[0] ** 2).sum(dim=0), ((eta[1] + eta[2]) ** 2).sum(dim=0)]).sqrt().cpu().numpy()      # ONE copy
        loc = eta.cpu().numpy() if decompose else None
        out = []
        for m, mu in enumerate(mus):
            alpha_bar = est.alpha(est.lambda_coeffs, mu, est.mu_bar)
            gamma_bar = est.gamma(est.lambda_coeffs, mu, est.mu_bar)
            alpha_hat = est.alpha(est.lambda_coeffs, mu, est.mu_hat)
            e = (np.sqrt(gamma_bar) * float(sq[0, m]) + (1. / np.sqrt(alpha_hat)) * float(sq[1, m])) * 1. / np.sqrt(alpha_bar)
            if not decompose:
                out.append(e)
                continue
            nc, r, df = (np.ascontiguousarray(loc[i][:, m:m + 1]) for i in range(3))
            ind = np.array([(2. / alpha_bar) * (gamma_bar * nc[ii] ** 2 + (1. / alpha_hat) * (r[ii] + df[ii]) ** 2)
                            for ii in range(est.num_subdomains)])
            out.append((e, (nc, r, df), ind))
        return out


class LRBMSReductor(LocalBasisSlab):

    def __init__(self, d, bases=None, products=None, order=None, num_cpus=1, solver_options=None):
        assert order is None or 0 <= order <= 1
        self.d = d
        self.solver_options = solver_options
        self.products = products            # the local energy products; applied through the engine's P_diag
        self.num_cpus = num_cpus            # accepted and ignored, as in the reference (reductor.py:19)
        eng = d.engine
        if bases is not None:
            self._V = self._bases_to_tensor(bases)
            self._nloc = self._nloc_in
        if order is None and bases is None:
            order = 0
        if order is not None:
            for ii in eng.local:            # reductor.py:29-31
                self.extend_basis_local(d.shape_functions(ii, order), _defer=True)
            self._flush_local()

    # ------------------------------------------------------------------ bases
    def _bases_to_tensor(self, bases):
        import torch
        eng = self.d.engine
        blocks = []
        for ii in eng.local:
            b = bases['domain_{}'.format(ii)]
            t = b.tensor[0] if isinstance(b, BlockVectorArray) else eng.ctx.from_numpy(np.asarray(b).T)
            blocks.append(t)
        nmax = max(int(b.shape[1]) for b in blocks)
        self._nloc_in = np.array([int(b.shape[1]) for b in blocks], dtype=np.int64)
        blocks = [torch.nn.functional.pad(b, (0, nmax - int(b.shape[1]))) for b in blocks]   # ragged: zero columns
        return torch.stack(blocks).contiguous()

    @property
    def bases(self):
        """dict space id -> array, as ``reductor.bases`` (keys 'domain_i'; after reduce() also 'OI_i', 'RT_i')."""
        eng = self.d.engine
        out = {}
        for i, ii in enumerate(eng.local):
            space = BlockVectorSpace([self.d.solution_space.subspaces[i]])
            out['domain_{}'.format(ii)] = (BlockVectorArray(self._V[i:i + 1, :, :int(self._nloc[i])], space)
                                           if self._V is not None else None)
        out.update(getattr(self, '_image_bases', {}))
        return out

    def _product_apply(self, X):
        """P X with P the local energy product (block-ELL) -- the product handed in at online_adaptive_lrbms.py:107."""
        return self.d.engine.ctx.blockell_apply(self.d.engine.P_diag, X.contiguous())

    def _as_slab(self, U):
        return U.tensor

    def _pod_product(self):
        return self.d.engine.P_diag

    def _pod_width(self, width):
        return int(width) + (int(width) & 1)          # even, as reserve() pads: the lean kernels of the fused pass take even N

    def _pod_mark_dirty(self, idx):
        local = self.d.engine.local
        self._dirty = getattr(self, '_dirty', set()) | {int(local[i]) for i in idx}

    def reserve(self, width):
        """Room for local bases of up to ``width`` vectors: pads the slab with zero columns (to an even width: the lean kernels
        of the fused pass take even N).  Zero columns project to zero rows / columns, so every result is unchanged; what changes is
        that later extensions fill existing columns, the slab keeps its width and ``reduce(touched=...)`` can update in place."""
        import torch
        width = int(width) + (int(width) & 1)
        if self._V is not None and width > self._V.shape[2]:
            self._V = torch.nn.functional.pad(self._V, (0, width - self._V.shape[2])).contiguous()
        return self.basis_size()

    def _append_columns(self, v, ok):
        ok_host = super()._append_columns(v, ok)
        local = self.d.engine.local          # _dirty: global ids of the subdomains whose basis changed since the last reduce()
        self._dirty = getattr(self, '_dirty', set()) | {int(local[i]) for i in np.where(ok_host)[0]}
        return ok_host

    def extend_basis_local(self, U, _defer=False):
        """Reference reductor.py:31,78: extend the basis of the ONE subdomain the single-block array ``U`` lives on.
        ``_defer`` collects one vector per subdomain (constructor, reductor.py:29-31) and extends all at once."""
        if _defer:
            self._pending = getattr(self, '_pending', [])
            self._pending.append(U.tensor)
            return
        eng = self.d.engine
        ii = int(str(U.space.subspaces[0].id).split('_')[1])
        ok = self._extend_marked([eng.local.index(ii)], U.tensor[:, :, :1])
        if not ok[0]:
            raise ExtensionError('local correction is (numerically) in the span of the local basis')

    def _flush_local(self):
        import torch
        pend = getattr(self, '_pending', [])
        if pend:
            self._gram_schmidt_extend(torch.cat(pend, dim=0))
            self._pending = []

    # ------------------------------------------------------------------ reduce
    def reduce(self, touched=None):
        """``reductor.reduce()`` (reductor.py:33-73).  ``touched``: global ids of the subdomains whose local bases changed since the
        previous ``reduce()`` -- on ANY rank of a sharded discretization (the marking of online_enrichment.py:38-47 is global) --:
        only they and their neighbours are re-projected, into the arrays of the previous reduced model, which the returned model
        shares (the previous one is superseded, as in the reference's loop, online_enrichment.py:52).  Falls back to the whole pass
        when there is no previous model of the same width or the fused pass does not support the shape."""
        return self._reduce(touched=touched)

    def _reduce(self, touched=None):
        d = self.d
        eng = d.engine
        if self._V is None:
            raise RuntimeError('no basis')
        N = self.basis_size()
        if eng.S_ext != eng.S:
            # sharded: after an enrichment round the widest local basis may live on another rank; the basis slabs
            # travel through the halo exchange, so every rank pads to the global width (one max all-reduce)
            import torch
            import torch.distributed as dist
            if dist.is_initialized():
                width = torch.tensor([N], dtype=torch.int64, device=self._V.device)
                staged = dist.get_backend(getattr(d.mpi_comm, 'group', None)) == 'gloo'
                if staged:
                    width = width.cpu()
                dist.all_reduce(width, op=dist.ReduceOp.MAX, group=getattr(d.mpi_comm, 'group', None))
                N = int(width.item())
            if N > self._V.shape[2]:
                self._V = torch.nn.functional.pad(self._V, (0, N - self._V.shape[2])).contiguous()
        V = d._with_halo(self._V)
        dirty = getattr(self, '_dirty', set())
        self._dirty = set()
        last = getattr(self, '_last_reduce', None)
        if (touched is not None and last is not None and last['N'] == N and len(last['grams']) == 8
                and eng.ctx.fused_supported(eng.Q, N, factored=True)):
            # incremental: the targets whose neighbourhood holds a changed basis, written into the previous model's arrays
            subset = eng.touched_targets(set(int(g) for g in touched) | dirty)
            eng.project_and_estimate(V, last, subset=subset)
            self.last_reduce_info = {'incremental': True, 'subdomains': len(subset)}
            return self._with_affine_source(ReducedDiscretization(self, last, N), V, last)
        if getattr(self, '_buffers', None) is None or self._buffers['N'] != N:
            self._buffers = eng.alloc_reduce_buffers(N)                   # scratch (and image bases if unfused): reused
        buf = dict(self._buffers)
        buf.update(eng.alloc_outputs(N))                                  # outputs: fresh, handed over to the reduced model
        buf = eng.project_and_estimate(V, buf)
        self._buffers['Wt'], self._buffers['Rt'] = buf['Wt'], buf['Rt']
        if buf['Wt'] is not None:                                         # only the unfused kernels materialise them
            self._image_bases = {'OI': buf['Wt'], 'RT': buf['Rt']}      # target-major image bases (device tensors)
        self._last_reduce = buf
        self.last_reduce_info = {'incremental': False, 'subdomains': eng.S}
        return self._with_affine_source(ReducedDiscretization(self, buf, N), V, buf)

    def _with_affine_source(self, rd, V, buf):
        """The K components of the stationary path's affine source projected like rhs_red / r_fd (``lrbms_project_sources`` on
        the basis and the divergence of its RT0 reconstruction images), into ``rd.rhs_red_K`` / ``rd.r_fd_K``.  On every
        subdomain, also after an incremental re-projection: the arrays are those of a whole ``reduce()``.  They live in the
        reduce buffers ``buf`` like the rest of the model, so an incremental reduce writes them in place and a previous model
        sharing those buffers stays consistent (as its B_sys and Grams do)."""
        src = getattr(self.d, '_affine_f', None)
        if src is not None:
            eng = self.d.engine
            V = V.contiguous()
            D = eng.ctx.div_apply(eng.ctx.flux_reconstruct(eng.F, V), mode=0)
            K, N = int(src['K']), int(V.shape[2])
            out = buf.get('src')
            if out is None or tuple(out[0].shape) != (K, eng.S, N):
                out = (eng.ctx.empty(K, eng.S, N), eng.ctx.empty(K, eng.S, 5 * eng.Q * N))
            rd.rhs_red_K, rd.r_fd_K = buf['src'] = eng.ctx.project_sources(eng.Q, src['b_K'], V, D, out=out)
            rd.rhs_red = None                                             # the projection of sum_j f_j: no parameter's
        return rd

    def image_bases(self):
        """The image bases the reference keeps as ``bases['OI_i']`` / ``bases['RT_i']`` (reductor.py:40-60), target-major:
        ``Wt`` [S, n, 5 N], ``Rt`` [S, n_rt, 5 Q N].  The fused pass never forms them; this applies K7 / K8 on demand."""
        eng = self.d.engine
        V = self.d._with_halo(self._V)
        Wt = eng.ctx.oswald_apply(V)
        Rt = eng.ctx.flux_reconstruct(eng.F, V)
        self._image_bases = {'OI': Wt, 'RT': Rt}
        return self._image_bases

    def reconstruct(self, u):
        import torch
        coef = u.tensor if hasattr(u, 'tensor') else u
        return BlockVectorArray(torch.einsum('snk,skl->snl', self._V, coef), self.d.solution_space)

    def reconstruct_local(self, u, space_id):
        i = self.d.engine.local.index(int(space_id.split('_')[1]))
        rec = self.reconstruct(u)
        return rec.block(i)

    def enrich_local(self, subdomain, U, mu=None):
        """Reference reductor.py:75-78: corrector solve on the neighbourhood of ``subdomain``, then extend its basis."""
        Us = None   # reconstruct_local of the neighbourhood (reductor.py:76) feeds only the commented-out Dirichlet lift
        local_correction = self.d.solve_for_local_correction(subdomain, Us, mu, inverse_options=self.solver_options)
        self.extend_basis_local(local_correction)

    def enrich_local_batch(self, subdomains, U, mu=None):
        """The loop of online_enrichment.py:49-50 as one batched corrector solve + one masked Gram-Schmidt step.
        Returns the list of subdomains whose basis grew (a correction already in the span of its basis is skipped)."""
        subdomains = [int(ii) for ii in subdomains]
        if not subdomains:
            return []
        eng = self.d.engine
        corrections = self.d.solve_for_local_corrections(subdomains, mu, inverse_options=self.solver_options)
        import torch
        vecs = torch.cat([c.tensor for c in corrections], dim=0)
        ok = self._extend_marked([eng.local.index(ii) for ii in subdomains], vecs)
        return [ii for ii, flag in zip(subdomains, ok) if flag]


class ParallelLRBMSReductor(LRBMSReductor):
    """Reference reductor.py:81-146: at HEAD ``_reduce`` returns the serial result (the Allreduce code after the
    early ``return`` at :125 is dead), so this is the same reductor with an ``mpi_comm``."""

    def __init__(self, d, bases=None, products=None, order=None, solver_options=None, mpi_comm=None):
        super().__init__(d, bases=bases, products=products, solver_options=solver_options, num_cpus=1, order=order)
        self.mpi_comm = mpi_comm


class InstationaryReducedDiscretization(ReducedDiscretization):
    """The reduced instationary model of the parabolic path: reduced implicit Euler (``lrbms_reduced_implicit_euler``, the
    whole trajectory in one native call) and the same ``ParabolicEstimator`` with the projected operators."""

    rhs_red_K = r_fd_K = None     # the projected source components (time-dependent source: ParabolicLRBMSReductor.reduce)

    def __init__(self, reductor, buffers, N):
        super().__init__(reductor, buffers, N)
        self.T, self.time_stepper = self.d.T, self.d.time_stepper
        self.mass = self.M_red

    def _tv(self):
        """The diffusion coefficients depend on time (theta_q(t, mu)): the ``_tv`` exports, one column for ``solve`` /
        ``estimate``."""
        return bool(getattr(self.d, '_tv', False))

    def solve(self, mu, inverse_options=None):
        eng = self.d.engine
        dt = self.T / self.time_stepper.nt
        if self._tv():
            U = self.solve_batch([mu])[0]
            return ReducedVectorArray(U.tensor.contiguous())
        if self.rhs_red_K is not None:                               # time-dependent source: sum_j phi[k+1][j] rhs_red_K[j]
            U, info = eng.ctx.reduced_implicit_euler_src(self.d.theta(mu), dt, self.time_stepper.nt, self.B_sys, self.M_red,
                                                         self.rhs_red_K, self.d._phi_device(mu))
            self.last_solve_info = info
            return ReducedVectorArray(U.permute(1, 2, 0))
        if eng.S_ext != eng.S:                                       # sharded: on the gathered reduced system, like rd.solve
            from pylrbms_amd.parallel import gather_subdomain_rows
            ctx, B_all, rhs_all = self._global_online()
            U, info = ctx.reduced_implicit_euler(self.d.theta(mu), dt, self.time_stepper.nt, B_all, self._gathered_mass(), rhs_all)
            U = U[:, self._torch.as_tensor(eng.local, device=U.device)]
        else:
            U, info = eng.ctx.reduced_implicit_euler(self.d.theta(mu), dt, self.time_stepper.nt, self.B_sys, self.M_red,
                                                     self.rhs_red)
        self.last_solve_info = info
        return ReducedVectorArray(U.permute(1, 2, 0))

    def solve_batch(self, mus):
        """Parameter sweep over the parabolic reduced model: one ``lrbms_reduced_implicit_euler_batch(_src)`` call per 64
        parameters (every time step is one panel PCG for all of them); returns a list with, per parameter, the
        ``ReducedVectorArray`` that ``solve(mu)`` returns, so ``estimate(U_m, mu_m)`` takes an entry as it is.  The entries of a
        call are views of its panel ``[nt + 1, S, N, nmu]`` (column m): ``estimate_batch`` takes the panel back without a copy."""
        eng = self.d.engine
        if eng.S_ext != eng.S:
            raise NotImplementedError('solve_batch of the parabolic reduced model needs all subdomains on one rank '
                                      '(lrbms_reduced_implicit_euler_batch: S_ext == S); solve(mu) works on a sharded discretization')
        mus = list(mus)
        nt = self.time_stepper.nt
        dt = self.T / nt
        out, its, rel = [], 0, 0.0
        for b0 in range(0, len(mus), 64):
            chunk = mus[b0:b0 + 64]
            if self._tv():                                           # a theta row per step; phi beside it with a time-dependent source
                theta_t = np.stack([self.d.diffusion_coefficients(mu) for mu in chunk])
                if self.rhs_red_K is not None:
                    phi = self._torch.stack([self.d._phi_device(mu) for mu in chunk]).contiguous()
                    U, info = eng.ctx.reduced_implicit_euler_batch_tv(theta_t, dt, nt, self.B_sys, self.M_red, self.rhs_red_K, phi=phi)
                else:
                    U, info = eng.ctx.reduced_implicit_euler_batch_tv(theta_t, dt, nt, self.B_sys, self.M_red, self.rhs_red)
                its, rel = its + info['iterations'], max(rel, info['relative_residual'])
                out += [ReducedVectorArray.view_of(U[..., m].permute(1, 2, 0)) for m in range(len(chunk))]
                continue
            thetas = np.array([self.d.theta(mu) for mu in chunk])
            if self.rhs_red_K is not None:                           # time-dependent source: a coefficient table per parameter
                phi = self._torch.stack([self.d._phi_device(mu) for mu in chunk]).contiguous()
                U, info = eng.ctx.reduced_implicit_euler_batch_src(thetas, dt, nt, self.B_sys, self.M_red, self.rhs_red_K, phi)
            else:
                U, info = eng.ctx.reduced_implicit_euler_batch(thetas, dt, nt, self.B_sys, self.M_red, self.rhs_red)
            its, rel = its + info['iterations'], max(rel, info['relative_residual'])
            out += [ReducedVectorArray.view_of(U[..., m].permute(1, 2, 0)) for m in range(len(chunk))]     # views of ONE panel
        self.last_solve_info = {'iterations': its, 'relative_residual': rel}
        return out

    def _panel_of(self, Us):
        """The panel [nt + 1, S, N, len(Us)] of a chunk of trajectories: the entries' own storage when they are the column views
        ``solve_batch`` built on one panel (no copy), otherwise stacked."""
        torch = self._torch
        nt1, S, N, nmu = self.time_stepper.nt + 1, self.d.engine.S, self.N, len(Us)
        ts = [u.tensor if hasattr(u, 'tensor') else u for u in Us]
        for t in ts:
            assert tuple(t.shape) == (S, N, nt1), 'estimate_batch: every trajectory is [S, N, nt + 1]'
        base = getattr(ts[0], '_base', None)
        if (base is not None and tuple(base.shape) == (nt1, S, N, nmu) and base.is_contiguous()
                and all(getattr(t, '_base', None) is base and t.stride() == (N * nmu, nmu, S * N * nmu)
                        and t.data_ptr() == base.data_ptr() + m * base.element_size() for m, t in enumerate(ts))):
            return base
        return torch.stack([t.permute(2, 0, 1) for t in ts], dim=3).contiguous()

    def estimate_batch(self, Us, mus):
        """The parabolic estimates of a parameter sweep in one native call per 64 parameters (``lrbms_reduced_parabolic_estimate_batch``;
        DESIGN.md 5.4.4).  ``Us``: the list ``solve_batch(mus)`` returned (its entries are views of one panel, which is used without
        a copy) or a panel tensor ``[nt + 1, S, N, len(mus)]``.  Returns the list of what ``estimate(U_m, mu_m)`` returns:
        ``(est, (local_eta_nc [S, nt + 1], local_eta_r, local_eta_df, time_residual [nt], time_deriv_nc [S, nt]))`` as NumPy
        arrays; everything stays on the device until ONE copy per output at the end.  With ``estimator.elliptic_reconstruction`` the
        per-trajectory loop runs instead."""
        eng = self.d.engine
        if eng.S_ext != eng.S:
            raise NotImplementedError('estimate_batch of the parabolic reduced model needs all subdomains on one rank '
                                      '(lrbms_reduced_parabolic_estimate_batch: S_ext == S); estimate(U, mu) works on a sharded '
                                      'discretization')
        mus = [self.parse_parameter(mu) for mu in mus]
        est = self.estimator
        nt = self.time_stepper.nt
        dt = self.T / nt
        panel = None
        if not isinstance(Us, (list, tuple)):
            panel = Us
            assert tuple(panel.shape) == (nt + 1, eng.S, self.N, len(mus)), 'estimate_batch: the panel is [nt + 1, S, N, len(mus)]'
        else:
            assert len(Us) == len(mus), 'estimate_batch: one trajectory per parameter'
        if getattr(est, 'elliptic_reconstruction', False) or self._affine():
            if panel is not None:
                Us = [ReducedVectorArray.view_of(panel[..., m].permute(1, 2, 0)) for m in range(len(mus))]
            return [self.estimate(U, mu) for U, mu in zip(Us, mus)]
        out = []
        for b0 in range(0, len(mus), 64):
            chunk = mus[b0:b0 + 64]
            U = panel[..., b0:b0 + len(chunk)].contiguous() if panel is not None else self._panel_of(Us[b0:b0 + len(chunk)])
            if self._tv():
                thetas = np.stack([self.d.diffusion_coefficients(mu) for mu in chunk])      # [len(chunk), nt + 1, Q]
                coef = np.stack([self.d._estimator_coefficients(mu) for mu in chunk])       # [len(chunk), nt + 1, 2]
                native = eng.ctx.reduced_parabolic_estimate_batch_tv
            else:
                thetas = np.array([self.d.theta(mu) for mu in chunk])
                coef = np.empty((len(chunk), 2))
                native = eng.ctx.reduced_parabolic_estimate_batch
                for m, mu in enumerate(chunk):
                    alpha_bar = est.alpha(est.lambda_coeffs, mu, est.mu_bar)
                    gamma_bar = est.gamma(est.lambda_coeffs, mu, est.mu_bar)
                    alpha_hat = est.alpha(est.lambda_coeffs, mu, est.mu_hat)
                    coef[m] = np.sqrt(gamma_bar) / np.sqrt(alpha_bar), (1. / np.sqrt(alpha_hat)) / np.sqrt(alpha_bar)
            src = {}
            if self.rhs_red_K is not None:
                src = dict(phi=self._torch.stack([self.d._phi_device(mu) for mu in chunk]).contiguous(), F2=self.d._src['F2'],
                           r_fd_K=self.r_fd_K)
            res = native(thetas, coef, dt, nt, U, self.B_sys, self.M_red, self.grams, eng.f2, eng.ceps, eng.hdiam,
                         sqrt_local=est.sqrt_local, **src)
            loc, tdn, tr, e = (res[k].cpu().numpy() for k in ('eta_loc', 'time_deriv_nc', 'time_residual', 'est'))
            for m in range(len(chunk)):
                out.append((float(e[m]), tuple(np.ascontiguousarray(loc[i, :, :, m].T) for i in range(3))
                            + (np.ascontiguousarray(tr[:, m]), np.ascontiguousarray(tdn[:, :, m].T))))
        return out

    def estimate(self, U, mu=None, decompose=False):
        """``(est, (local_eta_nc, local_eta_r, local_eta_df, time_residual, time_deriv_nc))``; with ``decompose=True`` a third entry
        ``indicators [S]``, what ``AdaptiveEnrichment`` marks subdomains with (``local_indicators``)."""
        if self._tv():
            if decompose:
                raise NotImplementedError('estimate(decompose=True): the diffusion coefficients depend on time (theta_q(t, mu)); '
                                          'alpha / gamma of the local indicators would change from step to step')
            return self.estimate_batch([U], [mu])[0]                 # one column of lrbms_reduced_parabolic_estimate_batch_tv
        est, parts = ReducedDiscretization.estimate(self, U, mu, decompose=False)
        if not decompose:
            return est, parts
        return est, parts, self.local_indicators(parts, mu)

    def local_indicators(self, parts, mu):
        """Per-subdomain indicators [S] of a parabolic estimate, from its ``parts``: per step the expression of the stationary
        ``estimate(decompose=True)`` (estimators.py:105-109: ``2 / alpha_bar (gamma_bar nc^2 + (r + df)^2 / alpha_hat)``, the same
        alpha / gamma and convention switches) on that step's ``(nc, r, df)`` columns, summed over the steps, plus
        ``sum_k time_deriv_nc[s, k]^2``.  The time-stepping residual is a global ``M^-1`` norm and has no local share, so the
        indicators do not sum to the estimate: a marking heuristic, not a bound."""
        est = self.estimator
        mu = self.parse_parameter(mu)
        nc, r, df, _, time_deriv_nc = parts
        alpha_bar = est.alpha(est.lambda_coeffs, mu, est.mu_bar)
        gamma_bar = est.gamma(est.lambda_coeffs, mu, est.mu_bar)
        alpha_hat = est.alpha(est.lambda_coeffs, mu, est.mu_hat)
        elliptic = (2. / alpha_bar) * (gamma_bar * nc ** 2 + (1. / alpha_hat) * (r + df) ** 2)        # [S, nt + 1]
        return elliptic.sum(axis=1) + (time_deriv_nc ** 2).sum(axis=1)

    def _local_estimates(self, U, mu):
        """With a time-dependent source: the reduced counterpart of InstationaryDuneDiscretization._local_estimates -- the
        batched estimate with f2 = 0, r_fd = 0 plus ``lrbms_reduced_source_terms`` on rhs_red_K's companions r_fd_K, F2."""
        if self.rhs_red_K is None:
            return ReducedDiscretization._local_estimates(self, U, mu)
        torch = self._torch
        eng = self.d.engine
        theta = self.d.theta(mu)
        u_all = U.tensor                                                   # [S, N, len(U)]
        rows = self.d._source_rows(mu, u_all.shape[2])
        zero_f2 = eng.ctx.zeros(eng.S)
        grams = list(self.grams)
        grams[1] = torch.zeros_like(grams[1])
        grams = tuple(grams)
        cols = []
        for c0 in range(0, u_all.shape[2], 16):
            u = u_all[:, :, c0:c0 + 16].contiguous()
            L = u.shape[2]
            eta = eng.ctx.reduced_estimate_batch(np.tile(theta, (L, 1)), u, grams, zero_f2, eng.ceps, eng.hdiam)
            if rows is not None:
                eta[1] += eng.ctx.reduced_source_terms(theta, rows[c0:c0 + L].contiguous(), self.d._src['F2'], self.r_fd_K, u,
                                                       eng.ceps, eng.hdiam)
            cols.append(eta)
        eta = torch.cat(cols, dim=2)
        return eta[0], eta[1], eta[2]

    def _gathered_mass(self):
        if getattr(self, '_M_all', None) is None:
            from pylrbms_amd.parallel import gather_subdomain_rows
            self._M_all = gather_subdomain_rows(self.M_red, self.d._owned_subdomains(), self.d.engine.grid.num_subdomains,
                                                getattr(self.d.mpi_comm, 'group', None)).contiguous()
        return self._M_all

    def _time_residual_norm2(self, dU, mu):
        eng = self.d.engine
        if eng.S_ext != eng.S:                                       # sharded: a global sum, on the gathered reduced system
            from pylrbms_amd.parallel import gather_subdomain_rows
            ctx, B_all, _ = self._global_online()
            dU_all = gather_subdomain_rows(dU.tensor.contiguous(), self.d._owned_subdomains(), eng.grid.num_subdomains,
                                           getattr(self.d.mpi_comm, 'group', None))
            out = ctx.reduced_time_residual(self.d.theta(mu), B_all, self._gathered_mass(), dU_all.permute(2, 0, 1).contiguous())
            return out.sum(dim=1).cpu().numpy()
        out = eng.ctx.reduced_time_residual(self.d.theta(mu), self.B_sys, self.M_red, dU.tensor.permute(2, 0, 1).contiguous())
        return out.sum(dim=1).cpu().numpy()

    def _projected_r_ud(self):
        """``V_s^T M_s Div_s Rt_s`` [S, N, 5 Q N]: the projection of ``r_ud_s`` (discretize_parabolic_block_swipdg.py:65-70)
        onto the local basis and the RT image basis, built on first use from K8, ``lrbms_div_apply`` and ``lrbms_gemm_tn``."""
        if getattr(self, '_G_ud', None) is None:
            eng = self.d.engine
            V = self.reductor._V.contiguous()
            MD = eng.ctx.div_apply(eng.ctx.flux_reconstruct(eng.F, V), mode=1)               # [S, n, 5 Q N]
            self._G_ud = eng.ctx.gemm_tn(V, MD)
        return self._G_ud

    def _reconstruction_terms(self, U, mu):
        """The elliptic-reconstruction terms with the projected operators (``lrbms_reduced_reconstruction_terms``) -> [S, len(U)]."""
        eng = self.d.engine
        if eng.S_ext != eng.S:
            raise NotImplementedError('the elliptic-reconstruction terms need all subdomains on one rank')
        out = eng.ctx.reduced_reconstruction_terms(self.d.theta(mu), self.B_sys, self.M_red, self.rhs_red, self._projected_r_ud(),
                                                   U.tensor.permute(2, 0, 1).contiguous())
        return out.t().contiguous()


class ParabolicLRBMSReductor(LRBMSReductor):
    """The reductor python/scripts/parabolic.py:9,42-45 asks for (imported there from ``dune.pylrbms.estimators``, where
    it does not exist at HEAD).  Same bases and projection as ``LRBMSReductor``; ``extend_basis`` takes a trajectory:
    its vectors are Gram-Schmidt-ed into the local bases one after the other, vectors that are numerically in the span
    of a local basis are skipped for that subdomain (pyMOR ``gram_schmidt`` semantics), ``ExtensionError`` if nothing
    was added anywhere; ``reduce()`` returns the instationary reduced model."""

    extend_basis = LocalBasisSlab._extend_basis_trajectory

    def enrich_local(self, subdomain, U, mu=None, pod_modes=1, rtol=1e-6):
        """``enrich_local_batch`` for the one subdomain; ``ExtensionError`` if its basis did not grow."""
        if not self.enrich_local_batch([subdomain], U, mu, pod_modes=pod_modes, rtol=rtol):
            raise ExtensionError('the local corrector trajectory is (numerically) in the span of the local basis')

    def enrich_local_batch(self, subdomains, U, mu=None, pod_modes=1, rtol=1e-6):
        """Online enrichment of the parabolic reduced model.  The stationary reductor adds the ONE
        elliptic corrector of a marked subdomain; here the corrector is a trajectory: implicit Euler on the neighbourhood of every
        marked subdomain with the time stepping, source and parameter of ``solve(mu)``
        (``d.solve_for_local_correction_trajectories``, all marked subdomains and all steps in one launch), compressed by the local
        POD against the current basis in the local energy product (``lrbms_local_pod``): at most ``pod_modes`` new vectors per marked
        subdomain, those with a singular value above ``rtol`` times the largest snapshot norm.

        The trajectories are scattered into a zero slab [S, n, nt]: a zero column has an exact zero singular value, so an unmarked
        subdomain gains nothing and its slab keeps its bits.  ``nt > 128`` runs in consecutive chunks of 128 columns as
        ``extend_basis_pod`` does, each against the basis the previous one has grown; a later chunk sees only the subdomains
        that have room left under ``pod_modes``.  ``U`` (the current reduced solution) is accepted and unused, as in the stationary
        reductor.  Returns the subdomains whose basis grew (they are marked dirty for ``reduce(touched=)``); adding nothing is
        not an error here."""
        subdomains = [int(ii) for ii in subdomains]
        if not subdomains:
            return []
        if int(pod_modes) < 1:
            raise ValueError('enrich_local_batch: pod_modes must be >= 1')
        if not rtol >= self.POD_MIN_RTOL:
            raise ValueError('enrich_local_batch: rtol < 1e-7: the Gram matrix squares the singular values, below that they are noise')
        eng = self.d.engine
        corr = self.d.solve_for_local_correction_trajectories(subdomains, mu, inverse_options=self.solver_options)   # [nmark, n, nt]
        rows_host = np.array([eng.local.index(ii) for ii in subdomains], dtype=np.int64)
        gained = self._extend_marked_pod(rows_host, corr, pod_modes, rtol)
        return [ii for ii, i in zip(subdomains, rows_host) if gained[i] > 0]

    def _reduce(self, touched=None):
        rd = super()._reduce(touched=touched)
        out = InstationaryReducedDiscretization(self, {'sys': (rd.B_sys, rd.rhs_red, rd.E_red, rd.M_red), 'grams': rd.grams},
                                                rd.N)
        src = getattr(self.d, '_src', None)
        if src is not None:
            # the K source components projected like rhs_red / r_fd: one lrbms_project_sources launch on the basis and the
            # divergence of its RT0 reconstruction images (lrbms_flux_reconstruct -> lrbms_div_apply mode 0)
            eng = self.d.engine
            V = self._V.contiguous()
            D = eng.ctx.div_apply(eng.ctx.flux_reconstruct(eng.F, V), mode=0)
            out.rhs_red_K, out.r_fd_K = eng.ctx.project_sources(eng.Q, src['b_K'], V, D)
        return out
