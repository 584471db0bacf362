"""NumPy restatement of the streamed local POD (incremental HAPOD; DESIGN.md 5.6.1, include/lrbms_hip.h:
lrbms_local_pod_stream_begin / _push / _finish) for one subdomain with a dense local product, the carried panel P B included, and
the inputs the host and the GPU tests share.  The single-call reference, the SVD in the product and the exact inputs come from
tests/local_pod_ref.py."""
import numpy as np

from local_pod_ref import (EPS, NOISE, RESOLVED, SIGMA_TOL, deflate, make_case, orthonormality, p_orthonormal,  # noqa: F401
                           product_svd, projection_error2, ragged_nloc, sigma_error, span_defect, spd_products, sym)

POD_MIN_RTOL = 1e-7                     # the noise floor of the Gram route (csrc/lrbms_pod.h)

# (L_total, cmax, keep): no node sees more than keep directions above its floor -> the POD of all columns
EXACT_CHUNKINGS = ((65, 64, 64), (200, 64, 64), (330, 17, 64), (130, 1, 64), (200, 64, 32), (200, 7, 12))
# (n, keep, L_total, cmax): every node with more than keep columns truncates
TRUNCATING_CASES = ((96, 8, 200, 64), (96, 8, 200, 17), (60, 5, 130, 7), (24, 5, 130, 1))
TRUNCATING_SEED = 5                     # of make_truncating_case: the gap condition holds with a margin (host tests)
GAP_MIN = 1e-3                        # (lam_keep - lam_keep+1) / lam_1 at every truncating node of the truncating inputs


def _eigh_desc(G):
    lam, Z = np.linalg.eigh(sym(G))
    order = np.argsort(-lam, kind='stable')
    return lam[order], Z[:, order]


class StreamOne:
    """begin .. push .. finish for ONE subdomain: V [n, Nw] with nloc P-orthonormal columns, dense P [n, n].  ``nodes`` records per
    push the eigenvalues and the retained count.  ``noise`` = (rng, eps): every Gram matrix is perturbed by a symmetric random matrix
    of size eps max|G| (the sensitivity study of the host tests)."""

    def __init__(self, V, nloc, P, keep, cmax, noise=None):
        assert 1 <= keep <= 64 and cmax >= 1 and keep + cmax <= 128
        self.V, self.nloc, self.P, self.keep, self.cmax, self.noise = V, int(nloc), P, keep, cmax, noise
        self.begin()

    def begin(self):
        n, Lx = self.V.shape[0], self.keep + self.cmax
        self.X, self.PX = np.zeros((n, Lx)), np.zeros((n, Lx))
        self.kb, self.lost, self.norm0sq, self.columns, self.nodes = 0, 0.0, 0.0, 0, []

    def _gram(self, A, PA):
        G = sym(A.T @ PA)
        if self.noise is not None:
            rng, eps = self.noise
            G = G + eps * np.abs(G).max() * sym(rng.uniform(-1.0, 1.0, G.shape))
        return G

    def push(self, U):
        P, V, keep = self.P, self.V, self.keep
        C = U.shape[1]
        assert 1 <= C <= self.cmax
        self.norm0sq = max(self.norm0sq, max(float(np.einsum('ij,ij->j', U, P @ U).max()), 0.0))      # 1
        R = deflate(U, V, P)                                                                           # 2
        self.X[:, keep:], self.PX[:, keep:] = 0.0, 0.0                                                 # 3
        self.X[:, keep:keep + C], self.PX[:, keep:keep + C] = R, P @ R
        lam, Z = _eigh_desc(self._gram(self.X, self.PX))
        cnt = 0                                                                                        # 4
        while cnt < len(lam) and cnt < keep and lam[cnt] > 0.0 and lam[cnt] > POD_MIN_RTOL ** 2 * lam[0]:
            cnt += 1
        self.lost += float(np.maximum(lam[cnt:], 0.0).sum())
        T = np.zeros((len(lam), keep))                                                                 # 5
        T[:, :cnt] = Z[:, :cnt]
        self.X[:, :keep], self.PX[:, :keep] = self.X @ T, self.PX @ T
        self.kb = cnt
        self.columns += C
        self.nodes.append(dict(lam=lam, kb=cnt, truncates=bool(cnt == keep and len(lam) > keep and lam[keep] > POD_MIN_RTOL ** 2 * lam[0])))

    def finish(self, modes, rtol=1e-6, atol=0.0):
        """(V_new, sv [keep], added, lost); the state is left as it is."""
        P, V, keep, nloc = self.P, self.V, self.keep, self.nloc
        B, PB = self.X[:, :keep], self.PX[:, :keep]
        lam, Z = _eigh_desc(self._gram(B, PB))                                                         # 1
        sv = np.sqrt(np.maximum(lam, 0.0))
        thr = max(atol, rtol * np.sqrt(self.norm0sq))
        k = int(min(np.count_nonzero(sv > thr), modes, V.shape[1] - nloc))                             # 2
        lost = self.lost + float(np.maximum(lam[k:], 0.0).sum())                                       # 3
        Vn = V.copy()
        if k > 0:                                                                                      # 4
            W = B @ (Z[:, :k] / sv[:k])
            W = W - V @ (V.T @ (P @ W))
            l2, Z2 = np.linalg.eigh(sym(W.T @ (P @ W)))
            Vn[:, nloc:nloc + k] = W @ ((Z2 / np.sqrt(l2)) @ Z2.T)
        return Vn, sv, k, lost


def chunks(L, cmax):
    return [(c0, min(c0 + cmax, L)) for c0 in range(0, L, cmax)]


def stream_ref(U, V, nloc, P, keep, cmax, modes, rtol=1e-6, atol=0.0, noise=None):
    """The batched stream on U [S, n, L] pushed in pieces of cmax columns.  Returns a dict: V, nloc, sv [S, keep], added, lost [S],
    kb [pushes, S] and the per-subdomain StreamOne objects (``streams``)."""
    S = U.shape[0]
    streams = [StreamOne(V[s], nloc[s], P[s], keep, cmax, noise) for s in range(S)]
    kb = []
    for c0, c1 in chunks(U.shape[2], cmax):
        for s in range(S):
            streams[s].push(U[s][:, c0:c1])
        kb.append([st.kb for st in streams])
    Vn, sv, added, lost = V.copy(), np.zeros((S, keep)), np.zeros(S, dtype=np.int64), np.zeros(S)
    for s in range(S):
        Vn[s], sv[s], added[s], lost[s] = streams[s].finish(modes, rtol, atol)
    return dict(V=Vn, nloc=np.asarray(nloc[:S]) + added, sv=sv, added=added, lost=lost, kb=np.array(kb), streams=streams)


def node_margin(streams):
    """Smallest factor between sqrt(lam_j / lam_1) of any node and the floor 1e-7, over the subdomains."""
    worst = np.inf
    for st in streams:
        for node in st.nodes:
            lam = node['lam']
            if lam[0] <= 0.0:
                continue
            ratio = np.sqrt(np.maximum(lam, 0.0) / lam[0]) / POD_MIN_RTOL
            ratio = np.maximum(ratio, 1.0 / np.maximum(ratio, 1e-300))
            worst = min(worst, float(ratio.min()))
    return worst


def final_margin(U, V, nloc, P, rtol=1e-6):
    """Smallest factor between a singular value of all deflated columns and the threshold rtol norm0, over the subdomains."""
    worst = np.inf
    for s in range(U.shape[0]):
        thr = rtol * np.sqrt(np.einsum('ij,ij->j', U[s], P[s] @ U[s]).max())
        sig, _ = product_svd(deflate(U[s], V[s], P[s]), P[s])
        ratio = np.maximum(sig / thr, thr / np.maximum(sig, 1e-300))
        worst = min(worst, float(ratio.min()))
    return worst


def node_gap(streams, keep):
    """Smallest (lam_keep - lam_keep+1) / lam_1 over the nodes that truncate (inf if none does)."""
    worst = np.inf
    for st in streams:
        for node in st.nodes:
            if node['truncates']:
                lam = node['lam']
                worst = min(worst, float((lam[keep - 1] - lam[keep]) / lam[0]))
    return worst


def make_truncating_case(P, L, Nw, seed=0, nloc=None, directions=30):
    """Inputs whose nodes truncate: per subdomain min(directions, n - nloc) directions outside span(V) with sigma_j = 10^(-0.1 j),
    mixed into ALL L columns by a random orthonormal factor, plus an O(1) part in span(V).  Returns (U, V, nloc, sigma [S][...])."""
    S, n = P.shape[0], P.shape[1]
    rng = np.random.default_rng(seed + 31 * L + 1000 * Nw + 7)
    nloc = ragged_nloc(S, Nw) if nloc is None else np.asarray(nloc, dtype=np.int64)
    U, V, sig_all = np.zeros((S, n, L)), np.zeros((S, n, Nw)), []
    for s in range(S):
        r = min(directions, L, n - int(nloc[s]))
        B = p_orthonormal(rng.standard_normal((n, int(nloc[s]) + r)), P[s])
        V[s][:, :nloc[s]] = B[:, :nloc[s]]
        sig = 10.0 ** (-0.1 * np.arange(r))
        O = np.linalg.qr(rng.standard_normal((L, r)))[0].T                       # r orthonormal rows
        U[s] = B[:, nloc[s]:] @ (sig[:, None] * O)
        if nloc[s]:
            U[s] += B[:, :nloc[s]] @ rng.uniform(0.5, 1.5, (int(nloc[s]), L))
        sig_all.append(sig)
    return U, V, nloc, sig_all


# --------------------------------------------------------------------------------------------------------------------------------
class FakeStream:
    """``LocalPodStream`` by the restatement on CPU tensors (host tests of the reductors)."""

    def __init__(self, ctx, P, V, nloc, keep, cmax):
        self.ctx, self.P, self.V, self.nloc, self.keep, self.cmax = ctx, P, V, nloc, keep, cmax
        self.columns = self.nodes = 0
        S = nloc.shape[0]
        self.width, self.nloc0 = int(V.shape[2]), nloc.numpy().copy()
        self.streams = [StreamOne(V[s].numpy().copy(), int(nloc[s]), P[s], keep, cmax) for s in range(S)]
        self.pushed, self.finishes = [], []

    def push(self, U):
        assert U.dim() == 3
        for c0 in range(0, U.shape[2], self.cmax):
            Uc = U[:, :, c0:c0 + self.cmax].contiguous().numpy()
            self.pushed.append(Uc.copy())
            for s, st in enumerate(self.streams):
                st.push(Uc[s])
            self.columns += Uc.shape[2]
            self.nodes += 1

    def finish(self, modes, rtol=1e-6, atol=0.0):
        torch = self.ctx.torch
        S = len(self.streams)
        assert np.array_equal(self.nloc.numpy(), self.nloc0) and self.V.shape[2] == self.width      # V and nloc did not change
        sv, added, lost = np.zeros((S, self.keep)), np.zeros(S, dtype=np.int32), np.zeros(S)
        for s, st in enumerate(self.streams):
            Vn, sv[s], added[s], lost[s] = st.finish(modes, rtol, atol)
            self.V[s] = torch.from_numpy(Vn)
        self.nloc += torch.from_numpy(added)
        self.finishes.append(dict(modes=int(modes), rtol=rtol, atol=atol))
        return torch.from_numpy(sv), torch.stack([torch.from_numpy(added), torch.zeros(S, dtype=torch.int32)]), torch.from_numpy(lost)
