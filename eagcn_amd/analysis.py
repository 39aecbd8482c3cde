"""The evaluation-time consumers of the atom representations, on the device: the dump of train.py:213-287 (``dump_atom_rep``: the
representations of the atoms whose sub-type lies in 1..18, with their sub-type and molecule index, plus the per-molecule graph
representations / indices / labels / predictions) and the k-means clustering the reference's analysis runs over that dump on the host
(kmeans_atomrep.py: ``kmeans_for_atom`` -> sklearn KMeans, compared with the atoms' sub-types through a confusion matrix).

The reference copies the padded [B, N, F] matrix of every batch to the host, walks its B x N rows in a Python loop
(train.py:264-268) and hands the result to scikit-learn.  Here the selected rows are gathered straight from the PACKED output of the
last layer behind a device-side row counter (csrc/reps.hip: eagcn_rep_gather; the padded matrix is never formed, nothing is read by the
host until ``finish``), and Lloyd's iterations run as HIP kernels that read every row once per iteration (eagcn_kmeans_*).

One documented deviation from scikit-learn: a cluster that runs EMPTY keeps its centroid (``n_empty`` counts them); scikit-learn
relocates it to the point farthest from its centre.

The second half of that analysis, the two-dimensional embeddings of tsnes.py and mol_to_vec_plot.py, is here as well: ``pca`` and an
EXACT ``tsne`` (csrc/embed.hip) over the rows of the dump -- ``tsne(d.X[subsample(d.subtype, classes, cap)])`` for atoms,
``tsne(d.graph_rep)`` for molecules -- without a copy of the rows to the host.

What one does with a learned fingerprint first, and what says whether an embedding kept the neighbourhoods, are here too (csrc/knn.hip):
``knn`` -- the k nearest rows of every query, exactly, without an n x n matrix: ``d.index[knn(d.graph_rep, 5).indices]`` --,
``neighbor_ranks``, scikit-learn's ``trustworthiness`` / ``continuity`` of an embedding and ``neighbor_agreement`` with a labelling.

And the scores of a clustering, which the reference reads off its confusion-matrix plot by eye (csrc/silhouette.hip): ``silhouette_samples``
/ ``silhouette_score`` without an n x n matrix, ``cluster_moments`` with ``davies_bouldin_score`` and ``calinski_harabasz_score``, and from
the matrix of ``confusion_matrix`` ``adjusted_rand_score``, ``normalized_mutual_info_score`` and ``purity``."""
import ctypes as C
from collections import namedtuple

import torch

from . import _lib as L

RepDump = namedtuple('RepDump', 'X subtype mol_index graph_rep index labels outputs')
KMeansResult = namedtuple('KMeansResult', 'centers labels inertia n_iter n_empty counts init_centers converged')


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class RepBuffers:
    """Device-resident dump of an evaluation pass: X [cap, F] fp32, subtype [cap] int32, mol_index [cap] int64 behind a device row
    counter, grown geometrically on the host-known upper bound of the rows (every appended batch may select all its B x N atoms)."""

    def __init__(self, device, subtype_range=(1, 18), cap=4096):
        self.device = torch.device(device)
        self.lo, self.hi = int(subtype_range[0]), int(subtype_range[1])
        self.cap, self.bound, self.F = int(cap), 0, None
        self.count = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.X = self.sub = self.mol = None
        self._mols = {'graph_rep': [], 'index': [], 'labels': [], 'outputs': []}

    def _reserve(self, extra, F):
        if self.F is None:
            self.F = int(F)
        elif self.F != int(F):
            raise L.EagcnHipError('RepBuffers.append: representations of width %d after width %d' % (F, self.F))
        need = self.bound + extra
        if need >= 2 ** 31:
            raise L.EagcnHipError('RepBuffers.append: %d rows do not fit the 32-bit row index' % need)
        if self.X is not None and need <= self.cap:
            return
        old = None if self.X is None else (self.X[:self.bound], self.sub[:self.bound], self.mol[:self.bound])
        self.cap = max(self.cap, need) if old is None else min(max(2 * self.cap, need), 2 ** 31 - 1)
        self.X = torch.empty((self.cap, self.F), dtype=torch.float32, device=self.device)
        self.sub = torch.empty(self.cap, dtype=torch.int32, device=self.device)
        self.mol = torch.empty(self.cap, dtype=torch.int64, device=self.device)
        if old is not None:
            self.X[:self.bound], self.sub[:self.bound], self.mol[:self.bound] = old

    def append(self, atom_rep, subtype, index, graph_rep=None, labels=None, outputs=None):
        """One batch: `atom_rep` the model's LazyAtomRep (gathered from the packed rows) or a dense device [B, N, F] tensor,
        `subtype` [B, N_in] integer sub-types, `index` [B] molecule indices.  No host synchronisation."""
        lib = L.load()
        subtype = torch.as_tensor(subtype).to(device=self.device, dtype=torch.int32).contiguous()
        index = torch.as_tensor(index).to(device=self.device, dtype=torch.int64).contiguous().view(-1)
        if subtype.dim() != 2 or subtype.shape[0] != index.numel():
            raise L.EagcnHipError('RepBuffers.append: subtype %s and index %s do not describe one batch'
                                  % (tuple(subtype.shape), tuple(index.shape)))
        B, n_in = subtype.shape
        args = getattr(atom_rep, '_args', None) if hasattr(atom_rep, '_ensure') else None
        scratch = torch.empty(B * n_in, dtype=torch.int32, device=self.device)
        if args is not None:
            atom_rep._ensure()
            idx = args[0]
            packed, pad_row, layout = atom_rep.packed
            c = idx.c
            want = c.n_logical if c.n_logical > 0 else c.N
            if (c.B, want) != (B, n_in):
                raise L.EagcnHipError('RepBuffers.append: subtype is [%d, %d], the batch [%d, %d]' % (B, n_in, c.B, want))
            self._reserve(B * n_in, layout.width)
            L.check(lib.eagcn_rep_gather(idx.ref(), packed.data_ptr(), C.byref(layout.c), None if pad_row is None else pad_row.data_ptr(),
                                         subtype.data_ptr(), self.lo, self.hi, index.data_ptr(), self.count.data_ptr(),
                                         scratch.data_ptr(), self.X.data_ptr(), self.sub.data_ptr(), self.mol.data_ptr(), self.cap,
                                         _stream()), 'eagcn_rep_gather')
        else:
            dense = atom_rep.cpu() if hasattr(atom_rep, '_ensure') else atom_rep          # (a LazyAtomRep that was already read)
            dense = torch.as_tensor(dense).to(device=self.device, dtype=torch.float32).contiguous()
            if dense.dim() != 3 or dense.shape[0] != B or dense.shape[1] < n_in:
                raise L.EagcnHipError('RepBuffers.append: atom_rep %s does not match subtype [%d, %d]' % (tuple(dense.shape), B, n_in))
            self._reserve(B * n_in, dense.shape[2])
            L.check(lib.eagcn_rep_gather_dense(dense.data_ptr(), B, dense.shape[1], dense.shape[2], subtype.data_ptr(), n_in, self.lo,
                                               self.hi, index.data_ptr(), self.count.data_ptr(), scratch.data_ptr(), self.X.data_ptr(),
                                               self.sub.data_ptr(), self.mol.data_ptr(), self.cap, _stream()), 'eagcn_rep_gather_dense')
        self.bound += B * n_in
        for name, t in (('graph_rep', graph_rep), ('index', index), ('labels', labels), ('outputs', outputs)):
            if t is not None:
                self._mols[name].append(torch.as_tensor(t).detach().to(self.device).clone())

    def finish(self):
        """Reads the row count (the one host synchronisation).  RepDump of device tensors: X [n, F], subtype [n], mol_index [n] and
        the per-molecule graph_rep / index / labels / outputs (None where nothing was appended)."""
        n = int(self.count.item())
        if self.X is None:
            raise L.EagcnHipError('RepBuffers.finish: nothing has been appended')
        per_mol = [torch.cat(v) if v else None for v in (self._mols[k] for k in ('graph_rep', 'index', 'labels', 'outputs'))]
        return RepDump(self.X[:n], self.sub[:n], self.mol[:n], *per_mol)

    def as_reference(self):
        """The two host lists that train.py:272 and :280 save: [rows, sub-types, molecule indices] (one numpy entry per selected atom)
        and [graph representations, molecule indices [M, 1], labels, predictions]."""
        d = self.finish()
        X, sub, mol = d.X.cpu().numpy(), d.subtype.cpu().numpy().astype('int64'), d.mol_index.cpu().numpy()
        atoms = [[X[i] for i in range(len(X))], [sub[i] for i in range(len(sub))], [mol[i:i + 1] for i in range(len(mol))]]

        def host(t, column=False):
            if t is None:
                return None
            t = t.cpu().numpy()
            return t.reshape(-1, 1) if column else t
        return atoms, [host(d.graph_rep), host(d.index, True), host(d.labels), host(d.outputs)]


@torch.no_grad()
def dump_atom_rep(model, batches, subtype_range=(1, 18), buffers=None):
    """train.py:213-287 on the device: eval-mode forward over `batches`, an iterable of (batch tuple, labels, subtype, index) -- a
    batch tuple that starts with a CompactBonds is (bonds, afms, size), as in training.evaluate -- into a RepBuffers.  The model is
    put back into the mode it was in."""
    was_training = model.training
    model.eval()
    try:
        for batch, labels, subtype, index in batches:
            compact = hasattr(batch[0], 'bond_mol')
            out, atom_rep, graph_rep = model.forward_compact(*batch) if compact else model(*batch)
            if buffers is None:
                buffers = RepBuffers(out.device, subtype_range)
            buffers.append(atom_rep, subtype, index, graph_rep=graph_rep, labels=labels, outputs=out)
    finally:
        model.train(was_training)
    return buffers


# ---- k-means -----------------------------------------------------------------------------------------------------------------------

def _a256(x):
    return (int(x) + 255) & ~255


def workspace_layout(n, F, k):
    """Byte offsets of the caller-visible parts of a k-means workspace (include/eagcn_hip.h): state, centroids, counts, labels, mind."""
    o_cen = 256
    o_cnt = o_cen + _a256(4 * k * F)
    o_lab = o_cnt + 256
    o_mind = o_lab + _a256(4 * n)
    return {'state': 0, 'centers': o_cen, 'counts': o_cnt, 'labels': o_lab, 'mind': o_mind, 'end': o_mind + _a256(4 * n)}


def workspace_bytes(n, F, k):
    """The header's formula for eagcn_kmeans_workspace_bytes, restated (tests compare the two)."""
    G, F4, kk = min(-(-n // 64), 768), L.pad4(F), max(k, 2)
    return workspace_layout(n, F, k)['end'] + _a256(8 * G * kk * F4) + _a256(64 * G) + _a256(4 * G) + _a256(8 * G) + 8192


class _Problem:
    """X as the kernels take it (fp32 device rows with unit column stride, ld >= F) and a workspace with typed views into it."""

    def __init__(self, X, k):
        if not isinstance(X, torch.Tensor) or not X.is_cuda or X.dtype != torch.float32 or X.dim() != 2:
            raise L.EagcnHipError('kmeans: X must be a float32 [n, F] tensor on the MI355X (eagcn_amd has no CPU path)')
        n, F = X.shape
        if n > 1 and (X.stride(1) != 1 or X.stride(0) < F) or n == 1 and X.stride(1) != 1:
            X = X.contiguous()
        self.X, self.n, self.F, self.k = X, int(n), int(F), int(k)
        self.ld = int(X.stride(0)) if n > 1 else int(F)
        self.lib = L.load()
        nbytes = self.lib.eagcn_kmeans_workspace_bytes(self.n, self.F, self.k)
        self.ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=X.device)
        o = workspace_layout(self.n, self.F, self.k)
        self.state_i = self.ws[0:16].view(torch.int32)
        self.state_d = self.ws[16:40].view(torch.float64)
        self.centers = self.ws[o['centers']:o['centers'] + 4 * self.k * self.F].view(torch.float32).view(self.k, self.F)
        self.counts = self.ws[o['counts']:o['counts'] + 4 * self.k].view(torch.int32)
        self.labels = self.ws[o['labels']:o['labels'] + 4 * self.n].view(torch.int32)
        self.mind = self.ws[o['mind']:o['mind'] + 4 * self.n].view(torch.float32)

    def _common(self):
        return (self.X.data_ptr(), self.n, self.F, self.ld, self.k)

    def begin(self, init, tol):
        L.check(self.lib.eagcn_kmeans_begin(*self._common(), init.data_ptr(), float(tol), self.ws.data_ptr(), self.ws.numel(), _stream()),
                'eagcn_kmeans_begin')

    def iterate(self):
        L.check(self.lib.eagcn_kmeans_iterate(*self._common(), self.ws.data_ptr(), self.ws.numel(), _stream()), 'eagcn_kmeans_iterate')

    def finish(self):
        L.check(self.lib.eagcn_kmeans_finish(*self._common(), self.ws.data_ptr(), self.ws.numel(), _stream()), 'eagcn_kmeans_finish')

    def assign(self, centers, labels, mind):
        """labels / minimal squared distances of every row against `centers` [m, F], m <= k"""
        L.check(self.lib.eagcn_kmeans_assign(self.X.data_ptr(), self.n, self.F, self.ld, centers.data_ptr(), centers.shape[0],
                                             labels.data_ptr(), mind.data_ptr(), self.ws.data_ptr(), self.ws.numel(), _stream()),
                'eagcn_kmeans_assign')


def _draw(weights, generator):
    """One index drawn with probability proportional to `weights` (a device vector), without a host read."""
    w = torch.nan_to_num(weights.double(), nan=0.0, posinf=0.0).clamp_min_(0.0)
    w = w + (w.sum() <= 0).to(w.dtype)                       # nothing left to choose by: uniform
    if w.numel() <= 2 ** 24:
        return torch.multinomial(w, 1, generator=generator)
    cdf = torch.cumsum(w, 0)                                 # torch.multinomial stops at 2^24 categories
    u = torch.rand(1, dtype=torch.float64, device=w.device, generator=generator) * cdf[-1]
    return torch.searchsorted(cdf, u).clamp_(max=w.numel() - 1)


def _init_centers(p, init, generator):
    X, n, F, k = p.X, p.n, p.F, p.k
    if isinstance(init, torch.Tensor):
        if tuple(init.shape) != (k, F):
            raise L.EagcnHipError('kmeans: init is %s, not [k, F] = [%d, %d]' % (tuple(init.shape), k, F))
        return init.to(device=X.device, dtype=torch.float32).contiguous().clone()
    if init == 'random':
        rows = torch.randperm(n, device=X.device, generator=generator)[:k]
        return X[rows, :F].contiguous()
    if init != 'k-means++':
        raise ValueError("kmeans: init must be a [k, F] tensor, 'random' or 'k-means++'")
    # plain D^2 sampling, one candidate per step: the next centre is a row drawn with probability proportional to its squared
    # distance to the nearest centre chosen so far (the assign pass's minimal distances)
    centers = torch.empty((k, F), dtype=torch.float32, device=X.device)
    centers[0] = X[_draw(torch.ones(n, device=X.device), generator), :F][0]
    labels, mind = torch.empty_like(p.labels), torch.empty_like(p.mind)
    for m in range(1, k):
        p.assign(centers[:m], labels, mind)
        centers[m] = X[_draw(mind, generator), :F][0]
    return centers


def kmeans(X, k, init='k-means++', n_init=1, max_iter=300, tol=1e-4, generator=None, sync_every=10):
    """Lloyd's k-means over the rows of the device tensor X [n, F] (csrc/reps.hip; semantics in include/eagcn_hip.h: those of
    sklearn.cluster.KMeans(algorithm='lloyd') except that an empty cluster keeps its centroid).  The host enqueues iterations in
    groups of `sync_every` and reads the `done` word once per group; iterations behind convergence are no-ops on the device, so
    the result does not depend on `sync_every`.  init: a [k, F] tensor, 'random' (k distinct rows) or 'k-means++' (drawn with
    `generator`, a torch.Generator of X's device); n_init > 1 keeps the run of least inertia.  Returns a KMeansResult."""
    k, n_init, max_iter, sync_every = int(k), int(n_init), int(max_iter), max(1, int(sync_every))
    if n_init < 1 or max_iter < 1:
        raise ValueError('kmeans: n_init and max_iter must be at least 1')
    p = _Problem(X, k)
    if isinstance(init, torch.Tensor):
        n_init = 1
    best = None
    for _ in range(n_init):
        c0 = _init_centers(p, init, generator)
        p.begin(c0, tol)
        it = 0
        while it < max_iter:
            m = min(sync_every, max_iter - it)
            for _j in range(m):
                p.iterate()
            it += m
            if int(p.state_i[0].item()):                     # the one host read of a group
                break
        p.finish()
        done, n_iter, _changed, n_empty = p.state_i.tolist()
        inertia = float(p.state_d[0].item())
        if best is None or inertia < best.inertia:
            best = KMeansResult(p.centers.clone(), p.labels.clone(), inertia, n_iter, n_empty, p.counts.clone().long(), c0, bool(done))
    return best


def confusion_matrix(y_true, labels, n_true, k):
    """[n_true, k] int64 on the device: entry (t, c) counts the rows of true class t in cluster c (sklearn.metrics.confusion_matrix
    with the classes 0 .. n_true - 1 against 0 .. k - 1)."""
    y = torch.as_tensor(y_true).to(device=labels.device, dtype=torch.int64).view(-1)
    c = labels.to(torch.int64).view(-1)
    if y.numel() != c.numel():
        raise ValueError('confusion_matrix: %d true classes for %d labels' % (y.numel(), c.numel()))
    return torch.bincount(y * int(k) + c, minlength=int(n_true) * int(k)).view(int(n_true), int(k))


# ---- PCA and exact t-SNE (csrc/embed.hip) ------------------------------------------------------------------------------------------

PCAResult = namedtuple('PCAResult', 'components explained_variance mean embedding')
TSNEResult = namedtuple('TSNEResult', 'embedding kl_divergence n_iter stop_reason learning_rate betas P')
STOP_REASONS = {0: 'running', 1: 'max_iter', 2: 'no_progress', 3: 'min_grad_norm'}      # EAGCN_TSNE_STOP_* of include/eagcn_hip.h
EXPLORATION_ITERS = 250                                                                  # TS_EXPLORE of csrc/embed.hip


def _rows(X, what):
    """X as the kernels take it: fp32 device rows with unit column stride (ld >= F).  (X, n, F, ld)"""
    if not isinstance(X, torch.Tensor) or not X.is_cuda or X.dtype != torch.float32 or X.dim() != 2:
        raise L.EagcnHipError('%s: X must be a float32 [n, F] tensor on the MI355X (eagcn_amd has no CPU path)' % what)
    n, F = X.shape
    if X.stride(1) != 1 or X.stride(0) < F:
        X = X.contiguous()
    return X, int(n), int(F), int(X.stride(0))


def sqdist(X):
    """[n, n] fp32 squared Euclidean distances between the rows of X: direct sums of squared differences (eagcn_sqdist)"""
    X, n, F, ld = _rows(X, 'sqdist')
    D = torch.empty((n, n), dtype=torch.float32, device=X.device)
    L.check(L.load().eagcn_sqdist(X.data_ptr(), n, F, ld, D.data_ptr(), _stream()), 'eagcn_sqdist')
    return D


def pca_cov(X):
    """(mean [F], cov [F, F]) in fp64 on the device (eagcn_pca_cov); no host read"""
    X, n, F, ld = _rows(X, 'pca')
    lib = L.load()
    ws = torch.empty(max(lib.eagcn_pca_workspace_bytes(n, F), 256), dtype=torch.uint8, device=X.device)
    mean = torch.empty(F, dtype=torch.float64, device=X.device)
    cov = torch.empty((F, F), dtype=torch.float64, device=X.device)
    L.check(lib.eagcn_pca_cov(X.data_ptr(), n, F, ld, mean.data_ptr(), cov.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), 'eagcn_pca_cov')
    return mean, cov


def pca(X, n_components=2):
    """sklearn.decomposition.PCA(n_components, svd_solver='full') of the device rows X [n, F]: column means and covariance on the
    device (eagcn_pca_cov), the F x F eigen-decomposition ONCE on the host in fp64 (torch.linalg.eigh: the one host synchronisation of
    this call), the projection on the device (eagcn_pca_project).  Signs as svd_flip(u_based_decision=False): the entry of largest
    magnitude of every component is positive.  PCAResult(components [k, F] fp32, explained_variance [k] fp64, mean [F] fp64,
    embedding [n, k] fp32), all on the device."""
    k = int(n_components)
    X, n, F, ld = _rows(X, 'pca')
    mean, cov = pca_cov(X)
    lam, vec = torch.linalg.eigh(cov.cpu())
    lam, vec = lam.flip(0)[:k], vec.flip(1)[:, :k].t().contiguous()               # descending, [k, F]
    big = vec.abs().argmax(dim=1)
    vec = vec * torch.sign(vec[torch.arange(vec.shape[0]), big]).unsqueeze(1)
    comp = vec.to(device=X.device, dtype=torch.float32).contiguous()
    emb = torch.empty((n, comp.shape[0]), dtype=torch.float32, device=X.device)
    L.check(L.load().eagcn_pca_project(X.data_ptr(), n, F, ld, mean.data_ptr(), comp.data_ptr(), k, emb.data_ptr(), _stream()),
            'eagcn_pca_project')
    return PCAResult(comp, lam.clamp_min(0.0).to(X.device), mean, emb)


class _TSNEProblem:
    """The joint probabilities P [n, ldp] (ldp = pad4(n): 16-byte rows) and a t-SNE workspace with typed views into it."""

    def __init__(self, n, device):
        self.lib = L.load()
        self.n, self.ldp = int(n), L.pad4(n)
        nbytes = self.lib.eagcn_tsne_workspace_bytes(self.n)
        self.ws = torch.empty(max(nbytes, 512), dtype=torch.uint8, device=device)
        self.state_i = self.ws[0:16].view(torch.int32)             # done | n_iter | reason | best_iter
        self.state_d = self.ws[16:40].view(torch.float64)          # best_err | last_kl | last_gnorm
        part = _a256(8 * self.n)
        self.Y, self.U, self.gains = ((self.ws[256 + j * part:256 + j * part + 8 * self.n].view(torch.float32).view(self.n, 2)
                                       if nbytes else None) for j in range(3))
        self.P = self.betas = self.steps = None

    def _ws(self):
        return (self.ws.data_ptr(), self.ws.numel(), _stream())

    def affinities(self, D, perplexity):
        """P, betas [n] fp64 and the search's step counts [n] int32 from squared distances D [n, n] (fp32, contiguous)"""
        self.P = torch.empty((self.n, self.ldp), dtype=torch.float32, device=D.device)
        self.betas = torch.empty(self.n, dtype=torch.float64, device=D.device)
        self.steps = torch.empty(self.n, dtype=torch.int32, device=D.device)
        L.check(self.lib.eagcn_tsne_affinities(D.data_ptr(), self.n, float(perplexity), self.P.data_ptr(), self.ldp, self.betas.data_ptr(),
                                               self.steps.data_ptr(), *self._ws()), 'eagcn_tsne_affinities')

    def set_P(self, P):
        """a joint P [n, n] computed elsewhere (tests): copied into the padded layout"""
        self.P = torch.zeros((self.n, self.ldp), dtype=torch.float32, device=P.device)
        self.P[:, :self.n] = P

    def gradient(self, Y, alpha, compute_kl=True):
        """(grad [n, 2] fp32, out [3] fp64 = Z | KL | |grad|) of one stand-alone gradient pass at Y [n, 2]"""
        Y = Y.to(torch.float32).contiguous()
        grad = torch.empty((self.n, 2), dtype=torch.float32, device=Y.device)
        out = torch.empty(3, dtype=torch.float64, device=Y.device)
        L.check(self.lib.eagcn_tsne_gradient(self.P.data_ptr(), self.ldp, Y.data_ptr(), self.n, float(alpha), int(bool(compute_kl)),
                                             grad.data_ptr(), out.data_ptr(), *self._ws()), 'eagcn_tsne_gradient')
        return grad, out

    def begin(self, Y0, early_exaggeration, learning_rate, max_iter, n_iter_without_progress, min_grad_norm):
        Y0 = Y0.to(torch.float32).contiguous()
        L.check(self.lib.eagcn_tsne_begin(self.P.data_ptr(), self.ldp, self.n, Y0.data_ptr(), float(early_exaggeration), float(learning_rate),
                                          int(max_iter), int(n_iter_without_progress), float(min_grad_norm), *self._ws()), 'eagcn_tsne_begin')

    def iterate(self):
        L.check(self.lib.eagcn_tsne_iterate(self.P.data_ptr(), self.ldp, self.n, *self._ws()), 'eagcn_tsne_iterate')

    def finish(self):
        L.check(self.lib.eagcn_tsne_finish(self.P.data_ptr(), self.ldp, self.n, *self._ws()), 'eagcn_tsne_finish')


def tsne(X, perplexity=30.0, early_exaggeration=12.0, learning_rate='auto', max_iter=1000, n_iter_without_progress=300, min_grad_norm=1e-7,
         init='pca', generator=None, sync_every=50):
    """Exact two-dimensional t-SNE of the device rows X [n, F] (csrc/embed.hip; semantics in include/eagcn_hip.h: those of
    sklearn.manifold.TSNE(method='exact', n_components=2) with the deviations listed there).  Distances, affinities and every
    iteration run on the device; the host enqueues iterations in groups of `sync_every` and reads the `done` word once per group --
    iterations behind a stop are no-ops on the device, so the result does not depend on `sync_every`.
      learning_rate 'auto': max(n / early_exaggeration / 4, 50).
      init 'random': 1e-4 N(0, 1) drawn on the device with `generator`; 'pca': this module's pca(X, 2) scaled to a standard deviation
        of 1e-4 in the first column (scikit-learn uses its randomized solver there: equal in kind, not in bits); or a [n, 2] tensor.
    Returns TSNEResult(embedding [n, 2], kl_divergence (of the final embedding against the un-exaggerated P), n_iter, stop_reason,
    learning_rate, betas [n] fp64, P [n, n] fp32 (a view of the padded matrix)); the tensors stay on the device."""
    X, n, F, ld = _rows(X, 'tsne')
    max_iter, sync_every = int(max_iter), max(1, int(sync_every))
    if max_iter < 1:
        raise ValueError('tsne: max_iter must be at least 1')
    lr = max(n / float(early_exaggeration) / 4.0, 50.0) if learning_rate == 'auto' else float(learning_rate)
    if isinstance(init, torch.Tensor):
        if tuple(init.shape) != (n, 2) or not init.is_cuda:
            raise L.EagcnHipError('tsne: init must be a device tensor of shape [n, 2] = [%d, 2]' % n)
        Y0 = init.to(torch.float32)
    elif init == 'random':
        Y0 = 1e-4 * torch.randn((n, 2), dtype=torch.float32, device=X.device, generator=generator)
    elif init == 'pca':
        Y0 = pca(X, 2).embedding
        Y0 = Y0 / Y0[:, 0].std(unbiased=False) * 1e-4
    else:
        raise ValueError("tsne: init must be a [n, 2] tensor, 'random' or 'pca'")
    p = _TSNEProblem(n, X.device)
    p.affinities(sqdist(X), perplexity)
    p.begin(Y0, early_exaggeration, lr, max_iter, n_iter_without_progress, min_grad_norm)
    it = 0
    while it < max_iter:
        m = min(sync_every, max_iter - it)
        for _j in range(m):
            p.iterate()
        it += m
        if int(p.state_i[0].item()):                         # the one host read of a group
            break
    p.finish()
    _done, n_iter, reason, _best = p.state_i.tolist()
    return TSNEResult(p.Y.clone(), float(p.state_d[1].item()), n_iter, STOP_REASONS.get(reason, str(reason)), lr, p.betas, p.P[:, :n])


def subsample(labels, classes, cap, generator=None):
    """Row indices (int64, ascending, on the device) of at most `cap` rows of every class in `classes`: the reference's selection in
    front of its embeddings (tsnes.py:62-86, 217-225).  Exactly min(count, cap) rows per class are kept, chosen uniformly at random
    with `generator` (the reference keeps each row with probability cap / count and so only approximates the cap).  torch ops only,
    no host read except the size of the result, which torch.nonzero needs."""
    lab = torch.as_tensor(labels)
    if not lab.is_cuda:
        raise L.EagcnHipError('subsample: labels must be a device tensor (eagcn_amd has no CPU path)')
    lab = lab.view(-1).to(torch.int64)
    cls = torch.as_tensor(classes, device=lab.device, dtype=torch.int64).view(-1)
    member = (lab.unsqueeze(1) == cls.unsqueeze(0)).any(dim=1)
    key = torch.rand(lab.numel(), dtype=torch.float64, device=lab.device, generator=generator)
    # sort by (class, random key): a row's rank within its class is its position minus the first position of the class
    order = torch.argsort(key)
    order = order[torch.argsort(lab[order], stable=True)]
    sl = lab[order]
    pos = torch.arange(lab.numel(), device=lab.device)
    first = torch.searchsorted(sl, sl, right=False)
    keep = torch.zeros(lab.numel(), dtype=torch.bool, device=lab.device)
    keep[order] = (pos - first) < int(cap)
    return torch.nonzero(keep & member).view(-1)


# ---- nearest neighbours and the trustworthiness of an embedding (csrc/knn.hip) ------------------------------------------------------

KNNResult = namedtuple('KNNResult', 'indices distances')
KNN_MAX_K = 128                                                                          # EAGCN_KNN_MAX_K of include/eagcn_hip.h


def knn_slabs(n, m, slabs=0):
    """The header's rule for the split of the data rows among workgroups, restated: the number of slabs a call runs with."""
    dt, qt = -(-int(n) // 64), -(-int(m) // 64)
    s = int(slabs) if slabs > 0 else min(-(-4096 // qt), 64)
    s = max(1, min(s, 4096, dt))
    per = -(-dt // s)
    return -(-dt // per)


def knn_workspace_bytes(n, m, F, k, slabs=0):
    """The header's formula for eagcn_knn_workspace_bytes, restated (tests compare the two)."""
    return _a256(8 * knn_slabs(n, m, slabs) * int(m) * int(k)) + _a256(8 * int(m) * int(k))


def _knn_ws(lib, n, m, F, k, slabs, device):
    return torch.empty(max(lib.eagcn_knn_workspace_bytes(n, m, F, k, slabs), 256), dtype=torch.uint8, device=device)


def knn(X, k, queries=None, metric='sqeuclidean', exclude_self=None, slabs=0):
    """The k nearest rows of the device tensor X [n, F] for every row of `queries` [m, F] (None: the rows of X themselves, a row not
    being its own neighbour unless exclude_self=False), exactly: csrc/knn.hip, semantics in include/eagcn_hip.h.  Neighbours ascend by
    (distance, row index), distances are the direct fp32 sums of `sqdist`; neither an n x n matrix nor a host synchronisation is
    involved, and the result does not depend on `slabs` (0: chosen by the library).
      metric 'sqeuclidean' | 'euclidean' (its square root) | 'cosine' (1 - cos: half the squared distance of L2-normalised copies).
    Returns KNNResult(indices [m, k] int32, distances [m, k] fp32) on the device."""
    if metric not in ('sqeuclidean', 'euclidean', 'cosine'):
        raise ValueError("knn: metric must be 'sqeuclidean', 'euclidean' or 'cosine'")
    X, n, F, ld = _rows(X, 'knn')
    self_join = queries is None
    if exclude_self is None:
        exclude_self = self_join
    if metric == 'cosine':
        X = X[:, :F] / X[:, :F].norm(dim=1, keepdim=True)
        ld = F
    if self_join:
        Q, m, ldq = X, n, ld
    else:
        Q, m, Fq, ldq = _rows(queries, 'knn')
        if Fq != F or Q.device != X.device:
            raise L.EagcnHipError('knn: queries [%d, %d] do not match X [%d, %d] on %s' % (m, Fq, n, F, X.device))
        if metric == 'cosine':
            Q = Q[:, :F] / Q[:, :F].norm(dim=1, keepdim=True)
            ldq = F
    k = int(k)
    lib = L.load()
    idx = torch.empty((m, k if 0 < k <= KNN_MAX_K else 1), dtype=torch.int32, device=X.device)
    dist = torch.empty(idx.shape, dtype=torch.float32, device=X.device)
    ws = _knn_ws(lib, n, m, F, k, int(slabs), X.device)
    L.check(lib.eagcn_knn(X.data_ptr(), n, F, ld, Q.data_ptr(), m, ldq, k, int(bool(exclude_self)), int(slabs), idx.data_ptr(), dist.data_ptr(),
                          ws.data_ptr(), ws.numel(), _stream()), 'eagcn_knn')
    if metric == 'euclidean':
        dist = dist.sqrt()
    elif metric == 'cosine':
        dist = dist * 0.5
    return KNNResult(idx, dist)


def neighbor_ranks(X, candidates, slabs=0):
    """int32 [n, k]: the 1-based position of row candidates[i, c] among the neighbours of row i of X [n, F] under the order of `knn`
    (eagcn_knn_rank); -1 where the candidate is i itself or no row of X.  No host synchronisation."""
    X, n, F, ld = _rows(X, 'neighbor_ranks')
    cand = torch.as_tensor(candidates)
    if not cand.is_cuda or cand.dim() != 2 or cand.shape[0] != n or cand.dtype not in (torch.int32, torch.int64):
        raise L.EagcnHipError('neighbor_ranks: candidates must be an integer device tensor [n = %d, k]' % n)
    k = int(cand.shape[1])
    if cand.dtype == torch.int64:
        cand = cand.clamp(-1, 2 ** 31 - 1)
    cand = cand.to(torch.int32).contiguous()
    lib = L.load()
    rank = torch.empty((n, max(k, 1)), dtype=torch.int32, device=X.device)
    ws = _knn_ws(lib, n, n, F, k, int(slabs), X.device)
    L.check(lib.eagcn_knn_rank(X.data_ptr(), n, F, ld, cand.data_ptr(), k, int(slabs), rank.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
            'eagcn_knn_rank')
    return rank


def trustworthiness(X, Y, n_neighbors=5):
    """sklearn.manifold.trustworthiness(X, Y, n_neighbors=k, metric='euclidean') of the embedding Y [n, .] of the device rows X [n, F]:
    the k neighbours of every row in Y (`knn`), their ranks in X (`neighbor_ranks`),
        T = 1 - 2 / (n k (2 n - 3 k - 1)) * sum max(0, rank - k),
    the sum in int64 on the device.  Returns a float: the one host synchronisation.  Ties are broken by the row index."""
    k, n = int(n_neighbors), int(X.shape[0])
    if Y.shape[0] != n:
        raise ValueError('trustworthiness: X has %d rows, Y %d' % (n, Y.shape[0]))
    if k < 1 or k >= n / 2:
        raise ValueError('n_neighbors (%d) should be less than n_samples / 2 (%g)' % (k, n / 2))
    ranks = neighbor_ranks(X, knn(Y, k).indices)
    penalty = (ranks.to(torch.int64) - k).clamp_min_(0).sum()
    return 1.0 - float(penalty.item()) * (2.0 / (n * k * (2.0 * n - 3.0 * k - 1.0)))


def continuity(X, Y, n_neighbors=5):
    """The trustworthiness with the two spaces exchanged: how far the neighbours in X stay neighbours in the embedding Y."""
    return trustworthiness(Y, X, n_neighbors)


def neighbor_agreement(indices, labels):
    """fp64 [m]: the share of every row's neighbours (`indices` [m, k], rows of a self-join) that carry the row's own label -- the
    reference reads 'atoms of one sub-type sit together' off its plots; this is the number.  torch ops only."""
    lab = torch.as_tensor(labels).to(indices.device).view(-1)
    if lab.numel() != indices.shape[0]:
        raise ValueError('neighbor_agreement: %d labels for %d rows' % (lab.numel(), indices.shape[0]))
    return (lab[indices.long()] == lab.unsqueeze(1)).double().mean(dim=1)


# ---- scores of a clustering (csrc/silhouette.hip) -----------------------------------------------------------------------------------

SilhouetteResult = namedtuple('SilhouetteResult', 'samples score cluster_means counts n_ignored')
ClusterMoments = namedtuple('ClusterMoments', 'centers scatter wss counts')
SIL_MAX_K = 256                                                                          # EAGCN_SIL_MAX_K of include/eagcn_hip.h


def silhouette_slabs(n, k, slabs=0):
    """The header's rule for the split of a silhouette call's data tiles -- at most ceil(n / 64) + k, every cluster cut into tiles of
    its own -- among workgroups, restated: the number of slabs a call runs with."""
    return knn_slabs(64 * (-(-int(n) // 64) + int(k)), n, slabs)


def _sort_bytes(n, k):
    w0 = min(-(-n // 1024), 1024)
    chunk = -(-(-(-n // w0)) // 64) * 64
    w = -(-n // chunk)
    return _a256(4 * w * (k + 1)) + _a256(4 * w * k) + 2 * _a256(4 * (k + 1)) + _a256(4 * n)


def silhouette_workspace_bytes(n, F, k, slabs=0):
    """The header's formula for eagcn_silhouette_workspace_bytes, restated (tests compare the two)."""
    n, k = int(n), int(k)
    tb = -(-n // 64) + k
    return _sort_bytes(n, k) + _a256(16 * tb) + _a256(8 * k) + _a256(8 * silhouette_slabs(n, k, slabs) * n * k)


def cluster_moments_workspace_bytes(n, F, k):
    """The header's formula for eagcn_cluster_moments_workspace_bytes, restated (tests compare the two)."""
    n, F, k = int(n), int(F), int(k)
    R = min(-(-n // 8192), 16)
    return _sort_bytes(n, k) + _a256(8 * R * k * F) + _a256(16 * R * k)


def _labels(labels, n, device, what):
    lab = torch.as_tensor(labels)
    if not lab.is_cuda or lab.is_floating_point() or lab.dtype == torch.bool or lab.dim() != 1 or lab.numel() != n or lab.device != device:
        raise L.EagcnHipError('%s: labels must be an integer device tensor [n = %d] beside X (eagcn_amd has no CPU path)' % (what, n))
    if lab.dtype != torch.int32:
        lab = lab.clamp(-1, 2 ** 31 - 1).to(torch.int32)
    return lab.contiguous()


def silhouette_samples(X, labels, n_clusters, slabs=0):
    """sklearn.metrics.silhouette_samples(X, labels, metric='euclidean') of the device rows X [n, F] under the labelling `labels` (any
    integer device tensor, e.g. kmeans(...).labels) with the clusters 0 .. n_clusters - 1 (the host must know k: no device read), exactly:
    csrc/silhouette.hip, semantics in include/eagcn_hip.h.  Distances are the square roots of `sqdist`'s fp32 sums, all sums fp64 in a
    fixed order; neither an n x n matrix nor a host synchronisation is involved.  A row whose label is outside 0 .. n_clusters - 1 is
    left out on both sides (its sample is NaN): silhouette_samples(X, torch.where(keep, labels, -1), k) scores a selection without a
    copy of the rows.  Returns SilhouetteResult(samples [n] fp64, score [] fp64 (the mean over the scored rows; NaN with fewer than two
    non-empty clusters), cluster_means [k] fp64, counts [k] int64, n_ignored [] int64) on the device."""
    X, n, F, ld = _rows(X, 'silhouette_samples')
    k = int(n_clusters)
    lab = _labels(labels, n, X.device, 'silhouette_samples')
    lib = L.load()
    kk = k if 2 <= k <= SIL_MAX_K else 2
    samples = torch.empty(n, dtype=torch.float64, device=X.device)
    means = torch.empty(kk, dtype=torch.float64, device=X.device)
    counts = torch.empty(kk, dtype=torch.int64, device=X.device)
    stats = torch.empty(4, dtype=torch.float64, device=X.device)
    ws = torch.empty(max(lib.eagcn_silhouette_workspace_bytes(n, F, k, int(slabs)), 256), dtype=torch.uint8, device=X.device)
    L.check(lib.eagcn_silhouette(X.data_ptr(), n, F, ld, lab.data_ptr(), k, int(slabs), samples.data_ptr(), means.data_ptr(), counts.data_ptr(),
                                 stats.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), 'eagcn_silhouette')
    return SilhouetteResult(samples, stats[0], means, counts, stats[3].to(torch.int64))


def _check_number_of_labels(n_labels, n_samples):
    if not 1 < n_labels < n_samples:
        raise ValueError('Number of labels is %d. Valid values are 2 to n_samples - 1 (inclusive)' % n_labels)


def silhouette_score(X, labels, n_clusters):
    """sklearn.metrics.silhouette_score(X, labels, metric='euclidean'): the mean of `silhouette_samples` over the scored rows.  Returns
    a float: the one host synchronisation.  ValueError as scikit-learn's when fewer than two clusters are non-empty or every scored row
    is alone in its cluster."""
    r = silhouette_samples(X, labels, n_clusters)
    score, n_labels, n_scored = torch.stack([r.score, (r.counts > 0).sum().double(), r.counts.sum().double()]).tolist()
    _check_number_of_labels(int(n_labels), int(n_scored))
    return score


def cluster_moments(X, labels, n_clusters):
    """Per cluster of the labelling `labels` (as for silhouette_samples) of the device rows X [n, F], in fp64 on the device
    (eagcn_cluster_moments): ClusterMoments(centers [k, F] the centroids, scatter [k] the mean Euclidean distance of a cluster's rows to
    its centre, wss [k] the sum of their squared distances, counts [k] int64).  centers and scatter of an empty cluster are NaN.  No
    host synchronisation."""
    X, n, F, ld = _rows(X, 'cluster_moments')
    k = int(n_clusters)
    lab = _labels(labels, n, X.device, 'cluster_moments')
    lib = L.load()
    kk = k if 2 <= k <= SIL_MAX_K else 2
    centers = torch.empty((kk, F), dtype=torch.float64, device=X.device)
    scatter, wss = (torch.empty(kk, dtype=torch.float64, device=X.device) for _ in range(2))
    counts = torch.empty(kk, dtype=torch.int64, device=X.device)
    ws = torch.empty(max(lib.eagcn_cluster_moments_workspace_bytes(n, F, k), 256), dtype=torch.uint8, device=X.device)
    L.check(lib.eagcn_cluster_moments(X.data_ptr(), n, F, ld, lab.data_ptr(), k, centers.data_ptr(), scatter.data_ptr(), wss.data_ptr(),
                                      counts.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), 'eagcn_cluster_moments')
    return ClusterMoments(centers, scatter, wss, counts)


def davies_bouldin_from_moments(m):
    """(score [] fp64, non-empty clusters [], rows []) on the device from ClusterMoments: sklearn.metrics.davies_bouldin_score -- the
    mean over the non-empty clusters of max_j (scatter_i + scatter_j) / |centre_i - centre_j|, a zero centre distance counted as
    infinite, and 0 when all scatters or all centre distances are (numpy.allclose to) 0."""
    there = m.counts > 0
    s = torch.where(there, m.scatter, torch.zeros_like(m.scatter))
    cen = torch.where(there.unsqueeze(1), m.centers, torch.zeros_like(m.centers))
    diff = cen.unsqueeze(1) - cen.unsqueeze(0)
    d = (diff * diff).sum(dim=2).sqrt()
    pair = there.unsqueeze(1) & there.unsqueeze(0)
    flat = (s.abs().max() <= 1e-8) | (torch.where(pair, d, torch.zeros_like(d)).abs().max() <= 1e-8)      # np.allclose(., 0)
    ratio = (s.unsqueeze(1) + s.unsqueeze(0)) / torch.where(d == 0, torch.full_like(d, float('inf')), d)
    ratio = torch.where(pair, ratio, torch.full_like(ratio, float('-inf')))
    worst = torch.where(there, ratio.max(dim=1).values, torch.zeros_like(s))
    score = torch.where(flat, torch.zeros_like(worst.sum()), worst.sum() / there.sum())
    return score, there.sum(), m.counts.sum()


def calinski_harabasz_from_moments(m):
    """(score [] fp64, non-empty clusters [], rows []) on the device from ClusterMoments: sklearn.metrics.calinski_harabasz_score =
    (between-cluster dispersion / (k - 1)) / (within-cluster dispersion / (n - k)) over the non-empty clusters, 1 where the within-cluster
    dispersion is 0."""
    there = m.counts > 0
    cnt = m.counts.double()
    cen = torch.where(there.unsqueeze(1), m.centers, torch.zeros_like(m.centers))
    n, k = cnt.sum(), there.sum().double()
    mean = (cen * cnt.unsqueeze(1)).sum(dim=0) / n
    extra = (cnt * ((cen - mean) ** 2).sum(dim=1)).sum()
    intra = m.wss.sum()
    score = torch.where(intra == 0, torch.ones_like(intra), extra * (n - k) / (intra * (k - 1.0)))
    return score, there.sum(), m.counts.sum()


def _moment_score(fn, X, labels, n_clusters):
    score, n_labels, n_scored = torch.stack([t.double() for t in fn(cluster_moments(X, labels, n_clusters))]).tolist()
    _check_number_of_labels(int(n_labels), int(n_scored))
    return score


def davies_bouldin_score(X, labels, n_clusters):
    """sklearn.metrics.davies_bouldin_score of the device rows X under `labels` (as for silhouette_samples; empty clusters are left
    out): `cluster_moments`, the k x k part in torch fp64 on the device.  Returns a float: the one host synchronisation."""
    return _moment_score(davies_bouldin_from_moments, X, labels, n_clusters)


def calinski_harabasz_score(X, labels, n_clusters):
    """sklearn.metrics.calinski_harabasz_score of the device rows X under `labels` (as for silhouette_samples; empty clusters are left
    out), from `cluster_moments`.  Returns a float: the one host synchronisation."""
    return _moment_score(calinski_harabasz_from_moments, X, labels, n_clusters)


def _contingency(cm, what):
    cm = torch.as_tensor(cm)
    if cm.dim() != 2 or cm.is_floating_point() or cm.dtype == torch.bool:
        raise ValueError('%s: needs the integer [n_true, k] matrix that confusion_matrix returns' % what)
    return cm.to(torch.int64)


def adjusted_rand_score(cm):
    """sklearn.metrics.adjusted_rand_score from the [n_true, k] matrix of `confusion_matrix`: the four pair counts in int64 where the
    matrix lives (exact: n < 2^31 rows keep n^2 inside int64), one read, the quotient in Python integers as scikit-learn does.
    Returns a float."""
    cm = _contingency(cm, 'adjusted_rand_score')
    n, sq = cm.sum(), (cm * cm).sum()
    rows, cols = cm.sum(dim=1), cm.sum(dim=0)
    c11 = sq - n
    c01 = (cm * cols.unsqueeze(0)).sum() - sq
    c10 = (cm * rows.unsqueeze(1)).sum() - sq
    c00 = n * n - c01 - c10 - sq
    tn, fp, fn, tp = torch.stack([c00, c01, c10, c11]).tolist()
    if fn == 0 and fp == 0:
        return 1.0
    return 2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))


def normalized_mutual_info_score(cm):
    """sklearn.metrics.normalized_mutual_info_score(average_method='arithmetic') from the [n_true, k] matrix of `confusion_matrix`, in
    fp64 where the matrix lives; empty rows and columns (classes or clusters without a row) do not count.  Returns a float."""
    cm = _contingency(cm, 'normalized_mutual_info_score')
    c = cm.double()
    n, pi, pj = c.sum(), c.sum(dim=1), c.sum(dim=0)
    nz = cm > 0
    one = torch.ones_like(c)
    logc = torch.log(torch.where(nz, c, one))
    outer = pi.unsqueeze(1) * pj.unsqueeze(0)
    log_outer = -torch.log(torch.where(nz, outer, one)) + 2.0 * torch.log(n)
    term = (c / n) * (logc - torch.log(n)) + (c / n) * log_outer
    term = torch.where(nz & (term.abs() >= 2.0 ** -52), term, torch.zeros_like(term))
    mi = term.sum().clamp_min(0.0)

    def entropy(p):
        live = p > 0
        h = -torch.where(live, (p / n) * (torch.log(torch.where(live, p, torch.ones_like(p))) - torch.log(n)), torch.zeros_like(p)).sum()
        return torch.where(live.sum() > 1, h, torch.zeros_like(h))

    mi, h_true, h_pred, n_true, n_pred = torch.stack([mi, entropy(pi), entropy(pj), (pi > 0).sum().double(), (pj > 0).sum().double()]).tolist()
    if n_true == n_pred and n_true <= 1:
        return 1.0
    if n_true == 1 or n_pred == 1 or mi == 0:
        return 0.0
    return mi / (0.5 * (h_true + h_pred))


def purity(cm):
    """The share of the rows that carry the most frequent true class of their cluster, from the [n_true, k] matrix of `confusion_matrix`:
    sum_c max_t cm[t, c] / n.  Returns a float."""
    cm = _contingency(cm, 'purity')
    if cm.numel() == 0:
        raise ValueError('purity: the matrix is empty')
    return float((cm.max(dim=0).values.sum().double() / cm.sum().double()).item())
