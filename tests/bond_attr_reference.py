"""The yardstick of the bond-attribution tests, built from the oracle's modules (any dtype; the tests run it in fp32 and float64).

Two evaluations of the per-view, per-bond scores S [K, B, N, N] of the scalar t = sum(out * dout) of an EVAL-mode oracle model:

``autograd_scores``  plain autograd.  mode 'attention': forward hooks on every view module ``retain_grad()`` the returned A1 =
    sigmoid(z) * adj (layers.py:82-83), S_k = sum over the layers of A1 * dt/dA1.  mode 'relation': the relation tensors get
    ``requires_grad_()``, S_k = sum_c rel_k[:, c] * dt/drel_k[:, c] (the tensors are shared by the layers, so the layers are summed
    by autograd).  GCN baseline (attention mode only; all attention values are 1): the hook retains the returned normalised
    matrix A^ = m u / rowsum(u), and the gradient with respect to the unnormalised entry follows by the quotient rule,
    D_ij = rs_i (dA^_ij - sum_j' A^_ij' dA^_ij'), rs_i = m_i / rowsum_i;  S = adj * D summed over the layers.

``formula_scores``  the closed form the device kernel implements (include/eagcn_hip.h, "bond attribution"), restated on dense
    tensors: per layer l and view k, with P = X W, Y = A^ P (pre-bias), sc = gamma / sqrt(rv + eps), sh = beta - (rm - bias) sc and
    dH the gradient at the view's output (hook: retain_grad on the returned activations),
        dY = sc [sc Y + sh > 0] dH,   D_ij = rs_i <dY_i, P_j - Y_i>,   S_k += f(z) adj D,
    f = sigmoid (attention) | sigmoid (1 - sigmoid) z (relation).
"""
import torch
import torch.nn.functional as F

from oracle.eagcn_ref import TINY, RefBlock, RefVanillaGCN, row_mask


def target_weights(B, nclass, target):
    """[B, nclass] weights of the attributed scalar: a task index selects one column."""
    if torch.is_tensor(target):
        return target.reshape(B, nclass).clone()
    w = torch.zeros(B, nclass)
    w[:, int(target)] = 1.0
    return w


def _views(model):
    """view modules in (layer, view) order"""
    return [m for m in model.modules() if isinstance(m, (RefBlock, RefVanillaGCN))]


def _n_views(model):
    return 1 if isinstance(_views(model)[0], RefVanillaGCN) else model.layer1.K


def _run(model, dense, dout, relation_grad=False):
    """forward + backward of t with hooks on every view module -> list of records per (layer, view)"""
    assert not model.training
    adj, afm, rels, size = dense[0], dense[1], list(dense[2:-1]), dense[-1]
    dt = next(model.parameters()).dtype
    cast = lambda t: t.to(dt)
    adj, afm = cast(adj), cast(afm)
    if isinstance(_views(model)[0], RefVanillaGCN):      # (the baseline's matrix depends on adj alone: give it a gradient to retain)
        adj = adj.clone().requires_grad_(True)
    rels = [cast(r).clone().requires_grad_(relation_grad) for r in rels]
    recs, handles = [], []

    def hook(mod, inputs, outputs):
        y, a = outputs
        if y.requires_grad:
            y.retain_grad()
        if a.requires_grad:
            a.retain_grad()
        recs.append(dict(mod=mod, adj=inputs[0], x=inputs[1], rel=inputs[2] if len(inputs) > 2 else None, y=y, a=a))
    for m in _views(model):
        handles.append(m.register_forward_hook(hook))
    try:
        x = afm.clone().requires_grad_(True)             # (so that every intermediate carries a gradient, frozen models included)
        out, _, _ = model(adj, x, *rels, size)
        (out * cast(dout)).sum().backward()
    finally:
        for h in handles:
            h.remove()
    model.zero_grad(set_to_none=True)
    return recs, adj.detach(), rels


def autograd_scores(model, dense, dout, mode='attention'):
    K = _n_views(model)
    recs, adj, rels = _run(model, dense, dout, relation_grad=(mode == 'relation'))
    B, N, _ = adj.shape
    S = torch.zeros(K, B, N, N, dtype=adj.dtype)
    if mode == 'relation':
        for k in range(K):
            S[k] = (rels[k] * rels[k].grad).sum(1).detach()
        return S
    for n, r in enumerate(recs):
        k = n % K
        if isinstance(r['mod'], RefVanillaGCN):
            a, da = r['a'].detach(), r['a'].grad
            m = row_mask(adj)
            u = adj + m.expand(B, N, N) * torch.eye(N, dtype=adj.dtype) + (1.0 - adj) * TINY
            rs = m / u.sum(2, keepdim=True)
            S[k] += adj * rs * (da - (a * da).sum(2, keepdim=True))
        else:
            S[k] += (r['a'] * r['a'].grad).detach()
    return S


def formula_scores(model, dense, dout, mode='attention'):
    K = _n_views(model)
    recs, adj, rels = _run(model, dense, dout)
    B, N, _ = adj.shape
    m = row_mask(adj)
    eye = torch.eye(N, dtype=adj.dtype)
    S = torch.zeros(K, B, N, N, dtype=adj.dtype)
    with torch.no_grad():
        for n, r in enumerate(recs):
            k, mod = n % K, r['mod']
            if isinstance(mod, RefVanillaGCN):
                z = torch.full((B, N, N), 40.0, dtype=adj.dtype)          # sigmoid = 1: every bond and the self loop weigh one
                u = adj + m.expand(B, N, N) * eye + (1.0 - adj) * TINY
            else:
                z = F.conv2d(r['rel'], mod.att.weight).view(B, N, N)
                u = torch.sigmoid(z) * adj + torch.sigmoid(mod.self_r) * (m.expand(B, N, N) * eye) + (1.0 - adj) * TINY
            rowsum = u.sum(2, keepdim=True)
            a_hat = u / rowsum * m
            rs = m / rowsum                                               # [B, N, 1]
            gc, bn = mod.graph_conv, mod.batch_norm.bn
            P = r['x'].detach() @ gc.weight                               # [B, N, F]
            Y = torch.bmm(a_hat, P)                                       # pre-bias
            sc = bn.weight / torch.sqrt(bn.running_var + bn.eps)
            sh = bn.bias - (bn.running_mean - gc.bias) * sc
            dY = sc * ((sc * Y + sh) > 0).to(adj.dtype) * r['y'].grad
            D = rs * (torch.bmm(dY, P.transpose(1, 2)) - (dY * Y).sum(2, keepdim=True))
            s = torch.sigmoid(z)
            f = s if mode == 'attention' else s * (1.0 - s) * z
            S[k] += f * adj * D
    return S
