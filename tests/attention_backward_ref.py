"""The gradients of legion_attention_rows by torch.autograd over the plain composition in float64 on the CPU: gather, u_dot_v, a masked
segment softmax, the weighted sum.  No formula of the backward pass is written here."""
import numpy as np
import torch


def gathered(X, ids, node_map=None, cache=None):
    """(the stored row of every entry as float64 [M, D], cached rows substituted as attention_ref.py does and zeros for a dead entry;
    which entries are live)."""
    live = (ids >= 0) & (ids < X.shape[0])
    safe = np.where(live, ids, 0)
    rows = X[safe].astype(np.float64)
    if node_map is not None:
        hit = live & (node_map[safe] >= 0)
        rows[hit] = cache[node_map[safe][hit]]
    rows[~live] = 0
    return rows, live


def attention_backward(X, offsets, ids, grad_out, queries=None, bias=None, scale=1.0, node_map=None, cache=None):
    """(out [n, H, D], grad_queries [n, H, D] or None, grad_bias [M, H] or None, grad_rows [M, D]) as float64 numpy.  The leaves are the
    queries, the bias and the gathered stored rows [M, D]; dead entries are masked out of the softmax, so their gradients are zeros."""
    n, M = offsets.size - 1, ids.size
    rows, live = gathered(X, ids, node_map, cache)
    leaf = lambda v: None if v is None else torch.tensor(np.asarray(v, np.float64), requires_grad=True)
    x, q, b = leaf(rows), leaf(queries), leaf(bias)
    H = (queries if queries is not None else bias).shape[1]
    seg = torch.from_numpy(np.repeat(np.arange(n), np.diff(offsets)))
    s = torch.zeros((M, H), dtype=torch.float64)
    if q is not None:
        s = s + float(np.float32(scale)) * torch.einsum("mhd,md->mh", q[seg], x)
    if b is not None:
        s = s + b
    s = s.masked_fill(torch.from_numpy(~live)[:, None], -np.inf)
    top = np.full((n, H), -np.inf)
    np.maximum.at(top, seg.numpy(), s.detach().numpy())               # (a shift of the exponent: no part of the graph)
    p = torch.exp(s - torch.from_numpy(np.where(np.isinf(top), 0.0, top))[seg])
    a = p / torch.zeros((n, H), dtype=torch.float64).index_add(0, seg, p).clamp_min(1e-300)[seg]
    out = torch.zeros((n, H, x.shape[1]), dtype=torch.float64).index_add(0, seg, a[:, :, None] * x[:, None, :])
    out.backward(torch.from_numpy(np.asarray(grad_out, np.float64)))
    grad = lambda t: None if t is None else t.grad.numpy()
    return out.detach().numpy(), grad(q), grad(b), grad(x)
