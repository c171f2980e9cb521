"""legion_row_update (include/legion_hip.h) restated in numpy: the contract, not the kernel.  The gradients of an id are summed in
float64 in ascending position; the optimizer's step is then repeated in np.float32, one correctly rounded operation at a time, in the
order of the rule's point 5."""
import numpy as np

F = np.float32


def combine(ids, grads, N):
    """(the distinct live ids ascending, float64 [U, D] sums of their rows, int64 [U] counts)."""
    live = np.flatnonzero((ids >= 0) & (ids < N))
    order = live[np.argsort(ids[live], kind="stable")]                 # ascending position inside every id
    uniq, start, count = np.unique(ids[order], return_index=True, return_counts=True)
    sums = np.add.reduceat(grads[order].astype(np.float64), start, axis=0) if uniq.size else np.zeros((0, grads.shape[1]))
    return uniq, sums, count


def update(table, ids, grads, combine_mode, optimizer, lr, eps=1e-10, betas=(0.9, 0.999), state=None, node_map=None, cache=None):
    """Applies one step in place to table, state (state1, state2, state_pow: those the optimizer needs) and cache, all float32;
    returns (the ids touched, the float64 sums, the counts)."""
    uniq, sums, count = combine(ids, grads, table.shape[0])
    g = sums.astype(F)
    if combine_mode == "mean":
        g = g / count.astype(F)[:, None]
    lr, eps, b1, b2 = F(lr), F(eps), F(betas[0]), F(betas[1])
    w = table[uniq]
    if optimizer == "sgd":
        w = w - lr * g
    elif optimizer == "adagrad":
        s = state["state1"][uniq] + g * g
        w = w - (lr * g) / (np.sqrt(s) + eps)
        state["state1"][uniq] = s
    else:
        p1, p2 = state["state_pow"][uniq, 0] * b1, state["state_pow"][uniq, 1] * b2
        m = b1 * state["state1"][uniq] + (F(1) - b1) * g
        u = b2 * state["state2"][uniq] + (F(1) - b2) * (g * g)
        w = w - (lr * (m / (F(1) - p1)[:, None])) / (np.sqrt(u / (F(1) - p2)[:, None]) + eps)
        state["state1"][uniq], state["state2"][uniq] = m, u
        state["state_pow"][uniq, 0], state["state_pow"][uniq, 1] = p1, p2
    assert w.dtype == F
    table[uniq] = w
    if node_map is not None:
        hit = node_map[uniq] >= 0
        cache[node_map[uniq][hit]] = w[hit]
    return uniq, sums, count
