"""U sequential Adam updates of one deep_cfr.MLP (Linear + ReLU per hidden layer, LayerNorm, Linear; the policy network
ends in a softmax) on Deep CFR's sqrt(iteration)-weighted MSE in NumPy float64: the reference of osg_deep_cfr_learn.
Parameters are flat in network.parameters() order: Linear weight, bias per hidden layer; LayerNorm; Linear."""
import numpy as np

BETA1, BETA2, EPS, LN_EPS = 0.9, 0.999, 1e-8, 1e-5
SMALL_ROOT = 1e-5      # an entry whose sqrt(v^) falls in (0, SMALL_ROOT) at any update is left out of a comparison

# (kind, game, hidden, B, U, seed): kind 0 advantage, 1 policy.  B: one row, a partial tile, the planner's tile height + 1
# (128 + 1; 64 + 1 for (128,)) and the example's 256.  U = 12 goes with the narrower networks: a wide one has too many
# distinct ReLU pre-activations over 12 updates for a seed to keep them all away from zero.  seed: the first from 1 for
# which the restatement alone leaves out at most 1 % of the parameters and keeps every nonzero ReLU pre-activation above
# 4e-4 (2e-3 for the policy network at U = 12, whose float32 deviations, and so its tolerance, are four times as large).
CASES = [
    (0, "kuhn_poker", (4, 2), 1, 12, 1), (0, "kuhn_poker", (20,), 17, 12, 1), (0, "leduc_poker", (24, 40), 129, 1, 1),
    (0, "leduc_poker", (64,), 256, 12, 2), (0, "leduc_poker", (128,), 65, 1, 1), (0, "leduc_poker", (128,), 256, 1, 1),
    (1, "kuhn_poker", (4, 2), 17, 12, 1), (1, "kuhn_poker", (20,), 129, 12, 7), (1, "leduc_poker", (24, 40), 256, 1, 1),
    (1, "leduc_poker", (64,), 1, 1, 1), (1, "leduc_poker", (128,), 65, 1, 3), (1, "leduc_poker", (128,), 17, 1, 3),
]


def unflatten(flat, widths):
    """([(weight, bias) per linear layer], LayerNorm weight, LayerNorm bias): views of `flat`."""
    layers, at, last = [], 0, len(widths) - 2
    for k, (i, o) in enumerate(zip(widths[:-1], widths[1:])):
        if k == last:
            gamma, beta = flat[at:at + i], flat[at + i:at + 2 * i]
            at += 2 * i
        layers.append((flat[at:at + o * i].reshape(o, i), flat[at + o * i:at + o * i + o]))
        at += o * i + o
    assert at == len(flat)
    return layers, gamma, beta


def gradient(kind, widths, params, x, it, t, margins):
    """(loss, dLoss/dparams flat) of one batch: inputs x [B, S], iterations it [B], targets t [B, A]."""
    layers, gamma, beta = unflatten(params, widths)
    grad = np.zeros_like(params)
    g_layers, g_gamma, g_beta = unflatten(grad, widths)
    acts = [x]
    for w, b in layers[:-1]:
        z = acts[-1] @ w.T + b
        if np.any(z != 0):
            margins.append(np.abs(z[z != 0]).min())
        acts.append(np.maximum(z, 0.0))
    h = acts[-1]
    mean, var = h.mean(1, keepdims=True), h.var(1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + LN_EPS)
    xh = (h - mean) * rstd
    n = gamma * xh + beta
    z = n @ layers[-1][0].T + layers[-1][1]
    y = z
    if kind == 1:
        e = np.exp(z - z.max(1, keepdims=True))
        y = e / e.sum(1, keepdims=True)
    B, A = y.shape
    loss = (it[:, None] * (y - t) ** 2).sum() / (B * A)
    dz = 2.0 * it[:, None] * (y - t) / (B * A)
    if kind == 1:
        dz = y * (dz - (dz * y).sum(1, keepdims=True))
    g_layers[-1][0][:], g_layers[-1][1][:] = dz.T @ n, dz.sum(0)
    dn = dz @ layers[-1][0]
    g_gamma[:], g_beta[:] = (dn * xh).sum(0), dn.sum(0)
    a = gamma * dn
    d = (a - a.mean(1, keepdims=True) - xh * (a * xh).mean(1, keepdims=True)) * rstd
    for k in range(len(layers) - 2, -1, -1):
        d = d * (acts[k + 1] > 0)
        g_layers[k][0][:], g_layers[k][1][:] = d.T @ acts[k], d.sum(0)
        d = d @ layers[k][0]
    return loss, grad


def learn(kind, widths, params, tensors, rows, lr, m=None, v=None, step0=0):
    """rows (info [U, B], iteration [U, B], target [U, B, A]).  Returns (params, m, v, losses [U], the smallest nonzero
    |pre-activation| at a ReLU, the entries to leave out)."""
    params = np.array(params, np.float64)
    m = np.zeros_like(params) if m is None else np.array(m, np.float64)
    v = np.zeros_like(params) if v is None else np.array(v, np.float64)
    tensors, margins, losses = np.asarray(tensors, np.float64), [], []
    small = np.zeros(len(params), bool)
    for u in range(rows[0].shape[0]):
        loss, g = gradient(kind, widths, params, tensors[rows[0][u].astype(np.int64)], rows[1][u].astype(np.float64),
                           rows[2][u].astype(np.float64), margins)
        losses.append(loss)
        step = step0 + u + 1
        m = BETA1 * m + (1 - BETA1) * g
        v = BETA2 * v + (1 - BETA2) * g * g
        root = np.sqrt(v) / np.sqrt(1 - BETA2 ** step)
        small |= (root > 0) & (root < SMALL_ROOT)
        params = params - lr / (1 - BETA1 ** step) * m / (root + EPS)
    return params, m, v, np.array(losses), float(min(margins)), small


def synthetic_rows(kind, seed, size, infostates, A, pool=3):
    """`size` buffer rows (info, iteration in 1..50, values [size, A] in [-2, 2] or on the simplex) over a few of `infostates`:
    few distinct ReLU pre-activations — each a chance of a small margin — so that a seed exists."""
    rng = np.random.default_rng(seed)
    some = rng.choice(np.asarray(infostates), min(pool, len(infostates)), replace=False)
    info = some[rng.integers(0, len(some), size)].astype(np.int32)
    iteration = rng.integers(1, 51, size).astype(np.int32)
    if kind == 0:
        return info, iteration, rng.uniform(-2, 2, (size, A)).astype(np.float32)
    values = rng.random((size, A)) + 0.05
    return info, iteration, (values / values.sum(1, keepdims=True)).astype(np.float32)


def dev(got, want, keep):
    """max |p - p64| / max |p64| over the parameters kept."""
    got, want = np.asarray(got, np.float64)[keep], np.asarray(want, np.float64)[keep]
    return float(np.abs(got - want).max() / np.abs(want).max())
