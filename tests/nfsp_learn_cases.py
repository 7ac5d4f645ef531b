"""U sequential DQN (dqn.py:501-569) or supervised (nfsp.py:364-409) SGD updates of one MLP, restated in NumPy float64:
the reference of the fused learner (osg_nfsp_learn).  Parameters are flat in nn.Linear layout (weight [out, in], then
bias, per layer).  Besides the parameters and the losses it returns the smallest margin to a branch that float32 and
float64 could take differently: |pre-activation| at a ReLU, the gap between the two largest legal next Q values,
||d| - beta| for Huber, | ||g|| - clip |."""
import numpy as np


def unflatten(flat, widths):
    layers, at = [], 0
    for i, o in zip(widths[:-1], widths[1:]):
        layers.append((flat[at:at + o * i].reshape(o, i), flat[at + o * i:at + o * i + o]))
        at += o * i + o
    return layers


def forward(layers, x, margins=None):
    acts = [x]
    for k, (w, b) in enumerate(layers):
        z = acts[-1] @ w.T + b
        if k + 1 < len(layers):
            if margins is not None:
                margins.append(np.abs(z).min())
            z = np.maximum(z, 0.0)
        acts.append(z)
    return acts


def backward(layers, acts, dy):
    grads = []
    for k in range(len(layers) - 1, -1, -1):
        grads.append((dy.T @ acts[k], dy.sum(0)))
        if k:
            dy = (dy @ layers[k][0]) * (acts[k] > 0)
    return grads[::-1]


def learn(kind, widths, params, target, tensors, mask, rows, lr, discount=1.0, loss="mse", beta=1.0, clip=None):
    """rows: kind 0 (info, action, reward, next_info, final) each [U, B]; kind 1 (info [U, B], probs [U, B, A]).
    Returns (params float64, losses [U], margin)."""
    params = np.array(params, np.float64)
    layers = unflatten(params, widths)     # views: the steps below move `params`
    tensors, margins, losses = np.asarray(tensors, np.float64), [], []
    U, B = rows[0].shape
    for u in range(U):
        info = rows[0][u].astype(np.int64)
        acts = forward(layers, tensors[info], margins)
        y = acts[-1]
        if kind == 0:
            action, reward, nxt, final = (r[u] for r in rows[1:])
            live = final == 0
            nxt = np.clip(nxt, 0, None).astype(np.int64)
            tq = forward(unflatten(np.asarray(target, np.float64), widths), tensors[nxt] * live[:, None])[-1]
            tq = np.where(mask[nxt] & live[:, None], tq, -np.inf)
            for row in tq[live]:
                top = np.sort(row[np.isfinite(row)])
                if len(top) > 1:
                    margins.append(top[-1] - top[-2])
            tgt = reward.astype(np.float64) + np.where(live, discount * np.where(live, tq.max(1), 0.0), 0.0)
            d = y[np.arange(B), action] - tgt
            if loss == "mse":
                per, g = d * d, 2.0 * d
            else:
                margins.append(np.abs(np.abs(d) - beta).min())
                small = np.abs(d) < beta
                per, g = np.where(small, 0.5 * d * d / beta, np.abs(d) - 0.5 * beta), np.where(small, d / beta, np.sign(d))
            dy = np.zeros_like(y)
            dy[np.arange(B), action] = g / B
        else:
            probs, legal = rows[1][u].astype(np.float64), mask[info]
            z = np.where(legal, y, -np.inf)
            z = z - z.max(1, keepdims=True)
            e = np.where(legal, np.exp(z), 0.0)
            logp = np.where(legal, z - np.log(e.sum(1, keepdims=True)), 0.0)
            per = -(probs * logp).sum(1)
            dy = np.where(legal, e / e.sum(1, keepdims=True) * probs.sum(1, keepdims=True) - probs, 0.0) / B
        losses.append(per.mean())
        grads = backward(layers, acts, dy)
        scale = 1.0
        if clip is not None:
            norm = np.sqrt(sum((gw * gw).sum() + (gb * gb).sum() for gw, gb in grads))
            margins.append(abs(norm - clip))
            scale = min(1.0, clip / (norm + 1e-6))
        for (w, b), (gw, gb) in zip(layers, grads):
            w -= lr * scale * gw
            b -= lr * scale * gb
    return params, np.array(losses), float(min(margins))


def single_action_mask(mask):
    """The game's mask with infostate 0 cut down to its first legal action."""
    mask = np.array(mask, bool)
    mask[0, np.argmax(mask[0]) + 1:] = False
    return mask


def synthetic_rows(kind, seed, size, mask, finals="mixed", pool=6):
    """`size` buffer rows over a few infostates (infostate 0 among them, in row 0): kind 0 (info, action, reward, next_info,
    final), kind 1 (info, probs on the legal ids).  Few distinct infostates keep the count of distinct ReLU
    pre-activations — each a chance of a small margin — low enough for a seed to exist."""
    rng = np.random.default_rng(seed)
    I, A = mask.shape
    some = np.concatenate([[0], rng.choice(np.arange(1, I), min(pool, I) - 1, replace=False)])
    info = some[rng.integers(0, len(some), size)].astype(np.int32)
    info[0] = 0
    if kind == 0:
        final = {"all": np.ones(size, bool), "none": np.zeros(size, bool)}.get(finals, rng.random(size) < 0.5).astype(np.uint8)
        nxt = np.where(final, -1, some[rng.integers(0, len(some), size)]).astype(np.int32)
        return info, rng.integers(0, A, size).astype(np.int32), rng.normal(0, 1, size).astype(np.float32), nxt, final
    probs = rng.random((size, A)) * mask[info]
    return info, (probs / probs.sum(1, keepdims=True)).astype(np.float32)


def dev(got, want):
    """The largest |x - x64| over parameters and losses, divided by max(1, max |x64|)."""
    got, want = (np.concatenate([np.ravel(p), np.ravel(l)]).astype(np.float64) for p, l in (got, want))
    return float(np.abs(got - want).max() / max(1.0, np.abs(want).max()))
