"""U sequential Adam updates of alpha_zero.VPNetMLP on its three losses in NumPy float64: the reference of
alpha_zero.VPNetLearner and osg_vpnet_learn.  Parameters are flat in VPNetMLP.flat's order."""
import numpy as np

from deep_cfr_learn_cases import BETA1, BETA2, EPS, SMALL_ROOT, dev  # noqa: F401 (dev: the tests' measure)

# The tests' weight decay.  A weight whose data gradient is zero (an observation cell no row of the batch sets) has the
# gradient weight_decay * w, and its sqrt(v^) falls below SMALL_ROOT where |w| < 1e-5 / weight_decay: at the model's default
# 1e-4 that is every such weight, at 0.1 one in some hundreds.
WEIGHT_DECAY = 0.1


def layers_of(flat, shape):
    """[(weight [out, in], bias [out])] per Linear: views of `flat`."""
    O, W, D, A = shape
    out, at = [], 0
    for o, i in [(W, O)] + [(W, W)] * D + [(W, W), (1, W), (W, W), (A, W)]:
        out.append((flat[at:at + o * i].reshape(o, i), flat[at + o * i:at + o * i + o]))
        at += o * i + o
    assert at == flat.size
    return out


def gradient(shape, params, obs, legal, t, z, wd, margins):
    """((policy, value, l2) losses, dLoss/dparams flat) of one batch."""
    D, B = shape[2], obs.shape[0]
    layers, grad = layers_of(params, shape), np.zeros_like(params)
    g = layers_of(grad, shape)

    def relu(pre):
        if np.any(pre != 0):
            margins.append(np.abs(pre[pre != 0]).min())
        return np.maximum(pre, 0.0)
    acts = [obs]
    for w, b in layers[:D + 1]:
        acts.append(relu(acts[-1] @ w.T + b))
    (wv1, bv1), (wv2, bv2), (wp1, bp1), (wp2, bp2) = layers[D + 1:]
    hv, hp = relu(acts[-1] @ wv1.T + bv1), relu(acts[-1] @ wp1.T + bp1)
    v = np.tanh(hv @ wv2.T + bv2)[:, 0]
    logits = hp @ wp2.T + bp2
    some = legal.any(1, keepdims=True)
    top = np.where(some, np.where(legal, logits, -np.inf).max(1, keepdims=True), 0.0)
    e = np.where(legal, np.exp(np.where(legal, logits - top, 0.0)), 0.0)
    mass = np.maximum(e.sum(1, keepdims=True), 1e-300)
    log_softmax = np.where(legal, logits - top - np.log(mass), 0.0)
    tl = np.where(legal, t, 0.0)
    losses = ((-tl * log_softmax).sum() / B, ((v - z) ** 2).mean(), sum(wd * (w ** 2).sum() / 2 for w, _ in layers))
    dz = (e / mass * tl.sum(1, keepdims=True) - tl) / B
    dy = (2.0 * (v - z) * (1.0 - v * v) / B)[:, None]
    g[D + 4][0][:], g[D + 4][1][:] = dz.T @ hp, dz.sum(0)
    dhp = (dz @ wp2) * (hp > 0)
    g[D + 3][0][:], g[D + 3][1][:] = dhp.T @ acts[-1], dhp.sum(0)
    g[D + 2][0][:], g[D + 2][1][:] = dy.T @ hv, dy.sum(0)
    dhv = (dy @ wv2) * (hv > 0)
    g[D + 1][0][:], g[D + 1][1][:] = dhv.T @ acts[-1], dhv.sum(0)
    d = dhv @ wv1 + dhp @ wp1
    for k in range(D, -1, -1):
        d = d * (acts[k + 1] > 0)
        g[k][0][:], g[k][1][:] = d.T @ acts[k], d.sum(0)
        d = d @ layers[k][0]
    for (w, _), (gw, _) in zip(layers, g):
        gw += wd * w
    return losses, grad


def learn(shape, params, obs, legal, policy, value, lr, wd, m=None, v=None, step0=0):
    """obs [U, B, O], legal [U, B, A] bool, policy [U, B, A], value [U, B].  Returns (params, m, v, losses [U, 3], the
    smallest nonzero |pre-activation| at a ReLU, the entries to leave out)."""
    params = np.array(params, np.float64)
    m = np.zeros_like(params) if m is None else np.array(m, np.float64)
    v = np.zeros_like(params) if v is None else np.array(v, np.float64)
    margins, losses, small = [], [], np.zeros(len(params), bool)
    for u in range(obs.shape[0]):
        loss, g = gradient(shape, params, np.asarray(obs[u], np.float64), np.asarray(legal[u], bool),
                           np.asarray(policy[u], np.float64), np.asarray(value[u], np.float64), wd, margins)
        losses.append(loss)
        step = step0 + u + 1
        m = BETA1 * m + (1 - BETA1) * g
        v = BETA2 * v + (1 - BETA2) * g * g
        root = np.sqrt(v) / np.sqrt(1 - BETA2 ** step)
        small |= (root > 0) & (root < SMALL_ROOT)
        params = params - lr / (1 - BETA1 ** step) * m / (root + EPS)
    return params, m, v, np.array(losses), float(min(margins)), small


def inputs(shape, B, U, seed, pool=3):
    """0 / 1 observations, random legal masks (row 1 of every batch with a single legal action), targets on the legal
    simplex, values in [-1, 1]: float32 / bool arrays [U, B, ...].  The rows' observations come from a pool of a few:
    few distinct ReLU pre-activations — each a chance of a small margin — so that a seed exists (as
    deep_cfr_learn_cases.synthetic_rows)."""
    O, _, _, A = shape
    rng = np.random.default_rng(seed)
    obs = (rng.random((pool, O)) < 0.3).astype(np.float32)[rng.integers(0, pool, (U, B))]
    legal = rng.random((U, B, A)) < 0.5
    legal[:, :, A - 1] |= ~legal.any(2)
    legal[:, min(1, B - 1)] = np.arange(A) == A // 2
    policy = (rng.random((U, B, A)) + 0.05) * legal
    policy = (policy / policy.sum(2, keepdims=True)).astype(np.float32)
    return obs, legal, policy, rng.uniform(-1, 1, (U, B)).astype(np.float32)
