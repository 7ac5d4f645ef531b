"""Decision rules and exact references for the statistical tests of the sampling layer (NumPy only; not a test module).

Replay parity (the oracle restates the counter generator and replays the device draw for draw) proves that the device
and the restatement agree; the rules here ask whether the draws they agree on have the right DISTRIBUTION.  Every rule
is closed-form, every threshold follows from N, the number of comparisons M, delta = 1e-9 and the variable's range or
exact variance — nothing is tuned to what the code under test gives.

  chi_square          Pearson X^2 of counts against exact probabilities, mapped to a normal score by Wilson-Hilferty;
                      accept |z| <= 6 (two-sided, ~2e-9).  A fit that is too good is a finding too.  Every expected
                      count must be >= 20 (asserted); no cell is merged or dropped.
  bernstein_bound     |mean - mu| <= t for a bounded variable of KNOWN variance
  hoeffding_bound     the same with unknown variance
  two_sample_mean_z   two independent estimates of one mean (a recorded reference estimate against the device's)
  check_means         rows against exact means: per-row Bernstein bound, exact equality where the variance is 0, and
                      the aggregate sum of z_i^2 as a chi-square (catches a small bias that every row shares)

  random_play_moments backward pass over a level-ordered edge table: E[return], E[return^2], E[plies] of uniformly
                      random play from every position
  es_expected_deltas  the expected regret / kSimple average-policy increment of ONE external-sampling trajectory per
                      traverser on a frozen table (external_sampling_mccfr.cc:122-186), by a plain recursion

and vectorised restatements of the generator and the keyed orders of open_spiel_amd/csrc/osg_common.h.
"""
import math

import numpy as np

Z_MAX = 6.0
DELTA = 1e-9
MIN_EXPECTED = 20.0


# ---------------------------------------------------------------------------------------------------------------
# decision rules
# ---------------------------------------------------------------------------------------------------------------
def wilson_hilferty(x2, d):
    """Normal score of a chi-square statistic with d degrees of freedom."""
    v = 2.0 / (9.0 * d)
    return ((x2 / d) ** (1.0 / 3.0) - (1.0 - v)) / math.sqrt(v)


def chi_square(counts, probs):
    """(z, X^2, d) of integer counts against exact cell probabilities (same shape; probabilities sum to 1)."""
    counts = np.asarray(counts, np.float64).ravel()
    probs = np.asarray(probs, np.float64).ravel()
    assert counts.shape == probs.shape and counts.size >= 2
    assert abs(probs.sum() - 1.0) < 1e-9 and (probs > 0).all()
    expected = counts.sum() * probs
    assert expected.min() >= MIN_EXPECTED, f"thin cell: expected count {expected.min():.2f} < {MIN_EXPECTED}"
    x2 = float((((counts - expected) ** 2) / expected).sum())
    d = counts.size - 1
    return wilson_hilferty(x2, d), x2, d


def chi_square_grouped(counts, expected, groups):
    """One X^2 over many independent multinomials (e.g. the children of every position): cells `counts` with exact
    `expected` counts, `groups` of them; degrees of freedom = cells - groups."""
    counts = np.asarray(counts, np.float64).ravel()
    expected = np.asarray(expected, np.float64).ravel()
    assert counts.shape == expected.shape and abs(counts.sum() - expected.sum()) < 1e-6 * max(1.0, expected.sum())
    assert expected.min() >= MIN_EXPECTED, f"thin cell: expected count {expected.min():.2f} < {MIN_EXPECTED}"
    x2 = float((((counts - expected) ** 2) / expected).sum())
    d = counts.size - int(groups)
    return wilson_hilferty(x2, d), x2, d


def accept(z):
    return abs(z) <= Z_MAX


def bernstein_bound(n, var, c, m=1, delta=DELTA):
    """t with 2 exp(-n t^2 / (2 var + 2 c t / 3)) = delta / m: the positive root of n t^2 - (2 c L / 3) t - 2 var L."""
    big_l = math.log(2.0 * m / delta)
    var = np.asarray(var, np.float64)
    b = 2.0 * c * big_l / 3.0
    return (b + np.sqrt(b * b + 8.0 * n * var * big_l)) / (2.0 * n)


def hoeffding_bound(n, c, m=1, delta=DELTA):
    """|mean - mu| <= c sqrt(ln(2 m / delta) / (2 n))."""
    return c * math.sqrt(math.log(2.0 * m / delta) / (2.0 * n))


def check_means(means, mu, var, n, c, delta=DELTA):
    """Rows of sample means (n samples each, range c) against exact means `mu` and exact variances `var`.
    Returns dict(worst: max |mean - mu| / bound over the rows with var > 0, exact: rows with var == 0 all equal,
    z, x2, d: the aggregate sum of z_i^2 over the rows with var > 0 as a chi-square, ok)."""
    means, mu, var = (np.asarray(a, np.float64).ravel() for a in (means, mu, var))
    assert means.shape == mu.shape == var.shape
    live = var > 0
    m = int(live.sum())
    exact = bool((means[~live] == mu[~live]).all())
    out = dict(rows=means.size, m=m, exact=exact, worst=0.0, worst_bound=0.0, worst_err=0.0, z=0.0, x2=0.0, d=0)
    if m:
        bound = bernstein_bound(n, var[live], c, m, delta)
        err = np.abs(means[live] - mu[live])
        k = int(np.argmax(err / bound))
        x2 = float((n * (means[live] - mu[live]) ** 2 / var[live]).sum())
        out.update(worst=float(err[k] / bound[k]), worst_bound=float(bound[k]), worst_err=float(err[k]),
                   x2=x2, d=m, z=wilson_hilferty(x2, m))
    out["ok"] = exact and out["worst"] <= 1.0 and (m < 2 or accept(out["z"]))
    return out


def two_sample_mean_z(mean1, var1, n1, mean2, var2, n2):
    """z of the difference of two independent sample means (per-sample variances var1, var2; n1, n2 samples)."""
    return (mean1 - mean2) / math.sqrt(var1 / n1 + var2 / n2)


# ---------------------------------------------------------------------------------------------------------------
# exact references
# ---------------------------------------------------------------------------------------------------------------
def random_play_moments(edge_off, edge_child, terminal_value):
    """Uniformly random play from every position of a level-ordered edge table (a child's index is above its
    parent's; position i has the edges edge_off[i] .. edge_off[i + 1]; a position without edges is terminal and
    terminal_value[i] is player 0's return there).  Returns (E[return], E[return^2], E[plies to the end]), float64
    arrays over the positions: a position's value is the mean of its children's."""
    edge_off = np.asarray(edge_off, np.int64)
    edge_child = np.asarray(edge_child, np.int64)
    n = edge_off.size - 1
    counts = np.diff(edge_off)
    parent = np.repeat(np.arange(n, dtype=np.int64), counts)
    assert edge_child.size == edge_off[-1] and (edge_child > parent).all(), "edge table is not level-ordered"
    terminal = counts == 0
    tv = np.where(terminal, np.asarray(terminal_value, np.float64), 0.0)
    m1, m2, plies = tv.copy(), tv * tv, np.zeros(n, np.float64)
    inner = ~terminal
    div = np.maximum(counts, 1).astype(np.float64)
    # a pass makes every position right whose children are; after (height of the table) passes nothing changes
    for _ in range(n + 1):
        s1 = np.bincount(parent, weights=m1[edge_child], minlength=n) / div
        s2 = np.bincount(parent, weights=m2[edge_child], minlength=n) / div
        sp = 1.0 + np.bincount(parent, weights=plies[edge_child], minlength=n) / div
        n1, n2, npl = np.where(inner, s1, m1), np.where(inner, s2, m2), np.where(inner, sp, 0.0)
        same = (n1 == m1).all() and (n2 == m2).all() and (npl == plies).all()
        m1, m2, plies = n1, n2, npl
        if same:
            break
    return m1, m2, plies


def regret_matching(regrets):
    r = np.maximum(np.asarray(regrets, np.float64), 0.0)
    s = r.sum()
    return r / s if s > 0 else np.full(r.size, 1.0 / r.size)


def es_expected_deltas(oracle_game, regrets=None):
    """Expected increments of one external-sampling traversal per traverser on a frozen table.

    regrets: {infostate key: regrets in LegalActions() order} (missing keys: zeros, i.e. the uniform policy);
    sigma = regret matching.  Returns (d_regret, d_policy), dicts {infostate key: float64 [|A(I)|]}:
      d_regret[I][a] = sum over h in I of pi_{-i}(h) (u_i(h a) - u_i(h)),      i = the player of I
      d_policy[I][a] = sum over h in I of pi_{-i}(h) sigma(I, a),              i = (player of I - 1) mod P
    pi_{-i} is the reach of chance and of every player but i; u_i the expected return of i under sigma."""
    regrets = regrets or {}
    num_players = oracle_game.num_players
    d_regret, d_policy = {}, {}

    def walk(state, reach_wo):   # reach_wo[i] = pi_{-i}(h); returns u(h) for every player
        if state.is_terminal():
            return np.asarray(state.returns(), np.float64)
        if state.is_chance_node():
            u = np.zeros(num_players)
            for a, pr in state.chance_outcomes():
                u += pr * walk(state.child(a), reach_wo * pr)
            return u
        p = state.current_player()
        key = state.information_state_string(p)
        legal = state.legal_actions()
        sigma = regret_matching(regrets.get(key, np.zeros(len(legal))))
        child_u = []
        for k, a in enumerate(legal):
            scaled = reach_wo * sigma[k]
            scaled[p] = reach_wo[p]
            child_u.append(walk(state.child(a), scaled))
        child_u = np.asarray(child_u)
        u = sigma @ child_u
        d_regret.setdefault(key, np.zeros(len(legal)))
        d_policy.setdefault(key, np.zeros(len(legal)))
        d_regret[key] += reach_wo[p] * (child_u[:, p] - u[p])
        d_policy[key] += reach_wo[(p - 1) % num_players] * sigma
        return u

    walk(oracle_game.new_initial_state(), np.ones(num_players))
    return d_regret, d_policy


# ---------------------------------------------------------------------------------------------------------------
# open_spiel_amd/csrc/osg_common.h, restated on uint64 / uint32 arrays
# ---------------------------------------------------------------------------------------------------------------
_U64 = np.uint64
_U32 = np.uint32


def _u64(x):
    return np.asarray(x).astype(_U64) if isinstance(x, np.ndarray) else _U64(int(x) & ((1 << 64) - 1))


def mix64(z):
    with np.errstate(over="ignore"):
        z = (z ^ (z >> _U64(30))) * _U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U64(27))) * _U64(0x94D049BB133111EB)
        return z ^ (z >> _U64(31))


def mix32(x):
    with np.errstate(over="ignore"):
        x = np.asarray(x, _U32)
        x = x ^ (x >> _U32(16))
        x = x * _U32(0x7FEB352D)
        x = x ^ (x >> _U32(15))
        x = x * _U32(0x846CA68B)
        return x ^ (x >> _U32(16))


class VecRng:
    """Rng of osg_common.h for arrays of (seed, stream, sub) (broadcast together)."""

    def __init__(self, seed, stream, sub=0):
        seed, stream, sub = np.broadcast_arrays(_u64(seed), _u64(stream), _u64(sub))
        with np.errstate(over="ignore"):
            a = mix64(seed + _U64(0x9E3779B97F4A7C15))
            b = mix64(a ^ (stream * _U64(0xD1342543DE82EF95) + _U64(0x632BE59BD9B4E019)))
            self.s = mix64(b ^ (sub * _U64(0xA0761D6478BD642F) + _U64(0xE7037ED1A0B428DB)))

    def next(self):
        with np.errstate(over="ignore"):
            self.s = self.s + _U64(0x9E3779B97F4A7C15)
        return mix64(self.s)

    def below(self, n):
        return (((self.next() >> _U64(32)) * _U64(n)) >> _U64(32)).astype(np.int64)

    def unit(self):
        return (self.next() >> _U64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


K_ORDER_SALT = 0x6F726465725F6B79
K_FILL_SALT = 0x66696C6C5F6B6579
PATH_HASH_ROOT = 0x243F6A8885A308D3


def _salted_base(seed, root, salt):
    with np.errstate(over="ignore"):
        return mix64(mix64(_u64(seed) ^ _U64(salt)) ^ (_u64(root) * _U64(0xD1342543DE82EF95) + _U64(0x632BE59BD9B4E019)))


def order_base(seed, root):
    return _salted_base(seed, root, K_ORDER_SALT)


def order_key(base, parent_path_hash, action):
    """[..., len(action)] uint32 keys of the siblings `action` (ascending key = first in the order)."""
    action = np.asarray(action, np.int64)
    with np.errstate(over="ignore"):
        lo = (np.asarray(base, _U64) & _U64(0xFFFFFFFF)).astype(_U32) ^ _U32(parent_path_hash & 0xFFFFFFFF)
        h = mix32(lo[..., None] ^ ((action + 1).astype(_U32) * _U32(0x9E3779B1)))
    return (h & _U32(0xFFFFFF00)) | (action & 0xFF).astype(_U32)


def fill_base(seed, root, sub):
    a = _salted_base(seed, root, K_FILL_SALT)
    word = (a & _U64(0xFFFFFFFF)).astype(_U32) ^ (a >> _U64(32)).astype(_U32)
    sub = np.asarray(_u64(sub))
    with np.errstate(over="ignore"):
        return mix32(word ^ ((sub & _U64(0xFFFFFFFF)).astype(_U32) * _U32(0x9E3779B1))
                     ^ ((sub >> _U64(32)).astype(_U32) * _U32(0x85EBCA6B)))


def fill_key(base, cell):
    """[..., len(cell)] uint64 keys of the cells (32 mixed bits << 8 | low byte of the cell id)."""
    cell = np.asarray(cell, np.int64)
    with np.errstate(over="ignore"):
        h = mix32(np.asarray(base, _U32)[..., None] ^ ((cell + 1).astype(_U32) * _U32(0x9E3779B1)))
    return (h.astype(_U64) << _U64(8)) | (cell & 0xFF).astype(_U64)


# ---------------------------------------------------------------------------------------------------------------
# small helpers shared by the CPU and the GPU tests
# ---------------------------------------------------------------------------------------------------------------
def permutation_index(order):
    """[..., k] orders (permutations of 0 .. k-1) -> their Lehmer rank in [0, k!)."""
    order = np.asarray(order, np.int64)
    k = order.shape[-1]
    rank = np.zeros(order.shape[:-1], np.int64)
    for i in range(k):
        smaller = (order[..., i + 1:] < order[..., i:i + 1]).sum(axis=-1)
        rank = rank * (k - i) + smaller
    return rank


def unordered_pair_index(a, b, k):
    """Index of the unordered pair {a, b} (a != b, both < k) in [0, k (k - 1) / 2)."""
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    return lo * (2 * k - lo - 1) // 2 + (hi - lo - 1)


def counts_of(index, cells):
    return np.bincount(np.asarray(index, np.int64).ravel(), minlength=cells)
