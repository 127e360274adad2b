"""ORACLE helper (test infrastructure only) for the flip-gain / quench layer:
numpy restatements, by the definitions of include/mjx.h, of

  * the brute-force flip gains: for every node i flip spin i of every replica,
    roll out T = p + c - 1 steps and compare sum s_end with the unflipped one;
  * consensus and the removable mask;
  * the sequential greedy quench, vectorised over the replicas: node after
    node in ``order``, every consensus replica with s_i = +1 tries s^i with a
    full rollout and keeps it when the end state is still all +1.

Nothing here uses a light cone or the monotonicity fact.  The step itself is
oracle.majority's (attractor_oracle.step_ell / step_csr).
"""
import numpy as np

from attractor_oracle import step_csr, step_ell  # noqa: F401  (re-exported for the tests)


def end_state(step, S, T):
    for _ in range(T):
        S = step(S)
    return S


def flip_gains(step, S, T):
    """S: (R, n) +-1.  -> dict gain int64 (R, n), consensus bool [R],
    removable bool (R, n), n_removable int64 [R]."""
    S = np.asarray(S, dtype=np.int64)
    R, n = S.shape
    F = end_state(step, S, T).sum(axis=1)
    gain = np.empty((R, n), np.int64)
    for i in range(n):
        Si = S.copy()
        Si[:, i] = -Si[:, i]
        gain[:, i] = end_state(step, Si, T).sum(axis=1) - F
    consensus = F == n
    removable = (S == 1) & consensus[:, None] & (F[:, None] + gain == n)
    return {"gain": gain, "consensus": consensus, "removable": removable,
            "n_removable": removable.sum(axis=1).astype(np.int64)}


def quench(step, S, T, order=None):
    """-> dict conf (R, n), flipped int64 [R], consensus bool [R] (of S),
    mag float64 [R], turned bool (R, n) (the spins the pass flipped)."""
    S = np.asarray(S, dtype=np.int64).copy()
    R, n = S.shape
    order = np.arange(n) if order is None else np.asarray(order)
    consensus = end_state(step, S, T).sum(axis=1) == n
    turned = np.zeros((R, n), bool)
    for i in order:
        try_ = np.flatnonzero(consensus & (S[:, i] == 1))
        if try_.size == 0:
            continue
        Si = S[try_].copy()
        Si[:, i] = -1
        keep = end_state(step, Si, T).sum(axis=1) == n
        S[try_[keep], i] = -1
        turned[try_[keep], i] = True
    return {"conf": S, "flipped": turned.sum(axis=1).astype(np.int64), "consensus": consensus,
            "mag": S.sum(axis=1) / n, "turned": turned}


def random_starts(R, n, m_init, seed):
    """(R, n) i.i.d. +-1 spins, +1 with probability (1 + m_init) / 2."""
    rng = np.random.default_rng(seed)
    return np.where(rng.random((R, n)) < (1.0 + m_init) / 2.0, 1, -1).astype(np.int64)


def unpack_mask(words, n, R):
    """Replica-packed mask words (n * W int64) -> bool (R, n) and "any padding bit set"."""
    W = (R + 63) // 64
    w = np.asarray(words).view(np.uint64).reshape(n, W)
    b = ((w[:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)).reshape(n, W * 64)
    return b[:, :R].T.astype(bool), bool(b[:, R:].any())
