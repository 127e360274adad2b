"""ORACLE helper (test infrastructure only) for the run-to-attractor layer:
numpy restatements of

  * the attractor of the synchronous majority dynamics, by the definitions of
    include/mjx.h: trajectory s(0) = s0, s(t+1) = onestep(s(t)); per replica
    p = min{t >= 0 : s(t+2) = s(t)}, c = 1 if s(p+1) = s(p) else 2,
    sum_att = (sum s(p), sum s(p+1)); p > t_max reports p = -1, c = 0;
  * Random123's philox4x32_10 block (ten rounds) on numpy uint32 arrays;
  * the random-start rule of mjx_random_spins_rp: spin (v, r) is +1 iff
    x < floor(prob[r] * 2^32), x = word r & 3 of
    philox4x32_10(counter (v_lo, v_hi, r >> 2, 0), key (seed_lo, seed_hi)).

The step itself is oracle.majority's (onestep_majority_batch on an (n, d)
neighbour array, onestep_majority_er on CSR).
"""
import numpy as np

from oracle import majority as orc


def step_ell(adj):
    adj = np.asarray(adj)
    return lambda S: orc.onestep_majority_batch(adj, S)


def step_csr(row_ptr, col):
    return lambda S: orc.onestep_majority_er(row_ptr, col, S)


def attractor(step, S0, t_max=4096, chunk=16):
    """Attractor of every row of S0 (R, n) under ``step``.

    The trajectory is followed in chunks of ``chunk`` steps and stops at the
    first chunk boundary where every replica has settled, or after t_max + 2
    steps (the last chunk is cut there): ``t_end`` is the number of steps made
    and ``state`` is s(t_end).  p, c and sum_att do not depend on ``chunk``.
    """
    S0 = np.asarray(S0, dtype=np.int64)
    R, n = S0.shape
    p = np.full(R, -1, np.int64)
    c = np.zeros(R, np.int64)
    sum_att = np.zeros((R, 2), np.int64)
    s_t, s_t1 = S0, None            # s(t), s(t+1) for the t tested next
    cur, k = S0, 0                  # cur = s(k)
    while k < t_max + 2:
        for _ in range(min(chunk, t_max + 2 - k)):
            nxt = step(cur)
            k += 1
            if k >= 2:
                t = k - 2           # s_t = s(t), s_t1 = s(t+1), nxt = s(t+2)
                hit = (p < 0) & np.all(nxt == s_t, axis=1)
                p[hit] = t
                c[hit] = np.where(np.all(s_t1[hit] == s_t[hit], axis=1), 1, 2)
                sum_att[hit, 0] = s_t[hit].sum(axis=1)
                sum_att[hit, 1] = s_t1[hit].sum(axis=1)
                s_t, s_t1 = s_t1, nxt
            else:
                s_t1 = nxt
            cur = nxt
        if np.all(p >= 0):
            break
    return {"p": p, "c": c, "sum_att": sum_att, "t_end": k, "state": cur}


# ---- Philox-4x32-10 -------------------------------------------------------
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_SH = np.uint64(32)


def philox4x32_10(ctr, key):
    """ctr: four uint32 arrays (broadcastable), key: two uint32 scalars or
    arrays -> four uint32 arrays."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(x, dtype=np.uint64) & _LO for x in ctr])
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for q in range(10):
        if q > 0:
            k0 = (k0 + _W0) & 0xFFFFFFFF
            k1 = (k1 + _W1) & 0xFFFFFFFF
        p0, p1 = _M0 * c0, _M1 * c2              # 32 x 32 -> 64, no overflow in uint64
        hi0, lo0 = p0 >> _SH, p0 & _LO
        hi1, lo1 = p1 >> _SH, p1 & _LO
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
    return tuple(x.astype(np.uint32) for x in (c0, c1, c2, c3))


def random_spins(n, R, prob, seed):
    """(R, n) int64 +-1 spins by the rule of mjx_random_spins_rp."""
    prob = np.broadcast_to(np.asarray(prob, dtype=np.float64), (R,))
    thr = np.floor(prob * 4294967296.0).astype(np.uint64)          # 0 .. 2^32
    v = np.arange(n, dtype=np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    key = (seed & 0xFFFFFFFF, seed >> 32)
    S = np.empty((R, n), np.int64)
    for g in range((R + 3) // 4):
        x = philox4x32_10((v & _LO, v >> _SH, np.uint64(g), np.uint64(0)), key)
        for j in range(4):
            r = 4 * g + j
            if r < R:
                S[r] = np.where(x[j].astype(np.uint64) < thr[r], 1, -1)
    return S


def unpack_rp(bits, n, R):
    """Replica-packed words (n * W int64/uint64) -> (R, n) +-1, and the padding
    bits (positions R .. 64 W - 1) as a boolean "any set"."""
    W = (R + 63) // 64
    w = np.asarray(bits).view(np.uint64).reshape(n, W)
    b = ((w[:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)).reshape(n, W * 64)
    return np.where(b[:, :R].T == 1, 1, -1).astype(np.int64), bool(b[:, R:].any())
