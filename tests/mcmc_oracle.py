"""fp64 restatement, in numpy and plain Python, of the MCMC strategy's kernels (csrc/mcmc.hip; DESIGN.md section 7f is the contract):
the Philox4x32-10 generator and its uniforms / normals, the weighted sampler with the kernel's block tree (as
tests/test_fixed_sum_gpu.py emulates block_sum: the same additions in the same order give the same bits), compute_relocation with
math.comb and math.fsum, relocation / growth on numpy arrays, and the noise.  No torch, no GPU."""
import math

import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
BLOCK, LANES, PER_LANE = 1024, 256, 4
MAX_RATIO = 51
STREAM_RELOCATE, STREAM_GROW, STREAM_NOISE_A, STREAM_NOISE_B = 0, 1, 2, 3


# ------------------------------------------------------------------------------------------------------------ random numbers

def philox(counter, key):
    """Philox4x32-10 on Python integers: counter (4 words), key (2 words) -> 4 words."""
    c, k = list(counter), list(key)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & MASK, (p0 >> 32) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + W0) & MASK, (k[1] + W1) & MASK]
    return c


def philox_np(c0, c1, c2, c3, k0, k1):
    """The same on uint64 arrays holding 32-bit words (broadcast against each other)."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(x, dtype=np.uint64) for x in np.broadcast_arrays(c0, c1, c2, c3, k0, k1))
    mask = np.uint64(MASK)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & mask, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & mask
        k0, k1 = (k0 + np.uint64(W0)) & mask, (k1 + np.uint64(W1)) & mask
    return c0, c1, c2, c3


def key_of(seed):
    return seed & MASK, (seed >> 32) & MASK


def draw(seed, slot, stream, step):
    """the four words of (slot, stream) at `step`: counter (slot, 0, stream, step), key = seed, low word first"""
    return philox((slot, 0, stream, step), key_of(seed))


def draw_np(seed, slots, stream, step):
    k0, k1 = key_of(seed)
    return philox_np(np.asarray(slots, dtype=np.uint64), 0, stream, step, k0, k1)


def uniform(x0, x1):
    """53 bits -> a double in [0, 1); integer arithmetic, then one exact conversion and one exact scaling"""
    return float((int(x0) >> 5) * (1 << 26) + (int(x1) >> 6)) * 2.0 ** -53


def uniform_np(x0, x1):
    return ((x0 >> np.uint64(5)) * np.uint64(1 << 26) + (x1 >> np.uint64(6))).astype(np.float64) * 2.0 ** -53


def normals(words):
    """Box-Muller in fp64: u1 from words (0, 1), u2 from (2, 3) -> (z0, z1)"""
    u1, u2 = uniform(words[0], words[1]), uniform(words[2], words[3])
    r = math.sqrt(-2.0 * math.log(1.0 - u1))
    return r * math.cos(2.0 * math.pi * u2), r * math.sin(2.0 * math.pi * u2)


def normals_np(words):
    u1, u2 = uniform_np(words[0], words[1]), uniform_np(words[2], words[3])
    r = np.sqrt(-2.0 * np.log(1.0 - u1))
    return r * np.cos(2.0 * math.pi * u2), r * np.sin(2.0 * math.pi * u2)


# ------------------------------------------------------------------------------------------------------------------- sampler

def pool_weights(weights, min_weight, alive_only):
    w32 = np.asarray(weights, dtype=np.float32)
    w = w32.astype(np.float64)
    return np.where(w32 > np.float32(min_weight), w, 0.0) if alive_only else w


def block_totals(pool):
    """T_b of blocks of 1024: each of 256 lanes adds its 4 consecutive elements in index order, then the halving tree of
    csrc/fixed_sum.h (red[t] += red[t + s], s = 128 ... 1).  Elements past the end count as +0.0 (x + 0.0 == x for x >= 0)."""
    nb = (len(pool) + BLOCK - 1) // BLOCK
    x = np.zeros(nb * BLOCK, dtype=np.float64)
    x[:len(pool)] = pool
    x = x.reshape(nb, LANES, PER_LANE)
    red = ((x[:, :, 0] + x[:, :, 1]) + x[:, :, 2]) + x[:, :, 3]
    s = LANES // 2
    while s > 0:
        red = red[:, :s] + red[:, s:2 * s]
        s //= 2
    return red[:, 0].copy()


def prefix(T):
    """P_b = T_0 + ... + T_(b-1) added sequentially, and the total"""
    P, run = np.zeros(len(T), dtype=np.float64), 0.0
    for b, t in enumerate(T.tolist()):
        P[b] = run
        run += t
    return P, run


def pick(pool, T, P, t):
    """The selection rule for one draw t, written out: the last block with T_b > 0 and P_b <= t, walked in index order."""
    cand = [b for b in range(len(T)) if T[b] > 0.0 and P[b] <= t]
    b = cand[-1]
    c, last = float(P[b]), -1
    for i in range(b * BLOCK, min((b + 1) * BLOCK, len(pool))):
        c += float(pool[i])
        if pool[i] > 0.0:
            if c > t:
                return i
            last = i
    return last


def sample(weights, min_weight, alive_only, n_slots, seed, stream, step, slow=False):
    """-> (src int32 [n_slots], counts int32 [U]) of v3a_mcmc_sample.  slow: every draw through pick() instead of the vectorised
    search (the two are compared in tests/test_mcmc_host.py)."""
    w32 = np.asarray(weights, dtype=np.float32)
    U = len(w32)
    pool = pool_weights(w32, min_weight, alive_only)
    T = block_totals(pool)
    P, total = prefix(T)
    src, counts = np.full(n_slots, -1, dtype=np.int32), np.zeros(U, dtype=np.int32)
    active = np.nonzero(w32 <= np.float32(min_weight))[0] if alive_only else np.arange(n_slots)
    if not total > 0.0 or len(active) == 0:
        return src, counts
    words = draw_np(seed, active, stream, step)
    t = uniform_np(words[0], words[1]) * total
    if slow:
        chosen = np.array([pick(pool, T, P, float(x)) for x in t], dtype=np.int64)
    else:
        nb = len(T)
        padded = np.zeros(nb * BLOCK, dtype=np.float64)
        padded[:U] = pool
        padded = padded.reshape(nb, BLOCK)
        cum = np.cumsum(np.concatenate([P[:, None], padded], axis=1), axis=1)[:, 1:]     # sequential: c = P_b; c += w_i
        positive = padded > 0.0
        last = np.where(positive.any(1), BLOCK - 1 - np.argmax(positive[:, ::-1], axis=1), -1)
        heavy = np.nonzero(T > 0.0)[0]
        b = heavy[np.searchsorted(P[heavy], t, side="right") - 1]
        chosen = np.empty(len(t), dtype=np.int64)
        for lo in range(0, len(t), 2048):
            bb, tt = b[lo:lo + 2048], t[lo:lo + 2048]
            ok = positive[bb] & (cum[bb] > tt[:, None])
            first = np.argmax(ok, axis=1)
            chosen[lo:lo + 2048] = bb * BLOCK + np.where(ok.any(1), first, last[bb])
    src[active] = chosen
    np.add.at(counts, chosen, 1)
    return src, counts


# ------------------------------------------------------------------------------------------------------- relocation and growth

def relocation_den(o1, r):
    return math.fsum(math.comb(i - 1, k) * ((-1) ** k / math.sqrt(k + 1)) * o1 ** (k + 1) for i in range(1, r + 1) for k in range(i))


def relocation(op, scale, count, min_opacity=0.005):
    """compute_relocation for a Gaussian of opacity `op` and scale(s) `scale` drawn `count` times -> (clamped new opacity, new
    scale(s), unclamped new opacity)"""
    r = min(count + 1, MAX_RATIO)
    o1 = 1.0 - (1.0 - op) ** (1.0 / r)
    coef = op / relocation_den(o1, r)
    o2 = min(max(o1, min_opacity), 1.0 - 2.0 ** -23)
    return o2, [coef * s for s in scale] if isinstance(scale, (list, tuple)) else coef * scale, o1


def new_values(logit, log_scales, count, min_opacity):
    """-> (new logit, [3 new log-scales]) in fp64 from the stored f32 values"""
    op = 1.0 / (1.0 + math.exp(-float(logit)))
    o2, sc, _ = relocation(op, [math.exp(float(x)) for x in log_scales], count, min_opacity)
    return math.log(o2 / (1.0 - o2)), [math.log(s) for s in sc]


def new_values_f32(logit, log_scales, count, min_opacity):
    """the same arithmetic in float32 throughout: the comparison figure of the parity tests"""
    f = np.float32
    r = min(count + 1, MAX_RATIO)
    op = f(1) / (f(1) + np.exp(-f(logit)))
    o1 = f(1) - np.power(f(1) - op, f(1) / f(r))
    den = f(0)
    for i in range(1, r + 1):
        for k in range(i):
            den = den + f(math.comb(i - 1, k)) * (f((-1) ** k) / np.sqrt(f(k + 1))) * np.power(o1, f(k + 1))
    coef = op / den
    o2 = min(max(o1, f(min_opacity)), f(1.0 - 2.0 ** -23))
    return float(np.log(o2 / (f(1) - o2))), [float(np.log(coef * np.exp(f(x)))) for x in log_scales]


NAMES = ("means", "scales", "quats", "opacities", "sh")


def relocate(src, counts, params, m, v, dst_offset, min_opacity, values=new_values):
    """v3a_mcmc_relocate on dicts of numpy f32 arrays -> (params, m, v, exact): new dicts, and `exact` = {"opacities": f64 [rows],
    "scales": f64 [rows,3]} holding the unrounded new values where a row got some (NaN elsewhere)."""
    U = len(counts)
    growth = dst_offset != 0
    assert dst_offset in (0, U) and (growth or len(src) == U)
    p2, m2, v2 = ({k: np.array(d[k], dtype=np.float32, copy=True) for k in NAMES} for d in (params, m, v))
    rows = len(p2["means"])
    assert rows == (U + len(src) if growth else U)
    exact = dict(opacities=np.full(rows, np.nan), scales=np.full((rows, 3), np.nan))
    fresh = {}
    for j in np.nonzero(np.asarray(counts) > 0)[0].tolist():
        fresh[j] = values(params["opacities"][j], params["scales"][j], int(counts[j]), min_opacity)
    for j, (lg, ls) in fresh.items():
        p2["opacities"][j], p2["scales"][j] = lg, ls
        exact["opacities"][j], exact["scales"][j] = lg, ls
        if not growth:
            for k in NAMES:
                m2[k][j], v2[k][j] = 0.0, 0.0
    for s, j in enumerate(np.asarray(src).tolist()):
        if j < 0:
            continue
        d = dst_offset + s
        lg, ls = fresh[j]
        p2["opacities"][d], p2["scales"][d] = lg, ls
        exact["opacities"][d], exact["scales"][d] = lg, ls
        for k in ("means", "quats", "sh"):
            p2[k][d] = params[k][j]
        if growth:
            for k in NAMES:
                m2[k][d], v2[k][d] = 0.0, 0.0
    return p2, m2, v2, exact


# --------------------------------------------------------------------------------------------------------------------- noise

def rotation(quats, dt=np.float64):
    """R [U,3,3] of raw quaternions (i, j, k, r) by v3a_splat_activate's expression, evaluated in `dt`"""
    q = np.asarray(quats, dtype=np.float32).astype(dt)
    n2 = ((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3]
    q = q * (dt(1) / (np.sqrt(n2) + dt(np.float32(1e-8))))[:, None]
    i, j, k, r = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    two_s = dt(2) / (((i * i + j * j) + k * k) + r * r)
    R = np.stack([1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                  two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                  two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)], axis=1)
    return R.reshape(-1, 3, 3)


def noise_gate(logits, dt=np.float64):
    op = dt(1) / (dt(1) + np.exp(-np.asarray(logits, dtype=np.float32).astype(dt)))
    with np.errstate(over="ignore"):      # float32: exp overflows to inf for an opaque Gaussian and the gate is 0
        return dt(1) / (dt(1) + np.exp(dt(-100) * ((dt(1) - op) - dt(0.995))))


def noise_draws(U, seed, step):
    """xi [U,3] in fp64: (z0, z1) of stream 2 and z0 of stream 3 at slot = row"""
    slots = np.arange(U)
    a0, a1 = normals_np(draw_np(seed, slots, STREAM_NOISE_A, step))
    b0, _ = normals_np(draw_np(seed, slots, STREAM_NOISE_B, step))
    return np.stack([a0, a1, b0], axis=1)


def noise(means, log_scales, quats, logits, scaler, seed, step, dt=np.float64):
    """v3a_mcmc_noise -> the new means in `dt`, NOT rounded to f32 (dt = float64: the exact side of the parity figure; float32: the
    same arithmetic in single precision, the comparison figure; the normal draws are fp64 values either way)"""
    U = len(logits)
    R = rotation(quats, dt)
    s2 = np.exp(dt(2) * np.asarray(log_scales, dtype=np.float32).astype(dt))
    n = noise_draws(U, seed, step).astype(dt) * (noise_gate(logits, dt) * dt(scaler))[:, None]
    d = np.zeros((U, 3), dtype=dt)
    for a in range(3):
        acc = np.zeros(U, dtype=dt)
        for b in range(3):
            cov = ((R[:, a, 0] * s2[:, 0]) * R[:, b, 0] + (R[:, a, 1] * s2[:, 1]) * R[:, b, 1]) + (R[:, a, 2] * s2[:, 2]) * R[:, b, 2]
            acc = acc + cov * n[:, b]
        d[:, a] = acc
    return np.asarray(means, dtype=np.float32).astype(dt) + d
