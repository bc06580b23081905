"""fp64 restatement, in numpy and plain Python, of the densification strategy's kernels (csrc/densify.hip; DESIGN.md section 7f is the
contract, gsplat's DefaultStrategy restated).  The random numbers are tests/mcmc_oracle.py's Philox and Box-Muller.  No torch, no GPU.

Per step:    accumulate   grad2d[g] += sqrt((gx W/2 C)^2 + (gy H/2 C)^2), count[g] += 1 for every camera with radii[c,g] > 0.
Per refine:  classify     avg = grad2d / max(count, 1); high = avg > grow_grad2d; small = max_k exp(ls) <= grow_scale3d;
                          fate = clone if high and small, split if high and not small, else keep (all keep with grow = False);
                          pruning judges the GROWN set: a keep's or clone's rows have the parent's opacity and scale, a split's two
                          children opacity o (or 1 - sqrt(1 - o), revised) and scale smax / 1.6; pruned = opacity < prune_opa or
                          (prune_big and scale > prune_scale3d).
             apply        rows in gsplat's order: A surviving non-split originals by index, B surviving clones by parent index,
                          C first children, D second children; A keeps its moments, B, C, D start with zeros; child c has
                          ls - log 1.6, the (revised) logit, the parent's quats and sh, and
                          means + R (exp(ls) * z), z = (z0, z1) of stream 4 + 2c and z0 of stream 5 + 2c at counter (g, 0, stream, t).
Reset:       logit = min(logit, logit(max_opacity)); m = v = 0."""
import math

import numpy as np

import mcmc_oracle as MO

KEEP, CLONE, SPLIT, PRUNED = 0, 1, 2, 4
NAMES = ("means", "scales", "quats", "opacities", "sh")
STREAMS = dict(split0=4, split1=6)          # each child: z0, z1 of stream s, z2 = z0 of stream s + 1


def accumulate(grad2d, count, d_means2d, radii, width, height, dt=np.float64):
    """-> (grad2d as `dt`, unrounded with dt = float64; count).  d_means2d [C,U,2], radii [C,U]."""
    C = d_means2d.shape[0]
    vis = radii > 0
    if dt == np.float64:
        gx = d_means2d[..., 0].astype(np.float64) * (0.5 * width * C)
        gy = d_means2d[..., 1].astype(np.float64) * (0.5 * height * C)
        s = np.zeros(grad2d.shape[0])
        for c in range(C):                                        # cameras in index order
            s = s + np.where(vis[c], np.sqrt(gx[c] * gx[c] + gy[c] * gy[c]), 0.0)
        return grad2d.astype(np.float64) + s, count + vis.sum(0).astype(count.dtype)
    g = grad2d.astype(np.float32).copy()
    for c in range(C):
        gx = d_means2d[c, :, 0] * np.float32(0.5 * width * C)
        gy = d_means2d[c, :, 1] * np.float32(0.5 * height * C)
        g = np.where(vis[c], g + np.sqrt(gx * gx + gy * gy, dtype=np.float32), g).astype(np.float32)
    return g, count + vis.sum(0).astype(count.dtype)


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, dtype=np.float64)))


def quantities(grad2d, count, ls, logits, revised):
    """the four numbers the decisions compare, fp64: avg, smax, and the (opacity, scale) of a split's children"""
    avg = grad2d.astype(np.float64) / np.maximum(count, 1).astype(np.float64)
    smax = np.exp(ls.astype(np.float64)).max(1)
    o = sigmoid(logits)
    return avg, smax, o, (1.0 - np.sqrt(1.0 - o)) if revised else o, smax / 1.6


def classify(grad2d, count, ls, logits, *, grow_grad2d, grow_scale3d, prune_opa, prune_scale3d, grow=True, prune_big=False, revised=False):
    """-> dict(fates uint8 [U] = fate | PRUNED, counts int32 [3,U], offsets int32 [3,U], totals int64 [3])"""
    avg, smax, o, o_child, s_child = quantities(grad2d, count, ls, logits, revised)
    high = (avg > grow_grad2d) & bool(grow)
    small = smax <= grow_scale3d
    fate = np.where(high & small, CLONE, np.where(high & ~small, SPLIT, KEEP))
    op = np.where(fate == SPLIT, o_child, o)
    sc = np.where(fate == SPLIT, s_child, smax)
    pruned = (op < prune_opa) | (bool(prune_big) & (sc > prune_scale3d))
    counts = np.stack([(fate != SPLIT) & ~pruned, (fate == CLONE) & ~pruned, (fate == SPLIT) & ~pruned]).astype(np.int32)
    offsets = (np.cumsum(counts, 1) - counts).astype(np.int32)
    return dict(fates=(fate | np.where(pruned, PRUNED, 0)).astype(np.uint8), counts=counts, offsets=offsets, totals=counts.sum(1).astype(np.int64))


def margin(grad2d, count, ls, logits, *, grow_grad2d, grow_scale3d, prune_opa, prune_scale3d, revised=False, **_):
    """the smallest relative distance of any compared quantity from its threshold (children's values included)"""
    avg, smax, o, o_child, s_child = quantities(grad2d, count, ls, logits, revised)
    rel = lambda x, t: float(np.min(np.abs(x - t) / t)) if len(x) else 1.0
    return min(rel(avg, grow_grad2d), rel(smax, grow_scale3d), rel(o, prune_opa), rel(o_child, prune_opa), rel(smax, prune_scale3d),
               rel(s_child, prune_scale3d))


def quat_R(q, dt=np.float64):
    """csrc/splat_quat.h on raw quaternions (i, j, k, r) [..., 4], in `dt` -> [..., 3, 3]"""
    q = np.asarray(q, dtype=dt)
    n2 = ((q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) + q[..., 2] * q[..., 2]) + q[..., 3] * q[..., 3]
    q = q * (dt(1) / (np.sqrt(n2) + dt(np.float32(1e-8))))[..., None]
    i, j, k, r = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    two_s = dt(2) / (i * i + j * j + k * k + r * r)
    rows = [[1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r)],
            [two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r)],
            [two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)]]
    return np.stack([np.stack(r_, -1) for r_ in rows], -2).astype(dt)


def child_draws(seed, g, t, child):
    """the three standard normals of child `child` (0 or 1) of parent g at `t` steps done"""
    s = STREAMS["split0" if child == 0 else "split1"]
    z0, z1 = MO.normals(MO.draw(seed, g, s, t))
    z2, _ = MO.normals(MO.draw(seed, g, s + 1, t))
    return np.array([z0, z1, z2])


def child_values(p, S, seed, t, child, revised, dt=np.float64):
    """(means [n,3], log-scales [n,3], logits [n]) of child `child` of the parents S (an index array), in `dt` (float64: unrounded);
    the draws are child_draws', vectorised"""
    S = np.asarray(S, dtype=np.int64)
    s = STREAMS["split0" if child == 0 else "split1"]
    z0, z1 = MO.normals_np(MO.draw_np(seed, S, s, t))
    z2, _ = MO.normals_np(MO.draw_np(seed, S, s + 1, t))
    ls, mu = p["scales"][S].astype(dt), p["means"][S].astype(dt)
    sz = np.exp(ls) * np.stack([z0, z1, z2], -1).astype(dt)
    R = quat_R(p["quats"][S], dt)
    off = (R[..., 0] * sz[:, None, 0] + R[..., 1] * sz[:, None, 1]) + R[..., 2] * sz[:, None, 2]
    logit = p["opacities"][S].astype(dt)
    if revised:
        o2 = dt(1) - np.sqrt(dt(1) - dt(1) / (dt(1) + np.exp(-logit)))
        logit = np.log(o2 / (dt(1) - o2))
    return mu + off, ls - dt(math.log(1.6)), logit


def apply(cls, p, m, v, seed, t, revised=False, dt=np.float64):
    """-> (params, m, v, computed): params as float64 arrays (the children's means, log-scales and logits evaluated in `dt`, unrounded
    for float64; every copied value exactly its float32 source), the moments float32, and `computed` bool [U_out]: the split
    children's rows.  Row order A, B, C, D."""
    fates = cls["fates"]
    fate, alive = fates & 3, (fates & PRUNED) == 0
    A = np.nonzero(alive & (fate != SPLIT))[0].tolist()
    B = np.nonzero(alive & (fate == CLONE))[0].tolist()
    S = np.nonzero(alive & (fate == SPLIT))[0].tolist()
    parents = np.array(A + B + S + S, dtype=np.int64)
    n = len(parents)
    P = {k: p[k][parents].astype(np.float64) for k in NAMES}
    M = {k: m[k][parents].copy() for k in NAMES}
    V = {k: v[k][parents].copy() for k in NAMES}
    for d in (M, V):
        for k in NAMES:
            d[k][len(A):] = 0.0
    computed = np.zeros(n, dtype=bool)
    for child in (0, 1):
        r0 = len(A) + len(B) + child * len(S)
        P["means"][r0:r0 + len(S)], P["scales"][r0:r0 + len(S)], P["opacities"][r0:r0 + len(S)] = child_values(p, S, seed, t, child, revised, dt)
        computed[r0:r0 + len(S)] = True
    return P, M, V, computed


def reset_opacity(logits, max_opacity, dt=np.float64):
    cap = dt(math.log(max_opacity / (1.0 - max_opacity))) if dt == np.float64 else np.log(dt(max_opacity) / (dt(1) - dt(max_opacity)))
    return np.minimum(logits.astype(dt), cap)


# gsplat's schedule, spelled out (DefaultStrategy.step_post_backward): what the trainer's three helpers must equal
def schedule(i, start, stop, every, reset, pause):
    """-> (active, refines, resets) after the optimiser step of 0-based step i"""
    if i >= stop:
        return False, False, False
    refines = i > start and i % every == 0 and i % reset >= pause
    resets = i % reset == 0 and i > 0                          # `i > 0` is this package's deviation
    return True, refines, resets
