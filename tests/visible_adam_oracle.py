"""numpy restatement of ops.adam_step_visible (gsplat's SelectiveAdam as include/vist3a_hip.h states it) and of ops.gs_visibility.
`dtype` float64 is the oracle; float32 is the same update carried in fp32 on the CPU, the comparison figure of the parity test."""
import numpy as np


def visibility(radii):
    """radii int [C,U] -> uint8 [U]: 1 where some camera's radius is positive"""
    return (np.asarray(radii) > 0).any(0).astype(np.uint8)


def adam_step_visible(p, g, m, v, visible, *, lr, betas=(0.9, 0.999), eps=1e-8, lr2=None, period=0, dtype=np.float64):
    """One update -> new (p, m, v) of `dtype`, shapes [U, ...].  Rows with visible == 0 are returned as they came, whatever their g
    holds.  No bias correction.  period > 0: flat element e of the whole tensor uses lr where e % period == 0 and lr2 elsewhere."""
    p, m, v = (np.array(t, dtype=dtype) for t in (p, m, v))
    g = np.asarray(g)
    rows = np.asarray(visible).astype(bool)
    b1, b2 = dtype(betas[0]), dtype(betas[1])
    one = dtype(1)
    rate = np.full(p.size, lr, dtype=dtype)
    if period > 0:
        rate[np.arange(p.size) % period != 0] = lr if lr2 is None else lr2
    rate = rate.reshape(p.shape)[rows]
    gr = g[rows].astype(dtype)
    mn = b1 * m[rows] + (one - b1) * gr
    vn = b2 * v[rows] + (one - b2) * gr * gr
    p[rows] = p[rows] - rate * mn / (np.sqrt(vn) + dtype(eps))
    m[rows] = mn
    v[rows] = vn
    return p, m, v
