"""LAMB in float64 (numpy): the restatement of include/plbert.h's definition that the LAMB tests compare the kernels with. It
takes what the kernels take — the fp32 buffers and the host-rounded fp32 scalars of every tensor (plb_lamb_plan's fields) —
and carries every operation out in double. Two forms written independently of each other: `lamb_ref` (vectorised per tensor)
and `lamb_ref_loop` (one Python expression per element); tests/test_lamb_host.py holds one against the other."""
import math

import numpy as np

SCALARS = ("omb1", "b2", "omb2", "eps", "bc2_sqrt", "inv_bc1", "weight_decay", "lr")


def scalars(lr, betas, eps, weight_decay, step):
    """plb_lamb_plan's scalars of one group at one step count: formed in double, rounded to fp32 once."""
    b1, b2 = betas
    f = lambda x: float(np.float32(x))
    return dict(omb1=f(1.0 - b1), b2=f(b2), omb2=f(1.0 - b2), eps=f(eps), bc2_sqrt=f(math.sqrt(1.0 - b2 ** step)),
                inv_bc1=f(1.0 / (1.0 - b1 ** step)), weight_decay=f(weight_decay), lr=f(lr))


def tensor(begin, end, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, step=1, adapt=1, slot=0, group=0):
    """One live tensor [begin, end) of the flat buffers with its scalars."""
    return dict(begin=int(begin), end=int(end), tensor=int(slot), group=int(group), step=int(step), adapt=int(adapt),
                **scalars(lr, betas, eps, weight_decay, step))


def lamb_ref(p, g, m, v, tensors, grad_scale=1.0, coef=None):
    """One step over the tensors (dicts of `tensor`); everything outside them is a hole and comes back unchanged.
    grad_scale and coef are the fp32 values the kernel multiplies with. Returns dict(p, m, v, u: float64 arrays of the
    buffers' length; wn, un, trust: one float per tensor)."""
    p64, g64 = np.asarray(p, np.float64), np.asarray(g, np.float64)
    out = dict(p=p64.copy(), m=np.asarray(m, np.float64).copy(), v=np.asarray(v, np.float64).copy(), u=np.zeros_like(p64),
               wn=[], un=[], trust=[])
    gs = float(np.float32(grad_scale)) * (1.0 if coef is None else float(np.float32(coef)))
    for t in tensors:
        sl = slice(t["begin"], t["end"])
        gg = g64[sl] * gs
        mm = out["m"][sl] + t["omb1"] * (gg - out["m"][sl])
        vv = t["b2"] * out["v"][sl] + t["omb2"] * (gg * gg)
        r = mm / (np.sqrt(vv) / t["bc2_sqrt"] + t["eps"])
        u = r * t["inv_bc1"] + t["weight_decay"] * p64[sl]
        wn, un = float(np.sqrt(np.sum(p64[sl] ** 2))), float(np.sqrt(np.sum(u ** 2)))
        trust = wn / un if t["adapt"] and wn > 0 and un > 0 else 1.0
        out["m"][sl], out["v"][sl], out["u"][sl] = mm, vv, u
        out["p"][sl] = p64[sl] - (t["lr"] * trust) * u
        out["wn"].append(wn); out["un"].append(un); out["trust"].append(trust)
    return out


def lamb_ref_loop(p, g, m, v, tensors, grad_scale=1.0, coef=None):
    """`lamb_ref`, element by element in Python floats (doubles), the norms as math.fsum of the squares."""
    P, M, V = ([float(x) for x in a] for a in (p, m, v))
    U = [0.0] * len(P)
    res = dict(wn=[], un=[], trust=[])
    for t in tensors:
        sp, su = [], []
        for i in range(t["begin"], t["end"]):
            gi = float(g[i]) * float(np.float32(grad_scale))
            if coef is not None:
                gi = gi * float(np.float32(coef))
            M[i] = M[i] + t["omb1"] * (gi - M[i])
            V[i] = t["b2"] * V[i] + t["omb2"] * (gi * gi)
            r = M[i] / (math.sqrt(V[i]) / t["bc2_sqrt"] + t["eps"])
            U[i] = r * t["inv_bc1"] + t["weight_decay"] * P[i]
            sp.append(P[i] * P[i]); su.append(U[i] * U[i])
        wn, un = math.sqrt(math.fsum(sp)), math.sqrt(math.fsum(su))
        trust = 1.0
        if t["adapt"] and wn > 0.0 and un > 0.0:
            trust = wn / un
        for i in range(t["begin"], t["end"]):
            P[i] = P[i] - (t["lr"] * trust) * U[i]
        res["wn"].append(wn); res["un"].append(un); res["trust"].append(trust)
    return dict(p=np.array(P), m=np.array(M), v=np.array(V), u=np.array(U), **res)


# ---- the bounds the GPU tests use (derived in tests/test_gpu_lamb_kernel.py's docstring) -----------------------------------
TRUST_RTOL = 1e-5          # the tolerance LAMB's definition sets for trust; the summation structure gives about 30 x 2^-24, see there
EPS = 2.0 ** -24           # unit roundoff of fp32


def ulp(x):
    """Spacing of fp32 at |x| (the smallest normal spacing for 0)."""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def p_bound(p_ref, u_ref, lr, trust, trust_rtol=TRUST_RTOL):
    """|p_gpu - p_f64| <= ulp(p)/2 + lr * trust * |u| * (trust's bound + 4 * 2^-24), element by element."""
    return 0.5 * ulp(p_ref) + lr * trust * np.abs(u_ref) * (trust_rtol + 4 * EPS)
