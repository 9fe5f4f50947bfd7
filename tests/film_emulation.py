"""filmgen_bwd_kernel of csrc/film.hip restated on the CPU in float32 with the kernel's own summation order: every dot product a
k = 0, 1, 2, ... chain of fused multiply-adds, the LayerNorm statistics and the two means of its backward accumulated by one
thread in index order, d relu summed over the outputs in output order. A float32 fma is the float64 product and sum rounded once
more to float32 (the product of two float32 is exact in float64).

tests/test_gpu_film_ops.py uses it for one purpose: a gradient tensor of the kernel that is further from float64 than four times
torch's float32 CPU run is must be that far because of this order, i.e. the emulation is as far, and the kernel agrees with it."""
import numpy as np

f32 = np.float32


def fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def _hidden(p, z, z_dim, hid):
    h = np.zeros(hid, f32)
    for k in range(z_dim):
        h = fma(p["w1"][:, k], z[k], h)
    h = (h + p["b1"]).astype(f32)
    m = f32(0)
    for k in range(hid):
        m = f32(m + h[k])
    m = f32(m / f32(hid))
    v = f32(0)
    for k in range(hid):
        d = f32(h[k] - m)
        v = fma(d, d, v)[()]
    v = f32(v / f32(hid))
    rstd = f32(f32(1) / np.sqrt(f32(v + f32(1e-5))))
    xhat = ((h - m).astype(f32) * rstd).astype(f32)
    return xhat, np.maximum(fma(xhat, p["ln_w"], p["ln_b"]), f32(0)), rstd


def backward(inputs, layout, z, c):
    """inputs = (parameters per generator, Dg, Db) as torch fp32 tensors, layout = [(out, kind, dst)], c = dl2 or None ->
    [{tensor: gradient}] per generator, in the kernel's arithmetic."""
    gens, Dg, Db = inputs
    Dg, Db, z = Dg.numpy(), Db.numpy(), z.numpy()
    l2g = f32(0) if c is None else f32(f32(2) * f32(c))
    grads = []
    for p, (out, kind, dst) in zip(gens, layout):
        p = {k: v.numpy() for k, v in p.items()}
        hid, z_dim = p["w1"].shape
        xhat, hr, rstd = _hidden(p, z, z_dim, hid)
        s = np.zeros(out, f32)
        for k in range(hid):
            s = fma(p["w2"][:, k], hr[k], s)
        s = (s + p["b2"]).astype(f32)
        dout = (Dg[dst:dst + out] * p["init"]).astype(f32) if kind == 0 else Db[dst:dst + out]
        dso = (dout * p["reg"]).astype(f32)
        g = {"reg": fma(l2g, p["reg"], (dout * s).astype(f32)), "b2": dso, "w2": (dso[:, None] * hr[None, :]).astype(f32)}
        dhr = np.zeros(hid, f32)
        for o in range(out):
            dhr = fma(dso[o], p["w2"][o], dhr)
        dn = np.where(hr > 0, dhr, f32(0)).astype(f32)
        g["ln_w"], g["ln_b"] = (dn * xhat).astype(f32), dn
        dxh = (dn * p["ln_w"]).astype(f32)
        m1, m2 = f32(0), f32(0)
        for k in range(hid):
            m1 = f32(m1 + dxh[k])
            m2 = fma(dxh[k], xhat[k], m2)[()]
        m1, m2 = f32(m1 / f32(hid)), f32(m2 / f32(hid))
        dh = (rstd * fma(-xhat, m2, (dxh - m1).astype(f32))).astype(f32)
        g["b1"], g["w1"] = dh, (dh[:, None] * z[None, :]).astype(f32)
        grads.append(g)
    return grads
