"""Running one plan of batch N on all N basis vectors of a kind and comparing the result with tests/stage_model.py: shared by
tests/test_gpu_basis_sweep.py and tools/basis_accuracy.py (test infrastructure, importable like elementwise_bound.py).

Transform p of the batch holds basis vector p: an impulse A delta_p in one plane, or the tone h16(exp(+2 pi i p t / N))."""
import functools

import numpy as np

import stage_model as sm

A = 1024.0                          # impulse amplitude: A / N = 4 .. 1/4, every single-pass length keeps its outputs normal
KERNEL = {256: "fft256_kernel", 512: "fft256r_kernel", 1024: "fft256r_kernel", 2048: "fft256r_kernel", 4096: "fft4096_kernel"}
PLANES = ("re", "im")
# profiles/basis_ulps.txt (tools/basis_accuracy.py): components that differ from the model, of 2 N^2; every direction and plane gives
# the same count. The cap of the tests is 4 x that share (room for a later, legitimate change of an fp32 summation order) and never
# more than 1 %; beyond 0.25 % measured the MODEL would lack a rounding.
DIFFERING = {256: 0, 512: 16, 1024: 128, 2048: 856, 4096: 8}
SHARE_CAP = {n: min(4.0 * c / (2.0 * n * n), 0.01) for n, c in DIFFERING.items()}


def unit(n):
    """u = ulp16(A / N), the unit of every impulse figure"""
    return float(sm.ulp16(A / n))


def impulse_planes(n, plane):
    """(re, im) binary16 [N][N]: transform p = A delta_p in the named plane"""
    hot = (np.eye(n) * A).astype(np.float16)
    zero = np.zeros_like(hot)
    return (hot, zero) if plane == "re" else (zero, hot)


@functools.lru_cache(maxsize=4)
def _forward_model(n, plane, mode):
    return sm.impulse_sweep(n, A if plane == "re" else 1j * A, mode)


def impulse_model(n, plane, inverse=False, mode="sequential"):
    """the model's answer to impulse_planes(n, plane) as binary16 (re, im) [p][k]; the forward sweeps are computed once and
    shared (the inverse is the forward model of the other plane with the output planes exchanged)"""
    if inverse:
        re, im = _forward_model(n, "im" if plane == "re" else "re", mode)
        return im, re
    return _forward_model(n, plane, mode)


def tone_planes(n):
    """(re, im) binary16 [N][N]: transform f = exp(+2 pi i f t / N) rounded to binary16, whose line is bin f"""
    t = np.arange(n)
    ang = 2.0 * np.pi * ((t[:, None] * t[None, :]) % n) / n
    return np.cos(ang).astype(np.float16), np.sin(ang).astype(np.float16)


def run(tf, torch, n, re, im, inverse=False, scale="sequential"):
    """one execution of the plan of length n and batch len(re) on binary16 planes [batch][n]; asserts that the plan is the
    single kernel meant; returns the binary16 (re, im) [batch][n]"""
    batch = re.shape[0]
    plan = tf.TfftPlan(n, batch, 0, scale=scale)
    assert plan.kernel_name == KERNEL[n] and plan.num_launches == 1, (n, plan.kernel_name, plan.num_launches)
    dev = torch.from_numpy(np.ascontiguousarray(np.stack([re, im], axis=1))).cuda().reshape(-1)
    out = torch.full_like(dev, float("nan"))
    (plan.exec_inverse if inverse else plan.exec)(dev, dev[n:], out, out[n:])
    torch.cuda.synchronize()
    o = out.cpu().numpy().reshape(batch, 2, n)
    plan.close()
    return o[:, 0], o[:, 1]


def compare(got, model, n):
    """got, model: (re, im) binary16 [p][k]. Returns the figures of the impulse check: share = the fraction of the 2 N^2 components
    that differ from the model at all (count of them), worst = the largest |got - model| in u, at = (p, k, plane) of it."""
    u = np.float32(unit(n))
    differ, worst, at = 0, 0.0, None
    for name, g, m in zip(PLANES, got, model):
        d = np.abs(g.astype(np.float32) - m.astype(np.float32))          # exact: both are binary16
        d[~np.isfinite(d)] = np.inf
        differ += int(np.count_nonzero(d))
        i = int(np.argmax(d))
        if float(d.flat[i]) / float(u) > worst:
            worst, at = float(d.flat[i]) / float(u), (i // n, i % n, name)
    return {"count": differ, "share": differ / (2.0 * n * n), "worst": worst, "at": at}


def differing(got, model, n, limit=12, names=PLANES):
    """the first (p, k, plane, got, model) that differ, and the digits that name the table entries: what a failure prints"""
    rows = []
    for name, g, m in zip(names, got, model):
        for p, k in np.argwhere(g.astype(np.float32) != m.astype(np.float32))[:limit]:
            rows.append(f"p = {p} {digits(n, int(p), 'n')}, k = {k} {digits(n, int(k), 'k')}, {name}: got {float(g[p, k])!r}, model {float(m[p, k])!r}")
    return rows


def digits(n, v, letter):
    """the digit indices of an input (letter n) or output (letter k) position, as the kernels' headers name them"""
    if n == 4096:
        return f"({letter}0 {v % 16}, {letter}1 {v // 16 % 16}, {letter}2 {v // 256})"
    if n == 256:
        return f"({letter}0 {v % 16}, {letter}1 {v // 16})"
    r = n // 256
    if letter == "n":
        return f"(r {v % r}, n0 {v // r % 16}, n1 {v // r // 16})"
    return f"(k0 {v % 16}, k1 {v // 16 % 16}, s {v // 256})"


def error_in_u(got, exact, n):
    """the worst component error against the exact (re, im) float64 [p][k], in u"""
    return max(float(np.abs(g.astype(np.float64) - e).max()) for g, e in zip(got, exact)) / unit(n)


def check_impulses(tf, torch, n, plane, inverse, share_cap):
    """The impulse check of tests/test_gpu_basis_sweep.py: one execution on x = A delta_p, every p, in the named plane. Every
    output component within 2 u of the model (derived in tests/test_stage_model_host.py), at most share_cap of them different
    from it at all, and exactly zero wherever both the exact answer's component and the model's are zero (for p = 0: a whole
    plane). Returns compare()'s figures."""
    got = run(tf, torch, n, *impulse_planes(n, plane), inverse=inverse)
    model = impulse_model(n, plane, inverse)
    c = compare(got, model, n)
    print(f"N = {n} {'inverse' if inverse else 'forward'} {plane}: {c['count']} of {2 * n * n} components differ from the model "
          f"(share {c['share']:.3e}), worst {c['worst']:.3f} u at {c['at']}")
    where = "\n".join(differing(got, model, n)) if c["count"] else ""
    assert c["worst"] <= 2.0, f"{c}\n{where}"
    assert c["share"] <= share_cap, f"{c} > {share_cap}\n{where}"
    exact = sm.impulse_exact(n, A if plane == "re" else 1j * A, inverse)
    for name, g, m, e in zip(PLANES, got, model, exact):
        must = (e == 0) & (m == 0)
        if name != plane:
            assert must[0].all(), "the model leaves the other plane of p = 0 empty"
        assert not g[must].any(), f"{name}: {int(np.count_nonzero(g[must]))} components that must be zero are not"
    return c
