"""The cost expansion of rsr_physics_cost_expand (include/rsr_physics.h) in numpy: once in float64 and once in float32 with the
header's summation order (every output element one chain: its state or ctrl part, then the sensor entries j ascending, three
roundings per matrix term, two per vector term, no fma), plus a seeded input generator and the cost the expansion is of.
tests/test_cost_expand_ref.py checks the float64 expansion against central differences of that cost on the CPU;
tests/test_cost_expand_gpu.py holds the kernel to both."""
import numpy as np

OUTPUTS = ("lx", "lu", "lxx", "luu", "lux")
TERMS = ("w_qpos", "w_qvel", "w_ctrl", "w_sensor")


def inputs(M, T, nv, nu, ny, seed, stride=None, fill=np.nan):
    """Seeded float32 inputs of one call, read-only: the cost rows (weights in [0, 2], about one in five exactly 0; references of
    order 0.1), the residual sources dx, ctrl, sensordata (residuals of order 0.1) and columns [M, T, nx + nu, stride] (stride
    >= nx + ny, default tight) with entries of order 1 in the sensor slice and `fill` (NaN) everywhere else."""
    rng = np.random.default_rng(seed)
    nx, ncol = 2 * nv, 2 * nv + nu
    stride = nx + ny if stride is None else stride
    assert stride >= nx + ny
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)

    def weight(w):
        x = rng.uniform(0.0, 2.0, size=(M, T, w))
        x[rng.uniform(size=x.shape) < 0.2] = 0.0
        return f(x)
    inp = dict(w_qpos=weight(nv), w_qvel=weight(nv), w_ctrl=weight(nu), w_sensor=weight(ny),
               ctrl_ref=f(rng.normal(scale=0.1, size=(M, T, nu))), sensor_ref=f(rng.normal(scale=0.1, size=(M, T, ny))),
               dx=f(rng.normal(scale=0.1, size=(M, T, nx))))
    inp["ctrl"] = f(inp["ctrl_ref"] + rng.normal(scale=0.1, size=(M, T, nu)))
    inp["sensordata"] = f(inp["sensor_ref"] + rng.normal(scale=0.1, size=(M, T, ny)))
    col = np.full((M, T, ncol, stride), fill, np.float32)
    col[..., nx:nx + ny] = rng.normal(size=(M, T, ncol, ny))
    inp["columns"] = col
    for a in inp.values():
        a.flags.writeable = False
    return inp


def repack(inp, stride, fill=np.nan, below=None):
    """inp with columns at another row stride (`fill` in the padding) and, with `below`, that value in the entries below nx"""
    col = inp["columns"]
    M, T, ncol, _ = col.shape
    ny = inp["w_sensor"].shape[2]
    nx = inp["dx"].shape[2]
    new = np.full((M, T, ncol, stride), fill, np.float32)
    new[..., :nx] = col[..., :nx] if below is None else below
    new[..., nx:nx + ny] = col[..., nx:nx + ny]
    return dict(inp, columns=new)


def expand(inp, dtype, terms=TERMS, refs=("ctrl_ref", "sensor_ref")):
    """The five outputs in arithmetic `dtype` (float64: the reference; float32: the header's order, operation for operation).
    terms: the weights that are given (the others are off); refs: the references that are given (the others are zeros)."""
    dt = np.dtype(dtype).type
    g = lambda k: inp[k].astype(dt)
    M, T, nv = inp["w_qpos"].shape
    nu, ny = inp["w_ctrl"].shape[2], inp["w_sensor"].shape[2]
    nx = 2 * nv
    lx, lu = np.zeros((M, T + 1, nx), dt), np.zeros((M, T, nu), dt)
    lxx, luu, lux = np.zeros((M, T + 1, nx, nx), dt), np.zeros((M, T, nu, nu), dt), np.zeros((M, T, nu, nx), dt)
    dx = g("dx")
    for name, sl in (("w_qpos", slice(0, nv)), ("w_qvel", slice(nv, nx))):
        if name in terms:
            w = g(name)
            lx[:, 1:, sl] = w * dx[..., sl]
            i = np.arange(sl.start, sl.stop)
            lxx[:, 1:, i, i] = w
    if "w_ctrl" in terms:
        w = g("w_ctrl")
        du = g("ctrl") - (g("ctrl_ref") if "ctrl_ref" in refs else dt(0))
        lu[:] = w * du
        i = np.arange(nu)
        luu[:, :, i, i] = w
    if "w_sensor" in terms:
        w = g("w_sensor")
        ds = g("sensordata") - (g("sensor_ref") if "sensor_ref" in refs else dt(0))
        gs = w * ds                                                 # [M, T, ny]
        cd = g("columns")[..., nx:nx + ny]                          # [M, T, ncol, ny]: rows a of C | D
        for j in range(ny):                                          # the chains, j ascending
            c = cd[..., j]                                           # [M, T, ncol]
            v = c * gs[..., j, None]
            lx[:, :T] = lx[:, :T] + v[..., :nx]
            lu[:] = lu + v[..., nx:]
            wj = w[..., j, None, None]
            lxx[:, :T] = lxx[:, :T] + (c[..., :nx, None] * c[..., None, :nx]) * wj
            lux[:] = lux + (c[..., nx:, None] * c[..., None, :nx]) * wj
            luu[:] = luu + (c[..., nx:, None] * c[..., None, nx:]) * wj
    return dict(lx=lx, lu=lu, lxx=lxx, luu=luu, lux=lux)


def cost(inp, s, x, u, terms=TERMS, refs=("ctrl_ref", "sensor_ref")):
    """The cost of slot s in float64 at deviations x [T+1, nx] of the states (x[t]: the state before control step t, x[T] the last)
    and u [T, nu] of the controls from the nominal run, under the linear sensor model ds + C dx + D du:
    sum over t of 1/2 (w_qpos (dq + x_{t+1})^2 + w_qvel (dv + ..)^2 + w_ctrl (du + u_t)^2 + w_sensor (ds + C_t x_t + D_t u_t)^2)."""
    g = lambda k: inp[k][s].astype(np.float64)
    T, nv = inp["w_qpos"].shape[1:]
    ny = inp["w_sensor"].shape[2]
    nx = 2 * nv
    total = 0.0
    r = g("dx") + x[1:]
    if "w_qpos" in terms:
        total += 0.5 * (g("w_qpos") * r[:, :nv] ** 2).sum()
    if "w_qvel" in terms:
        total += 0.5 * (g("w_qvel") * r[:, nv:] ** 2).sum()
    if "w_ctrl" in terms:
        du = g("ctrl") - (g("ctrl_ref") if "ctrl_ref" in refs else 0.0) + u
        total += 0.5 * (g("w_ctrl") * du ** 2).sum()
    if "w_sensor" in terms:
        cd = g("columns")[..., nx:nx + ny]                          # [T, ncol, ny]
        ds = g("sensordata") - (g("sensor_ref") if "sensor_ref" in refs else 0.0)
        ds = ds + np.einsum("taj,ta->tj", cd[:, :nx], x[:T]) + np.einsum("tpj,tp->tj", cd[:, nx:], u)
        total += 0.5 * (g("w_sensor") * ds ** 2).sum()
    return total
