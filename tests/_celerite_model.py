"""The p = 2, q = 2 model of the celerite kernels' end-to-end tests (tests/test_celerite_gpu.py): SHO and Rotation nodes,
CeleriteTerm and SquaredExponential weights, on N times over a span of 80 scaled to N (N = 45: the one-tile path, N = 130 and
150: the launch path).  tests/test_celerite.py confirms on the CPU that oracle.cpu_ref's two forms of a sweep (sweep_ref,
sweep_B) agree to 1e-9 on it, so that the B-form's own gap does not eat the project's 1e-8."""
import numpy as np

from gpyrn_amd import covfunc, meanfunc

P, Q = 2, 2
JITTERS = [0.3, 0.4]


def kernels():
    c = covfunc
    nodes = [c.SHO(1.0, 11.0, 3.0), c.Rotation(0.9, 9.0, 1.2, 0.3, 0.4)]
    # (CeleriteTerm is positive definite for a, c > 0 and |b d| < a c)
    weights = [c.CeleriteTerm(1.0, 0.1, 0.08, 0.3), c.SquaredExponential(1.1, 15.0),
               c.SquaredExponential(0.8, 12.0), c.CeleriteTerm(0.7, 0.05, 0.05, 0.2)]
    return nodes, weights


def means():
    return [meanfunc.Constant(0.1), meanfunc.Constant(0.0)]


def data(N):
    """(t, [y_1, e_1, y_2, e_2])"""
    rng = np.random.default_rng(500 + N)
    t = np.sort(rng.uniform(0.0, 80.0 * N / 200.0, N))
    args = []
    for i in range(P):
        args += [np.sin(t / (5.0 + i)) + 0.3 * rng.normal(size=N), rng.uniform(0.1, 0.3, N)]
    return t, args


def inference(N, **kw):
    import gpyrn_amd as gpyrn
    t, args = data(N)
    g = gpyrn.inference(Q, t, *args, **kw)
    nodes, weights = kernels()
    g.set_components(nodes, weights, means(), list(JITTERS))
    return g, t


def problem(N):
    """The model as tests/_bound_ref.py and oracle.cpu_ref take it: dict with time, nodes, weights, means, jitters, y_raw,
    yerr2 and args = (Kf, Kw, Lf, Lw, y - mean, y_raw, yerr2, jitt2); mu0, var0 the reference's starting state; the keys of
    tests/_mask_ref.problem beside them."""
    from oracle import cpu_ref
    t, args = data(N)
    nodes, weights = kernels()
    ms = means()
    y, e = np.array(args[0::2]), np.array(args[1::2])
    Kf, Kw, Lf, Lw, yres, jitt2 = cpu_ref.setup(t, nodes, weights, ms, JITTERS, y)
    mu0, var0 = cpu_ref.init_mu_var(y, [n.pars[0] for n in nodes], [w.pars[0] for w in weights], JITTERS)
    return dict(time=t, nodes=nodes, weights=weights, means=ms, jitters=list(JITTERS), y_raw=y, y_resid=yres, yerr2=e ** 2,
                jitt2=jitt2, Kf=Kf, Kw=Kw, args=(Kf, Kw, Lf, Lw, yres, y, e ** 2, jitt2), mu0=mu0, var0=var0)


def dk(kernel, t):
    """the NumPy closed forms, as tests/_bound_ref.gradient takes them"""
    r = t[:, None] - t[None, :]
    return [np.broadcast_to(np.asarray(d, dtype=float), r.shape) for d in kernel._dk_dpars(r)]
