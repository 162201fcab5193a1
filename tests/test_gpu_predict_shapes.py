"""sgp_predict, sgp_predict_var and sgp_out_message on the device at the shapes their first tests leave out
(tests/predict_shapes_ref.CASES), against the float64 reference of that file at its bounds: per-point means at 50 eps |k|'|mu|,
the diagonal of C at 50 eps (cond(K_uu) sigma2 + cond(Sigma_v) form) with cond(K_uu + jitter I) <= 1e6, and the comparisons that
carry no cond(K_uu) term at all -- off-diagonal entries, diagonal differences C_ii - C_00, and C_noise - C against W^-1 of a
non-diagonal W.  tests/test_predict_shapes_host.py holds the bounds against mpmath and shows that they see a dropped tile row, an
unmasked triangle, a block or mu read at the padded stride, a node's lost 65th point and a diagonal W^-1.

Which case runs which kernel instantiation (k_predict<DT, FAM> as launch_predict selects it; k_predvar_multi<DO> for d_out >= 2,
k_predvar_finish for d_out = 1):
    dout43x2/3/4, dout65x2/3/4   k_predvar_multi<2>, <3>, <4> at M = 43 (one ragged tile) and 65 (a second tile of one row); k_predict<3, SE>
    ragged{1,63,64,129}x{1,3,4}  k_predvar_finish and k_predvar_multi<3>, <4> with block rows of L_S starting at i M off the tile grid
                                 (M = 64: on it), ns = 1, 64, 65 (one point, one full workgroup of 64, one point into the second)
    {se,matern12,matern32,matern52}x{1,2,3,4}
                                 k_predict<0, SE>, <0, MATERN12>, <0, MATERN32>, <0, MATERN52> (D = 9) with every output count, ten
                                 points on or 1e-9 off inducing inputs; k_predvar_multi<2>, <3>, <4> with every Matern family
    dim1, dim2, dim4, dim8       k_predict<1, SE>, <2, SE>, <4, SE>, <8, SE>, ARD and isotropic (n_ell = 1), ns = 257
    dim5, dim32                  k_predict<0, SE> at D = 5 and at MAXD = 32
    blocks_{se,matern12}x{1,4}   k_predict<2, SE>, <0, MATERN12> at ns = 255, 256, 257, 513: its 256-thread blocks' edges
    nodes_se, nodes_matern12     k_out_message_finish at nodes of 1, 64, 65, 129, 200 and 3 points (six nodes: the second workgroup
                                 holds two), weights with zeros and negatives; k_predict<0, SE>, <0, MATERN12> at D = 7
    many                         k_out_message_finish over 1001 nodes: 251 workgroups, the last with one node
    limit                        d_out M = 4032: k_predvar_multi<4> over 63 tile columns of L_S
    ill_*                        jitter 1e-8: the ill-conditioned route at the old bound
    ragged63x3 after a sweep     the handle's own q(v): k_pad_square with Q = 189, Q_p = 192

Every comparison prints its worst error / bound ratio before it asserts; every covariance block is exactly symmetric, the mean
of sgp_predict_var is bitwise sgp_predict's, and calls of more than 64 points are repeated in chunks of 64 (SGP_PREDICT_CHUNK)
with bitwise the same results."""
import numpy as np
import pytest

from tests import predict_shapes_ref as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import gaussianprocessnode_amd as g
    return g


def device_for(G, c, n_max=64, **kw):
    dev = G.SGPDevice(n_max, c["M"], c["D"], c["d_out"], **kw)
    dev.set_inducing(c["Xu"])
    dev.set_kernel(c["sigma2"], c["ell_dev"], c["jitter"], family=c["family"])
    dev.set_noise(c["W"])
    return dev


def forward(dev, c, ns, qv=True):
    """(predict, predict_var's C, predict_var(noise=True)'s C) of the case's first ns points; the three means agree bitwise."""
    X = c["X"][:ns]
    q = (c["mu_v"], c["Sigma_v"]) if qv else ()
    pm = dev.predict(X, *q[:1])
    mv, C = dev.predict_var(X, *q)
    mn, Cn = dev.predict_var(X, *q, noise=True)
    assert np.array_equal(pm, mv) and np.array_equal(mv, mn)
    d = c["d_out"]
    return pm.reshape(-1, d), C.reshape(-1, d, d), Cn.reshape(-1, d, d)


def check(label, c, ns, out):
    pm, C, Cn = out
    rows = slice(0, ns)
    r = dict(mean=P.mean_ratio(c, pm, rows), **P.var_ratios(c, C, Cn, rows))
    print(f"case {label}: error / bound " + " ".join(f"{k} {v:.3g}" for k, v in r.items()))
    assert pm.shape == (ns, c["d_out"]) and C.shape == Cn.shape == (ns, c["d_out"], c["d_out"])
    assert all(np.isfinite(x).all() for x in out)
    for k, v in r.items():
        assert v <= 1.0, (label, k, v)
    assert np.array_equal(C, C.transpose(0, 2, 1)) and np.array_equal(Cn, Cn.transpose(0, 2, 1))


def run_case(G, monkeypatch, name, ns_list=None):
    """The case at each ns of ns_list (all its points by default) against the reference; shorter calls are bitwise the prefix of
    longer ones; with more than 64 points, once more in chunks of 64, bitwise."""
    c = P.reference(name)
    ns_list = sorted(ns_list or [len(c["X"])])
    out = {}
    for chunk in (None, "64"):
        if chunk:
            if ns_list[-1] <= 64:
                break
            monkeypatch.setenv("SGP_PREDICT_CHUNK", chunk)
        with device_for(G, c) as dev:
            out[chunk] = [forward(dev, c, ns) for ns in ns_list]
    for ns, res in zip(ns_list, out[None]):
        check(f"{name}/ns {ns}", c, ns, res)
        for a, b in zip(res, out[None][-1]):
            assert np.array_equal(a, b[:ns]), (name, ns)
    for res, chunked in zip(out[None], out.get("64", [])):
        for a, b in zip(res, chunked):
            assert np.array_equal(a, b), name
    return c, out[None][-1]


@pytest.mark.parametrize("name", P.group("dout"))
def test_output_counts(G, monkeypatch, name):
    run_case(G, monkeypatch, name)


@pytest.mark.parametrize("name", P.group("ragged"))
def test_ragged_m_and_q(G, monkeypatch, name):
    run_case(G, monkeypatch, name, P.RAGGED_NS)


@pytest.mark.parametrize("name", P.group("family"))
def test_families_and_outputs(G, monkeypatch, name):
    c, (pm, C, Cn) = run_case(G, monkeypatch, name)
    assert np.array_equal(c["X"][:5], c["Xu"][:5])                          # (the coincident points are among those compared)


@pytest.mark.parametrize("name", P.group("dims"))
def test_dimensions(G, monkeypatch, name):
    run_case(G, monkeypatch, name)


@pytest.mark.parametrize("name", P.group("blocks"))
def test_block_edges(G, monkeypatch, name):
    run_case(G, monkeypatch, name, P.BLOCK_NS)


@pytest.mark.parametrize("name", P.group("ill"))
def test_ill_conditioned_route_at_the_old_bound(G, monkeypatch, name):
    c, _ = run_case(G, monkeypatch, name)
    print(f"case {name}: cond(K_uu + 1e-8 I) {c['cond_kuu']:.3g}")


def test_size_limit(G, monkeypatch):
    c, _ = run_case(G, monkeypatch, "limit")
    print(f"case limit: cond(K_uu + 1e-6 I) {c['cond_kuu']:.3g} cond(Sigma_v) {c['cond_sigma']:.3g}")


def out_calls(dev, c):
    X, st, w, mu = c["X"], c["start"], c["wts"], c["mu_v"]
    mean, point = dev.out_message(X, st, w, mu, want_points=True)
    ones = dev.out_message(X, st, np.ones(len(X)), mu)
    unweighted = dev.out_message(X, st, None, mu)
    predicted = np.asarray(dev.predict(X, mu)).reshape(len(X), c["d_out"])
    assert np.array_equal(ones, unweighted)                               # weights = None is an all-ones call
    assert np.array_equal(point, predicted)                               # bitwise sgp_predict's values
    return mean, point, unweighted


@pytest.mark.parametrize("name", P.group("nodes") + P.group("many"))
def test_out_message_nodes(G, monkeypatch, name):
    c, (pm, _, _) = run_case(G, monkeypatch, name)
    out = {}
    for chunk in (None, "64"):
        if chunk:
            monkeypatch.setenv("SGP_PREDICT_CHUNK", chunk)
        with device_for(G, c) as dev:
            out[chunk] = out_calls(dev, c)
    mean, point, unweighted = out[None]
    ones = dict(c, wts=np.ones(len(c["X"])))
    ones.update(P.bounds(ones, c, c["cond_kuu"], c["cond_sigma"]), node_mean=P.evaluate(ones)["node_mean"])
    r = dict(node=P.node_ratio(c, mean), node_unweighted=P.node_ratio(ones, unweighted), point=P.mean_ratio(c, point))
    print(f"case {name}: out_message error / bound " + " ".join(f"{k} {v:.3g}" for k, v in r.items()))
    assert mean.shape == (c["nodes"], c["d_out"]) and np.isfinite(mean).all() and np.isfinite(point).all()
    for k, v in r.items():
        assert v <= 1.0, (name, k, v)
    assert np.array_equal(point, pm)
    for a, b in zip(out[None], out["64"]):
        assert np.array_equal(a, b)


def test_null_posterior_after_a_sweep(G):
    """ragged63x3's model after a real sweep (N = 300): with mu_v = Sigma_v = None the three calls are bitwise those given
    dev.posterior() explicitly -- the padded copy of the handle's Sigma_v at Q = 189, Q_p = 192 against the uploaded one."""
    c = dict(P.reference("ragged63x3"))
    rng = np.random.default_rng(1900)
    N, d = 300, c["d_out"]
    Xd = rng.uniform(-1.745, 1.745, (N, c["D"]))
    yd = np.stack([np.sin(Xd.sum(axis=1) + o) for o in range(d)], axis=1) + 0.1 * rng.normal(size=(N, d))
    with device_for(G, c, n_max=N) as dev:
        dev.set_data(Xd, yd)
        dev.set_prior_isotropic(50.0)
        dev.sweep()
        kind = dev.sweep_kind()
        mu, Sig, _ = dev.posterior(want_uv=False)
        c.update(mu_v=mu, Sigma_v=Sig)
        for ns in P.RAGGED_NS:
            null, explicit = forward(dev, c, ns, qv=False), forward(dev, c, ns)
            for a, b in zip(null, explicit):
                assert np.isfinite(a).all() and np.array_equal(a, b), ns
            assert np.array_equal(null[1], null[1].transpose(0, 2, 1))
        assert dev.sweep_kind() == kind
