"""Call sequences on the device: every state-changing call (tests/call_sequence_ref.MUTATORS: one entry per row of the "Entry point ->
effect" table of csrc/sgp_api.hip) in front of every reader, on three handles -- A with SGP_FLAG_REUSE_STATS, B without it and the
same calls, C created fresh and brought to the shadow model's normal form through the public setters and one sweep.  A and B agree
bitwise; A and C agree bitwise unless the history is "device-set" (theta or X_u came back from the device: the bounds of
tests/test_gpu_theta_descend.test_state_after_the_call and the parity suite's cond-scaled bounds).  A reader that hands out the
resident statistics as they are (stats, w_stats) behind a call that re-formed them is held against a handle swept at the values they
were re-formed at where setters reach those, and against B alone where they are the device's last EVALUATED theta's (the header
documents them as such).  A may answer where C refuses in two documented cases only (see `compare`).  Each cell prints one line
(CELL mutator reader problem outcome), from which profiles/call_sequences.txt was written."""
import numpy as np
import pytest

from tests import call_sequence_ref as CR
from tests.test_gpu_parity import kuu_tol, post_tol, relF
from tests.test_gpu_reuse_stats import snapshot

pytestmark = pytest.mark.gpu

CASES = [(m, p) for m, op in CR.MUTATORS.items() for p in op.problems]


@pytest.fixture(scope="module")
def G():
    import gaussianprocessnode_amd as g
    return g


def handle(G, P, reuse=False):
    return G.SGPDevice(P["N"], P["M"], P["D"], P["d_out"], keep_kuf=True, reuse_stats=reuse)


def call(G, op, dev, P):
    """(result, None) or (None, ("refused", status)): only the status of a refusal is compared"""
    try:
        return op.run(dev, P), None
    except G.SGPError as e:
        return None, ("refused", CR.ERR_ARG if "status -1" in str(e) else str(e))


def read(G, name, dev, P):
    if name == "sweep":
        try:
            dev.sweep()
        except G.SGPError as e:
            return None, ("refused", CR.ERR_ARG if "status -1" in str(e) else str(e))
        return snapshot(dev), None
    r, refused = call(G, CR.READERS[name], dev, P)
    return r, refused


def flat(name, r):
    return r if name == "sweep" else dict(enumerate(CR.READERS[name].out(r)))


def bitwise(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


def bounded(name, a, c):
    """worst error / bound of a device-set pair: values 1e-12 relative (to the array's largest entry), gradients rtol 1e-9 with
    atol 1e-9 max|grad|, sweep snapshots the parity suite's cond-scaled bounds"""
    worst = 0.0
    if name == "sweep":
        cond_K = np.linalg.cond(c["KuuL"]) ** 2
        cond_L = np.linalg.cond(np.linalg.inv(c["Sigma"]))
        for k in a:
            tol = kuu_tol(cond_K) if k == "KuuL" else post_tol(max(cond_L, cond_K))
            worst = max(worst, relF(a[k], c[k]) / tol)
        return worst
    for i in a:
        if i in CR.GRADIENTS.get(name, ()):
            tol = 1e-9 * np.abs(c[i]) + 1e-9 * np.abs(c[i]).max()
            worst = max(worst, float(np.max(np.abs(a[i] - c[i]) / np.maximum(tol, 1e-300))))
        else:
            worst = max(worst, float(np.max(np.abs(a[i] - c[i])) / max(1e-12 * np.max(np.abs(c[i])), 1e-300)))
    return worst


def compare(G, name, P, a, b, model, where, order_pair=False):
    """one reader on A, B and a fresh C; returns the cell's outcome and A's result"""
    ops = model.normal_form()
    ra, fa = read(G, name, a, P)
    rb, fb = read(G, name, b, P)
    assert fa == fb, f"{where}: A {fa} but B {fb}"
    if fa is None:
        assert bitwise(flat(name, ra), flat(name, rb)), f"{where}: A and B differ"
    with handle(G, P) as c:
        CR.build(c, ops)
        rc, fc = read(G, name, c, P)
    if model.kind is None and name != "sweep":
        return ("refused", None) if fa is not None else ("own-q(v)", ra)   # a training run's q(v) and theta are the run's: A against B only; only a sweep can be compared with C
    if name in CR.STATS_READERS and model.stats_stale:
        # the statistics were re-formed behind the sweep (the header: they are the last EVALUATED theta's; the descents also set
        # swept_local = false, so sgp_get_stats may refuse where C, at the host equivalent, answers).  Where setters reach the values
        # they were re-formed at, a handle swept THERE hands out the same statistics: bitwise (the re-evaluation enqueues the local
        # phase's own kernels).  w_stats mixes them with q(v) of the sweep, which no second handle has.
        if name == "stats" and fa is None and model.stats_at is not None:
            with handle(G, P) as c2:
                CR.build(c2, [("set", n, model.stats_at[n]) for n in CR.SETTERS if model.stats_at[n] is not None] + [("sweep",)])
                r2 = flat(name, CR.READERS[name].run(c2, P))
            assert bitwise(flat(name, ra), r2), f"{where}: the re-formed statistics are not those of a handle swept at their theta"
            return "stale=", ra
        return "documented-stale", ra
    if fa is not None:
        assert fc is not None and fc[1] == fa[1], f"{where}: A refuses ({fa}) but C answers"
        return "refused", None
    if fc is not None:
        # A answers where the fresh handle refuses: the staleness this file exists to catch, unless it is one of the two documented
        # differences of a device-moved X_u's host equivalent -- set_posterior carries no Sigma_v, and set_inducing drops the
        # statistics sgp_inducing_descend_psi leaves in place (stale, and handed out: the table says so)
        foreign = any(p[0] == "posterior" for p in model.post)
        if name == "stats" and "inducing" in model.dev and not model.stats_stale:
            return "C-refused", ra
        assert foreign and name in CR.EXPLICIT_QV, f"{where}: A answers but the fresh handle refuses ({fc})"
        mu, Sig, _ = a.posterior()                             # ... and then C is given A's q(v) explicitly
        with handle(G, P) as c:
            CR.build(c, ops)
            rc = CR.EXPLICIT_QV[name](c, P, mu, Sig)
        fa_, fc_ = flat(name, ra), flat(name, rc)
        ratio = 0.0 if bitwise(fa_, fc_) else bounded(name, fa_, fc_)
        assert model.device_set and ratio <= 1.0, f"{where}: worst error / bound {ratio:.3g} against C at A's q(v), given explicitly"
        return f"explicit-q(v) {ratio:.2g}", ra
    fa_, fc_ = flat(name, ra), flat(name, rc)
    if bitwise(fa_, fc_):
        return "bitwise", ra
    if order_pair:                                             # (CR.ORDER_PAIRS names the code that orders the sums differently)
        tol = post_tol(CR.kuu_cond(P, model.cur["kernel"], model.cur["family"]))
        ratio = max(float(np.max(np.abs(fa_[k] - fc_[k])) / (tol * np.max(np.abs(fc_[k])))) for k in fa_)
        assert ratio <= 1.0, f"{where}: worst error / parity bound {ratio:.3g}"
        return f"order-bound {ratio:.2g}", ra
    assert model.device_set, f"{where}: A and C differ without a device-set history: " + ", ".join(
        f"{k} {np.max(np.abs(fa_[k] - fc_[k])):.3e}" for k in fa_ if not np.array_equal(fa_[k], fc_[k]))
    ratio = bounded(name, fa_, fc_)
    assert ratio <= 1.0, f"{where}: worst error / bound {ratio:.3g}"
    return f"bound {ratio:.2g}", ra


def prepared(G, P, mname, stack):
    """A and B swept once, read, and through the mutator; the model of where they are"""
    a, b = stack.enter_context(handle(G, P, True)), stack.enter_context(handle(G, P))
    model = CR.start([a, b], P)
    mut = CR.MUTATORS[mname]
    ra, fa = call(G, mut, a, P)
    rb, fb = call(G, mut, b, P)
    assert fa == fb, (mname, fa, fb)
    if fa is None and mut.model:
        mut.model(model, P, ra, a)
    return a, b, model, fa


@pytest.mark.parametrize("mname,pname", CASES)
def test_next_sweep_kind_after(G, mname, pname):
    import contextlib
    P, mut = CR.problem(pname), CR.MUTATORS[mname]
    with contextlib.ExitStack() as stack:
        a, b, model, refused = prepared(G, P, mname, stack)
        assert refused is None, refused
        assert a.sweep_kind()[0] == mut.kind, (mname, a.sweep_kind(), mut.kind)
        assert b.sweep_kind() == (CR.FULL, CR.FULL if mut.last is None else mut.last)
        if mut.last is not None:                               # (a call that sweeps on its own documents its `last` for every handle)
            assert a.sweep_kind()[1] == mut.last, (mname, a.sweep_kind(), mut.last)
        if mut.restore:                                        # (the call leaves the handle without data)
            assert a.sweep_kind()[0] == CR.FULL
            mut.restore(a, P)
        a.sweep()
        assert a.sweep_kind()[1] == mut.kind, (mname, a.sweep_kind(), mut.kind)


@pytest.mark.parametrize("mname,pname", CASES)
def test_reader_after_mutator(G, mname, pname):
    import contextlib
    P = CR.problem(pname)
    for rname, reader in CR.READERS.items():
        if pname not in reader.problems:
            continue
        with contextlib.ExitStack() as stack:
            a, b, model, refused = prepared(G, P, mname, stack)
            assert refused is None, refused
            mut = CR.MUTATORS[mname]
            if mut.restore and rname == "sweep":                # (the call leaves the handle without data)
                mut.restore(a, P)
                mut.restore(b, P)
                mut.model_restore(model, P)
            cell, _ = compare(G, rname, P, a, b, model, f"{mname} -> {rname} [{pname}]", (mname, rname, pname) in CR.ORDER_PAIRS)
        print(f"CELL {mname} {rname} {pname} {cell}")


@pytest.mark.parametrize("pname", CR.PROBLEMS)
def test_nothing_calls_change_nothing(G, pname):
    P = CR.problem(pname)
    with handle(G, P, True) as a:
        CR.start([a], P)
        before, kinds = snapshot(a), a.sweep_kind()
        for mname, mut in CR.MUTATORS.items():
            if not mut.nothing or pname not in mut.problems:
                continue
            if mut.prepare:                                    # the call refuses the problem's state as it stands: behind what it needs
                mut.prepare(a, P)                              # and a sweep, it and every later call are held to THAT state
                a.sweep()
                before, kinds = snapshot(a), a.sweep_kind()
                mut.run(a, P, prepared=True)
            else:
                mut.run(a, P)
            after = snapshot(a)
            assert all(before[k].tobytes() == after[k].tobytes() for k in before), mname
            assert a.sweep_kind() == kinds == (CR.REUSED, CR.FULL), mname


def _answer(G, name, dev, P):
    """a reader's arrays, or what it raised (a failed factorisation is reported by the getters as LinAlgError, PosDefException or
    SGPError: the class and the text are compared)"""
    try:
        if name == "sweep":
            dev.sweep()
            return snapshot(dev), None
        return flat(name, CR.READERS[name].run(dev, P)), None
    except (G.SGPError, np.linalg.LinAlgError, ArithmeticError, ValueError) as e:
        return None, (type(e).__name__, str(e))


def failure_problem():
    """the `toy` case of tests/test_gpu_vmp_run.py (its test_failure_stop_and_recovery: two coincident inducing inputs and no jitter make
    K_uu fail at minor 6) with what the readers of this grid ask for"""
    from tests import test_gpu_vmp_run as V
    T = V.problem("toy")
    rng = np.random.default_rng(103)
    N, M, D = T["N"], T["M"], T["D"]
    Xu = T["Xu"].copy()
    Xu[5] = Xu[2]
    theta = (T["s2"], T["ell"], T["jitter"])
    return dict(name="toy", d_out=1, D=D, M=M, N=N, X=T["X"], Y=T["y"], vy=None, wts=None, n_nodes=None, Xu=T["Xu"], Xu_bad=Xu,
                Xu2=CR._grid_xu(rng, M, D), W=np.array([[20.0]]), prior=T["prior"], theta1=theta, theta_bad=(T["s2"], T["ell"], 0.0),
                raw2=CR.invsoftplus(np.concatenate([[1.1 * T["s2"]], 0.9 * T["ell"]])), Xq=rng.uniform(-1.7, 1.7, (37, D)),
                qstart=np.array([0, 5, 6, 20, 37]), Yq=rng.normal(size=(4, 1)), wq=rng.uniform(0.2, 1.0, 37))


def test_failed_vmp_run_leaves_no_q_v(G):
    """A run whose K_uu is not positive definite (a status, not a fault) returns the failing minor at iteration 0.  The statistics its
    sweep formed are not reusable, and no reader hands out on the SGP_FLAG_REUSE_STATS handle anything the plain handle does not: the
    same arrays or the same refusal."""
    import contextlib
    P = failure_problem()
    cells = []
    for rname, reader in CR.READERS.items():
        with contextlib.ExitStack() as stack:
            a, b = stack.enter_context(handle(G, P, True)), stack.enter_context(handle(G, P))
            CR.start([a, b], P)
            assert a.sweep_kind()[0] == CR.REUSED
            for d in (a, b):
                d.set_inducing(P["Xu_bad"])
                d.set_kernel(*P["theta_bad"])
                with pytest.raises(np.linalg.LinAlgError) as e:
                    d.vmp_run(4, gamma_prior=CR.VMP_PRIOR_G)
                assert e.value.minor == 6 and e.value.iterations_done == 0 and np.isnan(e.value.values).all()
                assert e.value.counts == (0, -6)
            assert a.sweep_kind()[0] == CR.FULL and b.sweep_kind()[0] == CR.FULL
            ra, fa = _answer(G, rname, a, P)
            rb, fb = _answer(G, rname, b, P)
            assert fa == fb, f"failed vmp_run -> {rname}: A {fa} but B {fb}"
            if fa is None:                                     # (bytes: a reader that does not look at the status words -- w_stats, after any
                # failed sweep -- hands out the NaN of the failed factor, on both handles alike)
                assert all(ra[k].tobytes() == rb[k].tobytes() for k in ra), f"failed vmp_run -> {rname}: A and B differ"
                finite = all(np.isfinite(ra[k]).all() for k in ra)
            cells.append((rname, ("same-answer" if finite else "same-answer non-finite") if fa is None else f"same-refusal {fa[0]}"))
    for rname, cell in cells:
        print(f"CELL vmp_run_failed {rname} toy {cell}")


def test_a_second_probit_run_needs_set_data(G):
    """behind a Probit run the resident targets are q(f) with its variances, no labels: the header asks for sgp_set_data first"""
    P = CR.problem("uni")
    with handle(G, P, True) as a:
        CR.start([a], P)
        CR.MUTATORS["vmp_run_probit_3"].run(a, P)
        with pytest.raises(G.SGPError, match="the resident data must have been set without y_var"):
            a.vmp_run(1, likelihood="probit", gamma_prior=CR.VMP_PRIOR_G)
        a.set_data(P["X"], CR.vmp_labels(P))
        assert a.vmp_run(1, likelihood="probit", gamma_prior=CR.VMP_PRIOR_G)[3] == 1


def test_stale_statistics_are_only_handed_out_where_documented(G):
    import contextlib
    P = CR.problem("multi")
    with contextlib.ExitStack() as stack:
        a, b = stack.enter_context(handle(G, P, True)), stack.enter_context(handle(G, P))
        model = CR.start([a, b], P)
        old = a.stats()
        mut = CR.MUTATORS["inducing_descend_psi_3"]
        ra = mut.run(a, P)
        mut.run(b, P)
        mut.model(model, P, ra, a)
        assert np.abs(ra[1] - P["Xu"]).max() > 1e-3            # the inducing inputs moved
        for x, y in zip(old, a.stats()):                       # documented: sgp_get_stats still hands out the OLD X_u's statistics
            assert np.array_equal(x, y)
        assert a.sweep_kind()[0] == CR.FULL
        cell, _ = compare(G, "sweep", P, a, b, model, "inducing_descend_psi -> sweep")   # C is at the moved X_u
        print("CELL stale inducing_descend_psi_3 sweep multi", cell)
        new = a.stats()
        assert not np.array_equal(old[0], new[0])


def test_output_cov_sum_leaves_the_objective_where_it_is(G):
    """The row the table left open: sgp_set_output_cov_sum marks the targets pending and leaves data_gen alone, so a following
    sgp_theta_objective stays on its fresh path and returns the value it returned before the call, to the bit.  That is right because
    the objective does not depend on the sum.  d_out > 1: by the formula, the MultiSGP objective has no y'y term.  d_out = 1: the sum
    enters S_YY and sum I2 alike and cancels to rounding -- held here against a handle that set the sum BEFORE its sweep, at the parity
    bound (measured 8e-13 relative on a value of -4564.5)."""
    P = CR.problem("uni")
    with handle(G, P, True) as a, handle(G, P) as c:
        CR.start([a], P)
        v0 = a.theta_objective()
        a.set_output_cov_sum([[3.0]])
        assert a.sweep_kind()[0] == CR.TARGETS
        v = a.theta_objective()
        vals = CR.first_setters(P)
        for n in CR.SETTERS:
            if n in vals:
                CR.apply_set(c, n, vals[n])
        c.set_output_cov_sum([[3.0]])
        c.sweep()
        vc = c.theta_objective()
    tol = post_tol(CR.kuu_cond(P, P["theta1"], "se"))
    print(f"CELL set_output_cov_sum(d_out=1) theta_objective uni v0 {v0:.12g} v {v:.12g} vC {vc:.12g}")
    assert v == v0 and abs(v - vc) <= tol * abs(vc), (v0, v, vc)


def test_w_stats_is_sized_by_the_resident_points_after_a_training_run(G):
    """sgp_w_stats writes one entry per resident point, after a run the last window's (72 here): the Python layer sizes its arrays by
    them -- also on a handle that never saw set_data, where it used to hand the library empty arrays to write 72 entries into"""
    P = CR.problem("uni")
    res = []
    for with_data in (True, False):
        with handle(G, P, True) as d:
            vals = CR.first_setters(P)
            for n in CR.SETTERS:
                if n in vals and (with_data or n != "data"):
                    CR.apply_set(d, n, vals[n])
            if with_data:
                d.sweep()
            CR._train(d, P)
            I1, I2 = d.w_stats()
            assert I1.shape == I2.shape == (72,) and np.isfinite(I1).all() and np.isfinite(I2).all()
            res.append((I1, I2))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])     # the run's, whatever came before it


WALK_LENGTH = 25


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_walks(G, seed):
    import contextlib
    P = CR.problem("multi")
    rng = np.random.default_rng(1000 + seed)
    names = [("m", n) for n, op in CR.MUTATORS.items() if "multi" in op.problems and n != "train_run"]
    names += [("r", n) for n, op in CR.READERS.items() if "multi" in op.problems]
    log = []
    with contextlib.ExitStack() as stack:
        a, b = stack.enter_context(handle(G, P, True)), stack.enter_context(handle(G, P))
        model = CR.start([a, b], P)
        try:
            for step in range(WALK_LENGTH):
                kind, name = names[rng.integers(len(names))]
                log.append(name if kind == "m" else f"read:{name}")
                if kind == "m":
                    mut = CR.MUTATORS[name]
                    ra, fa = call(G, mut, a, P)
                    rb, fb = call(G, mut, b, P)
                    assert fa == fb, (name, fa, fb)
                    if fa is None and mut.model:
                        mut.model(model, P, ra, a)
                    continue
                if name == "sweep" and model.cur["data"] is None:
                    CR._restore_data(a, P), CR._restore_data(b, P), CR._m_restore_data(model, P)
                reader = CR.READERS[name]
                cell, ra = compare(G, name, P, a, b, model, f"walk {seed} step {step}: {name}")
                log[-1] += f" [{cell}]"
                if cell != "refused" and reader.model:
                    reader.model(model, P, ra, a)
        except BaseException:
            print(f"walk {seed} failed after:", log)
            raise
    print(f"WALK {seed}: {len(log)} calls:", ", ".join(log))
