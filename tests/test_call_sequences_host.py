"""Call sequences without a GPU: the ledger (every exported entry point and every row of the "Entry point -> effect" table has a
class and an entry in tests/call_sequence_ref.py), the A-against-C harness over tests/cpu_engine.OracleDevice -- as it is, and with
four seeded staleness faults it must see --, the shadow model's normal form, and the conditioning of the two problems."""
import os

import numpy as np
import pytest

from tests import call_sequence_ref as CR
from tests.cpu_engine import OracleDevice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- ledger -------------------------------------------------------------------------------------------------------------------
def test_every_exported_entry_point_is_classified():
    from gaussianprocessnode_amd import _lib
    names = CR.exported_names(open(os.path.join(ROOT, "include", "sgp_hip.h")).read())
    assert len(names) > 60 and set(names) == set(_lib.EXPORTS)
    missing = [n for n in names if n not in CR.ENTRY_POINTS]
    assert not missing, f"classify {missing} in tests/call_sequence_ref.ENTRY_POINTS (and give a mutator a row in MUTATORS)"
    assert not set(CR.ENTRY_POINTS) - set(names), "ENTRY_POINTS names something the header does not declare"
    assert set(CR.ENTRY_POINTS.values()) == {CR.MUTATOR, CR.READER, CR.NO_STATE}


def test_every_row_of_the_comment_table_has_a_mutator_entry():
    api = open(os.path.join(ROOT, "gaussianprocessnode_amd", "csrc", "sgp_api.hip")).read()
    rows = CR.table_rows(api)
    assert len(rows) >= 20, len(rows)
    covered = {r for op in CR.MUTATORS.values() for r in op.rows}
    for names, line in rows:
        assert names, line
        for n in names:
            if n in CR.UNREACHABLE_ROWS or n == "use_rccl":
                continue
            assert n in covered, f"no MUTATORS entry stands for the table row of {n}: {line.strip()}"
    assert "tests/call_sequence_ref.py" in api.split("Entry point -> effect:", 1)[1].split("struct StatsRecord", 1)[0]
    # the variants the table distinguishes
    for name in ("set_kernel_same", "set_kernel_new", "set_kernel_family_same", "set_kernel_family_other", "theta_objective_same",
                 "theta_objective_other", "theta_objective_xu_same", "theta_objective_xu_other", "theta_descend_0", "theta_descend_3",
                 "theta_descend_psi_0", "theta_descend_psi_3", "inducing_descend_0", "inducing_descend_3", "inducing_descend_3_xu_only",
                 "inducing_descend_psi_0", "inducing_descend_psi_3", "inducing_descend_psi_3_xu_only", "train_run", "set_posterior",
                 "carry_posterior", "set_targets", "set_output_cov_sum", "sweep_local_psi+finish", "psi_stats", "theta_objective_psi",
                 "theta_objective_psi_xu", "psi_in_grad", "psi_predict", "predict", "predict_var", "w_stats", "in_message",
                 "in_message_grad", "out_message", "vmp_run_0", "vmp_run_hold_3", "vmp_run_gauss_3", "vmp_run_probit_3",
                 "vmp_run_tol_stop"):
        assert name in CR.MUTATORS, name
    for name, op in CR.MUTATORS.items():                      # sgp_vmp_run refuses d_out > 1
        if "sgp_vmp_run" in op.rows:
            assert op.problems == ("uni",) and op.kind == CR.REUSED, name
    assert {n: CR.MUTATORS[n].last for n in CR.MUTATORS if CR.MUTATORS[n].last is not None} == {
        "vmp_run_hold_3": CR.REUSED, "vmp_run_gauss_3": CR.FULL, "vmp_run_probit_3": CR.FULL, "vmp_run_tol_stop": CR.REUSED}
    assert CR.ENTRY_POINTS["sgp_vmp_run"] == CR.MUTATOR
    assert CR.MUTATORS["set_output_cov_sum"].problems == ("multi",) and CR.MUTATORS["train_run"].problems == ("uni",)
    assert all(op.kind == CR.REUSED for op in CR.MUTATORS.values() if op.nothing)


# ---- the harness can see staleness ------------------------------------------------------------------------------------------------
HOST_MUTATORS = ("set_inducing", "set_data", "set_kernel_new", "set_kernel_same", "set_prior", "set_noise")
HOST_READERS = ("theta_objective", "w_stats", "predict", "sweep")


class StaleDevice(OracleDevice):
    """OracleDevice with one seeded fault: it keeps the last sweep's statistics (or its q(v)) across a call it should not."""

    def __init__(self, *a, fault=None, **kw):
        super().__init__(*a, **kw)
        self.fault, self.kept, self.keep_qv = fault, None, False

    def set_kernel_family(self, family):
        assert family == "se"

    def set_inducing(self, Xu):
        super().set_inducing(Xu)
        if self.fault != "set_inducing":
            self.kept = None

    def set_data(self, *a, **kw):
        super().set_data(*a, **kw)
        if self.fault != "set_data":
            self.kept = None

    def set_kernel(self, sigma2, ell, jitter=0.0):
        same = hasattr(self, "s2") and (sigma2, jitter) == (self.s2, self.jitter) and np.array_equal(ell, self.ell)
        super().set_kernel(sigma2, ell, jitter)
        if not same and self.fault != "set_kernel":
            self.kept = None

    def set_prior_isotropic(self, var):
        super().set_prior_isotropic(var)
        self.keep_qv = self.fault == "set_prior" and hasattr(self, "res")

    def sweep(self, stream=0):
        from oracle import sgp_oracle as O
        if self.keep_qv:                                      # the fault: q(v) kept across set_prior
            self.keep_qv = False
            return
        if self.kept is not None:                             # a reused sweep: phase 2 over the kept statistics
            self.res = O.vmp_sweep(self.Xu, None, None, None, self.s2, self.ell, self.w, E_logw=self.E_logw, jitter=self.jitter,
                                   Lambda0=self.Lambda0, xi0=self.xi0, stats=self.kept)
        else:
            super().sweep(stream)
        self.kept = self.res.stats


def _read(dev, name, P):
    if name == "sweep":
        dev.sweep()
        return tuple(dev.posterior()) + (dev.kuu_chol(),)
    if name == "theta_objective":
        return (np.array([dev.theta_objective()]),)
    if name == "w_stats":
        return tuple(dev.w_stats())
    return (dev.predict(P["Xq"]),)


def run_harness(fault=None):
    """[(mutator, reader, worst relative difference A against C)] over the oracle engine, in the order the calls are made"""
    P = CR.problem("uni")
    out = []
    for mname in HOST_MUTATORS:
        mut = CR.MUTATORS[mname]
        for rname in HOST_READERS:                            # a fresh A per reader: each is read directly behind the mutator
            a = StaleDevice(P["N"], P["M"], P["D"], fault=fault)
            model = CR.start([a], P)
            mut.run(a, P)
            mut.model(model, P, None, a)
            if rname != "sweep" and model.cur["inducing"] is not model.at["inducing"]:
                continue                                      # (after set_inducing the device has no q(v); the oracle keeps none apart)
            c = CR.build(StaleDevice(P["N"], P["M"], P["D"]), model.normal_form())
            ra, rc = _read(a, rname, P), _read(c, rname, P)
            out.append((mname, rname, max(np.max(np.abs(x - y)) / np.max(np.abs(y)) for x, y in zip(ra, rc))))
    return out


@pytest.fixture(scope="module")
def passing():
    return run_harness()


def test_the_harness_passes_over_the_oracle_engine(passing):
    worst = max(e for _, _, e in passing)
    print(f"{len(passing)} mutator x reader pairs, worst relative difference {worst:.3e}")
    assert len(passing) >= 20
    assert worst <= 1e-12, [p for p in passing if p[2] > 1e-12]


@pytest.mark.parametrize("fault,mutator", [("set_inducing", "set_inducing"), ("set_kernel", "set_kernel_new"),
                                           ("set_data", "set_data"), ("set_prior", "set_prior")])
def test_a_seeded_fault_is_reported_at_the_first_reader_behind_it(passing, fault, mutator):
    worst = max(max(e for _, _, e in passing), np.finfo(float).eps)
    res = run_harness(fault)
    failing = [(m, r, e) for m, r, e in res if e > 1e-12]
    print(f"{fault}: first report {failing[:1]}, passing worst {worst:.3e}")
    # the faults keep statistics (or q(v)) for the NEXT sweep: the readers in front of it see nothing, the sweep is the first behind it
    assert failing and failing[0][:2] == (mutator, "sweep"), failing[:3]
    assert failing[0][2] >= 1e6 * worst
    assert all(m == mutator for m, _, _ in failing)           # and nowhere in front of it


# ---- the shadow model ---------------------------------------------------------------------------------------------------------
def test_the_normal_form_of_a_ten_call_history():
    P = CR.problem("multi")
    m = CR.Shadow()
    v = CR.first_setters(P)
    m.set("inducing", v["inducing"])                           # 1
    m.set("data", v["data"])                                  # 2
    m.set("cov_sum", P["S_y"])                                # 3
    m.set("kernel", P["theta2"])                              # 4
    m.set("kernel", P["theta1"])                              # 5: only the last value counts
    m.set("prior", P["prior"])                                # 6
    m.set("noise", P["W"])                                    # 7
    m.swept()                                                 # 8
    m.set("noise", P["W2"])                                   # 9
    m.set("targets", (P["Y2"], None))                         # 10: resets the output-covariance sum
    nf = m.normal_form()
    assert [o[:2] for o in nf] == [("set", "inducing"), ("set", "data"), ("set", "cov_sum"), ("set", "kernel"), ("set", "family"),
                                   ("set", "prior"), ("set", "noise"), ("sweep",), ("set", "noise"), ("set", "targets")]
    assert nf[3][2] is P["theta1"] and nf[6][2] is P["W"] and nf[8][2] is P["W2"]
    assert m.cur["cov_sum"] is None and not m.device_set and not m.stats_stale
    # a device-set kernel flags the history, through the next sweep, until a host setter replaces it
    m.set("kernel", (1.0, np.array([0.5, 0.5]), CR.JITTER), device=True)
    assert m.device_set
    m.swept()
    assert m.device_set and m.normal_form()[-1] == ("sweep",)
    m.set("kernel", P["theta1"])
    assert m.device_set                                        # (q(v) is still that sweep's)
    m.swept()
    assert not m.device_set
    # a noise with its E[log w] (what sgp_vmp_run leaves: psi(a) - log b, not set_noise's default log w) travels as one value; one
    # that came back from the device flags the history like a device-set kernel
    class Recorder:
        def set_noise(self, W, E_logw=None):
            self.noise = (np.asarray(W), E_logw)
    n1, n2 = CR._gamma_noise((3.0, 2.0)), CR._gamma_noise((5.0, 2.0))
    assert n1.W.shape == (1, 1) and n1.W[0, 0] == 1.5 and abs(n1.E_logw - (0.9227843350984671 - np.log(2.0))) < 1e-15   # psi(3) = 3/2 - gamma
    assert n1.E_logw < np.log(1.5) and CR.noise_matrix(n1) is n1.W and CR.noise_matrix(P["W"]).shape == P["W"].shape
    m.set("noise", n1, device=True)
    m.swept()
    m.set("noise", n2, device=True)
    nf = m.normal_form()
    assert m.device_set and [o[:2] for o in nf[-3:]] == [("set", "noise"), ("sweep",), ("set", "noise")]
    assert nf[-3][2] is n1 and nf[-1][2] is n2
    rec = Recorder()
    CR.apply_set(rec, "noise", nf[-1][2])
    assert rec.noise[0][0, 0] == 2.5 and rec.noise[1] == n2.E_logw
    CR.apply_set(rec, "noise", P["W"])
    assert rec.noise[0] is P["W"] and rec.noise[1] is None
    m.set("noise", P["W"])
    m.swept()
    assert not m.device_set
    # the exact-Psi sweep leaves the handle without data
    m.swept("psi", (P["mean"], P["cov"], P["Yn"]))
    assert m.cur["data"] is None and m.normal_form()[-1][0] == "psi_sweep"
    assert not any(o[:2] in (("set", "data"), ("set", "cov_sum")) for o in m.normal_form())


# ---- conditioning ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CR.PROBLEMS)
def test_kuu_is_well_conditioned_at_every_theta_of_the_tables(name):
    P = CR.problem(name)
    assert P["N"] == (200 if name == "uni" else 150) and P["M"] == (70 if name == "uni" else 48)
    for theta in (P["theta1"], P["theta2"], CR._kernel_of(P["raw1"]), CR._kernel_of(P["raw2"])):
        for fam in (P["family"], P["family2"]):
            for xu in ("Xu", "Xu2"):                          # (Xu2: set_inducing and the one-step inducing descent)
                c = CR.kuu_cond(P, theta, fam, P[xu])
                print(name, xu, fam, theta[0], theta[1], f"cond {c:.3e}")
                assert c < 1e6
    if name == "multi":                                       # the points and the Gaussians describe one model
        w = P["wts"].reshape(P["T"], 5)
        pts = P["X"].reshape(P["T"], 5, P["D"])
        np.testing.assert_allclose(w.sum(axis=1), 1.0, rtol=1e-14)
        np.testing.assert_allclose(np.einsum("tp,tpi->ti", w, pts), P["mean"], rtol=1e-12, atol=1e-14)
        dev = pts - P["mean"][:, None, :]
        np.testing.assert_allclose(np.einsum("tp,tpi,tpj->tij", w, dev, dev), P["cov"], rtol=1e-10, atol=1e-14)


def test_the_tol_of_vmp_run_tol_stop_separates_two_decrements_of_the_restatement():
    tol, k = CR.vmp_tol_stop("uni")
    assert k == 3 and 0.0 < tol < 1.0
    P = CR.problem("uni")
    lab = CR.vmp_labels(P)
    assert set(np.unique(lab)) == {0.0, 1.0} and 0.3 < lab.mean() < 0.7
