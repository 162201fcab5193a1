// The optimiser state of the device-paced runs (sgp_train_*, sgp_theta_descend, sgp_theta_descend_psi, sgp_inducing_descend,
// sgp_inducing_descend_psi) as the device keeps it, and the mapping between it and the ABI's `opt_state`.  Plain C++, no HIP:
// sgp_kernels.hip.h includes this file for the struct, and tools/descent_state_check.cpp checks the mapping on the host.
#pragma once

#include <cstring>

namespace sgp {

constexpr int THETA_SLOTS = 33;     // 1 + MAXD raw kernel parameters (sgp_kernels.hip.h asserts the sum)

struct TrainState {
    double theta[THETA_SLOTS];  // raw (pre-softplus) parameters: sigma2 first, then the lengthscale(s)
    double m[THETA_SLOTS];      // AdaMax first moment
    double u[THETA_SLOTS];      // AdaMax infinity-norm accumulator
    double bp[2];               // running powers of beta
    double eta, beta1, beta2, eps;
    double steps, rejected;     // optimiser steps taken / minibatches whose factorisations failed (theta left alone)
    // classification (SGP_LIKELIHOOD_PROBIT): q(w) = Gamma(ga, gb), carried over the minibatches and never reset
    // (experiments/classification_banana.ipynb cell 9: `shape, rate = params(qw)`)
    double ga, gb;
    double kind;                // 0 Gaussian likelihood with a fixed w (regression), 1 Probit with a Gamma q(w)
    double stop;                // the descents: 0 running; the K_uu status word (> 0 the failing minor) or -1 (a device-word wait or a
                                // twin workgroup gave up) of the step at which the descent stopped; the exact-Psi pair also -(t + 2)
                                // for an indefinite node t.  Latched: later steps change nothing
};

// The optimised vector of a descent: x = [theta (nt) | vec Xu (nx)], np entries.  theta-only runs have nx = 0; an inducing run that
// holds theta (learn = false) has nt = 0 and still carries all ntheta raw parameters.  opt_state (the ABI, AdaMax.get_state's layout):
// [m (np) | u (np) | beta1^t, beta2^t].  On the device theta's moments are TrainState.m / .u, the inducing coordinates' are
// Mom = [m (nx) | u (nx)] in call scratch, and the powers are TrainState.bp.
struct DescentLayout {
    int ntheta = 0;                 // 1 + n_ell
    int nt = 0, nx = 0, np = 0;
    bool learn = false;
};
static inline DescentLayout descent_layout(int n_ell, bool learn, int nx) {
    DescentLayout l;
    l.ntheta = 1 + n_ell;
    l.learn = learn;
    l.nt = learn ? l.ntheta : 0;
    l.nx = nx;
    l.np = l.nt + nx;
    return l;
}

// where opt_state keeps what Mom holds: m of the inducing coordinates, and u (nx entries each)
template <class T> static inline T* descent_state_mx(const DescentLayout& l, T* opt_state) { return opt_state + l.nt; }
template <class T> static inline T* descent_state_ux(const DescentLayout& l, T* opt_state) { return opt_state + l.np + l.nt; }

// a running power is beta^t, t >= 1: inside (0, 1), or exactly 0 for a beta of 0
static inline bool descent_powers_ok(const DescentLayout& l, const double* opt_state, double beta1, double beta2) {
    const double b[2] = {beta1, beta2};
    for (int i = 0; i < 2; ++i) {
        const double pw = opt_state[2 * (size_t)l.np + i];
        if (!(pw < 1.0) || !(pw > 0.0 || (pw == 0.0 && b[i] == 0.0))) return false;
    }
    return true;
}

// A run's first state: theta, its moments (zero without an opt_state, and when theta is held) and the powers (beta itself without
// one: the first step is t = 1), the optimiser's constants, and zero everywhere else
static inline void descent_pack(const DescentLayout& l, const double* theta_raw, const double* opt_state, double eta, double beta1,
                                double beta2, double eps, TrainState* st) {
    memset(st, 0, sizeof *st);
    for (int i = 0; i < l.ntheta; ++i) st->theta[i] = theta_raw[i];
    for (int i = 0; opt_state && i < l.nt; ++i) { st->m[i] = opt_state[i]; st->u[i] = opt_state[l.np + i]; }
    st->bp[0] = opt_state ? opt_state[2 * (size_t)l.np] : beta1;
    st->bp[1] = opt_state ? opt_state[2 * (size_t)l.np + 1] : beta2;
    st->eta = eta; st->beta1 = beta1; st->beta2 = beta2; st->eps = eps;
}

// ... and its last one back: theta always, theta's moments where it was optimised, the powers
static inline void descent_unpack(const DescentLayout& l, const TrainState& st, double* theta_raw, double* opt_state) {
    for (int i = 0; i < l.ntheta; ++i) theta_raw[i] = st.theta[i];
    if (!opt_state) return;
    for (int i = 0; i < l.nt; ++i) { opt_state[i] = st.m[i]; opt_state[l.np + i] = st.u[i]; }
    opt_state[2 * (size_t)l.np] = st.bp[0];
    opt_state[2 * (size_t)l.np + 1] = st.bp[1];
}

}  // namespace sgp
