// Host check of the descents' optimiser-state mapping (gaussianprocessnode_amd/csrc/descent_state.h), next to
// tools/point_scratch_check.cpp: over n_ell in {1, 2, MAXD}, theta learned or held, nx in {0, 1, 5, 64 * 32} inducing coordinates and
// opt_state given or NULL, descent_pack + the two moment copies into Mom, then the copies back + descent_unpack are the identity on
// theta_raw and opt_state; a held theta's moments are neither read nor written; every entry of [0, 2 np + 2) of opt_state is written
// back and nothing outside it is touched (guard words on either side, and a second pass over allocations of exactly that size, so
// that the sanitizer sees an access past them).  Then descent_powers_ok at and around the ends of (0, 1).  No GPU:
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -o tools/descent_state_check tools/descent_state_check.cpp
//   (or any C++17 compiler with -fsanitize=address,undefined) && tools/descent_state_check
#include "../gaussianprocessnode_amd/csrc/descent_state.h"

#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

using namespace sgp;

namespace {
constexpr int MAXD = THETA_SLOTS - 1;
constexpr size_t GUARD = 8;
constexpr double GUARD_WORD = -12345.0, POISON = 6.02e23;
long failures = 0, checks = 0;

void expect(bool ok, const DescentLayout& l, bool have_state, const char* what) {
    ++checks;
    if (!ok && ++failures <= 20)
        std::fprintf(stderr, "ntheta %d learn %d nx %d opt_state %s: %s\n", l.ntheta, (int)l.learn, l.nx, have_state ? "given" : "NULL", what);
}

// One combination.  `guarded`: opt_state sits between guard words; otherwise it is an allocation of exactly 2 np + 2 doubles.
void round_trip(int n_ell, bool learn, int nx, bool have_state, bool guarded) {
    const DescentLayout l = descent_layout(n_ell, learn, nx);
    auto bad = [&](bool ok, const char* what) { expect(ok, l, have_state, what); };
    bad(l.ntheta == 1 + n_ell && l.nt == (learn ? 1 + n_ell : 0) && l.np == l.nt + nx, "the layout's counts");
    const size_t len = 2 * (size_t)l.np + 2, pad = guarded ? GUARD : 0;
    const double eta = 1e-3, beta1 = 0.9, beta2 = 0.999, eps = 1e-8;

    // distinct values everywhere: entry i of opt_state is 1000 + i, the powers are in (0, 1)
    std::vector<double> theta((size_t)l.ntheta), in(pad + len + pad, GUARD_WORD);
    for (int i = 0; i < l.ntheta; ++i) theta[(size_t)i] = -3.0 + 0.25 * i;
    for (size_t i = 0; i < len; ++i) in[pad + i] = 1000.0 + (double)i;
    in[pad + len - 2] = 0.729;
    in[pad + len - 1] = 0.997;
    const std::vector<double> in0 = in;
    const double* opt_in = have_state ? in.data() + pad : nullptr;

    // onto the "device": TrainState, and Mom = [m | u] of the inducing coordinates as descent_begin copies it (zero without a state)
    TrainState st;
    memset(&st, 0x5a, sizeof st);
    descent_pack(l, theta.data(), opt_in, eta, beta1, beta2, eps, &st);
    std::vector<double> mom(2 * (size_t)nx, 0.0);
    if (opt_in && nx) {
        memcpy(mom.data(), descent_state_mx(l, opt_in), sizeof(double) * (size_t)nx);
        memcpy(mom.data() + nx, descent_state_ux(l, opt_in), sizeof(double) * (size_t)nx);
    }
    bad(in == in0, "descent_pack wrote to opt_state");
    for (int i = 0; i < THETA_SLOTS; ++i) {
        const bool moments = have_state && i < l.nt;
        bad(st.theta[i] == (i < l.ntheta ? theta[(size_t)i] : 0.0), "theta on the device");
        bad(st.m[i] == (moments ? 1000.0 + i : 0.0), "theta's first moment on the device (zero where theta is held or no state is given)");
        bad(st.u[i] == (moments ? 1000.0 + l.np + i : 0.0), "theta's second moment on the device");
    }
    bad(st.bp[0] == (have_state ? 0.729 : beta1) && st.bp[1] == (have_state ? 0.997 : beta2), "the running powers on the device");
    bad(st.eta == eta && st.beta1 == beta1 && st.beta2 == beta2 && st.eps == eps, "the optimiser's constants");
    bad(st.steps == 0.0 && st.rejected == 0.0 && st.ga == 0.0 && st.gb == 0.0 && st.kind == 0.0 && st.stop == 0.0, "the rest of the state is zero");
    for (int i = 0; i < nx; ++i)
        bad(mom[(size_t)i] == (have_state ? 1000.0 + l.nt + i : 0.0) && mom[(size_t)nx + i] == (have_state ? 1000.0 + l.np + l.nt + i : 0.0),
            "the inducing coordinates' moments on the device");

    // a held theta's moments on the device are not the caller's: whatever they hold must not come back
    if (!learn)
        for (int i = 0; i < THETA_SLOTS; ++i) st.m[i] = st.u[i] = POISON;

    // and back, into buffers that hold nothing of the answer
    std::vector<double> theta_out((size_t)l.ntheta, POISON), out(pad + len + pad, GUARD_WORD);
    for (size_t i = 0; i < len; ++i) out[pad + i] = POISON;
    double* opt_out = have_state ? out.data() + pad : nullptr;
    descent_unpack(l, st, theta_out.data(), opt_out);
    if (opt_out && nx) {
        memcpy(descent_state_mx(l, opt_out), mom.data(), sizeof(double) * (size_t)nx);
        memcpy(descent_state_ux(l, opt_out), mom.data() + nx, sizeof(double) * (size_t)nx);
    }
    bad(theta_out == theta, "theta_raw does not come back");
    if (have_state) {
        bad(out == in0, "opt_state does not come back (an entry not written, written from the wrong place, or a guard word touched)");
    } else {
        for (size_t i = 0; i < out.size(); ++i) bad(out[i] == (i < pad || i >= pad + len ? GUARD_WORD : POISON), "written without an opt_state");
    }
}

void powers() {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    struct Case { double pw, beta; bool ok; const char* what; };
    const Case cases[] = {
        {0.0, 0.0, true, "0 with beta = 0 is accepted"},
        {0.0, 0.9, false, "0 with beta > 0 is refused"},
        {1.0, 0.9, false, "1 is refused"},
        {1.0, 0.0, false, "1 with beta = 0 is refused"},
        {0.5, 0.9, true, "inside (0, 1) is accepted"},
        {0.5, 0.0, true, "inside (0, 1) with beta = 0 is accepted"},
        {std::nextafter(0.0, 1.0), 0.9, true, "the smallest positive power is accepted"},
        {std::nextafter(1.0, 0.0), 0.9, true, "the largest power below 1 is accepted"},
        {-0.25, 0.9, false, "a negative power is refused"},
        {-0.0, 0.9, false, "-0 with beta > 0 is refused"},
        {1.5, 0.9, false, "a power above 1 is refused"},
        {nan, 0.9, false, "NaN is refused"},
    };
    for (int n_ell : {1, MAXD})
        for (int nx : {0, 5}) {
            const DescentLayout l = descent_layout(n_ell, true, nx);
            std::vector<double> st(2 * (size_t)l.np + 2, nan);      // (the moments are not the check's business: NaN there changes nothing)
            for (const Case& c : cases)
                for (int slot = 0; slot < 2; ++slot) {
                    // the slot under test against its own beta, the other one fine
                    double beta[2] = {0.9, 0.999};
                    st[2 * (size_t)l.np + (size_t)(1 - slot)] = 0.5;
                    st[2 * (size_t)l.np + (size_t)slot] = c.pw;
                    beta[slot] = c.beta;
                    expect(descent_powers_ok(l, st.data(), beta[0], beta[1]) == c.ok, l, true, c.what);
                }
        }
}
}  // namespace

int main() {
    long combos = 0;
    for (int n_ell : {1, 2, MAXD})
        for (int learn = 0; learn < 2; ++learn)
            for (int nx : {0, 1, 5, 64 * 32})
                for (int have_state = 0; have_state < 2; ++have_state)
                    for (int guarded = 0; guarded < 2; ++guarded, ++combos) round_trip(n_ell, learn != 0, nx, have_state != 0, guarded != 0);
    const long trip_checks = checks;
    powers();
    std::printf("descent_state_check: %ld round trips (%ld checks), %ld running-power checks, %ld failures\n", combos, trip_checks,
                checks - trip_checks, failures);
    return failures ? 1 : 0;
}
