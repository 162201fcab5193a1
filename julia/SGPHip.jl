# SGPHip.jl -- the binding a GaussianProcessNode maintainer would add to route the UniSGP / MultiSGP hot path through
# libsgp_hip.so (include/sgp_hip.h).  WRITTEN BLIND: Julia is not available in the build pipeline, so this file has never
# been executed.  It mirrors, call for call, the Python host mirror (gaussianprocessnode_amd/unisgp.py, multisgp.py),
# which IS tested against the reference's rule tests on the GPU.
#
# The reference's rule bodies are not edited.  The only change in user code is the meta constructor:
#
#     include("GPnode/UniSGPnode.jl"); include("GPnode/MultiSGPnode.jl")
#     include("SGPHip.jl"); using .SGPHip
#     @meta function meta_gp_regression(Xu, Ψ0, Ψ1_trans, Ψ2, KuuL, kernel, Uv)
#         UniSGP() -> HipSGPMeta(UniSGPMeta(nothing, Xu, Ψ0, Ψ1_trans, Ψ2, KuuL, kernel, Uv, 0, batch_size);
#                                kernel_params = θ -> (softplus(θ[1]), softplus.(θ[2:end])))
#     end
#
# `HipSGPMeta` wraps the reference's meta and owns a device handle.  The methods below dispatch on it.  The PointMass-input
# rules (the hot path: `:v`, the N-fold product, `:w`, the average energy, `:out`) run on the device inside the sweep.  The
# cold rules run on the device too, call for call like gaussianprocessnode_amd/unisgp.py:183-387: uncertain inputs enter `:v`
# and `:out` as cubature-weighted data, and the per-node clamped `:w` / average energy of an uncertain input, the `:in`
# closure and the three `:θ` closures are stand-alone per-point evaluations (`stats_at`: sgp_set_data + sgp_sweep_local +
# sgp_set_posterior + sgp_w_stats on an auxiliary handle) at whatever q_v / meta.Uv the caller passes -- the wrapped
# `UniSGPMeta`'s `Uv`, `KuuL` and `counter` are kept up to date exactly as GPnode/UniSGPnode.jl:64-71 does.
# `HipMultiSGPMeta` does the same for the MultiSGP node: the cubature Ψ-statistics of a step (GPnode/MultiSGPnode.jl:11-35,
# 5 Gram columns and 5 rank-1 M × M updates per step in the reference) come from the device, and so do the `:in` and `:θ`
# closures (multisgp.py:169-278); the D × D algebra around them stays as the reference has it.
module SGPHip

using ReactiveMP, LinearAlgebra
import KernelFunctions                         # (the kernel family of a kernel object, kernel_family_id)
import Optim                                   # (the reference's MultiSGP(:in) Laplace rule uses it, GPnode/MultiSGPnode.jl:229)
import ReactiveMP: @rule, @average_energy, @call_rule, GenericProd, PointMass, MvNormalMeanCovariance,
                   MvNormalMeanPrecision, MvNormalWeightedMeanPrecision, NormalMeanPrecision, GammaShapeRate, Wishart,
                   NormalDistributionsFamily, UnivariateGaussianDistributionsFamily, MultivariateNormalDistributionsFamily,
                   MultivariateGaussianDistributionsFamily, UnivariateNormalDistributionsFamily, mean, var, cov, mean_cov,
                   mean_var, AverageEnergy, ContinuousUnivariateLogPdf, ContinuousMultivariateLogPdf, UnspecifiedDomain
import ..UniSGP, ..UniSGPMeta, ..MultiSGP, ..MultiSGPMeta, ..WishartFast, ..approximate_kernel_expectation!

export HipSGPMeta, HipMultiSGPMeta, predict, predictive, theta_objective, theta_objective_xu, theta_objective_psi_xu, inducing_descend!, inducing_descend_psi!, select_inducing, carry_posterior!, multisgp_sweep!

const LIB = get(ENV, "SGP_HIP_LIB", "libsgp_hip.so")

# ------------------------------------------------------------------------------------------------------------------
# the C ABI (include/sgp_hip.h)
# ------------------------------------------------------------------------------------------------------------------
struct SGPConfig
    n_max::Int64; m::Int32; d::Int32; d_out::Int32; device::Int32; flags::Int32; reserved::Int32
end
const SGP_FLAG_KEEP_KUF = Int32(2)
const SGP_FLAG_REUSE_STATS = Int32(16)
const SGP_SWEEP_FULL, SGP_SWEEP_TARGETS, SGP_SWEEP_REUSED, SGP_SWEEP_REWEIGHTED = 0, 1, 2, 3
const SGP_KERNEL_SE, SGP_KERNEL_MATERN12, SGP_KERNEL_MATERN32, SGP_KERNEL_MATERN52 = Int32(0), Int32(1), Int32(2), Int32(3)

# the kernel family (include/sgp_hip.h, SGP_KERNEL_*) of a `kernel_family` argument: a name (:se, :matern12, :matern32,
# :matern52), an id, or the kernel object kernel(θ) returns (σ² * with_lengthscale(base, ℓ): the base kernel decides)
kernel_family_id(i::Integer) = Int32(i)
kernel_family_id(s::Symbol) = Dict(:se => SGP_KERNEL_SE, :matern12 => SGP_KERNEL_MATERN12, :matern32 => SGP_KERNEL_MATERN32,
                                   :matern52 => SGP_KERNEL_MATERN52)[s]
kernel_family_id(k::KernelFunctions.ScaledKernel) = kernel_family_id(k.kernel)
kernel_family_id(k::KernelFunctions.TransformedKernel) = kernel_family_id(k.kernel)
kernel_family_id(::KernelFunctions.SqExponentialKernel) = SGP_KERNEL_SE             # SEKernel
kernel_family_id(::KernelFunctions.ExponentialKernel) = SGP_KERNEL_MATERN12         # Matern12Kernel
kernel_family_id(::KernelFunctions.Matern32Kernel) = SGP_KERNEL_MATERN32
kernel_family_id(::KernelFunctions.Matern52Kernel) = SGP_KERNEL_MATERN52
const SGP_S_COUNT = 8
const SGP_R_COUNT = 8

function check(rc::Cint, h)
    rc == 0 && return
    msg = unsafe_string(ccall((:sgp_last_error, LIB), Cstring, (Ptr{Cvoid},), h))
    rc > 0 ? throw(PosDefException(rc)) : error("libsgp_hip: status $rc: $msg")     # fastcholesky's failure mode
end

mutable struct Handle
    ptr::Ptr{Cvoid}
    m::Int; d::Int; d_out::Int; n_max::Int
    family::Int32                     # kernel family (sgp_set_kernel_family), set once at creation
end

function Handle(n_max, Xu::Matrix{Float64}, d_out; device = 0, flags = SGP_FLAG_KEEP_KUF, family = SGP_KERNEL_SE)
    D, M = size(Xu)                                            # D × M column-major = M points of D doubles: the ABI layout
    cfg = Ref(SGPConfig(n_max, M, D, d_out, device, flags, 0))
    p = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:sgp_create, LIB), Cint, (Ref{SGPConfig}, Ref{Ptr{Cvoid}}), cfg, p), C_NULL)
    h = Handle(p[], M, D, d_out, n_max, Int32(family))
    finalizer(x -> ccall((:sgp_destroy, LIB), Cint, (Ptr{Cvoid},), x.ptr), h)
    check(ccall((:sgp_set_inducing, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}), h.ptr, Xu), h.ptr)
    check(ccall((:sgp_set_kernel_family, LIB), Cint, (Ptr{Cvoid}, Int32), h.ptr, h.family), h.ptr)
    return h
end

inducing_matrix(Xu) = Xu[1] isa Number ? reshape(collect(Float64, Xu), 1, :) : reduce(hcat, [collect(Float64, u) for u in Xu])

set_data!(h::Handle, X::Matrix{Float64}, y, yv, ω, n_nodes) =
    check(ccall((:sgp_set_data, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Float64),
                h.ptr, X, y, yv === nothing ? C_NULL : yv, ω === nothing ? C_NULL : ω, size(X, 2), n_nodes), h.ptr)
set_kernel!(h::Handle, σ², ℓ::Vector{Float64}, jitter) =
    check(ccall((:sgp_set_kernel, LIB), Cint, (Ptr{Cvoid}, Float64, Ptr{Float64}, Int32, Float64), h.ptr, σ², ℓ, length(ℓ), jitter), h.ptr)
set_noise!(h::Handle, W::Matrix{Float64}, ElogW) =
    check(ccall((:sgp_set_noise, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Float64), h.ptr, W, ElogW), h.ptr)
set_prior!(h::Handle, vec, mat::Matrix{Float64}, form) =
    check(ccall((:sgp_set_prior, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int32), h.ptr, vec, mat, form), h.ptr)
# new targets for the resident inputs (X, weights and n_nodes of the last set_data!): with SGP_FLAG_REUSE_STATS the next sweep!
# forms only B and the data scalars
set_targets!(h::Handle, y, yv) =
    check(ccall((:sgp_set_targets, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), h.ptr, y, yv === nothing ? C_NULL : yv), h.ptr)
sweep!(h::Handle) = check(ccall((:sgp_sweep, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), h.ptr, C_NULL), h.ptr)
# (next, last) kind of sweep: SGP_SWEEP_FULL, SGP_SWEEP_TARGETS or SGP_SWEEP_REUSED (include/sgp_hip.h, sgp_sweep_kind)
function sweep_kind(h::Handle)
    nxt = Ref{Int32}(0); last = Ref{Int32}(0)
    check(ccall((:sgp_sweep_kind, LIB), Cint, (Ptr{Cvoid}, Ref{Int32}, Ref{Int32}), h.ptr, nxt, last), h.ptr)
    return (Int(nxt[]), Int(last[]))
end
# the plan of the last sweep as a bit mask (include/sgp_hip.h, sgp_sweep_plan): 1 overlapped, 2 pack, 4 events, 8 join_word,
# 16 kuu_interleaved, 32 stats_first, 64 gate_side, 128 resident
function sweep_plan(h::Handle)
    bits = Ref{Int32}(0)
    check(ccall((:sgp_sweep_plan, LIB), Cint, (Ptr{Cvoid}, Ref{Int32}), h.ptr, bits), h.ptr)
    return Int(bits[])
end
sweep_local!(h::Handle) = check(ccall((:sgp_sweep_local, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), h.ptr, C_NULL), h.ptr)
wait!(h::Handle) = check(ccall((:sgp_wait, LIB), Cint, (Ptr{Cvoid},), h.ptr), h.ptr)      # polled drain of the handle's streams

function posterior(h::Handle)
    Q = h.m * h.d_out
    μ = zeros(Q); Σ = zeros(Q, Q); Uv = zeros(Q, Q)
    check(ccall((:sgp_get_posterior, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), h.ptr, μ, Σ, Uv), h.ptr)
    return μ, Σ, Uv
end
function stats(h::Handle)
    Ψ2 = zeros(h.m, h.m); B = zeros(h.m, h.d_out); sc = zeros(SGP_S_COUNT)
    check(ccall((:sgp_get_stats, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), h.ptr, Ψ2, B, sc), h.ptr)
    return Ψ2, B, sc
end
function scalars(h::Handle)
    out = zeros(SGP_R_COUNT)
    check(ccall((:sgp_get_scalars, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}), h.ptr, out), h.ptr)
    return out                                                 # [ΣI1, ΣI2, energy, info Kuu, info Λ, info prior, logdet Kuu, logdet Λ]
end
function w_stats(h::Handle, n)
    I1 = zeros(n); I2 = zeros(n)
    check(ccall((:sgp_w_stats, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}), h.ptr, I1, I2, C_NULL), h.ptr)
    return I1, I2
end
function wishart_invscale(h::Handle)
    S = zeros(h.d_out, h.d_out)
    check(ccall((:sgp_get_wishart_invscale, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}), h.ptr, S), h.ptr)
    return S
end
function predict_mean(h::Handle, Xstar::Matrix{Float64}, μ_v::Vector{Float64})
    out = zeros(size(Xstar, 2), h.d_out)
    check(ccall((:sgp_predict, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}), h.ptr, Xstar, size(Xstar, 2), μ_v, out), h.ptr)
    return out
end

# predictive mean and (co)variance (include/sgp_hip.h, sgp_predict_var): μ_v = Σ_v = nothing uses the handle's last sweep;
# var is a Vector (d_out = 1) or d_out × d_out × ns (column-major [ns][d_out][d_out] is the same memory, blocks symmetric)
function predict_var(h::Handle, Xstar::Matrix{Float64}, μ_v = nothing, Σ_v = nothing; noise::Bool = false)
    ns = size(Xstar, 2)
    mean = zeros(ns, h.d_out)
    var = h.d_out == 1 ? zeros(ns) : zeros(h.d_out, h.d_out, ns)
    μp = μ_v === nothing ? C_NULL : Vector{Float64}(μ_v)
    Σp = Σ_v === nothing ? C_NULL : Matrix{Float64}(Σ_v)
    check(ccall((:sgp_predict_var, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}),
                h.ptr, Xstar, ns, μp, Σp, Int32(noise ? 1 : 0), mean, var), h.ptr)
    return mean, var
end

# predictive mean and JOINT covariance over all test points (include/sgp_hip.h, sgp_predict_joint), call for call with the Python
# layer's SGPDevice.predict_joint: cov is R × R, R = ns d_out, exactly symmetric; row i ns + s (0-based) is output i at point s,
# the order of vec(mean).  Like the rest of this file it has never been executed: only the ccall signature is stated here.
function predict_joint(h::Handle, Xstar::Matrix{Float64}, μ_v = nothing, Σ_v = nothing; noise::Bool = false)
    ns = size(Xstar, 2)
    R = ns * h.d_out
    mean = zeros(ns, h.d_out)
    cov = zeros(R, R)
    μp = μ_v === nothing ? C_NULL : Vector{Float64}(μ_v)
    Σp = Σ_v === nothing ? C_NULL : Matrix{Float64}(Σ_v)
    check(ccall((:sgp_predict_joint, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}),
                h.ptr, Xstar, ns, μp, Σp, Int32(noise ? 1 : 0), mean, cov), h.ptr)
    return mean, cov
end

# predictive derivatives at test inputs (include/sgp_hip.h, sgp_predict_grad), call for call with the Python layer's
# SGPDevice.predict_grad: mean ns × d_out, jac D × d_out × ns (∂mean_o/∂x_d), var d_out × d_out × ns, var_grad D × d_out × d_out × ns
# (∂C_f[i, j]/∂x_d; C_f is symmetric, so the column-major reading of the C layout is the same array) and jac_cov
# (d_out D) × (d_out D) × ns, the covariance of vec(∂f/∂x) with 0-based row index i D + d, exactly symmetric.  An output that is
# switched off is `nothing`.  Like the rest of this file it has never been executed: only the ccall signature is stated here.
function predict_grad(h::Handle, Xstar::Matrix{Float64}, μ_v = nothing, Σ_v = nothing; noise::Bool = false, var::Bool = true,
                      var_grad::Bool = true, jac_cov::Bool = false)
    D, ns = size(Xstar)
    o = h.d_out
    mean = zeros(ns, o)
    jac = zeros(D, o, ns)
    v = var ? zeros(o, o, ns) : nothing
    vg = var_grad ? zeros(D, o, o, ns) : nothing
    jc = jac_cov ? zeros(o * D, o * D, ns) : nothing
    μp = μ_v === nothing ? C_NULL : Vector{Float64}(μ_v)
    Σp = Σ_v === nothing ? C_NULL : Matrix{Float64}(Σ_v)
    check(ccall((:sgp_predict_grad, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64},
                                                Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                h.ptr, Xstar, ns, μp, Σp, Int32(noise ? 1 : 0), mean, jac, v === nothing ? C_NULL : v, vg === nothing ? C_NULL : vg,
                jc === nothing ? C_NULL : jc), h.ptr)
    return mean, jac, v, vg, jc
end

# posterior function samples (sgp_sample_f), call for call with SGPDevice.sample_f: samples[:, k] = vec(mean) + L_C eps[:, k] with
# L_C L_C' = cov + sample_jitter I and the caller's standard normals eps (R × n_samples; the library holds no random state)
function sample_f(h::Handle, Xstar::Matrix{Float64}, eps::Matrix{Float64}, μ_v = nothing, Σ_v = nothing; sample_jitter::Float64 = 0.0,
                  noise::Bool = false)
    ns = size(Xstar, 2)
    R = ns * h.d_out
    size(eps, 1) == R || error("sample_f: eps must have ns * d_out = $R rows")
    n_samples = size(eps, 2)
    mean = zeros(ns, h.d_out)
    samples = zeros(R, n_samples)
    info = zeros(Int64, 3)
    μp = μ_v === nothing ? C_NULL : Vector{Float64}(μ_v)
    Σp = Σ_v === nothing ? C_NULL : Matrix{Float64}(Σ_v)
    check(ccall((:sgp_sample_f, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Int32, Float64, Ptr{Float64}, Int64,
                                            Ptr{Float64}, Ptr{Float64}, Ptr{Int64}),
                h.ptr, Xstar, ns, μp, Σp, Int32(noise ? 1 : 0), sample_jitter, eps, n_samples, mean, samples, info), h.ptr)
    return mean, samples
end

# pathwise (Matheron) posterior function samples (sgp_sample_path), call for call with SGPDevice.sample_path: ω (D × L) and phase (L)
# are the random Fourier features of the current kernel on 1/ℓ-scaled inputs, feat_w (L × d_out × n_samples) and eps_v (Q × n_samples)
# the caller's standard normals.  Returns samples R × n_samples, row (i - 1) ns + s output i at point s; the same four arrays give
# the same functions at any other points, and ns is not limited.  Like the rest of this file it has never been executed.
function sample_path(h::Handle, Xstar::Matrix{Float64}, ω::Matrix{Float64}, phase::Vector{Float64}, feat_w::Array{Float64,3},
                     eps_v::Matrix{Float64}, μ_v = nothing, Σ_v = nothing)
    ns = size(Xstar, 2)
    L = size(ω, 2)
    (length(phase) == L && size(feat_w, 1) == L && size(feat_w, 2) == h.d_out) || error("sample_path: ω, phase and feat_w disagree on L or d_out")
    n_samples = size(feat_w, 3)
    size(eps_v, 2) == n_samples || error("sample_path: eps_v must have n_samples = $n_samples columns")
    samples = zeros(ns * h.d_out, n_samples)
    info = zeros(Int64, 2)
    μp = μ_v === nothing ? C_NULL : Vector{Float64}(μ_v)
    Σp = Σ_v === nothing ? C_NULL : Matrix{Float64}(Σ_v)
    check(ccall((:sgp_sample_path, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32,
                                               Ptr{Float64}, Ptr{Float64}, Int64, Int32, Ptr{Float64}, Ptr{Int64}),
                h.ptr, Xstar, ns, μp, Σp, ω, phase, Int32(L), feat_w, eps_v, n_samples, Int32(0), samples, info), h.ptr)
    return samples
end

# the :in log-messages of many nodes and their moment-matched marginals in one call (include/sgp_hip.h, sgp_in_message): X is
# D × n, node t owns the columns node_start[t] + 1 : node_start[t + 1] (0-based offsets, n_nodes + 1 entries), y_mean is
# n_nodes × d_out; weights === nothing returns the closure values alone, else (logpdf, log_norm, mean D × n_nodes,
# cov D × D × n_nodes).  Like the rest of this file it has never been executed: only the ccall signature is stated here, no
# rule dispatches on it yet.
function in_message(h::Handle, X::Matrix{Float64}, node_start::Vector{Int64}, y_mean::Matrix{Float64}, weights = nothing,
                    μ_v = nothing, Σ_v = nothing)
    n = size(X, 2); n_nodes = length(node_start) - 1
    logpdf = zeros(n)
    log_norm = zeros(n_nodes); m = zeros(h.d, n_nodes); C = zeros(h.d, h.d, n_nodes)
    moments = weights !== nothing
    μp = μ_v === nothing ? C_NULL : Vector{Float64}(μ_v)
    Σp = Σ_v === nothing ? C_NULL : Matrix{Float64}(Σ_v)
    check(ccall((:sgp_in_message, LIB), Cint,
                (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Int64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                 Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                h.ptr, X, n, node_start, n_nodes, y_mean, moments ? Vector{Float64}(weights) : C_NULL, μp, Σp, logpdf,
                moments ? log_norm : C_NULL, moments ? m : C_NULL, moments ? C : C_NULL), h.ptr)
    return moments ? (logpdf, log_norm, m, C) : logpdf
end

# the :in log-messages with their analytic gradients and Hessians with respect to the input (include/sgp_hip.h,
# sgp_in_message_grad): what the Laplace form of @rule MultiSGP(:in) (GPnode/MultiSGPnode.jl:210-236) takes from ForwardDiff /
# Zygote, for the points of all nodes in one call.  X, node_start, y_mean, μ_v, Σ_v as in `in_message`; returns (logpdf n,
# grad D × n, hess D × D × n or nothing).  Written blind like the rest of this file, never executed: only the ccall signature is
# stated here, no rule dispatches on it yet (gaussianprocessnode_amd/multisgp.py, rule_in_laplace_batch, is the tested host loop).
function in_message_grad(h::Handle, X::Matrix{Float64}, node_start::Vector{Int64}, y_mean::Matrix{Float64}, μ_v = nothing,
                         Σ_v = nothing; hessian = true)
    n = size(X, 2); n_nodes = length(node_start) - 1
    logpdf = zeros(n); grad = zeros(h.d, n)
    hess = hessian ? zeros(h.d, h.d, n) : nothing
    μp = μ_v === nothing ? C_NULL : Vector{Float64}(μ_v)
    Σp = Σ_v === nothing ? C_NULL : Matrix{Float64}(Σ_v)
    check(ccall((:sgp_in_message_grad, LIB), Cint,
                (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Int64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                 Ptr{Float64}, Ptr{Float64}),
                h.ptr, X, n, node_start, n_nodes, y_mean, μp, Σp, logpdf, grad, hessian ? hess : C_NULL), h.ptr)
    return logpdf, grad, hess
end

# the :out message means of many nodes in one call (include/sgp_hip.h, sgp_out_message): X is D × n, node t owns the columns
# node_start[t] + 1 : node_start[t + 1] (0-based offsets, n_nodes + 1 entries); weights === nothing: every weight 1; μ_v === nothing:
# the handle's current posterior mean.  Returns mean n_nodes × d_out, or (mean, point_mean n × d_out) with points = true.  Written
# blind like the rest of this file, never executed: only the ccall signature is stated here, no rule dispatches on it yet
# (gaussianprocessnode_amd/multisgp.py, rule_out_batch, is the tested host function).
function out_message!(h::Handle, X::Matrix{Float64}, node_start::Vector{Int64}, weights = nothing, μ_v = nothing; points = false)
    n = size(X, 2); n_nodes = length(node_start) - 1
    mean = zeros(n_nodes, h.d_out)
    point_mean = points ? zeros(n, h.d_out) : nothing
    μp = μ_v === nothing ? C_NULL : Vector{Float64}(μ_v)
    check(ccall((:sgp_out_message, LIB), Cint,
                (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Int64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                h.ptr, X, n, node_start, n_nodes, weights === nothing ? C_NULL : Vector{Float64}(weights), μp, mean,
                points ? point_mean : C_NULL), h.ptr)
    return points ? (mean, point_mean) : mean
end

# the closed-form SE Psi-statistics of Gaussian inputs (include/sgp_hip.h, sgp_psi_stats): m is D × T, S is D × D × T or nothing
# (every S_t = 0), w === nothing: every node weight 1, μ_v === nothing: the handle's current posterior mean.  Returns (Ψ1 M × T,
# Ψ2 M × M = Σ_t w_t Ψ2_t, out_mean T × d_out).  Written blind like the rest of this file, never executed; a node whose S_t is not
# positive semi-definite comes back as status t + 1, which `check` rethrows as PosDefException(t + 1).
function psi_stats!(h::Handle, m::Matrix{Float64}, S = nothing, w = nothing, μ_v = nothing)
    T = size(m, 2)
    Ψ1 = zeros(h.m, T); Ψ2 = zeros(h.m, h.m); out = zeros(T, h.d_out)
    check(ccall((:sgp_psi_stats, LIB), Cint,
                (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                h.ptr, m, S === nothing ? C_NULL : Array{Float64,3}(S), T, w === nothing ? C_NULL : Vector{Float64}(w),
                μ_v === nothing ? C_NULL : Vector{Float64}(μ_v), Ψ1, Ψ2, out), h.ptr)
    return Ψ1, Ψ2, out
end
# the local phase of a sweep over those exact statistics (sgp_sweep_local_psi): y is T × d_out, y_var T or nothing; sweep_finish!
# follows.  The handle holds no data afterwards (set_data! before the next sweep!).
sweep_local_psi!(h::Handle, m::Matrix{Float64}, S, y::Matrix{Float64}, y_var = nothing; stream = C_NULL) =
    check(ccall((:sgp_sweep_local_psi, LIB), Cint,
                (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Cvoid}),
                h.ptr, m, S === nothing ? C_NULL : Array{Float64,3}(S), y, y_var === nothing ? C_NULL : Vector{Float64}(y_var),
                size(m, 2), stream), h.ptr)

# q(v) installed from outside for the per-point outputs (include/sgp_hip.h, sgp_set_posterior): mean and the upper factor
# Uv = chol(Σ_v + μ μ').U, column-major Q × Q -- a Julia Matrix as it is
set_posterior!(h::Handle, μ_v::Vector{Float64}, Uv::Matrix{Float64}) =
    check(ccall((:sgp_set_posterior, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), h.ptr, μ_v, Uv), h.ptr)
function kuu_chol(h::Handle)
    L = zeros(h.m, h.m)
    check(ccall((:sgp_get_kuu_chol, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}), h.ptr, L), h.ptr)
    return L
end
# stand-alone dense building blocks on the device (host in / host out): lower Cholesky factor, SPD inverse, K(A, B)
function potrf(A::Matrix{Float64}; device = 0)
    n = size(A, 1); L = zeros(n, n)
    check(ccall((:sgp_potrf, LIB), Cint, (Int32, Ptr{Float64}, Int32, Ptr{Float64}), device, A, n, L), C_NULL)
    return L
end
function potri(A::Matrix{Float64}; device = 0)
    n = size(A, 1); Ai = zeros(n, n)
    check(ccall((:sgp_potri, LIB), Cint, (Int32, Ptr{Float64}, Int32, Ptr{Float64}), device, A, n, Ai), C_NULL)
    return Ai
end
function kernelmatrix_dev(A::Matrix{Float64}, B::Matrix{Float64}, σ², ℓ::Vector{Float64}; device = 0,
                          kernel_family = SGP_KERNEL_SE)                                     # A: D × na, B: D × nb
    K = zeros(size(A, 2), size(B, 2))
    check(ccall((:sgp_kernelmatrix_family, LIB), Cint,
                (Int32, Int32, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Int32, Float64, Ptr{Float64}, Int32, Ptr{Float64}),
                device, kernel_family_id(kernel_family), A, size(A, 2), B, size(B, 2), size(A, 1), σ², ℓ, length(ℓ), K), C_NULL)
    return K
end

# ------------------------------------------------------------------------------------------------------------------
# UniSGP
# ------------------------------------------------------------------------------------------------------------------
mutable struct HipSGPMeta{R<:UniSGPMeta}
    ref::R                            # the reference's meta: Xu, kernel, N, and the `Uv` / `counter` fields the hook maintains
    handle::Handle
    kernel_params::Function           # θ -> (σ², ℓ::Vector{Float64}) of `ref.kernel`
    jitter::Float64
    xs::Vector{Vector{Float64}}       # points of the batch being folded
    ys::Vector{Float64}
    vs::Vector{Float64}
    prior::Any
    w::Float64
    Elogw::Float64
    θ::Vector{Float64}
    index::Dict{Vector{Float64},Int}  # point -> column of the last swept batch
    I1::Vector{Float64}               # per-point :w quantities of the last sweep (fetched on first use)
    I2::Vector{Float64}
    ωs::Vector{Float64}               # cubature weights of the batch being folded (uncertain inputs: one entry per cubature point)
    uncertain::Bool                   # the batch being folded consists of uncertain-input nodes (GPnode/UniSGPnode.jl:125-140)
    aux::Union{Nothing,Handle}        # second handle for stand-alone rule evaluations (it replaces data and posterior)
    device::Int
    μ_last::Vector{Float64}           # mean of the last swept q(v): the per-point pass belongs to it
end

function HipSGPMeta(ref::UniSGPMeta; kernel_params, jitter = 0.0, device = 0, cubature_points = 21, reuse_stats = false,
                    kernel_family = :se)
    # (uncertain inputs enter the sweep as `cubature_points` weighted points per node: size the handle for them)
    # reuse_stats: SGP_FLAG_REUSE_STATS -- sweeps at unchanged kernel and inputs reuse K_uf, Psi2 and the K_uu factor
    # kernel_family: the base kernel of ref.kernel(θ) (:se, :matern12, :matern32, :matern52, or a kernel object such as
    # ref.kernel(θ0)); kernel_params maps θ exactly as for SE
    flags = SGP_FLAG_KEEP_KUF | (reuse_stats ? SGP_FLAG_REUSE_STATS : 0)
    h = Handle(ref.N * max(1, cubature_points), inducing_matrix(ref.Xu), 1; device = device, flags = flags,
               family = kernel_family_id(kernel_family))
    return HipSGPMeta(ref, h, kernel_params, Float64(jitter), Vector{Float64}[], Float64[], Float64[], nothing, 1.0, 0.0,
                      Float64[], Dict{Vector{Float64},Int}(), Float64[], Float64[], Float64[], false, nothing, device, Float64[])
end

# the token the per-point :v rule returns instead of an M × M message (replaces BufferUniSGP, GPnode/UniSGPnode.jl:56-60)
struct HipBuffer{T<:HipSGPMeta}
    index::Int
    meta::T
end

point(q) = collect(Float64, mean(q) isa Number ? [mean(q)] : mean(q))
elog(q_w) = q_w isa GammaShapeRate ? mean(log, q_w) : log(mean(q_w))

# ---- :v  (GPnode/UniSGPnode.jl:144-158 PointMass output, :161-173 Gaussian output): O(1) token -------------------
function push_point!(meta::HipSGPMeta, q_out, q_in, q_w, q_θ)
    push!(meta.xs, point(q_in)); push!(meta.ys, mean(q_out)); push!(meta.vs, q_out isa PointMass ? 0.0 : var(q_out))
    meta.w = mean(q_w); meta.Elogw = elog(q_w); meta.θ = collect(Float64, mean(q_θ))
    return HipBuffer(length(meta.xs), meta)
end
@rule UniSGP(:v, Marginalisation) (q_out::PointMass, q_in::PointMass, q_w::Any, q_θ::PointMass, meta::HipSGPMeta) =
    push_point!(meta, q_out, q_in, q_w, q_θ)
@rule UniSGP(:v, Marginalisation) (q_out::UnivariateGaussianDistributionsFamily, q_in::PointMass, q_w::Any, q_θ::PointMass, meta::HipSGPMeta) =
    push_point!(meta, q_out, q_in, q_w, q_θ)

# ---- the N-fold product (GPnode/UniSGPnode.jl:62-73): one device sweep when counter == N -------------------------
function ReactiveMP.prod(::GenericProd, left::NormalDistributionsFamily, right::HipBuffer)
    meta = right.meta; ref = meta.ref
    ref.counter += 1                                           # :63-64
    ref.counter == 1 && (meta.prior = left)
    ref.counter < ref.N && return meta.prior                   # nothing consumes the partial products
    h = meta.handle
    X = reduce(hcat, meta.xs)
    μ0, Σ0 = mean_cov(meta.prior)
    if meta.uncertain
        # cubature points as weighted data, N nodes (unisgp.py:138-147); every one of the N messages carries Ψ2 + 1e-8 I
        # (GPnode/UniSGPnode.jl:135,138): the prior's precision gains 1e-8 w N on the diagonal
        set_data!(h, X, meta.ys, nothing, meta.ωs, Float64(ref.N))
        Λ0 = potri(Matrix{Float64}(Σ0); device = meta.device)
        ξ0 = Λ0 * collect(Float64, μ0)
        Λ0 += 1e-8 * meta.w * ref.N * I
        set_prior!(h, ξ0, Matrix{Float64}(Λ0), 1)
    else
        set_data!(h, X, meta.ys, any(!iszero, meta.vs) ? meta.vs : nothing, nothing, -1.0)
        set_prior!(h, collect(Float64, μ0), Matrix{Float64}(Σ0), 0)
    end
    σ², ℓ = meta.kernel_params(meta.θ)
    set_kernel!(h, σ², collect(Float64, ℓ), meta.jitter)
    set_noise!(h, fill(meta.w, 1, 1), meta.Elogw)
    sweep!(h)
    μ, Σ, Uv = posterior(h)
    ref.Uv = UpperTriangular(Uv)                               # :67-69  meta.Uv = chol(Σ + μμ').U
    ref.KuuL = LowerTriangular(kuu_chol(h))                    # (the cold rules read meta.KuuL: the factor this sweep used)
    ref.counter = 0                                            # :70
    meta.index = meta.uncertain ? Dict{Vector{Float64},Int}() : Dict(x => i for (i, x) in enumerate(meta.xs))
    meta.I1 = Float64[]; meta.I2 = Float64[]; meta.μ_last = copy(μ)
    empty!(meta.xs); empty!(meta.ys); empty!(meta.vs); empty!(meta.ωs); meta.uncertain = false
    return MvNormalMeanCovariance(μ, Σ)
end

# ---- :v with an uncertain input (GPnode/UniSGPnode.jl:125-140): the node's cubature points join the batch as weighted data --
cubature_1d(meta::HipSGPMeta, q_in) = (m = mean(q_in); v = var(q_in);
    (collect(Float64, ReactiveMP.getpoints(meta.ref.method, m, v)), collect(Float64, ReactiveMP.getweights(meta.ref.method, m, v))))
@rule UniSGP(:v, Marginalisation) (q_out::UnivariateNormalDistributionsFamily, q_in::UnivariateNormalDistributionsFamily, q_w::Any, q_θ::PointMass, meta::HipSGPMeta) = begin
    isempty(meta.xs) || meta.uncertain || error("PointMass and uncertain inputs mixed in one graph")
    pts, ω = cubature_1d(meta, q_in)
    for (p, wt) in zip(pts, ω)
        push!(meta.xs, [p]); push!(meta.ys, mean(q_out)); push!(meta.vs, 0.0); push!(meta.ωs, wt)
    end
    meta.uncertain = true
    meta.w = mean(q_w); meta.Elogw = elog(q_w); meta.θ = collect(Float64, mean(q_θ))
    return HipBuffer(length(meta.xs), meta)
end

# ---- :w and the average energy at PointMass inputs (GPnode/UniSGPnode.jl:196-238, 337-387, 411-436) ---------------
# (I1_n, I2_n) of one node: from the per-point pass over the last swept batch when the point and q_v belong to it, else
# evaluated stand-alone at (q_v, meta.Uv) like the reference's rule would (unisgp.py: _point_stats)
function point_stats(q_out, q_in::PointMass, q_v, q_θ, meta::HipSGPMeta)
    x = point(q_in)
    if haskey(meta.index, x) && isapprox(collect(Float64, mean(q_v)), meta.μ_last; rtol = 1e-12, atol = 0)
        isempty(meta.I1) && ((meta.I1, meta.I2) = w_stats(meta.handle, length(meta.index)))
        i = meta.index[x]
        return meta.I1[i], meta.I2[i]
    end
    yv = q_out isa PointMass ? nothing : [Float64(var(q_out))]
    I1, I2 = stats_at(meta, mean(q_θ), reshape(x, :, 1), [Float64(mean(q_out))], yv, collect(Float64, mean(q_v)), Matrix{Float64}(meta.ref.Uv))
    return I1[1], I2[1]
end
@rule UniSGP(:w, Marginalisation) (q_out::PointMass, q_in::PointMass, q_v::MultivariateNormalDistributionsFamily, q_θ::PointMass, meta::HipSGPMeta) =
    (I = point_stats(q_out, q_in, q_v, q_θ, meta); GammaShapeRate(1.5, 0.5 * (I[1] + I[2])))
@rule UniSGP(:w, Marginalisation) (q_out::UnivariateGaussianDistributionsFamily, q_in::PointMass, q_v::MultivariateNormalDistributionsFamily, q_θ::PointMass, meta::HipSGPMeta) =
    (I = point_stats(q_out, q_in, q_v, q_θ, meta); GammaShapeRate(1.5, 0.5 * (I[1] + I[2])))

hip_energy(q_out, q_in, q_v, q_w, q_θ, meta) = (I = point_stats(q_out, q_in, q_v, q_θ, meta); w = mean(q_w); 0.5 * (I[1] * w - elog(q_w) + log(2π) + I[2] * w))
@average_energy UniSGP (q_out::PointMass, q_in::PointMass, q_v::MultivariateNormalDistributionsFamily, q_w::GammaShapeRate, q_θ::PointMass, meta::HipSGPMeta) = hip_energy(q_out, q_in, q_v, q_w, q_θ, meta)
@average_energy UniSGP (q_out::UnivariateGaussianDistributionsFamily, q_in::PointMass, q_v::MultivariateNormalDistributionsFamily, q_w::GammaShapeRate, q_θ::PointMass, meta::HipSGPMeta) = hip_energy(q_out, q_in, q_v, q_w, q_θ, meta)
@average_energy UniSGP (q_out::PointMass, q_in::PointMass, q_v::MultivariateNormalDistributionsFamily, q_w::PointMass, q_θ::PointMass, meta::HipSGPMeta) = hip_energy(q_out, q_in, q_v, q_w, q_θ, meta)
@average_energy UniSGP (q_out::UnivariateGaussianDistributionsFamily, q_in::PointMass, q_v::MultivariateNormalDistributionsFamily, q_w::PointMass, q_θ::PointMass, meta::HipSGPMeta) = hip_energy(q_out, q_in, q_v, q_w, q_θ, meta)

# ---- :out at a PointMass input (GPnode/UniSGPnode.jl:96-104); `predict` does a whole test set in one call ---------
@rule UniSGP(:out, Marginalisation) (q_in::PointMass, q_v::MultivariateNormalDistributionsFamily, q_w::Any, q_θ::PointMass, meta::HipSGPMeta) = begin
    m = predict(meta, reshape(point(q_in), :, 1), collect(Float64, mean(q_v)), mean(q_θ))
    return NormalMeanPrecision(m[1], mean(q_w))
end
function predict(meta::HipSGPMeta, Xstar::Matrix{Float64}, μ_v::Vector{Float64}, θ)      # experiments/regression_kin40k.ipynb:288-304
    σ², ℓ = meta.kernel_params(θ)
    set_kernel!(meta.handle, σ², collect(Float64, ℓ), meta.jitter)
    return vec(predict_mean(meta.handle, Xstar, μ_v))
end
# predictive mean and variance of y = f + noise at the explicit q(v) (unisgp.py `predictive`): (means, variances), ns each
function predictive(meta::HipSGPMeta, Xstar::Matrix{Float64}, q_v, θ; w̄::Float64)
    σ², ℓ = meta.kernel_params(θ)
    set_kernel!(meta.handle, σ², collect(Float64, ℓ), meta.jitter)
    set_noise!(meta.handle, fill(w̄, 1, 1), log(w̄))
    μ_v, Σ_v = mean_cov(q_v)
    m, v = predict_var(meta.handle, Xstar, μ_v, Σ_v; noise = true)
    return vec(m), v
end

# ---- the cold rules, device-backed (unisgp.py:183-387; VERDICT r3 item 7) -----------------------------------------------
# Stand-alone per-point (I1_n, I2_n) of GPnode/UniSGPnode.jl:196-238 for arbitrary points X (D × n), at kernel(θ) and at the
# q(v) given by (μ_v, Uv = chol(Σ_v + μ μ').U): K_uu chain and K_uf on the device, then the per-point quadratic forms.  On an
# auxiliary handle: the main one holds the last swept batch.
function aux_handle!(meta::HipSGPMeta, n::Int)
    if meta.aux === nothing || meta.aux.n_max < n
        meta.aux = Handle(max(n, 64), inducing_matrix(meta.ref.Xu), 1; device = meta.device, family = meta.handle.family)
    end
    return meta.aux
end
function stats_at(meta::HipSGPMeta, θ, X::Matrix{Float64}, y::Vector{Float64}, yv, μ_v::Vector{Float64}, Uv)
    h = aux_handle!(meta, size(X, 2))
    set_data!(h, X, y, yv, nothing, -1.0)
    σ², ℓ = meta.kernel_params(θ)
    set_kernel!(h, σ², collect(Float64, ℓ), meta.jitter)
    sweep_local!(h)
    set_posterior!(h, μ_v, Matrix{Float64}(Uv))
    return w_stats(h, size(X, 2))
end
# chol(Σ_v + μ μ').U of an explicit q_v, factored on the device
uv_of(q_v, meta::HipSGPMeta) = (μ = mean(q_v); Matrix(potrf(Matrix{Float64}(cov(q_v) + μ * μ'); device = meta.device)'))

# (I1, I2) of ONE node whose input is uncertain: Ψ-statistics by the meta's cubature, Ψ2 + jitter_psi2 I, clamped like the
# reference (GPnode/UniSGPnode.jl:186-190)
function node_I(q_out, q_in, μ_v, Uv, θ, meta::HipSGPMeta, jitter_psi2, clamped)
    pts, ω = cubature_1d(meta, q_in)
    μ_y = mean(q_out); v_y = q_out isa PointMass ? 0.0 : var(q_out)
    I1q, I2q = stats_at(meta, θ, reshape(pts, 1, :), fill(Float64(μ_y), length(ω)), nothing, collect(Float64, μ_v), Uv)
    I1 = dot(ω, I1q)
    I2 = dot(ω, I2q) + μ_y^2 * (1.0 - sum(ω)) + v_y
    if jitter_psi2 != 0
        KuuL = Matrix{Float64}(meta.ref.KuuL)
        I1 -= jitter_psi2 * tr(potri(KuuL * KuuL'; device = meta.device))      # tr(Kuu^-1 (jitter I))
        I2 += jitter_psi2 * sum(abs2, Uv)                                      # tr(Uv'Uv (jitter I))
    end
    clamped && ((I1, I2) = (clamp(I1, 1e-12, 1e12), clamp(I2, 1e-12, 1e12)))
    return I1, I2
end

# :out with an uncertain input (GPnode/UniSGPnode.jl:85-93): Ψ1 = Σ_s ω_s K(Xu, x_s), mean = Ψ1 · μ_v
@rule UniSGP(:out, Marginalisation) (q_in::UnivariateGaussianDistributionsFamily, q_v::MultivariateNormalDistributionsFamily, q_w::Any, q_θ::PointMass, meta::HipSGPMeta) = begin
    pts, ω = cubature_1d(meta, q_in)
    f = predict(meta, reshape(pts, 1, :), collect(Float64, mean(q_v)), mean(q_θ))
    return NormalMeanPrecision(dot(ω, f), mean(q_w))
end
# :w with an uncertain input (GPnode/UniSGPnode.jl:177-192): meta.Uv, Ψ2 + 1e-8 I, clamped
@rule UniSGP(:w, Marginalisation) (q_out::UnivariateGaussianDistributionsFamily, q_in::UnivariateGaussianDistributionsFamily, q_v::MultivariateNormalDistributionsFamily, q_θ::PointMass, meta::HipSGPMeta) =
    (I = node_I(q_out, q_in, mean(q_v), Matrix{Float64}(meta.ref.Uv), mean(q_θ), meta, 1e-8, true); GammaShapeRate(1.5, 0.5 * (I[1] + I[2])))
# average energy with an uncertain input: Gamma q_w (GPnode/UniSGPnode.jl:290-313: meta.KuuL / meta.Uv, Ψ2 + 1e-8 I, clamped) and
# PointMass q_w (:390-409: Σ_v + μ μ' from q_v itself; the reference's `.+ 1e-8` on every entry is not reproduced, < 1e-6)
@average_energy UniSGP (q_out::UnivariateNormalDistributionsFamily, q_in::UnivariateGaussianDistributionsFamily, q_v::MultivariateNormalDistributionsFamily, q_w::GammaShapeRate, q_θ::PointMass, meta::HipSGPMeta) = begin
    I1, I2 = node_I(q_out, q_in, mean(q_v), Matrix{Float64}(meta.ref.Uv), mean(q_θ), meta, 1e-8, true)
    w = mean(q_w)
    return 0.5 * (I1 * w - elog(q_w) + log(2π) + I2 * w)
end
@average_energy UniSGP (q_out::UnivariateNormalDistributionsFamily, q_in::UnivariateGaussianDistributionsFamily, q_v::MultivariateNormalDistributionsFamily, q_w::PointMass, q_θ::PointMass, meta::HipSGPMeta) = begin
    I1, I2 = node_I(q_out, q_in, mean(q_v), uv_of(q_v, meta), mean(q_θ), meta, 0.0, true)
    w = mean(q_w)
    return 0.5 * (I1 * w - elog(q_w) + log(2π) + I2 * w)
end
# :in (GPnode/UniSGPnode.jl:107-122): x -> -w/2 A(x) + w μ_y B(x)·μ_v - w/2 |Uv B(x)|² = -w/2 (I1(x) + I2(x) - μ_y²), every
# evaluation one device pass (K_uu chain, K_uf column, the two quadratic forms); meta.Uv as the reference's rule reads it
@rule UniSGP(:in, Marginalisation) (q_out::UnivariateNormalDistributionsFamily, q_v::MultivariateNormalDistributionsFamily, q_w::Any, q_θ::PointMass, meta::HipSGPMeta) = begin
    w = mean(q_w); μ_y = mean(q_out); μ_v = collect(Float64, mean(q_v)); θ = mean(q_θ); Uv = Matrix{Float64}(meta.ref.Uv)
    log_backwardmess = (x) -> begin
        I1, I2 = stats_at(meta, θ, reshape(collect(Float64, x), :, 1), [Float64(μ_y)], nothing, μ_v, Uv)
        -0.5 * w * (I1[1] + I2[1] - μ_y^2)
    end
    return ContinuousUnivariateLogPdf(log_backwardmess)
end
# :θ (GPnode/UniSGPnode.jl:242-287, three methods): θ -> w μ_y Ψ1(θ)·μ_v - w/2 (Ψ0(θ) + tr(Ψ2(θ) (Rv - Kuu^-1(θ))))
#    = -w/2 (Σ_q ω_q (I1_q + I2_q) - μ_y² Σ_q ω_q),   Rv from q_v itself
function theta_closure(q_out, q_in, q_v, q_w, meta::HipSGPMeta)
    w = mean(q_w); μ_y = Float64(mean(q_out)); μ_v = collect(Float64, mean(q_v)); Uv = uv_of(q_v, meta)
    pts, ω = q_in isa PointMass ? (point(q_in), [1.0]) : cubature_1d(meta, q_in)
    X = q_in isa PointMass ? reshape(pts, :, 1) : reshape(pts, 1, :)
    log_backwardmess = (θ) -> begin
        I1, I2 = stats_at(meta, θ, X, fill(μ_y, length(ω)), nothing, μ_v, Uv)
        -0.5 * w * (dot(ω, I1 .+ I2) - μ_y^2 * sum(ω))
    end
    return ContinuousMultivariateLogPdf(UnspecifiedDomain(), log_backwardmess)
end
@rule UniSGP(:θ, Marginalisation) (q_out::PointMass, q_in::PointMass, q_v::MultivariateNormalDistributionsFamily, q_w::Any, meta::HipSGPMeta) =
    theta_closure(q_out, q_in, q_v, q_w, meta)
@rule UniSGP(:θ, Marginalisation) (q_out::UnivariateGaussianDistributionsFamily, q_in::PointMass, q_v::MultivariateNormalDistributionsFamily, q_w::Any, meta::HipSGPMeta) =
    theta_closure(q_out, q_in, q_v, q_w, meta)
@rule UniSGP(:θ, Marginalisation) (q_out::UnivariateNormalDistributionsFamily, q_in::UnivariateNormalDistributionsFamily, q_v::MultivariateGaussianDistributionsFamily, q_w::Any, meta::HipSGPMeta) =
    theta_closure(q_out, q_in, q_v, q_w, meta)
# (The Gaussian × log-pdf product of GPnode/UniSGPnode.jl:39-54 dispatches on the message types, not on the meta: the reference's
# own method applies unchanged -- its 21 closure evaluations are 21 device passes.)

# ---- hyper-parameter objective and gradient (neg_log_backwardmess_fast / grad_llh_new!,
# helper_functions/derivative_helper.jl:23-39,55-63) at the θ of the last sweep, q(v) fixed ---------------------------
# Returns (F, dF/d(σ², ℓ...)); the caller applies the chain rule of its kernel_gp(θ) (softplus in the notebooks).
function theta_objective(meta::HipSGPMeta, nparams::Int)
    f = Ref{Float64}(0.0); g = zeros(nparams)
    check(ccall((:sgp_theta_objective, LIB), Cint, (Ptr{Cvoid}, Ref{Float64}, Ptr{Float64}), meta.handle.ptr, f, g), meta.handle.ptr)
    return f[], g
end
# The same value and gradient and, behind them, dF/dXu at the resident inducing inputs (sgp_theta_objective_xu): D × M, the
# layout of the handle's Xu.  q(v) is held: moving z_m reinterprets v_m as the function value at the new location.
function theta_objective_xu(meta::HipSGPMeta, nparams::Int)
    h = meta.handle
    f = Ref{Float64}(0.0); g = zeros(nparams); gxu = zeros(h.d, h.m)
    check(ccall((:sgp_theta_objective_xu, LIB), Cint, (Ptr{Cvoid}, Ref{Float64}, Ptr{Float64}, Ptr{Float64}), h.ptr, f, g, gxu), h.ptr)
    return f[], g, gxu
end

# Greedy inducing-input selection (include/sgp_hip.h, sgp_select_inducing): up to m of the columns of X (D × n) at the handle's
# current kernel, by partial pivoted Cholesky of K_ff.  Returns (idx, trace): idx the picks in order, 1-based (columns of X), trace[j + 1]
# = tr(K_ff - Q_ff) of the first j picks; both cut at the number of picks made (tol, min_var stop early).  Nothing of the handle changes:
# X[:, idx] is the Xu to create the next Handle with (or to pass to sgp_set_inducing on this one).
function select_inducing(meta, X::Matrix{Float64}, m::Integer; tol::Float64 = 0.0,     # meta: HipSGPMeta or HipMultiSGPMeta
                         min_var::Float64 = 1e-12)
    h = meta.handle
    idx = fill(Int64(-1), max(m, 1)); trace = fill(NaN, max(m, 1) + 1); count = Ref{Int32}(0)
    check(ccall((:sgp_select_inducing, LIB), Cint,
                (Ptr{Cvoid}, Ptr{Float64}, Int64, Int32, Float64, Float64, Ptr{Int64}, Ptr{Float64}, Ref{Int32}),
                h.ptr, X, size(X, 2), Int32(m), tol, min_var, idx, trace, count), h.ptr)
    return idx[1:count[]] .+ 1, trace[1:count[]+1]
end

# ---- minibatch loops (experiments/regression_kin40k.ipynb:205-212): prior <- posterior without leaving the device --
carry_posterior!(meta::HipSGPMeta) =
    check(ccall((:sgp_carry_posterior, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), meta.handle.ptr, C_NULL), meta.handle.ptr)

# ---- the whole PerformInference loop on the device (experiments/regression_kin40k.ipynb:196-230; sgp_train_*) -------
# X is D × N (one point per column), θ the raw (pre-softplus) parameters of kernel_gp.  Returns θ after the last step.
function train!(meta::HipSGPMeta, X::Matrix{Float64}, y::Vector{Float64}, θ::Vector{Float64}; batch, epochs, w, prior_var = 50.0,
                η = 1e-3, β = (0.9, 0.999), ϵ = 1e-8)
    h = meta.handle; N = length(y)
    set_noise!(h, fill(Float64(w), 1, 1), log(w))
    set_prior!(h, C_NULL, fill(Float64(prior_var), 1, 1), 2)
    check(ccall((:sgp_train_begin, LIB), Cint,
                (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Int32, Float64, Float64, Float64, Float64, Float64),
                h.ptr, X, y, N, θ, length(θ) - 1, meta.jitter, η, β[1], β[2], ϵ), h.ptr)
    for _ in 1:epochs, o in 0:batch:N-1
        flags = Int32(1) | (o == 0 ? Int32(2) : Int32(0))       # SGP_TRAIN_LEARN | SGP_TRAIN_RESET_PRIOR (:203-204)
        check(ccall((:sgp_train_step, LIB), Cint, (Ptr{Cvoid}, Int64, Int64, Int32), h.ptr, o, min(batch, N - o), flags), h.ptr)
    end
    θout = similar(θ); counts = zeros(Int64, 2)
    check(ccall((:sgp_train_end, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Int64}), h.ptr, θout, counts), h.ptr)
    counts[2] == 0 || throw(PosDefException(Int(counts[2])))
    return θout
end

# ---- phase 2 of the pendulum's PerformInference (experiments/Pendulum_Wishart_2d.ipynb cell 16) on the device: `steps` times
# grad_llh_multi! (grad_llh_new! on a UniSGP handle) + Flux.Optimise.update!(AdaMax, θ, grad) at the held q(v), data and noise
# (sgp_theta_descend).  θ: the raw (pre-softplus) parameters of kernel_gp, updated in place.  `state` = [m | u | β1^t, β2^t]
# (2 length(θ) + 2 entries) carries the optimiser from call to call, as the notebook's single Flux.AdaMax() does; `nothing` starts
# from zero moments and returns none.  Returns (θ, values, steps_taken); PosDefException(k) when K_uu failed at some θ_k (θ and
# `state` are then those of that step).
function theta_descend!(meta::HipSGPMeta, θ::Vector{Float64}, steps::Integer; η = 1e-3, β = (0.9, 0.999), ϵ = 1e-8,
                        state::Union{Nothing, Vector{Float64}} = nothing)
    h = meta.handle
    state === nothing || length(state) == 2 * length(θ) + 2 || throw(ArgumentError("theta_descend!: state needs 2 length(θ) + 2 entries"))
    values = fill(NaN, max(steps, 0)); counts = zeros(Int64, 2)
    check(ccall((:sgp_theta_descend, LIB), Cint,
                (Ptr{Cvoid}, Ptr{Float64}, Int32, Int32, Float64, Float64, Float64, Float64, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}),
                h.ptr, θ, length(θ) - 1, steps, η, β[1], β[2], ϵ, state === nothing ? C_NULL : state, values, counts), h.ptr)
    return θ, values, Int(counts[1])
end

# ---- device-paced VMP iterations with the free energy (sgp_vmp_run): `infer(iterations = K, free_energy = true)` over the resident
# data.  likelihood 0 Gaussian, 1 Probit (labels in {0, 1}); γ0 = (shape0, rate0), γ = q(w) entering the run (in/out; nothing with
# hold_w = true, which keeps the last set_noise); μ_init the mean of the first Probit forward message (nothing: 0).  Returns
# (values, terms, γ, iterations_done, converged); PosDefException(k) when K_uu or Λ failed (values from that iteration on are NaN).
function vmp_run!(meta::HipSGPMeta, iterations::Integer; likelihood::Integer = 0, γ0 = nothing, γ = nothing, μ_init = nothing,
                  tol = 0.0, hold_w::Bool = false)
    h = meta.handle
    hold_w || γ0 !== nothing || throw(ArgumentError("vmp_run!: γ0 = (shape0, rate0) is required without hold_w"))
    g0 = hold_w ? nothing : Float64[γ0[1], γ0[2]]
    g = hold_w ? nothing : (γ === nothing ? copy(g0) : Float64[γ[1], γ[2]])
    values = fill(NaN, max(iterations, 0)); terms = fill(NaN, 4, max(iterations, 0)); counts = zeros(Int64, 2)
    check(ccall((:sgp_vmp_run, LIB), Cint,
                (Ptr{Cvoid}, Int32, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Float64, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}),
                h.ptr, likelihood, hold_w ? 1 : 0, iterations, g0 === nothing ? C_NULL : g0, g === nothing ? C_NULL : g,
                μ_init === nothing ? C_NULL : μ_init, tol, values, terms, counts), h.ptr)
    return values, terms, g, Int(counts[1]), counts[2] == 1
end

# ---- device-paced VMP iterations of Student-t regression (sgp_vmp_run_t): y_i ~ N(f_i, 1 / (w τ_i)), τ_i ~ Gamma(ν/2, ν/2).  The handle
# needs SGP_FLAG_KEEP_KUF.  β: the rates of q(τ_i) entering the run (in/out; nothing: (ν + 1) / 2, none returned); γ0, γ, tol, hold_w as
# in vmp_run!.  Returns (values, terms, γ, β, iterations_done, converged).
function vmp_run_t!(meta::HipSGPMeta, iterations::Integer, ν::Real; β = nothing, γ0 = nothing, γ = nothing, tol = 0.0, hold_w::Bool = false)
    h = meta.handle
    hold_w || γ0 !== nothing || throw(ArgumentError("vmp_run_t!: γ0 = (shape0, rate0) is required without hold_w"))
    g0 = hold_w ? nothing : Float64[γ0[1], γ0[2]]
    g = hold_w ? nothing : (γ === nothing ? copy(g0) : Float64[γ[1], γ[2]])
    values = fill(NaN, max(iterations, 0)); terms = fill(NaN, 4, max(iterations, 0)); counts = zeros(Int64, 2)
    check(ccall((:sgp_vmp_run_t, LIB), Cint,
                (Ptr{Cvoid}, Float64, Ptr{Float64}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Float64, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}),
                h.ptr, ν, β === nothing ? C_NULL : β, hold_w ? 1 : 0, iterations, g0 === nothing ? C_NULL : g0, g === nothing ? C_NULL : g,
                tol, values, terms, counts), h.ptr)
    return values, terms, g, β, Int(counts[1]), counts[2] == 1
end

# ---- the same objective and descent over the exact Psi-statistics of Gaussian inputs x_t ~ N(m_t, S_t) (SE kernel only;
# sgp_theta_objective_psi, sgp_theta_descend_psi): m is D × T, S is D × D × T or nothing (S = 0), y is T × d_out.  No resident data are
# needed; q(v) and W are the handle's.  theta_objective_psi returns (value, gradient w.r.t. (σ², ℓ...)); theta_descend_psi! is
# theta_descend! on it.  PosDefException(t + 1) names an indefinite node, PosDefException(k) a K_uu that failed.
function theta_objective_psi(h::Handle, m::Matrix{Float64}, S, y::Matrix{Float64}, n_ell::Integer)
    T = size(m, 2); value = Ref{Float64}(0.0); grad = zeros(1 + n_ell); info = zeros(Int64, 2)
    check(ccall((:sgp_theta_objective_psi, LIB), Cint,
                (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}),
                h.ptr, m, S === nothing ? C_NULL : S, y, T, value, grad, info), h.ptr)
    return value[], grad
end

# The same value and gradient and, behind them, dF/dXu at the resident inducing inputs (sgp_theta_objective_psi_xu): D × M, the
# column-major image of the M × D row-major array the ABI writes.  q(v), W, θ and the Gaussian inputs are held.
function theta_objective_psi_xu(h::Handle, m::Matrix{Float64}, S, y::Matrix{Float64}, n_ell::Integer, M::Integer)
    D, T = size(m); value = Ref{Float64}(0.0); grad = zeros(1 + n_ell); gxu = zeros(D, M); info = zeros(Int64, 2)
    check(ccall((:sgp_theta_objective_psi_xu, LIB), Cint,
                (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}),
                h.ptr, m, S === nothing ? C_NULL : S, y, T, value, grad, gxu, info), h.ptr)
    return value[], grad, gxu
end

function theta_descend_psi!(meta::HipSGPMeta, m::Matrix{Float64}, S, y::Matrix{Float64}, θ::Vector{Float64}, steps::Integer;
                            η = 1e-3, β = (0.9, 0.999), ϵ = 1e-8, state::Union{Nothing, Vector{Float64}} = nothing)
    h = meta.handle
    state === nothing || length(state) == 2 * length(θ) + 2 || throw(ArgumentError("theta_descend_psi!: state needs 2 length(θ) + 2 entries"))
    values = fill(NaN, max(steps, 0)); counts = zeros(Int64, 3)
    check(ccall((:sgp_theta_descend_psi, LIB), Cint,
                (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Int32, Int32, Float64, Float64, Float64,
                 Float64, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}),
                h.ptr, m, S === nothing ? C_NULL : S, y, size(m, 2), θ, length(θ) - 1, steps, η, β[1], β[2], ϵ,
                state === nothing ? C_NULL : state, values, counts), h.ptr)
    return θ, values, Int(counts[1])
end

# Device-paced AdaMax in the inducing inputs at a held q(v) (sgp_inducing_descend, sgp_inducing_descend_psi): on [θ | vec Xu], or on
# Xu alone with learn_theta = false.  Xu is D × M (column m is inducing point m: the memory layout sgp_set_inducing takes); θ and Xu are
# updated in place.  state: [m | u | β1^t, β2^t] of the joint vector, 2 P + 2 entries with P = (learn_theta ? length(θ) : 0) + D M.
# Returns (θ, Xu, values, steps taken); afterwards the handle's kernel is softplus(θ) and its inducing inputs are Xu.
function inducing_descend!(meta::HipSGPMeta, θ::Vector{Float64}, Xu::Matrix{Float64}, steps::Integer; learn_theta::Bool = true,
                           η = 1e-3, β = (0.9, 0.999), ϵ = 1e-8, state::Union{Nothing, Vector{Float64}} = nothing)
    h = meta.handle
    P = (learn_theta ? length(θ) : 0) + length(Xu)
    state === nothing || length(state) == 2 * P + 2 || throw(ArgumentError("inducing_descend!: state needs 2 P + 2 entries"))
    values = fill(NaN, max(steps, 0)); counts = zeros(Int64, 2)
    check(ccall((:sgp_inducing_descend, LIB), Cint,
                (Ptr{Cvoid}, Ptr{Float64}, Int32, Ptr{Float64}, Int32, Int32, Float64, Float64, Float64, Float64, Ptr{Float64},
                 Ptr{Float64}, Ptr{Int64}),
                h.ptr, θ, length(θ) - 1, Xu, learn_theta ? 3 : 2, steps, η, β[1], β[2], ϵ, state === nothing ? C_NULL : state, values,
                counts), h.ptr)
    return θ, Xu, values, Int(counts[1])
end

function inducing_descend_psi!(meta::HipSGPMeta, m::Matrix{Float64}, S, y::Matrix{Float64}, θ::Vector{Float64}, Xu::Matrix{Float64},
                               steps::Integer; learn_theta::Bool = true, η = 1e-3, β = (0.9, 0.999), ϵ = 1e-8,
                               state::Union{Nothing, Vector{Float64}} = nothing)
    h = meta.handle
    P = (learn_theta ? length(θ) : 0) + length(Xu)
    state === nothing || length(state) == 2 * P + 2 || throw(ArgumentError("inducing_descend_psi!: state needs 2 P + 2 entries"))
    values = fill(NaN, max(steps, 0)); counts = zeros(Int64, 3)
    check(ccall((:sgp_inducing_descend_psi, LIB), Cint,
                (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Int32, Ptr{Float64}, Int32, Int32, Float64,
                 Float64, Float64, Float64, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}),
                h.ptr, m, S === nothing ? C_NULL : S, y, size(m, 2), θ, length(θ) - 1, Xu, learn_theta ? 3 : 2, steps, η, β[1], β[2], ϵ,
                state === nothing ? C_NULL : state, values, counts), h.ptr)
    return θ, Xu, values, Int(counts[1])
end

# ---- the exact-Psi input messages (sgp_psi_in_grad; SE kernel only, D <= 8): per node t with input x_t ~ N(m_t, S_t) the part U_t of its
# average energy that depends on the input, γ_t = ∂U_t/∂m_t and Γ_t = ∂U_t/∂S_t (symmetric).  m is D × T, S is D × D × T or nothing
# (S = 0), y is T × d_out; q(v) and W are the handle's.  Returns (U, γ (D × T), Γ (D × D × T)).  PosDefException(t + 1) names an
# indefinite node, PosDefException(k) a K_uu that failed.
function psi_in_grad(h::Handle, m::Matrix{Float64}, S, y::Matrix{Float64})
    D, T = size(m); U = zeros(T); γ = zeros(D, T); Γ = zeros(D, D, T); info = zeros(Int64, 2)
    check(ccall((:sgp_psi_in_grad, LIB), Cint,
                (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}),
                h.ptr, m, S === nothing ? C_NULL : S, y, T, U, γ, Γ, info), h.ptr)
    return U, γ, Γ
end

# ---- closed-form prediction at Gaussian inputs (sgp_psi_predict; SE kernel only, D <= 32): per node t with input x_t ~ N(m_t, S_t) the
# mean and covariance of f(x_t) with x_t and v both integrated out, and Cov[x_t, f(x_t)].  m is D × T, S is D × D × T or nothing
# (S = 0); q(v) and W are the handle's; noise = true adds W⁻¹.  Returns (mean (T × d_out), C_f (d_out × d_out × T; a vector of T for
# d_out = 1), cross (D × d_out × T)).  PosDefException(t + 1) names an indefinite node, PosDefException(k) a K_uu that failed.
function psi_predict(h::Handle, m::Matrix{Float64}, S, d_out::Integer; noise::Bool = false)
    D, T = size(m); μ = zeros(T, d_out); info = zeros(Int64, 2)
    C = d_out == 1 ? zeros(T) : zeros(d_out, d_out, T); X = zeros(D, d_out, T)
    check(ccall((:sgp_psi_predict, LIB), Cint,
                (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}),
                h.ptr, m, S === nothing ? C_NULL : S, T, noise ? Int32(1) : Int32(0), μ, C, X, info), h.ptr)
    return μ, C, X
end

# The classification loop (experiments/classification_banana.ipynb cell 9: `y[i] ~ Probit(f[i])`, q(w) = GammaShapeRate carried
# over the minibatches, q(v) never reset): labels 0 / 1 in y; returns (θ, shape, rate).  sgp_train_likelihood turns the run
# opened by sgp_train_begin into this loop -- forward message, Probit moment matching, Gamma update and AdaMax on the device.
function train_classification!(meta::HipSGPMeta, X::Matrix{Float64}, y::Vector{Float64}, θ::Vector{Float64}; batch, epochs,
                               shape = 0.01, rate = 0.01, prior_var = 50.0, η = 1e-3, β = (0.9, 0.999), ϵ = 1e-8)
    h = meta.handle; N = length(y)
    set_prior!(h, C_NULL, fill(Float64(prior_var), 1, 1), 2)
    check(ccall((:sgp_train_begin, LIB), Cint,
                (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Int32, Float64, Float64, Float64, Float64, Float64),
                h.ptr, X, y, N, θ, length(θ) - 1, meta.jitter, η, β[1], β[2], ϵ), h.ptr)
    check(ccall((:sgp_train_likelihood, LIB), Cint, (Ptr{Cvoid}, Int32, Float64, Float64), h.ptr, Int32(1), shape, rate), h.ptr)   # SGP_LIKELIHOOD_PROBIT
    for _ in 1:epochs, o in 0:batch:N-1
        check(ccall((:sgp_train_step, LIB), Cint, (Ptr{Cvoid}, Int64, Int64, Int32), h.ptr, o, min(batch, N - o), Int32(1)), h.ptr)
    end
    θout = similar(θ); counts = zeros(Int64, 2); ab = zeros(2)
    check(ccall((:sgp_train_end, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Int64}), h.ptr, θout, counts), h.ptr)
    check(ccall((:sgp_train_get_gamma, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}), h.ptr, ab), h.ptr)
    counts[2] == 0 || throw(PosDefException(Int(counts[2])))
    return θout, ab[1], ab[2]
end

# Multi-GPU (one Julia process per GPU, e.g. under MPI.jl): register the communicator once; sgp_sweep / sgp_theta_objective /
# sgp_train_step then sum what has to be summed inside the library -- the exchange buffer [lower tiles of Ψ2 | B | scalars] and
# the data half of the θ gradient -- and every rank sees the statistics, the objective and the gradient of all shards.
use_rccl!(h::Handle, comm::Ptr{Cvoid}) = check(ccall((:sgp_use_rccl, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), h.ptr, comm), h.ptr)

# ------------------------------------------------------------------------------------------------------------------
# MultiSGP
# ------------------------------------------------------------------------------------------------------------------
mutable struct HipMultiSGPMeta{R<:MultiSGPMeta}
    ref::R
    d_out::Int
    handle::Handle                    # d_out outputs: the batched sweep (multisgp_sweep!)
    step::Handle                      # single-output handle for the per-step Ψ-statistics
    kernel_params::Function
    jitter::Float64
    aux::Union{Nothing,Handle}        # single-output handle for the :in / :θ closures (it replaces data and posterior)
    device::Int
end

function HipMultiSGPMeta(ref::MultiSGPMeta, d_out::Int; kernel_params, n_steps, jitter = 0.0, device = 0, kernel_family = :se)
    Xu = inducing_matrix(ref.Xu)
    npts = 2 * size(Xu, 1) + 1                                 # srcubature: 2 d_in + 1 points per step
    fam = kernel_family_id(kernel_family)                      # (as HipSGPMeta)
    return HipMultiSGPMeta(ref, d_out, Handle(n_steps * npts, Xu, d_out; device = device, family = fam),
                           Handle(npts, Xu, 1; device = device, family = fam), kernel_params, Float64(jitter), nothing, device)
end

# cubature points / weights of q_in as the reference's approximate_kernel_expectation! walks them (GPnode/MultiSGPnode.jl:11-35)
function cubature(meta::HipMultiSGPMeta, q_in)
    m, P = mean_cov(q_in)
    weights = ReactiveMP.getweights(meta.ref.method, m, P)
    points = ReactiveMP.getpoints(meta.ref.method, m, P)
    return reduce(hcat, [collect(Float64, p) for p in points]), collect(Float64, weights)
end

# Ψ0, Ψ1, Ψ2 of ONE step on the device: the step's cubature points as weighted data, statistics without a posterior
function psi_statistics!(meta::HipMultiSGPMeta, q_in, θ)
    X, ω = cubature(meta, q_in)
    h = meta.step
    set_data!(h, X, ones(length(ω)), nothing, ω, 1.0)
    σ², ℓ = meta.kernel_params(θ)
    set_kernel!(h, σ², collect(Float64, ℓ), meta.jitter)
    sweep_local!(h)
    Ψ2, B, sc = stats(h)
    ref = meta.ref
    ref.Ψ0 .= σ² * sc[2]; ref.Ψ1_trans .= B; ref.Ψ2 .= Ψ2     # the buffers the reference's rules fill (:299-302)
    return ref.Ψ0, ref.Ψ1_trans, ref.Ψ2
end

# ---- :v for one step (GPnode/MultiSGPnode.jl:290-328): ξ = vcat(Ψ1 (μ_y' W)_d), Λ = kron(W, Ψ2) ---------------------
function hip_multi_v(q_out, q_in, q_w, q_θ, meta::HipMultiSGPMeta)
    W = mean(q_w); μ_y = mean(q_out)
    _, Ψ1, Ψ2 = psi_statistics!(meta, q_in, mean(q_θ))
    row = μ_y' * W
    return MvNormalWeightedMeanPrecision(vcat([vec(Ψ1) .* row[d] for d in 1:length(μ_y)]...), kron(W, Ψ2))
end
@rule MultiSGP(:v, Marginalisation) (q_out::MultivariateGaussianDistributionsFamily, q_in::MultivariateGaussianDistributionsFamily, q_w::Any, q_θ::PointMass, meta::HipMultiSGPMeta) =
    hip_multi_v(q_out, q_in, q_w, q_θ, meta)
@rule MultiSGP(:v, Marginalisation) (q_out::PointMass, q_in::MultivariateGaussianDistributionsFamily, q_w::Any, q_θ::PointMass, meta::HipMultiSGPMeta) =
    hip_multi_v(q_out, q_in, q_w, q_θ, meta)

# ---- :w for one step (GPnode/MultiSGPnode.jl:367-444): WishartFast(D + 2, I1 + I2) ---------------------------------
# I1 = (Ψ0 - tr(Kuu^-1 Ψ2)) I,  I2[i,j] = Σ_y[i,j] + μ_y μ_y' - μ_y E' - E μ_y' + tr(Rv_blk[i][j] Ψ2),  E_d = Ψ1 · μ_v^(d)
function hip_multi_w(q_out, q_in, q_v, q_θ, meta::HipMultiSGPMeta)
    Ψ0, Ψ1, Ψ2 = psi_statistics!(meta, q_in, mean(q_θ))
    μ_y = mean(q_out); D = length(μ_y); M = meta.step.m
    Σ_y = q_out isa PointMass ? zeros(D, D) : cov(q_out)
    μ_v, Σ_v = mean_cov(q_v)
    Rv = Σ_v + μ_v * μ_v'
    E = [dot(vec(Ψ1), view(μ_v, (d-1)*M+1:d*M)) for d in 1:D]
    Ψ4 = [sum(view(Rv, (i-1)*M+1:i*M, (j-1)*M+1:j*M) .* Ψ2') for i in 1:D, j in 1:D]
    I1 = (Ψ0[1] - tr(meta.ref.Kuu_inverse * Ψ2)) * Matrix(I, D, D)
    tmp = μ_y * E'
    return WishartFast(D + 2, Ψ4 + Σ_y + μ_y * μ_y' - tmp - tmp' + I1)
end
@rule MultiSGP(:w, Marginalisation) (q_out::MultivariateNormalDistributionsFamily, q_in::MultivariateNormalDistributionsFamily, q_v::MultivariateNormalDistributionsFamily, q_θ::PointMass, meta::HipMultiSGPMeta) =
    hip_multi_w(q_out, q_in, q_v, q_θ, meta)
@rule MultiSGP(:w, Marginalisation) (q_out::PointMass, q_in::MultivariateNormalDistributionsFamily, q_v::MultivariateNormalDistributionsFamily, q_θ::PointMass, meta::HipMultiSGPMeta) =
    hip_multi_w(q_out, q_in, q_v, q_θ, meta)

# ---- :out for one step (GPnode/MultiSGPnode.jl:90-120): mean_d = Ψ1 · μ_v^(d), precision mean(q_w) -----------------
@rule MultiSGP(:out, Marginalisation) (q_in::MultivariateNormalDistributionsFamily, q_v::MultivariateNormalDistributionsFamily, q_w::Any, q_θ::PointMass, meta::HipMultiSGPMeta) = begin
    X, ω = cubature(meta, q_in)
    σ², ℓ = meta.kernel_params(mean(q_θ))
    set_kernel!(meta.handle, σ², collect(Float64, ℓ), meta.jitter)
    F = predict_mean(meta.handle, X, collect(Float64, mean(q_v)))            # points × d_out
    return MvNormalMeanPrecision(vec(ω' * F), mean(q_w))
end

# ---- :in and :θ (multisgp.py:169-278) -- both closures are per-point device quantities at a PSEUDO-posterior ------------------
# s = Σ_d μ_v^(d) (μ_y' W)_d  (sum_diagonal_M) and S = Σ_ij W_ij Rv_blk[i][j]  (create_blockmatrix), Rv = Σ_v + μ μ': what the
# closures keep of q(v) (GPnode/MultiSGPnode.jl:176-179).  With mean s, factor chol(S).U and pseudo-observations y = 1,
# sgp_w_stats returns I1(x) = k(x,x) - k' Kuu^-1 k and I2(x) = 1 - 2 s·k + k' S k.
function second_moment_contraction(q_out, q_v, W, M)
    μ_y = collect(Float64, mean(q_out)); D = length(μ_y)
    μ_v, Σ_v = mean_cov(q_v)
    Rv = Σ_v + μ_v * μ_v'
    row = μ_y' * W
    s = sum(view(μ_v, (d-1)*M+1:d*M) .* row[d] for d in 1:D)
    S = sum(view(Rv, (i-1)*M+1:i*M, (j-1)*M+1:j*M) .* W[i, j] for i in 1:D, j in 1:D)
    return collect(Float64, s), Matrix{Float64}(0.5 * (S + S'))
end
function aux_handle!(meta::HipMultiSGPMeta, n::Int)
    if meta.aux === nothing || meta.aux.n_max < n
        meta.aux = Handle(max(n, 64), inducing_matrix(meta.ref.Xu), 1; device = meta.device, family = meta.handle.family)
    end
    return meta.aux
end
function pseudo_stats(meta::HipMultiSGPMeta, X::Matrix{Float64}, σ², ℓ, jitter, s, US)
    h = aux_handle!(meta, size(X, 2))
    set_data!(h, X, ones(size(X, 2)), nothing, nothing, -1.0)
    set_kernel!(h, σ², collect(Float64, ℓ), jitter)
    sweep_local!(h)
    set_posterior!(h, s, US)
    return w_stats(h, size(X, 2))
end
# :in (GPnode/MultiSGPnode.jl:162-208): x -> -1/2 tr(W) I1(x) + s·k(x) - 1/2 k(x)' S k(x) = -1/2 tr(W) I1 - 1/2 (I2 - 1)
function multi_in_closure(q_out, q_v, q_w, q_θ, meta::HipMultiSGPMeta)
    W = Matrix{Float64}(mean(q_w)); M = meta.step.m
    s, S = second_moment_contraction(q_out, q_v, W, M)
    US = Matrix(potrf(S; device = meta.device)')                # upper factor: |US k|² = k' S k
    σ², ℓ = meta.kernel_params(mean(q_θ))
    trW = tr(W)
    return (x) -> begin
        I1, I2 = pseudo_stats(meta, reshape(collect(Float64, x), :, 1), σ², ℓ, meta.jitter, s, US)
        -0.5 * trW * I1[1] - 0.5 * (I2[1] - 1.0)
    end
end
@rule MultiSGP(:in, Marginalisation) (q_out::Any, q_v::MultivariateNormalDistributionsFamily, q_w::Any, q_θ::PointMass, meta::HipMultiSGPMeta) =
    ContinuousMultivariateLogPdf(UnspecifiedDomain(), multi_in_closure(q_out, q_v, q_w, q_θ, meta))
# the Laplace variant (:210-236: q_out::PointMass, Gaussian q_in, point-mass q_w) minimises the same closure; the reference's own
# optimiser code runs unchanged on it -- every evaluation is one device pass
@rule MultiSGP(:in, Marginalisation) (q_out::PointMass, q_in::MultivariateGaussianDistributionsFamily, q_v::MultivariateGaussianDistributionsFamily, q_w::Any, q_θ::PointMass, meta::HipMultiSGPMeta) = begin
    f = multi_in_closure(q_out, q_v, q_w, q_θ, meta)
    neg = (x) -> -f(x)
    D = length(mean(q_in)); E = Matrix{Float64}(I, D, D); h1 = 1e-5
    # (the reference differentiates with ForwardDiff / Zygote, :227-231; a ccall cannot be traced, so gradient and Hessian are
    # central differences of the device-evaluated closure, as in multisgp.py: rule_in_laplace)
    grad! = (G, x) -> (for a in 1:D; G[a] = (neg(x + h1 * E[:, a]) - neg(x - h1 * E[:, a])) / (2 * h1); end; G)
    m_z = Optim.optimize(neg, grad!, collect(Float64, mean(q_in)), Optim.LBFGS(), Optim.Options(iterations = 20); inplace = true).minimizer   # :229
    hh = 1e-4
    W_z = [(neg(m_z + hh * (E[:, a] + E[:, b])) - neg(m_z + hh * (E[:, a] - E[:, b])) - neg(m_z - hh * (E[:, a] - E[:, b])) + neg(m_z - hh * (E[:, a] + E[:, b]))) / (4 * hh^2)
           for a in 1:D, b in 1:D]                               # Hessian at the minimiser by central differences (:231-233 uses ForwardDiff)
    return MvNormalWeightedMeanPrecision(W_z * m_z, W_z)        # :235
end
# :θ (GPnode/MultiSGPnode.jl:447-466): θ -> -1/2 tr(W) (Ψ0 - tr(Kuu^-1 Ψ2')) + Ψ1·s - 1/2 tr(Ψ2' S), Ψ2' = Ψ2 + 1e-7 I (:458),
# Kuu(θ) without jitter (:455): per cubature point the :in closure; the 1e-7 I term adds 1e-7 (tr(W) tr(Kuu^-1) - tr(S)) / 2
@rule MultiSGP(:θ, Marginalisation) (q_out::Any, q_in::MultivariateGaussianDistributionsFamily, q_v::MultivariateGaussianDistributionsFamily, q_w::Any, meta::HipMultiSGPMeta) = begin
    W = Matrix{Float64}(mean(q_w)); M = meta.step.m
    s, S = second_moment_contraction(q_out, q_v, W, M)
    US = Matrix(potrf(S; device = meta.device)')
    trW, trS = tr(W), tr(S)
    X, ω = cubature(meta, q_in)
    Xu = inducing_matrix(meta.ref.Xu)
    log_backwardmess = (θ) -> begin
        σ², ℓ = meta.kernel_params(θ)
        I1, I2 = pseudo_stats(meta, X, σ², ℓ, 0.0, s, US)
        tr_kinv = tr(potri(kernelmatrix_dev(Xu, Xu, σ², collect(Float64, ℓ); device = meta.device,
                                                 kernel_family = meta.handle.family); device = meta.device))
        dot(ω, -0.5 * trW .* I1 .- 0.5 .* (I2 .- 1.0)) + 0.5e-7 * (trW * tr_kinv - trS)
    end
    return ContinuousMultivariateLogPdf(UnspecifiedDomain(), log_backwardmess)
end
# the per-step average energy: the reference's own method with the wrapped meta (its Ψ-statistics buffers were filled by the
# device through psi_statistics! in the :v / :w rules of the same step)
@average_energy MultiSGP (q_out::Any, q_in::MultivariateGaussianDistributionsFamily, q_v::MultivariateNormalDistributionsFamily, q_w::Any, q_θ::PointMass, meta::HipMultiSGPMeta) =
    ReactiveMP.score(AverageEnergy(), MultiSGP, Val{(:out, :in, :v, :w, :θ)}(), (q_out, q_in, q_v, q_w, q_θ), meta.ref)

# ---- the batched form: ALL steps in one sweep (what gaussianprocessnode_amd.multisgp.sweep does) -------------------
# q(v) from every step's :v message folded with `prior`; also returns Σ_t (I1_t + I2_t) (the Wishart inverse scales add,
# GPnode/MultiSGPnode.jl:367-444) and the summed average energy (:544-632), so a smoother's M-step is one call.
function multisgp_sweep!(meta::HipMultiSGPMeta, q_outs, q_ins, q_w, q_θ::PointMass, prior)
    h = meta.handle; D = meta.d_out
    Xs = Matrix{Float64}[]; ωs = Vector{Float64}[]; Ys = Matrix{Float64}[]; Σsum = zeros(D, D)
    for (q_in, q_out) in zip(q_ins, q_outs)
        X, ω = cubature(meta, q_in)
        push!(Xs, X); push!(ωs, ω); push!(Ys, repeat(collect(Float64, mean(q_out))', length(ω)))
        q_out isa PointMass || (Σsum .+= cov(q_out))
    end
    X = reduce(hcat, Xs); ω = reduce(vcat, ωs); Y = reduce(vcat, Ys)            # Y: points × d_out, column-major = per-output blocks
    set_data!(h, X, vec(Y), nothing, ω, Float64(length(q_ins)))
    any(!iszero, Σsum) && check(ccall((:sgp_set_output_cov_sum, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}), h.ptr, Σsum), h.ptr)
    σ², ℓ = meta.kernel_params(mean(q_θ))
    set_kernel!(h, σ², collect(Float64, ℓ), meta.jitter)
    W = Matrix{Float64}(mean(q_w))
    set_noise!(h, W, q_w isa Union{Wishart,WishartFast} ? mean(logdet, q_w) : logdet(W))
    μ0, Σ0 = mean_cov(prior)
    set_prior!(h, collect(Float64, μ0), Matrix{Float64}(Σ0), 0)
    sweep!(h)
    μ, Σ, _ = posterior(h)
    return MvNormalMeanCovariance(μ, Σ), wishart_invscale(h), scalars(h)[3]
end

# ---- device-paced VMP iterations of MultiSGP with Wishart noise (sgp_vmp_run_w): y_t ~ MultiSGP(x_t, v, W, θ), W ~ Wishart, on the
# d_out = 2:4 handle of a HipMultiSGPMeta, over the resident data, kernel and prior (what multisgp_sweep! loaded, for instance).
# W0 = (ν0, R0) the prior and W = (ν, R) the q(W) entering the run (default the prior), R the d × d inverse scale (WishartFast);
# nothing with hold_w = true, which keeps the last set_noise.  Returns (values, terms, (ν, R), iterations_done, converged);
# PosDefException(k) when K_uu, Λ or R0 + S failed.
function vmp_run_w!(meta::HipMultiSGPMeta, iterations::Integer; W0 = nothing, W = nothing, tol = 0.0, hold_w::Bool = false)
    h = meta.handle
    hold_w || W0 !== nothing || throw(ArgumentError("vmp_run_w!: W0 = (ν0, R0) is required without hold_w"))
    pack(q) = vcat(Float64(q[1]), vec(Matrix{Float64}(q[2])))        # (Julia's matrices are column-major already)
    p0 = hold_w ? nothing : pack(W0)
    q = hold_w ? nothing : (W === nothing ? copy(p0) : pack(W))
    values = fill(NaN, max(iterations, 0)); terms = fill(NaN, 4, max(iterations, 0)); counts = zeros(Int64, 2)
    check(ccall((:sgp_vmp_run_w, LIB), Cint,
                (Ptr{Cvoid}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Float64, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}),
                h.ptr, hold_w ? 1 : 0, iterations, p0 === nothing ? C_NULL : p0, q === nothing ? C_NULL : q, tol, values, terms, counts),
          h.ptr)
    d = q === nothing ? 0 : isqrt(length(q) - 1)
    return values, terms, q === nothing ? nothing : (q[1], reshape(q[2:end], d, d)), Int(counts[1]), counts[2] == 1
end

end # module
