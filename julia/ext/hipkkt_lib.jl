# Shared pieces of the two plugin seams: where the library is, how options and errors cross the C ABI.
using SparseArrays, Clarabel
import Clarabel: DefaultInt, LinearSolverInfo

# export CLARABEL_HIPKKT_LIB=/path/to/clarabel.jl_amd/libclarabel_hipkkt.so   (built by clarabel.jl_amd/csrc/build.sh)
const libhipkkt = get(ENV, "CLARABEL_HIPKKT_LIB", "libclarabel_hipkkt.so")

# the GPU a solver lives on: one process (or Julia thread) per GPU drives its own solvers (SURVEY.md section 8e)
hip_device() = Int32(parse(Int, get(ENV, "CLARABEL_HIP_DEVICE", "0")))

# mirrors `struct hipkkt_opts` (include/hipkkt.h)
struct HipKKTOpts
    index_base::Int32; supernode_max_width::Int32; relax_supernodes::Int32
    update_policy::Int32; update_batch::Int32; front_min_panels::Int32
    dynamic_reg_eps::Float64; dynamic_reg_delta::Float64; amd_dense_scale::Float64
    user_perm::Ptr{Int64}
end

function hip_default_opts(settings)
    r = Ref{HipKKTOpts}()
    ccall((:hipkkt_default_opts, libhipkkt), Cvoid, (Ref{HipKKTOpts},), r)
    o = r[]
    # index_base = 1: Julia's 1-based colptr / rowval / index vectors go through as they are
    HipKKTOpts(1, o.supernode_max_width, o.relax_supernodes, o.update_policy, o.update_batch, 0,
               settings.dynamic_regularization_eps, settings.dynamic_regularization_delta,
               1.5, C_NULL)                       # 1.5 = amd_dense_scale of directldl_qdldl.jl:24
end

hip_last_error(handle::Ptr{Cvoid} = C_NULL) =
    unsafe_string(ccall((:hipkkt_last_error, libhipkkt), Cstring, (Ptr{Cvoid},), handle))

# include/hipkkt.h HIPKKT_ABI_VERSION this file was written against: signatures may change between versions, never within one
const HIPKKT_ABI_VERSION = Int32(5)
function hip_check_abi()
    v = ccall((:hipkkt_abi_version, libhipkkt), Int32, ())
    v == HIPKKT_ABI_VERSION || error("libclarabel_hipkkt implements ABI version $v, this extension was written against $HIPKKT_ABI_VERSION")
    return true
end

hip_is_available() = hip_check_abi() && ccall((:hipkkt_is_available, libhipkkt), Int32, ()) > 0

# gives the library's cache of device memory blocks back to the driver (e.g. before another package needs the HBM)
hip_trim_cache() = ccall((:hipkkt_trim_cache, libhipkkt), Int32, (Int32,), hip_device())

function hip_destroy!(x)
    x.handle == C_NULL || ccall((:hipkkt_destroy, libhipkkt), Cvoid, (Ptr{Cvoid},), x.handle)
    x.handle = C_NULL
    return nothing
end

function hip_linear_solver_info(handle::Ptr{Cvoid})
    nnzA = Ref{Int64}(0); nnzL = Ref{Int64}(0)
    ccall((:hipkkt_info, libhipkkt), Int32, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}), handle, nnzA, nnzL)
    LinearSolverInfo(:hip, 1, true, nnzA[], nnzL[])
end

# ---- the interior-point step on the device (include/hipkkt.h hipkkt_cone_* / hipkkt_step_*), Zero / Nonnegative / SecondOrder cone sets.
# Thin wrappers on the handle: the solver object of kktsolver_hip.jl passes ks.handle.  The *_dev arguments are DEVICE pointers (e.g.
# pointer(::ROCArray{Float64})): xzs = [x | z | s], res = [rx | rz | rx_inf | rz_inf | Px], the buffers of hipkkt_residuals_dev.
# INTEGRATION.md ("The step on the device") says which hooks of the core would call them and how long the buffers must live.
hip_step_check(handle::Ptr{Cvoid}, rc::Int32, what::String) =
    rc < 0 ? error("$what failed ($rc): " * hip_last_error(handle)) : rc == 0

function hip_cone_affine_ds!(handle::Ptr{Cvoid}, ds::Vector{Float64})
    rc = ccall((:hipkkt_cone_affine_ds, libhipkkt), Int32, (Ptr{Cvoid}, Ptr{Float64}), handle, ds)
    return hip_step_check(handle, rc, "hipkkt_cone_affine_ds")
end
function hip_cone_combined_ds_shift!(handle::Ptr{Cvoid}, shift::Vector{Float64}, step_z::Vector{Float64}, step_s::Vector{Float64}, σμ::Float64)
    rc = ccall((:hipkkt_cone_combined_ds_shift, libhipkkt), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Float64, Ptr{Float64}),
               handle, step_z, step_s, σμ, shift)
    return hip_step_check(handle, rc, "hipkkt_cone_combined_ds_shift")
end
function hip_cone_ds_from_dz_offset!(handle::Ptr{Cvoid}, out::Vector{Float64}, ds::Vector{Float64})
    rc = ccall((:hipkkt_cone_ds_from_dz_offset, libhipkkt), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), handle, ds, out)
    return hip_step_check(handle, rc, "hipkkt_cone_ds_from_dz_offset")
end
function hip_cone_mul_hs!(handle::Ptr{Cvoid}, y::Vector{Float64}, x::Vector{Float64})
    rc = ccall((:hipkkt_cone_mul_hs, libhipkkt), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), handle, x, y)
    return hip_step_check(handle, rc, "hipkkt_cone_mul_hs")
end
function hip_cone_step_length(handle::Ptr{Cvoid}, dz::Vector{Float64}, ds::Vector{Float64}, αmax::Float64)
    out = zeros(Float64, 2)
    rc = ccall((:hipkkt_cone_step_length, libhipkkt), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Float64, Ptr{Float64}),
               handle, dz, ds, αmax, out)
    hip_step_check(handle, rc, "hipkkt_cone_step_length")
    return (out[1], out[2])
end
function hip_set_equilibration!(handle::Ptr{Cvoid}, d::Vector{Float64}, e::Vector{Float64})
    rc = ccall((:hipkkt_set_equilibration, libhipkkt), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), handle, d, e)
    return hip_step_check(handle, rc, "hipkkt_set_equilibration")
end
# -> (is_success, scal_out15 = α, Δτ, Δκ, α_z, α_s, the ten scalars of hipkkt_kkt_solve_reduced); ir = (enable, reltol, abstol, max_iter, stop_ratio)
function hip_step_affine_dev!(handle::Ptr{Cvoid}, xzs_dev::Ptr{Float64}, res_dev::Ptr{Float64}, τ::Float64, κ::Float64, rτ::Float64,
                              const_pending::Bool, ir::Tuple{Bool,Float64,Float64,Int64,Float64})
    scal_in = Float64[τ, κ, rτ]
    scal_out = zeros(Float64, 15)
    rc = ccall((:hipkkt_step_affine_dev, libhipkkt), Int32,
               (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}, Int32, Float64, Float64, Int64, Float64, Ptr{Int64}),
               handle, xzs_dev, res_dev, scal_in, const_pending ? 1 : 0, scal_out, ir[1], ir[2], ir[3], ir[4], ir[5], C_NULL)
    return (hip_step_check(handle, rc, "hipkkt_step_affine_dev"), scal_out)
end
function hip_step_combined_dev!(handle::Ptr{Cvoid}, xzs_dev::Ptr{Float64}, res_dev::Ptr{Float64}, τ::Float64, κ::Float64, rτ::Float64,
                                Δτ_aff::Float64, Δκ_aff::Float64, σ::Float64, μ::Float64, m_corr::Float64, max_step_fraction::Float64,
                                ir::Tuple{Bool,Float64,Float64,Int64,Float64})
    scal_in = Float64[τ, κ, rτ, Δτ_aff, Δκ_aff, σ, μ, m_corr, max_step_fraction]
    scal_out = zeros(Float64, 15)
    rc = ccall((:hipkkt_step_combined_dev, libhipkkt), Int32,
               (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}, Int32, Float64, Float64, Int64, Float64, Ptr{Int64}),
               handle, xzs_dev, res_dev, scal_in, 0, scal_out, ir[1], ir[2], ir[3], ir[4], ir[5], C_NULL)
    return (hip_step_check(handle, rc, "hipkkt_step_combined_dev"), scal_out)
end
# not synchronised with the host: xzs_dev stays valid (and is not read by the host) until the next synchronising call on the handle
function hip_step_apply_dev!(handle::Ptr{Cvoid}, α::Float64, xzs_dev::Ptr{Float64})
    rc = ccall((:hipkkt_step_apply_dev, libhipkkt), Int32, (Ptr{Cvoid}, Float64, Ptr{Float64}), handle, α, xzs_dev)
    return hip_step_check(handle, rc, "hipkkt_step_apply_dev")
end
function hip_step_info_norms_dev(handle::Ptr{Cvoid}, xzs_dev::Ptr{Float64}, res_dev::Ptr{Float64})
    out = zeros(Float64, 8)
    rc = ccall((:hipkkt_step_info_norms_dev, libhipkkt), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), handle, xzs_dev, res_dev, out)
    hip_step_check(handle, rc, "hipkkt_step_info_norms_dev")
    return out
end
# opt-in per registration: the step entry points also serve the Exponential / Power cones (kinds 4, 5) of the handle
function hip_step_enable_cone3!(handle::Ptr{Cvoid}, enable::Bool, backtrack_step::Float64, min_terminate_step_length::Float64)
    rc = ccall((:hipkkt_step_enable_cone3, libhipkkt), Int32, (Ptr{Cvoid}, Int32, Float64, Float64), handle, enable ? 1 : 0,
               backtrack_step, min_terminate_step_length)
    return hip_step_check(handle, rc, "hipkkt_step_enable_cone3")
end
# the same for a registration with Generalized Power cones (kind 6); its Exponential / Power members step with the same parameters
function hip_step_enable_genpow!(handle::Ptr{Cvoid}, enable::Bool, backtrack_step::Float64, min_terminate_step_length::Float64)
    rc = ccall((:hipkkt_step_enable_genpow, libhipkkt), Int32, (Ptr{Cvoid}, Int32, Float64, Float64), handle, enable ? 1 : 0,
               backtrack_step, min_terminate_step_length)
    return hip_step_check(handle, rc, "hipkkt_step_enable_genpow")
end
# the same for a symmetric registration with PSD triangle cones (kind 3) of side <= 64: the step works on the caller's factors
function hip_step_enable_psd!(handle::Ptr{Cvoid}, enable::Bool)
    rc = ccall((:hipkkt_step_enable_psd, libhipkkt), Int32, (Ptr{Cvoid}, Int32), handle, enable ? 1 : 0)
    return hip_step_check(handle, rc, "hipkkt_step_enable_psd")
end
# the same with the side limit 128: cones of side 65 .. 128 keep their matrices in device memory (same arithmetic); the scaling's
# Cholesky / SVD and the default start of such a set stay with the caller
function hip_step_enable_psd_large!(handle::Ptr{Cvoid}, enable::Bool)
    rc = ccall((:hipkkt_step_enable_psd_large, libhipkkt), Int32, (Ptr{Cvoid}, Int32), handle, enable ? 1 : 0)
    return hip_step_check(handle, rc, "hipkkt_step_enable_psd_large")
end
# PSD triangle cones (side <= 64) next to Exponential / Power / Generalized Power cones: each family steps as after its own enable, the
# barrier calls add the PSD cones' log-det barrier; sides above 64 in such a set and its unit initialisation stay with the caller
function hip_step_enable_mixed!(handle::Ptr{Cvoid}, enable::Bool, backtrack_step::Float64, min_terminate_step_length::Float64)
    rc = ccall((:hipkkt_step_enable_mixed, libhipkkt), Int32, (Ptr{Cvoid}, Int32, Float64, Float64), handle, enable ? 1 : 0,
               backtrack_step, min_terminate_step_length)
    return hip_step_check(handle, rc, "hipkkt_step_enable_mixed")
end
# the same with PSD sides up to 128 (the larger cones through the kernels of hip_step_enable_psd_large!, their barrier with one matrix
# in LDS); hip_psd_scaling_enable_large! is the scaling opt-in of such a handle, its start stays the unit initialisation
function hip_step_enable_mixed_large!(handle::Ptr{Cvoid}, enable::Bool, backtrack_step::Float64, min_terminate_step_length::Float64)
    rc = ccall((:hipkkt_step_enable_mixed_large, libhipkkt), Int32, (Ptr{Cvoid}, Int32, Float64, Float64), handle, enable ? 1 : 0,
               backtrack_step, min_terminate_step_length)
    return hip_step_check(handle, rc, "hipkkt_step_enable_mixed_large")
end
# Rinv_all: the cones' Rinv (n x n column-major each, concatenated like psd_R), λ_all: their λ; consumed by the next hip update_scaling
function hip_psd_set_factors!(handle::Ptr{Cvoid}, Rinv_all::Vector{Float64}, λ_all::Vector{Float64})
    rc = ccall((:hipkkt_psd_set_factors, libhipkkt), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), handle, Rinv_all, λ_all)
    return hip_step_check(handle, rc, "hipkkt_psd_set_factors")
end
# device pointers; not synchronised with the host: both stay valid until the next synchronising call on the handle
function hip_psd_set_factors_dev!(handle::Ptr{Cvoid}, Rinv_dev::Ptr{Float64}, λ_dev::Ptr{Float64})
    rc = ccall((:hipkkt_psd_set_factors_dev, libhipkkt), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), handle, Rinv_dev, λ_dev)
    return hip_step_check(handle, rc, "hipkkt_psd_set_factors_dev")
end
# after hip_step_enable_psd!: a hip update_scaling without psd_R computes the PSD cones' (R, R⁻¹, λ) on the device
# (update_scaling!(::PSDTriangleCone), coneops_psdtrianglecone.jl:78-143)
function hip_psd_scaling_enable!(handle::Ptr{Cvoid}, enable::Bool)
    rc = ccall((:hipkkt_psd_scaling_enable, libhipkkt), Int32, (Ptr{Cvoid}, Int32), handle, enable ? 1 : 0)
    return hip_step_check(handle, rc, "hipkkt_psd_scaling_enable")
end
# after hip_step_enable_psd_large!: the same for a set with a side of 65 .. 128 (those cones with one matrix in LDS and the others in
# device memory, same arithmetic), and the default start of such a set (hip_cone_set_identity_scaling! and its group); not wired
# into the core like the others
function hip_psd_scaling_enable_large!(handle::Ptr{Cvoid}, enable::Bool)
    rc = ccall((:hipkkt_psd_scaling_enable_large, libhipkkt), Int32, (Ptr{Cvoid}, Int32), handle, enable ? 1 : 0)
    return hip_step_check(handle, rc, "hipkkt_psd_scaling_enable_large")
end
function hip_step_default_start_enable_psd_large!(handle::Ptr{Cvoid}, enable::Bool)
    rc = ccall((:hipkkt_step_default_start_enable_psd_large, libhipkkt), Int32, (Ptr{Cvoid}, Int32), handle, enable ? 1 : 0)
    return hip_step_check(handle, rc, "hipkkt_step_default_start_enable_psd_large")
end
# the resident factors of the last scaling (K.data.R, .Rinv, .λ): n x n column-major per cone, concatenated like psd_R; λ n per cone
function hip_psd_get_factors!(handle::Ptr{Cvoid}, R_all::Vector{Float64}, Rinv_all::Vector{Float64}, λ_all::Vector{Float64})
    rc = ccall((:hipkkt_psd_get_factors, libhipkkt), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), handle, R_all,
               Rinv_all, λ_all)
    return hip_step_check(handle, rc, "hipkkt_psd_get_factors")
end
# -> out[2j-1] = the cones' barrier, out[2j] = <z + αⱼΔz, s + αⱼΔs> for at most 8 candidates αⱼ
function hip_cone_barrier(handle::Ptr{Cvoid}, Δz::Vector{Float64}, Δs::Vector{Float64}, αs::Vector{Float64})
    out = zeros(Float64, 2 * length(αs))
    rc = ccall((:hipkkt_cone_barrier, libhipkkt), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}),
               handle, Δz, Δs, αs, length(αs), out)
    hip_step_check(handle, rc, "hipkkt_cone_barrier")
    return out
end
function hip_step_barrier_dev(handle::Ptr{Cvoid}, xzs_dev::Ptr{Float64}, αs::Vector{Float64})
    out = zeros(Float64, 2 * length(αs))
    rc = ccall((:hipkkt_step_barrier_dev, libhipkkt), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}),
               handle, xzs_dev, αs, length(αs), out)
    hip_step_check(handle, rc, "hipkkt_step_barrier_dev")
    return out
end
function hip_step_get!(handle::Ptr{Cvoid}, out::Vector{Float64})
    rc = ccall((:hipkkt_step_get, libhipkkt), Int32, (Ptr{Cvoid}, Ptr{Float64}), handle, out)
    return hip_step_check(handle, rc, "hipkkt_step_get")
end

# The default start of a symmetric cone set on the device (include/hipkkt.h "The default start ..."; solver.jl:383-405).  pd: 0 primal, 1 dual.
function hip_cone_set_identity_scaling!(handle::Ptr{Cvoid})
    rc = ccall((:hipkkt_cone_set_identity_scaling, libhipkkt), Int32, (Ptr{Cvoid},), handle)
    return hip_step_check(handle, rc, "hipkkt_cone_set_identity_scaling")
end
# -> (α, β) of margins(::CompositeCone)
function hip_cone_margins(handle::Ptr{Cvoid}, v::Vector{Float64}, pd::Integer)
    out = zeros(Float64, 2)
    rc = ccall((:hipkkt_cone_margins, libhipkkt), Int32, (Ptr{Cvoid}, Ptr{Float64}, Int32, Ptr{Float64}), handle, v, pd, out)
    hip_step_check(handle, rc, "hipkkt_cone_margins")
    return (out[1], out[2])
end
# _shift_to_cone_interior!(v) in place -> (min_margin, pos_margin, target, branch 0 / 1 / 2)
function hip_cone_shift_to_interior!(handle::Ptr{Cvoid}, v::Vector{Float64}, pd::Integer)
    out = zeros(Float64, 4)
    rc = ccall((:hipkkt_cone_shift_to_interior, libhipkkt), Int32, (Ptr{Cvoid}, Ptr{Float64}, Int32, Ptr{Float64}), handle, v, pd, out)
    hip_step_check(handle, rc, "hipkkt_cone_shift_to_interior")
    return (out[1], out[2], out[3], Int(out[4]))
end
# -> (is_success, scal_out8 = eps_used, regularised pivots, (min_margin, pos_margin, target) of s and of z); sreg = (enable, constant, proportional)
function hip_step_default_start_dev!(handle::Ptr{Cvoid}, xzs_dev::Ptr{Float64}, sreg::Tuple{Bool,Float64,Float64},
                                     ir::Tuple{Bool,Float64,Float64,Int64,Float64})
    scal_out = zeros(Float64, 8)
    rc = ccall((:hipkkt_step_default_start_dev, libhipkkt), Int32,
               (Ptr{Cvoid}, Ptr{Float64}, Int32, Float64, Float64, Int32, Float64, Float64, Int64, Float64, Ptr{Float64}, Ptr{Int64}),
               handle, xzs_dev, sreg[1], sreg[2], sreg[3], ir[1], ir[2], ir[3], ir[4], ir[5], scal_out, C_NULL)
    return (hip_step_check(handle, rc, "hipkkt_step_default_start_dev"), scal_out)
end
