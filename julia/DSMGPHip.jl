# DSMGPHip.jl -- reference-side binding of the MI355X GP-expert path (libdsmgp_hip.so, C ABI: include/dsmgp_hip.h).
#
# What a maintainer of trappmartin/DeepStructuredMixtures adds next to `src/` to run the hot path on the GPU:
#
#     using DeepStructuredMixtures
#     include("julia/DSMGPHip.jl"); using .DSMGPHip
#     model = buildDSMGP(x, y, 3, 4; M = 200, kernel = IsoSE(log(0.3), 0.0), logNoise = log(0.1))   # host build, as before
#     DSMGPHip.attach!(model)                 # upload X, y and the leaf table once; from here on the methods below run
#     fit!(model); update!(model); μ, σ² = predict(model, xtest); train!(model, ADAM())
#
# The file re-defines exactly the methods whose bodies are the hot path (SURVEY.md section 8(b)); everything else --
# tree construction, routing (`getchild`), `update!`/`infer!`, the `train!`/`finetune!` loops, Flux -- runs as it is:
#
#   fit!(spn, D, gpmap; τ)          src/fit.jl:71-122      schedule decided here as there, executed by dsmgp_set_sharing + dsmgp_fit
#   fit_naive!(spn)                 src/fit.jl:294-304     dsmgp_set_sharing(NULL) + dsmgp_fit
#   update_cholesky!(gp)            src/gaussianprocess.jl:82-108   one-leaf session (a GP that is not a leaf of an attached model)
#   mll(gp)                         src/gaussianprocess.jl:163      per-leaf value returned by dsmgp_fit
#   prediction(gp, xtest)           src/gaussianprocess.jl:131-137  dsmgp_predict_leaves on the GP's session
#   predict(model, x)               src/common.jl:294-307  DSMGP: rows routed on the device (dsmgp_set_tree once per attach!,
#                                                          dsmgp_set_test_routed per test set), ONE dsmgp_predict_run +
#                                                          dsmgp_aggregate; PoE family: every row to every expert
#   updategradients!(spn)           src/fit.jl:306-311     dsmgp_gradients, results written to kernel.∂ℓ/∂σ and gp.∂ϵ
#   ∇mll(gp)                        src/gaussianprocess.jl:185-190  reads those fields (no second updategradients!)
#   setparams!(spn, hyp)            src/optimize.jl:188-198 unchanged on the host; fit! pushes the vectors (dsmgp_set_hyper)
#
# Julia is not installed in the image this repository is built in: the file has been written against the reference's
# sources and the header, line by line, and NOT executed.  The same entry points in the same order are exercised by
# tests/c_abi_smoke.c (plain C) and by the Python mirror (deepstructuredmixtures_amd/hipabi.py, model.py).
module DSMGPHip

using LinearAlgebra
using Libdl
using DeepStructuredMixtures
import DeepStructuredMixtures: fit!, fit_naive!, update_cholesky!, prediction, mll, predict, updategradients!, ∇mll
using DeepStructuredMixtures: GPNode, GPSumNode, GPSplitNode, DSMGP, PoE, gPoE, rBCM, BiDict, GaussianProcess,
                              IsoSE, ArdSE, IsoLinear, ArdLinear, ConstMean, getLeaves, getchild, children, logweights, getnoise

export attach!, detach!, census, append_rows!, append_stats, resume_stats, download_vt, predict_cov, predict_sample, predict_cov_factor, predict_gradients, aggregate_gradients, aggregate_columns, aggregate_columns_gradients, loo, loo_gradients, kfold, kfold_seconds, solve_targets, predict_targets, predict_targets_gradients, targets_fetch, targets_gradients, loo_targets, loo_targets_gradients, ArdSEProduct, IsoMatern32, IsoMatern52, ArdMatern32, ArdMatern52, IsoRQ, ArdRQ

# ---------------------------------------------------------------------------------------------- ArdSEProduct
"""
    ArdSEProduct(logℓ, logσ)

The product-form ARD squared exponential σ² exp(-½ Σ_d (a_d - b_d)² / ℓ_d²) (GPML's covSEard), with ArdSE's fields.  The
reference's ArdSE is the additive form (src/kernels.jl:39-49); this kernel lives on the device only (kind 4), so of the
reference's kernel methods it has just what GaussianProcess (src/gaussianprocess.jl:50-58) and params / setparams!
(:139-161) call on a kernel.  Its gradients are the true derivatives, written into ∂ℓ and ∂σ by updategradients!.
"""
mutable struct ArdSEProduct{T<:AbstractFloat} <: DeepStructuredMixtures.ArdKernel
    logℓ::Vector{T}
    logσ::T
    ∂ℓ::Vector{T}
    ∂σ::T
end
ArdSEProduct(logℓ, logσ) = ArdSEProduct(logℓ, logσ, zero(logℓ), zero(logσ))
DeepStructuredMixtures.getvariance(k::ArdSEProduct; logscale=false) = logscale ? k.logσ : exp(2 * k.logσ)
DeepStructuredMixtures.getstd(k::ArdSEProduct) = exp(k.logσ)
DeepStructuredMixtures.setvariance!(k::ArdSEProduct, v::AbstractFloat) = (k.logσ = v)
DeepStructuredMixtures.getlengthscales(k::ArdSEProduct; logscale=false) = logscale ? k.logℓ : exp.(k.logℓ)
DeepStructuredMixtures.setlengthscale!(k::ArdSEProduct{T}, l::AbstractVector{T}) where {T} = (k.logℓ[:] = l)
# the per-dimension squared distances GaussianProcess stores in gp.P (the array ArdSE builds; the device never reads it)
DeepStructuredMixtures.getdistancematrix(k::ArdSEProduct{T}, x1::AbstractMatrix{T}, x2::AbstractMatrix{T}) where {T} =
    DeepStructuredMixtures.getdistancematrix(ArdSE(k.logℓ, k.logσ), x1, x2)

# ---------------------------------------------------------------------------------------------- Matérn 3/2 and 5/2
"""
    IsoMatern32(logℓ, logσ), IsoMatern52(logℓ, logσ), ArdMatern32(logℓ, logσ), ArdMatern52(logℓ, logσ)

Matérn kernels in the distance form (GPML's covMaterniso / covMaternard): r² = Σ_d (a_d - b_d)² / ℓ_d², s = √(2ν) r,
k = σ² (1 + s) e^(-s) for ν = 3/2 and σ² (1 + s + s²/3) e^(-s) for ν = 5/2.  The iso types have IsoSE's fields, the ARD types
ArdSE's.  Not kernels of the reference: they live on the device only (kinds 5-8), with just the methods GaussianProcess
(src/gaussianprocess.jl:50-58) and params / setparams! (:139-161) call on a kernel.  Their gradients are the true derivatives,
written into ∂ℓ and ∂σ by updategradients!.
"""
mutable struct IsoMatern32{T<:AbstractFloat} <: DeepStructuredMixtures.IsoKernel
    logℓ::T
    logσ::T
    ∂ℓ::T
    ∂σ::T
end
mutable struct IsoMatern52{T<:AbstractFloat} <: DeepStructuredMixtures.IsoKernel
    logℓ::T
    logσ::T
    ∂ℓ::T
    ∂σ::T
end
mutable struct ArdMatern32{T<:AbstractFloat} <: DeepStructuredMixtures.ArdKernel
    logℓ::Vector{T}
    logσ::T
    ∂ℓ::Vector{T}
    ∂σ::T
end
mutable struct ArdMatern52{T<:AbstractFloat} <: DeepStructuredMixtures.ArdKernel
    logℓ::Vector{T}
    logσ::T
    ∂ℓ::Vector{T}
    ∂σ::T
end
IsoMatern32(logℓ, logσ) = IsoMatern32(logℓ, logσ, zero(logℓ), zero(logσ))
IsoMatern52(logℓ, logσ) = IsoMatern52(logℓ, logσ, zero(logℓ), zero(logσ))
ArdMatern32(logℓ, logσ) = ArdMatern32(logℓ, logσ, zero(logℓ), zero(logσ))
ArdMatern52(logℓ, logσ) = ArdMatern52(logℓ, logσ, zero(logℓ), zero(logσ))
const IsoMatern = Union{IsoMatern32,IsoMatern52}
const ArdMatern = Union{ArdMatern32,ArdMatern52}
DeepStructuredMixtures.getvariance(k::Union{IsoMatern,ArdMatern}; logscale=false) = logscale ? k.logσ : exp(2 * k.logσ)
DeepStructuredMixtures.getstd(k::Union{IsoMatern,ArdMatern}) = exp(k.logσ)
DeepStructuredMixtures.setvariance!(k::Union{IsoMatern,ArdMatern}, v::AbstractFloat) = (k.logσ = v)
DeepStructuredMixtures.getlengthscales(k::IsoMatern; logscale=false) = logscale ? k.logℓ : exp(k.logℓ)
DeepStructuredMixtures.getlengthscales(k::ArdMatern; logscale=false) = logscale ? k.logℓ : exp.(k.logℓ)
DeepStructuredMixtures.setlengthscale!(k::IsoMatern, l::AbstractFloat) = (k.logℓ = l)
DeepStructuredMixtures.setlengthscale!(k::ArdMatern, l::AbstractVector) = (k.logℓ[:] = l)
# the distance arrays GaussianProcess stores in gp.P (those IsoSE and ArdSE build; the device never reads them)
DeepStructuredMixtures.getdistancematrix(k::IsoMatern, x1::AbstractMatrix, x2::AbstractMatrix) =
    DeepStructuredMixtures.getdistancematrix(IsoSE(k.logℓ, k.logσ), x1, x2)
DeepStructuredMixtures.getdistancematrix(k::ArdMatern, x1::AbstractMatrix, x2::AbstractMatrix) =
    DeepStructuredMixtures.getdistancematrix(ArdSE(k.logℓ, k.logσ), x1, x2)

# ---------------------------------------------------------------------------------------------- rational quadratic
"""
    IsoRQ(logℓ, logα, logσ), ArdRQ(logℓ, logα, logσ)

Rational quadratic kernels (GPML's covRQiso / covRQard): k = σ² (1 + w)^(-α), w = Σ_d (a_d - b_d)² / (2 α ℓ_d²), α = exp(logα).
IsoSE's / ArdSE's fields plus the shape logα and its gradient ∂α.  Not kernels of the reference: they live on the device only
(kinds 9 and 10); hyper-vector [logℓ..., logα, logσ, logNoise], gradient row [∂ℓ..., ∂α, ∂σ, ∂ϵ], all true derivatives.
"""
mutable struct IsoRQ{T<:AbstractFloat} <: DeepStructuredMixtures.IsoKernel
    logℓ::T
    logα::T
    logσ::T
    ∂ℓ::T
    ∂α::T
    ∂σ::T
end
mutable struct ArdRQ{T<:AbstractFloat} <: DeepStructuredMixtures.ArdKernel
    logℓ::Vector{T}
    logα::T
    logσ::T
    ∂ℓ::Vector{T}
    ∂α::T
    ∂σ::T
end
IsoRQ(logℓ, logα, logσ) = IsoRQ(logℓ, logα, logσ, zero(logℓ), zero(logα), zero(logσ))
ArdRQ(logℓ, logα, logσ) = ArdRQ(logℓ, logα, logσ, zero(logℓ), zero(logα), zero(logσ))
const RQ = Union{IsoRQ,ArdRQ}
DeepStructuredMixtures.getvariance(k::RQ; logscale=false) = logscale ? k.logσ : exp(2 * k.logσ)
DeepStructuredMixtures.getstd(k::RQ) = exp(k.logσ)
DeepStructuredMixtures.setvariance!(k::RQ, v::AbstractFloat) = (k.logσ = v)
DeepStructuredMixtures.getlengthscales(k::IsoRQ; logscale=false) = logscale ? k.logℓ : exp(k.logℓ)
DeepStructuredMixtures.getlengthscales(k::ArdRQ; logscale=false) = logscale ? k.logℓ : exp.(k.logℓ)
DeepStructuredMixtures.setlengthscale!(k::IsoRQ, l::AbstractFloat) = (k.logℓ = l)
DeepStructuredMixtures.setlengthscale!(k::ArdRQ, l::AbstractVector) = (k.logℓ[:] = l)
DeepStructuredMixtures.getdistancematrix(k::IsoRQ, x1::AbstractMatrix, x2::AbstractMatrix) =
    DeepStructuredMixtures.getdistancematrix(IsoSE(k.logℓ, k.logσ), x1, x2)
DeepStructuredMixtures.getdistancematrix(k::ArdRQ, x1::AbstractMatrix, x2::AbstractMatrix) =
    DeepStructuredMixtures.getdistancematrix(ArdSE(k.logℓ, k.logσ), x1, x2)

# ---------------------------------------------------------------------------------------------- library
const LIB = Ref{Ptr{Cvoid}}(C_NULL)
function lib()
    if LIB[] == C_NULL
        LIB[] = dlopen(get(ENV, "DSMGP_HIP_LIB", "libdsmgp_hip.so"))
    end
    return LIB[]
end
sym(s::Symbol) = dlsym(lib(), s)

const SHARE_FULL, SHARE_COPY, SHARE_PREFIX = Int32(0), Int32(1), Int32(2)      # DSMGP_SHARE_*
const AGG_MIXTURE, AGG_POE, AGG_GPOE, AGG_RBCM = Int32(0), Int32(1), Int32(2), Int32(3)   # DSMGP_AGG_*

kind(::IsoSE) = Int32(0)
kind(::ArdSE) = Int32(1)
kind(::IsoLinear) = Int32(2)
kind(::ArdLinear) = Int32(3)     # DSMGP_KIND_ARD_LINEAR: sum_d a_d b_d / ℓ_d² (the reference's own methods cannot fit it, src/kernels.jl:232,247)
kind(::ArdSEProduct) = Int32(4)  # DSMGP_KIND_ARD_SE_PRODUCT: σ² exp(-½ Σ_d (a_d - b_d)² / ℓ_d²), not a kernel of the reference
kind(::IsoMatern32) = Int32(5)   # DSMGP_KIND_ISO_MATERN32: σ² (1 + s) e^(-s), s = √3 r; not kernels of the reference
kind(::IsoMatern52) = Int32(6)   # DSMGP_KIND_ISO_MATERN52: σ² (1 + s + s²/3) e^(-s), s = √5 r
kind(::ArdMatern32) = Int32(7)   # DSMGP_KIND_ARD_MATERN32: as 5 with one ℓ_d per dimension
kind(::ArdMatern52) = Int32(8)   # DSMGP_KIND_ARD_MATERN52: as 6 with one ℓ_d per dimension
kind(::IsoRQ) = Int32(9)         # DSMGP_KIND_ISO_RQ: σ² (1 + w)^(-α), w = r² / (2 α); not kernels of the reference
kind(::ArdRQ) = Int32(10)        # DSMGP_KIND_ARD_RQ: as 9 with one ℓ_d per dimension
# hyper-vector of one kernel id on the reference's log scale, [logℓ..., logσ, logNoise] (src/gaussianprocess.jl:141-161)
loghyp(k::IsoSE, ln) = Float64[k.logℓ, k.logσ, ln]
loghyp(k::ArdSE, ln) = Float64[k.logℓ..., k.logσ, ln]
loghyp(k::IsoLinear, ln) = Float64[k.logℓ, 0.0, ln]             # the variance slot is a dummy (src/kernels.jl:181-183)
loghyp(k::ArdLinear, ln) = Float64[k.logℓ..., 0.0, ln]          # ... here too (src/kernels.jl:216-218)
loghyp(k::ArdSEProduct, ln) = Float64[k.logℓ..., k.logσ, ln]    # the layout of ArdSE
loghyp(k::IsoMatern, ln) = Float64[k.logℓ, k.logσ, ln]          # the layout of IsoSE
loghyp(k::ArdMatern, ln) = Float64[k.logℓ..., k.logσ, ln]       # the layout of ArdSE
loghyp(k::IsoRQ, ln) = Float64[k.logℓ, getfield(k, :logα), k.logσ, ln]      # the shape sits between the length-scales and logσ
loghyp(k::ArdRQ, ln) = Float64[k.logℓ..., getfield(k, :logα), k.logσ, ln]

# ---------------------------------------------------------------------------------------------- session
"One device context + the leaf table of one model (or of one stand-alone GaussianProcess)."
mutable struct Session
    h::Ptr{Cvoid}
    leaves::Vector{GPNode}                 # leaf l of the ABI (0-based there) = leaves[l + 1]: order of getLeaves(root)
    gps::Vector{GaussianProcess}           # leaves[l].dist, or the single GP
    index::IdDict{Any,Int}                 # GaussianProcess -> position in gps
    leafmll::Vector{Float64}
    info::Vector{Int32}
    grad::Matrix{Float64}                  # stride x L, column l = [∂ℓ..., ∂σ, ∂ϵ] of leaf l (src/gaussianprocess.jl:212-214)
    stride::Int
    testkey::UInt                          # hash of the registered test set (dsmgp_set_test is called once per test set)
    testptr::Vector{Int64}
    census::Dict{Symbol,Any}
    fitted::Bool
    targets::Int                           # columns of the last solve_targets (0: none)
    testnt::Int                            # rows of the registered test set
end

const SESSIONS = IdDict{Any,Session}()     # root node (or GaussianProcess) -> session
const OWNER = IdDict{Any,Session}()        # GaussianProcess -> the session whose leaf it is

lasterror(h) = unsafe_string(ccall(sym(:dsmgp_last_error), Cstring, (Ptr{Cvoid},), h))
chk(s::Session, rc) = rc == 0 ? nothing : error("dsmgp error $rc: " * lasterror(s.h))

function newsession(device::Integer)
    r = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall(sym(:dsmgp_create), Cint, (Int32, Ref{Ptr{Cvoid}}), Int32(device), r)
    rc == 0 || error("dsmgp_create: " * lasterror(C_NULL))        # no GPU: the path has no CPU fallback
    s = Session(r[], GPNode[], GaussianProcess[], IdDict{Any,Int}(), Float64[], Int32[], zeros(0, 0), 0, UInt(0), Int64[],
                Dict{Symbol,Any}(), false, 0, 0)
    finalizer(x -> (x.h != C_NULL && ccall(sym(:dsmgp_destroy), Cint, (Ptr{Cvoid},), x.h); x.h = C_NULL), s)
    return s
end

"Upload the training data and the leaf table (dsmgp_set_train / dsmgp_set_leaves).  gp.x are views of the rows of the
training matrix and gp.y is mean-subtracted (src/gaussianprocess.jl:72-74), so X and y are rebuilt from the leaves."
function upload!(s::Session, gps::Vector, obs::Vector{Vector{Int}}, kernelids::Vector{Int})
    N = maximum(maximum, obs)
    Dm = size(gps[1].x, 2)
    X = zeros(Float64, N, Dm)
    y = zeros(Float64, N)
    for (gp, o) in zip(gps, obs)
        X[o, :] = gp.x
        y[o] = gp.y .+ gp.mean.m
    end
    GC.@preserve X y chk(s, ccall(sym(:dsmgp_set_train), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Int32),
                                  s.h, X, y, N, Dm))
    ptr = Int64[0]
    for o in obs
        push!(ptr, ptr[end] + length(o))
    end
    idx = Int64.(reduce(vcat, obs)) .- 1                         # 1-based in Julia, 0-based in the ABI; ascending per leaf
    kid = Int32.(kernelids .- 1)
    m = Float64[gp.mean.m for gp in gps]
    GC.@preserve ptr idx kid m chk(s, ccall(sym(:dsmgp_set_leaves), Cint,
        (Ptr{Cvoid}, Int32, Ptr{Int64}, Ptr{Int64}, Ptr{Int32}, Ptr{Float64}), s.h, length(gps), ptr, idx, kid, m))
    s.gps = collect(gps)
    empty!(s.index)
    for (l, gp) in enumerate(gps)
        s.index[gp] = l
        OWNER[gp] = s
    end
    s.leafmll = fill(NaN, length(gps))
    s.info = zeros(Int32, length(gps))
    s.stride = maximum(sum(DeepStructuredMixtures.nparams(gp)) for gp in gps)
    s.grad = zeros(s.stride, length(gps))
    s.testkey = UInt(0)
    s.fitted = false
    return s
end

"attach!(model; device = 0): route the hot-path methods of `model` to the GPU.  Returns the session."
function attach!(model::Union{DSMGP,PoE,gPoE,rBCM}; device::Integer = 0)
    return attach!(model.root; device = device)
end
function attach!(root::Union{GPSumNode,GPSplitNode}; device::Integer = 0)
    s = newsession(device)
    s.leaves = getLeaves(root)
    upload!(s, [l.dist for l in s.leaves], [l.obs for l in s.leaves], [l.kernelid for l in s.leaves])
    settree!(s, root)
    SESSIONS[root] = s
    return s
end

"The tree as the flat arrays dsmgp_set_tree takes (breadth-first, the children of a node consecutive, 0-based indices): kind
0 region / 1 split / 2 sum, first child, number of children, split dimension, ascending thresholds (column i of a thr_ld x
n_nodes matrix = node i, the last one its upper bound), leaf index of a region in the session's leaf table.  After it the
routing of predict (getchild, src/common.jl:101-122, walked per node in :181-196,275-292) runs on the device."
function settree!(s::Session, root)
    nodes = Any[root]
    kind = Int8[]; first = Int64[]; nchild = Int64[]; sdim = Int64[]; leaf = Int64[]; thr = Vector{Float64}[]
    leafidx = Dict(l.id => i - 1 for (i, l) in enumerate(s.leaves))
    i = 1
    while i <= length(nodes)
        nd = nodes[i]
        if nd isa GPNode
            push!(kind, Int8(0)); push!(first, 0); push!(nchild, 0); push!(sdim, 0); push!(leaf, leafidx[nd.id]); push!(thr, Float64[])
        else
            ch = children(nd)
            push!(kind, nd isa GPSplitNode ? Int8(1) : Int8(2))
            push!(first, length(nodes))            # 0-based index of the first child: it is appended next
            push!(nchild, length(ch)); push!(leaf, -1)
            push!(sdim, nd isa GPSplitNode ? nd.split[1][1] - 1 : 0)
            push!(thr, nd isa GPSplitNode ? Float64[t for (_, t) in nd.split] : Float64[])
            append!(nodes, ch)
        end
        i += 1
    end
    ld = max(1, maximum(length, thr))
    T = fill(Inf, ld, length(nodes))
    for (j, t) in enumerate(thr)
        T[1:length(t), j] = t
    end
    GC.@preserve kind first nchild sdim T leaf chk(s, ccall(sym(:dsmgp_set_tree), Cint,
        (Ptr{Cvoid}, Int64, Ptr{Int8}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Int64, Ptr{Int64}),
        s.h, length(nodes), kind, first, nchild, sdim, T, ld, leaf))
end
function detach!(root)
    s = pop!(SESSIONS, root, nothing)
    if s !== nothing
        foreach(gp -> delete!(OWNER, gp), s.gps)
        finalize(s)
    end
end
session(root) = get(() -> error("DSMGPHip: call attach!(model) first"), SESSIONS, root)

"Session of a GaussianProcess that is not a leaf of an attached model: a one-leaf table, created on first use."
function session(gp::GaussianProcess)
    haskey(OWNER, gp) && return OWNER[gp]
    s = newsession(0)
    upload!(s, [gp], [collect(1:gp.N)], [1])
    SESSIONS[gp] = s
    return s
end

"dsmgp_set_hyper for every kernel id, from the leaves' current fields: setparams!(spn, hyp) (src/optimize.jl:188-198) gives
every leaf of an id the same vector, so the first leaf of each id speaks for it."
function pushhyper!(s::Session, kernelids)
    seen = Set{Int}()
    for (gp, id) in zip(s.gps, kernelids)
        id in seen && continue
        push!(seen, id)
        h = loghyp(gp.kernel, gp.logNoise.value)
        GC.@preserve h chk(s, ccall(sym(:dsmgp_set_hyper), Cint, (Ptr{Cvoid}, Int32, Int32, Ptr{Float64}, Int32),
                                    s.h, Int32(id - 1), kind(gp.kernel), h, Int32(length(h))))
    end
end

function runfit!(s::Session)
    L = length(s.gps)
    sec = Ref{Float64}(0.0)
    mllv, info = s.leafmll, s.info
    GC.@preserve mllv info chk(s, ccall(sym(:dsmgp_fit), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Int32}, Ref{Float64}),
                                        s.h, mllv, info, sec))
    bad = findfirst(!=(0), info)
    bad === nothing || throw(PosDefException(Int(info[bad])))   # LAPACK's info, which src/gaussianprocess.jl:101 ignores
    s.fitted = true
    return sec[]
end

# ---------------------------------------------------------------------------------------------- fit!
"""
    fit!(spn, D, gpmap; τ = 0.05)      (src/fit.jl:71-122)

The decisions of the reference's loop -- main leaf `argmax(D[:,j] .* D[j,:])`, processing order by `counts`, the arm of
`fitcontained!` -- are taken here exactly as there; instead of factorising leaf by leaf they are recorded as
`(op, src, plen)` and executed in one batched call.  COPY (`:132-143`) and PREFIX (`chol_continue!`, `:276-278`) are
exact and kept; the row-deletion arm (`:174-201`) is numerically defective in the reference (SURVEY F4) and becomes a
full factorisation -- `census(spn)[:lowrank_leaves]` lists the leaves it would have taken.  Returns seconds, as `@elapsed`
does there.
"""
function fit!(spn::Union{GPSumNode,GPSplitNode}, D::Matrix, gpmap::BiDict; τ = 0.05)
    s = session(spn)
    leaves = s.leaves                                           # fixed order: leaf l of the device table
    n = length(leaves)
    pos = Dict(l.id => i for (i, l) in enumerate(leaves))       # node id -> device leaf (1-based)
    counts = zeros(Int, n)
    S = Vector{Int}(undef, n)                                   # main leaf of j, in gpmap numbering
    for j in 1:n
        i = argmax(D[:, j] .* D[j, :])                          # :79
        counts[i] += 1
        S[j] = i
    end
    order = sort(collect(1:n), by = j -> counts[j])             # :86 (gpmap numbering; sort is stable like sort!)
    node(j) = leaves[pos[gpmap.fx[j]]]
    op = fill(SHARE_FULL, n); src = fill(Int32(-1), n); plen = zeros(Int64, n)      # indexed by DEVICE leaf
    arm = fill(:full, n)
    processed = falses(n)
    for j in order
        processed[j] && continue
        i = S[j]
        processed[i] = true                                     # :97-100: the main leaf is factorised in full
        processed[j] = true
        i == j && continue
        jn, mn = node(j), node(i)
        dj, di = pos[jn.id], pos[mn.id]
        (mn.kernelid != jn.kernelid || first(jn.obs) < first(mn.obs)) && continue          # :107-112
        ione = D[i, j] == one(eltype(D))
        jone = D[j, i] == one(eltype(D))
        if ione && jone                                         # identical observation sets (:132-143)
            arm[dj] = :copy
            if op[di] == SHARE_FULL
                op[dj], src[dj] = SHARE_COPY, Int32(di - 1)
            elseif op[di] == SHARE_COPY
                op[dj], src[dj] = SHARE_COPY, src[di]
            end
        elseif ione && !jone && τ > 0                           # j contains the main leaf (:208-292)
            p = mn.nobs
            if first(jn.obs) == first(mn.obs) && jn.nobs > p && jn.obs[1:p] == mn.obs
                arm[dj] = :prefix
                if op[di] == SHARE_FULL
                    op[dj], src[dj], plen[dj] = SHARE_PREFIX, Int32(di - 1), p
                end
            end
        elseif jone && !ione                                    # j is contained in the main leaf (:145-206)
            e = findfirst(==(last(jn.obs)), mn.obs)             # :168
            ndel = e - jn.nobs                                  # |setdiff(mainNode.obs[1:e], jNode.obs)| (:170)
            if ndel / jn.nobs < τ                               # :173
                arm[dj] = ndel > 0 ? :lowrank_as_full : :leading_as_full
            end
        end
    end
    s.census = Dict{Symbol,Any}(:full => count(==(:full), arm), :copy => count(==(:copy), arm),
                                :prefix => count(==(:prefix), arm), :lowrank_as_full => count(==(:lowrank_as_full), arm),
                                :leading_as_full => count(==(:leading_as_full), arm),
                                :lowrank_leaves => [leaves[l].id for l in findall(==(:lowrank_as_full), arm)],
                                :leading_leaves => [leaves[l].id for l in findall(==(:leading_as_full), arm)])
    pushhyper!(s, [l.kernelid for l in leaves])
    GC.@preserve op src plen chk(s, ccall(sym(:dsmgp_set_sharing), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}, Ptr{Int64}),
                                          s.h, op, src, plen))
    return runfit!(s)
end

"Census of the last fit!: counts of the reference's arms and the ids of the leaves computed in full instead."
census(spn) = session(spn).census

function fit_naive!(spn::Union{GPSplitNode,GPSumNode})          # src/fit.jl:294-304
    s = session(spn)
    pushhyper!(s, [l.kernelid for l in s.leaves])
    chk(s, ccall(sym(:dsmgp_set_sharing), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}, Ptr{Int64}), s.h, C_NULL, C_NULL, C_NULL))
    return runfit!(s)
end

# ---------------------------------------------------------------------------------------------- single GP
"update_cholesky!(gp) (src/gaussianprocess.jl:82-108).  A leaf of an attached model is refitted with its whole table
(one batched call: that is what fit! does there, leaf by leaf); any other GP has a one-leaf session of its own."
function update_cholesky!(gp::GaussianProcess)
    s = session(gp)
    pushhyper!(s, isempty(s.leaves) ? [1] : [l.kernelid for l in s.leaves])
    isempty(s.leaves) && chk(s, ccall(sym(:dsmgp_set_sharing), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}, Ptr{Int64}),
                                      s.h, C_NULL, C_NULL, C_NULL))
    runfit!(s)
    return gp
end

"mll(gp) (src/gaussianprocess.jl:163): the per-leaf value dsmgp_fit returned (−(y·α + logdet + N log 2π)/2 with y·α = z·z)."
function mll(gp::GaussianProcess)
    s = session(gp)
    s.fitted || update_cholesky!(gp)
    return s.leafmll[s.index[gp]]
end

"prediction(gp, xtest) (src/gaussianprocess.jl:131-137) -> (μ, Σ).  Only diag(Σ) is ever consumed (src/common.jl:136,147);
Σ comes back as a Diagonal (K_tt and VᵀV are never formed), noise added, no ϵ, no clamp (that is the caller's, :137)."
function prediction(gp::GaussianProcess, xtest::AbstractMatrix)
    s = session(gp)
    s.fitted || update_cholesky!(gp)
    l = s.index[gp]
    xt = Matrix{Float64}(xtest)
    nt = size(xt, 1)
    ptr = zeros(Int64, length(s.gps) + 1)
    ptr[(l + 1):end] .= nt                                      # only leaf l predicts
    idx = Int64.(0:(nt - 1))
    μ = Vector{Float64}(undef, nt); σ² = similar(μ)
    GC.@preserve xt ptr idx μ σ² chk(s, ccall(sym(:dsmgp_predict_leaves), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Int64, Int32, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}),
        s.h, xt, nt, size(xt, 2), ptr, idx, μ, σ²))
    s.testkey = UInt(0)
    return μ, Diagonal(σ²)
end

"predict_cov(s, leaf; with_noise=true): the full Σ of prediction(gp, xtest) as the reference writes it (src/gaussianprocess.jl:110-137)
for leaf `leaf` (1-based, the order of `s.leaves`) over ITS routed rows of the registered test set, in route order:
K_tt − VᵀV (+ exp(2 logNoise) I), from dsmgp_predict_cov.  Needs a prediction on the current fit (dsmgp_predict_run); symmetric to
the bit.  A leaf without routed rows gives a 0×0 matrix."
function predict_cov(s::Session, leaf::Integer; with_noise::Bool=true)
    ptr = Vector{Int64}(undef, length(s.leaves) + 1)
    GC.@preserve ptr chk(s, ccall(sym(:dsmgp_routes), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}), s.h, ptr, C_NULL))
    nt = Int(ptr[leaf + 1] - ptr[leaf])
    Σ = Matrix{Float64}(undef, nt, nt)
    nt == 0 && return Σ
    sec = Ref{Float64}(0.0)
    GC.@preserve Σ chk(s, ccall(sym(:dsmgp_predict_cov), Cint, (Ptr{Cvoid}, Int32, Int32, Ptr{Float64}, Int64, Ref{Float64}),
                           s.h, Int32(leaf - 1), Int32(with_noise), Σ, nt, sec))
    return Σ
end

"predict_sample(s, eps; with_noise=false, jitter=nothing): joint posterior draws of every leaf GP over its routed rows of the
registered test set from the caller's standard normals (dsmgp_predict_sample; needs a prediction on the current fit).  `eps` is
`route_total × S` in the entry order of the per-leaf moments; returns (draws, info): draws `route_total × S`, column s =
μ + chol(Σ_l + jitter·I) eps_l[:, s] per leaf (leaves are independent of each other), and info per leaf: 0, the order of the first
leading minor that is not positive definite, or −1 for a leaf whose fit failed (NaN entries either way).  `jitter` defaults to the
reference's ϵ = 1e-8 without noise and to 0 with it.  The factors stay on the device for the next call with the same
(with_noise, jitter).  (The scalar `jitter` goes by value: the call is written with @ccall.)"
function predict_sample(s::Session, eps::AbstractMatrix{<:Real}; with_noise::Bool=false, jitter::Union{Nothing,Real}=nothing)
    ptr = Vector{Int64}(undef, length(s.leaves) + 1)
    GC.@preserve ptr chk(s, ccall(sym(:dsmgp_routes), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}), s.h, ptr, C_NULL))
    nr = Int(ptr[end])
    size(eps, 1) == nr || throw(ArgumentError("predict_sample: eps must have route_total = $nr rows"))
    E = Matrix{Float64}(eps)
    S = size(E, 2)
    jit = Float64(jitter === nothing ? (with_noise ? 0.0 : 1e-8) : jitter)
    out = Matrix{Float64}(undef, nr, S)
    info = zeros(Int32, length(s.leaves))
    sec = Ref{Float64}(0.0)
    fptr = sym(:dsmgp_predict_sample)
    GC.@preserve E out info chk(s, @ccall $fptr(s.h::Ptr{Cvoid}, Int32(with_noise)::Int32, jit::Float64, pointer(E)::Ptr{Float64},
                                                max(1, nr)::Int64, Int32(S)::Int32, pointer(out)::Ptr{Float64}, max(1, nr)::Int64,
                                                pointer(info)::Ptr{Int32}, sec::Ref{Float64})::Cint)
    return out, info
end

"predict_cov_factor(s, leaf): the lower Cholesky factor of leaf `leaf` (1-based) the last predict_sample made, over its routed rows
(dsmgp_predict_cov_factor; inspection): the strict upper triangle is exactly 0.  A leaf without routed rows gives a 0×0 matrix."
function predict_cov_factor(s::Session, leaf::Integer)
    ptr = Vector{Int64}(undef, length(s.leaves) + 1)
    GC.@preserve ptr chk(s, ccall(sym(:dsmgp_routes), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}), s.h, ptr, C_NULL))
    nt = Int(ptr[leaf + 1] - ptr[leaf])
    Lc = zeros(Float64, nt, nt)
    nt == 0 && return Lc
    GC.@preserve Lc chk(s, ccall(sym(:dsmgp_predict_cov_factor), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64),
                            s.h, Int32(leaf - 1), Lc, nt))
    return Lc
end

"loo(s): leave-one-out cross-validation of every leaf GP on the current fit (GPML §5.4.2, eqs. 5.10–5.12; dsmgp_loo), mean and
hyper-parameters held fixed.  Returns (μ, σ², lpd): per leaf, in the order of `s.leaves`, the moments at its own observations (in
the order of its observation list) of the leaf's GP fitted without that observation — σ² with noise and the fit's 1e-8 jitter —
and the leaf's summed LOO log predictive density.  Leaves whose fit reported info ≠ 0 come back as NaN.  L⁻ᵀ is reused when
updategradients! or loo already built it for this fit."
function loo(s::Session)
    L = length(s.leaves)
    cnt = [length(lf.obs) for lf in s.leaves]
    tot = sum(cnt)
    μ = Vector{Float64}(undef, tot)
    σ² = Vector{Float64}(undef, tot)
    lpd = Vector{Float64}(undef, L)
    sec = Ref{Float64}(0.0)
    GC.@preserve μ σ² lpd chk(s, ccall(sym(:dsmgp_loo), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Float64}),
                                       s.h, μ, σ², lpd, sec))
    off = cumsum(vcat(0, cnt))
    return [μ[off[l]+1:off[l+1]] for l in 1:L], [σ²[off[l]+1:off[l+1]] for l in 1:L], lpd
end

"kfold(s, fold, K; want_var=true): k-fold cross-validation of every leaf GP on the current fit (dsmgp_kfold; the multiple-fold
residual formulas), mean and hyper-parameters held fixed.  `fold[r]` is the label of training row r in the ABI's numbering,
-1 (never held out) and 0 … K-1.  Returns (μ, σ², lpd, info): per leaf, in the order of `s.leaves` and aligned with its observation
list, the joint held-out moments of the row's block (NaN for label -1; `σ² === nothing` with `want_var=false`, and none of the
work behind it runs), and the `L × K` tables of the blocks' joint log predictive densities and flags.  L⁻ᵀ is reused as by loo."
function kfold(s::Session, fold::AbstractVector{<:Integer}, K::Integer; want_var::Bool=true)
    L = length(s.leaves)
    cnt = [length(lf.obs) for lf in s.leaves]
    tot = sum(cnt)
    f = Vector{Int32}(fold)
    μ = Vector{Float64}(undef, tot)
    σ² = Vector{Float64}(undef, want_var ? tot : 0)
    lpd = Matrix{Float64}(undef, L, K)
    info = Matrix{Int32}(undef, L, K)
    sec = Ref{Float64}(0.0)
    GC.@preserve f μ σ² lpd info chk(s, ccall(sym(:dsmgp_kfold), Cint,
        (Ptr{Cvoid}, Ptr{Int32}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ref{Float64}),
        s.h, f, Int32(K), μ, want_var ? pointer(σ²) : Ptr{Float64}(C_NULL), lpd, info, sec))
    off = cumsum(vcat(0, cnt))
    return [μ[off[l]+1:off[l+1]] for l in 1:L], (want_var ? [σ²[off[l]+1:off[l+1]] for l in 1:L] : nothing), lpd, info
end

"kfold_seconds(s): device seconds of the last kfold, split into (L⁻ᵀ inversion — 0 when it was current, packing and G_FF,
factorisation, solves and moments)."
function kfold_seconds(s::Session)
    out = zeros(Float64, 4)
    GC.@preserve out chk(s, ccall(sym(:dsmgp_kfold_seconds), Cint, (Ptr{Cvoid}, Ptr{Float64}), s.h, out))
    return out
end

"predict_gradients(s; want_var=true): the gradients of the predictive mean and variance of every (leaf, routed test row) entry of
the last prediction with respect to the test point (dsmgp_predict_gradients; needs the prediction of the registered rows on the
current fit).  Returns (dmu, dvar), both `route_total × D` in the entry order of the per-leaf moments; `dvar === nothing` with
`want_var=false`, which computes neither L⁻ᵀ nor K_tn K_y⁻¹.  Entries of leaves whose fit reported info ≠ 0 come back as NaN."
function predict_gradients(s::Session; want_var::Bool=true)
    ptr = Vector{Int64}(undef, length(s.leaves) + 1)
    GC.@preserve ptr chk(s, ccall(sym(:dsmgp_routes), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}), s.h, ptr, C_NULL))
    nr = Int(ptr[end])
    D = size(s.gps[1].x, 2)
    dmu = Matrix{Float64}(undef, nr, D)
    dvar = want_var ? Matrix{Float64}(undef, nr, D) : nothing
    sec = Ref{Float64}(0.0)
    GC.@preserve dmu dvar chk(s, ccall(sym(:dsmgp_predict_gradients), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Ref{Float64}),
                                       s.h, dmu, want_var ? pointer(dvar) : Ptr{Float64}(C_NULL), Int64(max(nr, 1)), sec))
    return dmu, dvar
end

"aggregate_gradients(s; plain=false, prior_kernel_id=0): the gradients of the aggregated prediction of the last `predict` with
respect to the test point, reduced on the device over the leaves of every registered test row (dsmgp_aggregate_gradients; family,
coefficients and groups are those of that prediction's dsmgp_aggregate).  Returns (dmu, dvar), both `n_t × D`.  `plain` is true for
a model whose root is a single GP; `prior_kernel_id` is the zero-based kernel id of the first leaf of an rBCM.  The per-entry
gradients are made on the device first unless `predict_gradients(s)` left them for this prediction."
function aggregate_gradients(s::Session; plain::Bool=false, prior_kernel_id::Integer=0)
    nt = s.testnt
    D = size(s.gps[1].x, 2)
    dmu = Matrix{Float64}(undef, nt, D)
    dvar = Matrix{Float64}(undef, nt, D)
    sec = Ref{Float64}(0.0)
    GC.@preserve dmu dvar chk(s, ccall(sym(:dsmgp_aggregate_gradients), Cint,
        (Ptr{Cvoid}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Int64, Ref{Float64}),
        s.h, Int32(plain), Int32(prior_kernel_id), dmu, dvar, Int64(max(nt, 1)), sec))
    return dmu, dvar
end

"aggregate_columns(s, family, coef, group, G; plain=false, prior_kernel_id=0): `dsmgp_aggregate` for every column of the last
`solve_targets` on the prediction of the registered rows (dsmgp_aggregate_columns).  `coef` (length L, or `nothing` for an rBCM)
and `group` (zero-based root child per leaf, or `nothing`) serve all columns.  Returns (mu, var), both `n_t × Q`."
function aggregate_columns(s::Session, family::Integer, coef, group, G::Integer; plain::Bool=false, prior_kernel_id::Integer=0)
    nt, Q = s.testnt, s.targets
    μ = Matrix{Float64}(undef, nt, Q); σ² = similar(μ)
    cf = coef === nothing ? nothing : Vector{Float64}(coef)
    gr = group === nothing ? nothing : Vector{Int32}(group)
    sec = Ref{Float64}(0.0)
    GC.@preserve cf gr μ σ² chk(s, ccall(sym(:dsmgp_aggregate_columns), Cint,
        (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Int32}, Int32, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Int64, Ref{Float64}),
        s.h, Int32(family), cf === nothing ? Ptr{Float64}(C_NULL) : pointer(cf), gr === nothing ? Ptr{Int32}(C_NULL) : pointer(gr),
        Int32(G), Int32(plain), Int32(prior_kernel_id), μ, σ², Int64(max(nt, 1)), sec))
    return μ, σ²
end

"aggregate_columns_gradients(s; plain=false, prior_kernel_id=0): the input gradients of `aggregate_columns`' moments, with its
family and coefficients (dsmgp_aggregate_columns_gradients; `aggregate_columns` first).  Returns (dmu, dvar), both `n_t × D × Q`."
function aggregate_columns_gradients(s::Session; plain::Bool=false, prior_kernel_id::Integer=0)
    nt, Q = s.testnt, s.targets
    D = size(s.gps[1].x, 2)
    dmu = Array{Float64,3}(undef, nt, D, Q)
    dvar = Array{Float64,3}(undef, nt, D, Q)
    sec = Ref{Float64}(0.0)
    GC.@preserve dmu dvar chk(s, ccall(sym(:dsmgp_aggregate_columns_gradients), Cint,
        (Ptr{Cvoid}, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Int64, Ref{Float64}),
        s.h, Int32(plain), Int32(prior_kernel_id), dmu, dvar, Int64(max(nt, 1)), sec))
    return dmu, dvar
end

"loo_gradients(s): the true derivatives of every leaf's LOO log predictive density with respect to its log-scale hyper-vector
(GPML §5.4.2, eq. 5.13; dsmgp_loo_gradients), mean held fixed.  Returns (g, lpd): `g[:, l]` in the order [∂ℓ…, ∂σ, ∂ϵ] of
updategradients! for leaf `l` of `s.leaves` (every component the true derivative: no factor σ for IsoSE, true length-scale
derivatives for ArdSE; zeros past the leaf's hyper-vector) and `lpd`, the densities of `loo(s)`, same bits.  Leaves whose fit
reported info ≠ 0 come back as NaN.  Nothing is written to the kernels' gradient fields."
function loo_gradients(s::Session)
    L = length(s.leaves)
    g = Matrix{Float64}(undef, s.stride, L)
    lpd = Vector{Float64}(undef, L)
    sec = Ref{Float64}(0.0)
    GC.@preserve g lpd chk(s, ccall(sym(:dsmgp_loo_gradients), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int32, Ptr{Float64}, Ref{Float64}),
                                    s.h, g, Int32(s.stride), lpd, sec))
    return g, lpd
end

"solve_targets(s, Y; mean=nothing): several target columns over the same inputs on the current fit (dsmgp_solve_targets).  `Y` is
`N × Q` over the rows of the training data, `mean` `L × Q` with the constant mean of every leaf (the order of `s.leaves`) and
column (`nothing`: zeros).  Leaves Z = L⁻¹ (Y[obs, :] − mean) of every leaf resident on the device and returns the `L × Q` table of
log marginal likelihoods.  Nothing the fit left is touched; leaves whose fit reported info ≠ 0 have NaN rows."
function solve_targets(s::Session, Y::AbstractMatrix; mean::Union{Nothing,AbstractMatrix}=nothing)
    Yc = Matrix{Float64}(Y)
    N, Q = size(Yc)
    L = length(s.leaves)
    M = mean === nothing ? nothing : Matrix{Float64}(mean)
    M === nothing || size(M) == (L, Q) || throw(DimensionMismatch("mean must be L × Q"))
    out = Matrix{Float64}(undef, L, Q)
    sec = Ref{Float64}(0.0)
    GC.@preserve Yc M out chk(s, ccall(sym(:dsmgp_solve_targets), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Int64, Int32, Int64, Ptr{Float64}, Ptr{Float64}, Ref{Float64}),
        s.h, Yc, Int64(N), Int32(Q), Int64(max(N, 1)), M === nothing ? Ptr{Float64}(C_NULL) : pointer(M), out, sec))
    s.targets = Q
    return out
end

"predict_targets(s): the predictive mean of every (leaf, routed test row) entry of the last prediction under every column of the
last solve_targets (dsmgp_predict_targets; needs both on the current fit): `route_total × Q`, in the entry order of the per-leaf
moments.  The predictive variance does not depend on the targets: it is the one of the prediction for every column."
function predict_targets(s::Session)
    ptr = Vector{Int64}(undef, length(s.leaves) + 1)
    GC.@preserve ptr chk(s, ccall(sym(:dsmgp_routes), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}), s.h, ptr, C_NULL))
    nr = Int(ptr[end])
    Q = s.targets
    μ = Matrix{Float64}(undef, nr, Q)
    sec = Ref{Float64}(0.0)
    GC.@preserve μ chk(s, ccall(sym(:dsmgp_predict_targets), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Ref{Float64}),
                            s.h, μ, Int64(max(nr, 1)), sec))
    return μ
end

"predict_targets_gradients(s): the gradient of the predictive mean of every (leaf, routed test row) entry of the last prediction
with respect to the test point, under every column of the last solve_targets (dsmgp_predict_columns_gradients; needs both on the
current fit): `route_total × D × Q`, in the entry order of the per-leaf moments; slice `[:, :, q]` has the layout of
predict_gradients' `dmu`.  The gradient of the variance does not depend on the targets: it is predict_gradients' `dvar` for
every column.  Entries of leaves whose fit reported info ≠ 0 come back as NaN."
function predict_targets_gradients(s::Session)
    ptr = Vector{Int64}(undef, length(s.leaves) + 1)
    GC.@preserve ptr chk(s, ccall(sym(:dsmgp_routes), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}), s.h, ptr, C_NULL))
    nr = Int(ptr[end])
    D = size(s.gps[1].x, 2)
    dmu = Array{Float64,3}(undef, nr, D, s.targets)
    sec = Ref{Float64}(0.0)
    GC.@preserve dmu chk(s, ccall(sym(:dsmgp_predict_columns_gradients), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Ref{Float64}),
                              s.h, dmu, Int64(max(nr, 1)), sec))
    return dmu
end

"targets_fetch(s, leaf): Z = L⁻¹ (Y[obs, :] − mean) of leaf `leaf` (1-based, the order of `s.leaves`) as the last solve_targets left
it, `n × Q` (dsmgp_targets_fetch; inspection)."
function targets_fetch(s::Session, leaf::Integer)
    n = length(s.leaves[leaf].obs)
    Z = Matrix{Float64}(undef, n, s.targets)
    GC.@preserve Z chk(s, ccall(sym(:dsmgp_targets_fetch), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}), s.h, Int32(leaf - 1), Z))
    return Z
end

"append_rows!(s, Xnew, ynew, add_ptr, add_idx; mean=nothing): append training rows to the fitted session without refactorising it
(dsmgp_append_rows).  `Xnew` is `m × D`, `ynew` has `m` entries; leaf `l` (the order of `s.leaves`) takes the rows
`Xnew[add_idx[add_ptr[l]+1:add_ptr[l+1]], :]` behind its list: `add_ptr` has `L + 1` entries starting at 0, `add_idx` holds 1-based
row numbers of `Xnew`, strictly ascending per leaf.  `mean`: the constant mean of every leaf from now on (`nothing`: unchanged).
Every factor owner keeps the leading ⌊n/128⌋ blocks of its factor and only the rest is factorised; a COPY leaf stays a COPY only
where it received the rows of its source; the registered test set, the resident targets and the gradient lists are dropped.  Needs
a current fit.  The node objects of the reference are not touched: the caller grows them.  Returns the device seconds.
`keep_test=true` (dsmgp_add_rows_keep_test): the registered test set stays registered -- the routes of its rows do not change -- and
the next prediction on the same rows resumes K_tn L⁻ᵀ from the block columns the call kept instead of sweeping it from block 0
(`resume_stats`); the set is dropped only where its new arena does not fit."
function append_rows!(s::Session, Xnew::AbstractMatrix, ynew::AbstractVector, add_ptr::AbstractVector{<:Integer},
                      add_idx::AbstractVector{<:Integer}; mean::Union{Nothing,AbstractVector}=nothing, keep_test::Bool=false)
    X = Matrix{Float64}(Xnew)
    y = Vector{Float64}(ynew)
    m, Dm = size(X)
    L = length(s.gps)
    length(y) == m || throw(DimensionMismatch("ynew needs one entry per row of Xnew"))
    length(add_ptr) == L + 1 || throw(DimensionMismatch("add_ptr needs L + 1 entries"))
    ptr = Vector{Int64}(add_ptr)
    idx = isempty(add_idx) ? Int64[0] : Vector{Int64}(add_idx) .- 1        # 1-based in Julia, 0-based in the ABI
    M = mean === nothing ? nothing : Vector{Float64}(mean)
    M === nothing || length(M) == L || throw(DimensionMismatch("mean needs one entry per leaf"))
    sec = Ref{Float64}(0.0)
    mllv, info = s.leafmll, s.info
    if keep_test
        GC.@preserve X y ptr idx M mllv info chk(s, ccall(sym(:dsmgp_add_rows_keep_test), Cint,
            (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Int32, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ref{Float64}),
            s.h, X, y, Int64(m), Int32(Dm), ptr, idx, M === nothing ? Ptr{Float64}(C_NULL) : pointer(M), mllv, info, sec))
        resume_stats(s).test_set_dropped == 0 || (s.testkey = UInt(0))
    else
        GC.@preserve X y ptr idx M mllv info chk(s, ccall(sym(:dsmgp_append_rows), Cint,
            (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Int32, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ref{Float64}),
            s.h, X, y, Int64(m), Int32(Dm), ptr, idx, M === nothing ? Ptr{Float64}(C_NULL) : pointer(M), mllv, info, sec))
        s.testkey = UInt(0)
    end
    s.targets = 0
    bad = findfirst(!=(0), info)
    bad === nothing || throw(PosDefException(Int(info[bad])))
    return sec[]
end

"append_stats(s): what the last append_rows! did (dsmgp_append_stats), as a named tuple: owners continued, leaves untouched,
bytes of factor and Dinv relocated (0: the call ran in place), block columns factorised, owners restarted from block 0, COPY
relations dissolved."
function append_stats(s::Session)
    out = zeros(Int64, 6)
    GC.@preserve out chk(s, ccall(sym(:dsmgp_append_stats), Cint, (Ptr{Cvoid}, Ptr{Int64}), s.h, out))
    return (owners_continued = out[1], leaves_untouched = out[2], bytes_relocated = out[3], block_columns_factorised = out[4],
            owners_restarted = out[5], copies_dissolved = out[6])
end

"resume_stats(s): what the last append_rows!(…; keep_test=true) kept of the registered test set and what the prediction after it
swept (dsmgp_resume_stats), as a named tuple: leaves that kept columns of K_tn L⁻ᵀ, block columns kept, bytes relocated (0: in
place), block columns swept by the resumed prediction (-1 until it has run), leaves swept from block 0, 1 if the test set had to be
dropped for lack of memory."
function resume_stats(s::Session)
    out = zeros(Int64, 6)
    GC.@preserve out chk(s, ccall(sym(:dsmgp_resume_stats), Cint, (Ptr{Cvoid}, Ptr{Int64}), s.h, out))
    return (leaves_kept = out[1], block_columns_kept = out[2], bytes_relocated = out[3], block_columns_swept = out[4],
            leaves_from_block_0 = out[5], test_set_dropped = out[6])
end

"download_vt(s, leaf): K_tn L⁻ᵀ of leaf `leaf` (1-based, the order of `s.leaves`) over its routed test rows and its training rows,
`nt × n` (dsmgp_download_vt; inspection).  Needs a prediction on the current fit."
function download_vt(s::Session, leaf::Integer)
    nt = Int(s.testptr[leaf + 1] - s.testptr[leaf])
    n = length(s.leaves[leaf].obs)
    V = Matrix{Float64}(undef, nt, n)
    GC.@preserve V chk(s, ccall(sym(:dsmgp_download_vt), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64), s.h, Int32(leaf - 1), V, Int64(max(nt, 1))))
    return V
end

"targets_gradients(s; col_weight=nothing): hyper-parameter gradients of the weighted sum of the per-column log marginal likelihoods
of the last solve_targets (dsmgp_mll_columns_gradients): `g[:, l] = Σ_q col_weight[l, q] ∂mll[l, q]/∂θ` in the layout and with the
conventions of updategradients! ([∂ℓ…, ∂σ, ∂ϵ]; zeros past the leaf's hyper-vector).  `col_weight` is `L × Q` (the order of
`s.leaves`), any sign, zero columns allowed; `nothing`: ones.  One inversion and one contraction per leaf whatever Q is.  Needs
solve_targets on the current fit; leaves whose fit reported info ≠ 0 come back as NaN.  Nothing is written to the kernels'
gradient fields."
function targets_gradients(s::Session; col_weight::Union{Nothing,AbstractMatrix}=nothing)
    L = length(s.leaves)
    W = col_weight === nothing ? nothing : Matrix{Float64}(col_weight)
    W === nothing || size(W) == (L, s.targets) || throw(DimensionMismatch("col_weight must be L × Q"))
    g = Matrix{Float64}(undef, s.stride, L)
    sec = Ref{Float64}(0.0)
    GC.@preserve g W chk(s, ccall(sym(:dsmgp_mll_columns_gradients), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int32, Ptr{Float64}, Ref{Float64}),
                                  s.h, g, Int32(s.stride), W === nothing ? Ptr{Float64}(C_NULL) : pointer(W), sec))
    return g
end

"loo_targets(s): leave-one-out moments of every leaf under every column of the last solve_targets, on the one factorisation
(dsmgp_loo_columns; GPML §5.4.2, eqs. 5.10-5.12 per column).  Returns (μ, σ², lpd): `μ[l]` is `n_l × Q` and `σ²[l]` of length `n_l`
(the same for every column: that of `loo(s)`, same bits), aligned with `s.leaves[l].obs`; `lpd` is `L × Q`.  Needs solve_targets on
the current fit; leaves whose fit reported info ≠ 0 come back as NaN."
function loo_targets(s::Session)
    L = length(s.leaves)
    Q = s.targets
    off = cumsum([0; [length(lf.obs) for lf in s.leaves]])
    n = off[end]
    μ = Matrix{Float64}(undef, n, Q)
    σ² = Vector{Float64}(undef, n)
    lpd = Matrix{Float64}(undef, L, Q)
    sec = Ref{Float64}(0.0)
    GC.@preserve μ σ² lpd chk(s, ccall(sym(:dsmgp_loo_columns), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ref{Float64}), s.h, μ, Int64(max(n, 1)), σ², lpd, sec))
    return [μ[off[l]+1:off[l+1], :] for l in 1:L], [σ²[off[l]+1:off[l+1]] for l in 1:L], lpd
end

"loo_targets_gradients(s; col_weight=nothing): `g[:, l] = Σ_q col_weight[l, q] ∂lpd[l, q]/∂θ`, every component the true derivative
as loo_gradients defines them (dsmgp_loo_columns_gradients; GPML eq. 5.13 summed over the columns: one inverse and one contraction
per leaf whatever Q is).  `col_weight` is `L × Q` (the order of `s.leaves`), finite and ≥ 0; `nothing`: ones; a leaf whose weights
are all zero gets a column of zeros.  Returns (g, lpd), `lpd` the `L × Q` table of loo_targets, same bits.  Needs solve_targets on
the current fit; leaves whose fit reported info ≠ 0 come back as NaN.  Nothing is written to the kernels' gradient fields."
function loo_targets_gradients(s::Session; col_weight::Union{Nothing,AbstractMatrix}=nothing)
    L = length(s.leaves)
    W = col_weight === nothing ? nothing : Matrix{Float64}(col_weight)
    W === nothing || size(W) == (L, s.targets) || throw(DimensionMismatch("col_weight must be L × Q"))
    g = Matrix{Float64}(undef, s.stride, L)
    lpd = Matrix{Float64}(undef, L, s.targets)
    sec = Ref{Float64}(0.0)
    GC.@preserve g W lpd chk(s, ccall(sym(:dsmgp_loo_columns_gradients), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, Ref{Float64}),
        s.h, g, Int32(s.stride), W === nothing ? Ptr{Float64}(C_NULL) : pointer(W), lpd, sec))
    return g, lpd
end

# ---------------------------------------------------------------------------------------------- predict
"Rows of `x` every leaf is asked to predict: sums forward all rows to all children, splits one child per row
(src/common.jl:181-196,275-292 with getchild :101-122)."
function route!(rows::Dict{Symbol,Vector{Int}}, node::GPNode, x, sel::Vector{Int})
    rows[node.id] = sel
end
function route!(rows, node::GPSumNode, x, sel)
    foreach(c -> route!(rows, c, x, sel), children(node))
end
function route!(rows, node::GPSplitNode, x, sel)
    idx = getchild(node, x[sel, :])
    for (k, c) in enumerate(children(node))
        route!(rows, c, x, sel[findall(idx .== k)])
    end
end
function routeall!(rows, node::GPNode, x, sel)                  # PoE family: every expert predicts every row (:198-208)
    rows[node.id] = sel
end
routeall!(rows, node, x, sel) = foreach(c -> routeall!(rows, c, x, sel), children(node))

"Product of the sum-node weights on every leaf's path: the nested log-domain recursion of _predict (src/common.jl:275-302)
is linear in (μ, μ², σ²), i.e. the flat mixture over the visited leaves with these weights."
function pathweights!(w::Dict{Symbol,Float64}, node::GPNode, acc::Float64)
    w[node.id] = exp(acc)
end
function pathweights!(w, node::GPSumNode, acc)
    for (k, c) in enumerate(children(node))
        pathweights!(w, c, acc + logweights(node)[k])
    end
end
pathweights!(w, node::GPSplitNode, acc) = foreach(c -> pathweights!(w, c, acc), children(node))

"Register the test rows once per test set (dsmgp_set_test); a following fit! then carries them through the factorisation."
function settest!(s::Session, x::Matrix{Float64}, rows::Dict{Symbol,Vector{Int}})
    key = hash((size(x), x, [rows[l.id] for l in s.leaves]))
    key == s.testkey && return
    ptr = Int64[0]
    for l in s.leaves
        push!(ptr, ptr[end] + length(rows[l.id]))
    end
    idx = Int64.(reduce(vcat, [rows[l.id] for l in s.leaves])) .- 1
    isempty(idx) && push!(idx, 0)
    GC.@preserve x ptr idx chk(s, ccall(sym(:dsmgp_set_test), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Int32, Ptr{Int64}, Ptr{Int64}),
                                        s.h, x, size(x, 1), size(x, 2), ptr, idx))
    s.testkey = key
    s.testptr = ptr
    s.testnt = size(x, 1)
end

"Register the test rows of a DSMGP and let the device route them (dsmgp_set_test_routed: one thread per row walks the tree
handed over by settree!); only the per-leaf row offsets come back."
function settestrouted!(s::Session, x::Matrix{Float64})
    key = hash((size(x), x, :routed))
    key == s.testkey && return
    GC.@preserve x chk(s, ccall(sym(:dsmgp_set_test_routed), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Int32), s.h, x, size(x, 1), size(x, 2)))
    ptr = Vector{Int64}(undef, length(s.leaves) + 1)
    GC.@preserve ptr chk(s, ccall(sym(:dsmgp_routes), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}), s.h, ptr, C_NULL))
    s.testkey = key
    s.testptr = ptr
    s.testnt = size(x, 1)
end

function aggregate(s::Session, family::Int32, coef, group, G::Integer, plain::Bool, priorkid::Integer, nt::Integer)
    sec = Ref{Float64}(0.0)
    chk(s, ccall(sym(:dsmgp_predict_run), Cint, (Ptr{Cvoid}, Ref{Float64}), s.h, sec))
    μ = Vector{Float64}(undef, nt); σ² = similar(μ)
    c = coef === nothing ? C_NULL : pointer(coef)
    g = group === nothing ? C_NULL : pointer(group)
    GC.@preserve coef group μ σ² chk(s, ccall(sym(:dsmgp_aggregate), Cint,
        (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Int32}, Int32, Int32, Int32, Ptr{Float64}, Ptr{Float64}),
        s.h, family, c, g, Int32(G), Int32(plain), Int32(priorkid), μ, σ²))
    return μ, σ²
end

"Do the weights of every sum node add up to one?  (Every path of the reference keeps them so; `logweights` is a plain field.)"
weightsnormalised(node::GPNode) = true
weightsnormalised(node::GPSplitNode) = all(weightsnormalised, children(node))
weightsnormalised(node::GPSumNode) = abs(sum(exp.(logweights(node))) - 1) <= 1e-12 && all(weightsnormalised, children(node))

"predict(model::DSMGP, x) (src/common.jl:294-304): (μ, σ²) of the mixture; σ² ≤ 0 of a leaf → ϵ inside the aggregation (:137)."
function predict(model::DSMGP, x::AbstractMatrix)
    # `_predict` shifts the means by μmin - 1 before it weighs them (src/common.jl:134-143,275-302): with weights that add up to
    # one the recursion IS the flat mixture the device aggregates; with hand-assigned ones it is not, and the reference's own
    # recursion runs (its leaf predictions come from the device through prediction(gp, x) above)
    size(x, 1) == 0 && return Float64[], Float64[]            # (dsmgp_set_test* refuse n_t = 0)
    weightsnormalised(model.root) || return predict(model.root, x)
    s = session(model.root)
    xt = Matrix{Float64}(x)
    settestrouted!(s, xt)          # (route! + settest! above are the host form of the same lists: rows in ascending order per leaf)
    w = Dict{Symbol,Float64}()
    pathweights!(w, model.root, 0.0)
    coef = Float64[w[l.id] for l in s.leaves]
    return aggregate(s, AGG_MIXTURE, coef, nothing, 0, model.root isa GPNode, 0, size(xt, 1))
end

function predictfamily(model, x::AbstractMatrix, family::Int32)
    size(x, 1) == 0 && return Float64[], Float64[]
    s = session(model.root)
    xt = Matrix{Float64}(x)
    rows = Dict{Symbol,Vector{Int}}()
    routeall!(rows, model.root, xt, collect(1:size(xt, 1)))
    settest!(s, xt, rows)
    L = length(s.leaves)
    if family == AGG_RBCM                                       # per root child (src/common.jl:224-241); prior of leftGP (:227)
        group = zeros(Int32, L)
        for (g, c) in enumerate(children(model.root)), l in getLeaves(c)
            group[s.index[l.dist]] = Int32(g - 1)
        end
        return aggregate(s, family, nothing, group, length(children(model.root)), false, s.leaves[1].kernelid - 1, size(xt, 1))
    end
    β = family == AGG_GPOE ? 1.0 / length(children(model.root)) : 1.0        # :215
    return aggregate(s, family, fill(β, L), nothing, 0, false, 0, size(xt, 1))
end
predict(model::PoE, x::AbstractMatrix) = predictfamily(model, x, AGG_POE)      # src/common.jl:305
predict(model::gPoE, x::AbstractMatrix) = predictfamily(model, x, AGG_GPOE)    # :306
predict(model::rBCM, x::AbstractMatrix) = predictfamily(model, x, AGG_RBCM)    # :307

# ---------------------------------------------------------------------------------------------- gradients
"""
    updategradients!(spn)      (src/fit.jl:306-311)

One batched dsmgp_gradients call (L⁻ᵀ by blocked triangular inversion + the contraction tiles: ≈ 2× the Cholesky flops
instead of the ≈ 36× of src/gaussianprocess.jl:165-178 + src/kernels.jl:85-99); the results land where the reference
keeps them -- `kernel.∂ℓ`, `kernel.∂σ`, `gp.∂ϵ.value` -- with its scaling (IsoSE gradients carry the extra factor σ,
ArdSE length-scale gradients are identically zero: SURVEY F6/F7).
"""
function updategradients!(spn::Union{GPSumNode,GPSplitNode})
    fetchgradients!(session(spn))
end
function updategradients!(gp::GaussianProcess)
    fetchgradients!(session(gp))
end
function fetchgradients!(s::Session)
    g = s.grad
    GC.@preserve g chk(s, ccall(sym(:dsmgp_gradients), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int32), s.h, g, Int32(s.stride)))
    for (l, gp) in enumerate(s.gps)
        k = gp.kernel
        nl = k isa Union{ArdSE,ArdLinear} || k isa ArdSEProduct || k isa ArdMatern || k isa ArdRQ ? length(k.logℓ) : 1
        if k isa Union{ArdSE,ArdLinear} || k isa ArdSEProduct || k isa ArdMatern || k isa ArdRQ
            k.∂ℓ[:] = g[1:nl, l]        # ArdLinear: written in place, never through getgradients (src/kernels.jl:247 cannot run)
        else
            k.∂ℓ = g[1, l]
        end
        if k isa RQ                      # rational quadratic: [∂ℓ..., ∂α, ∂σ, ∂ϵ]
            setfield!(k, :∂α, g[nl + 1, l])     # a field of this binding's own types, not of a reference struct
            k.∂σ = g[nl + 2, l]
            gp.∂ϵ.value = g[nl + 3, l]
            continue
        end
        k isa Union{IsoLinear,ArdLinear} || (k.∂σ = g[nl + 1, l])
        gp.∂ϵ.value = g[nl + 2, l]
    end
    return nothing
end

"∇mll(gp) (src/gaussianprocess.jl:185-190) = [∂ℓ..., ∂σ, ∂ϵ].  The reference calls updategradients!(gp) again here (a
second 6n³ per leaf and iteration, src/optimize.jl:49); the values of the batched call are still valid: read them."
function ∇mll(gp::GaussianProcess)
    s = session(gp)
    l = s.index[gp]
    n = sum(DeepStructuredMixtures.nparams(gp))
    return s.grad[1:n, l]
end

end # module
