# BazingaHIP.jl — the reference-side binding a Bazinga.jl maintainer would add.
#
# NOT EXECUTED — PARITY UNPINNED: there is no `julia` in the build container or on the GPU box, so this file has
# never run.  It is written against include/bazinga_hip.h and kept in sync with the ctypes binding
# bazinga.jl_amd/_lib.py, whose struct layouts ARE tested against the header (tests/test_abi.py) and which
# exercises every entry point used here (tests/, -m gpu).
#
# Usage — nothing else in user code changes:
#     using Bazinga, BazingaHIP
#     out = Bazinga.alps(f, g, c, D, x0, y0; subsolver = BazingaHIP.PANOCplus)      # seam alps.jl:24,64-66
# or, with device-resident outer loop:
#     out = BazingaHIP.alps(f, g, c, D, x0, y0)
module BazingaHIP

using Bazinga
import ProximalOperators
using SparseArrays: SparseMatrixCSC, sparse

const lib = get(ENV, "BAZINGA_HIP_LIB", "libbazinga_hip.so")

# ---- mirrors of the C structs (include/bazinga_hip.h) ----------------------------------------
struct CtxOpts
    device::Int32; rank::Int32; nranks::Int32; flags::Int32; comm_id::Ptr{Cvoid}      # flags: BZ_CTX_RUNTIME_TUNING = 1, BZ_CTX_SHARED_DEVICE = 2
end
Base.@kwdef mutable struct ProblemDesc
    dtype::Int32 = 0; f_kind::Int32 = 0; g_kind::Int32 = 0; c_kind::Int32 = 0; D_kind::Int32 = 0
    slack::Int32 = 0
    n::Int64 = 0; ny::Int64 = 0
    f_q::Ptr{Cvoid} = C_NULL; f_b::Ptr{Cvoid} = C_NULL; f_grid_nx::Int64 = 0; f_grid_ny::Int64 = 0
    f_A::Ptr{Cvoid} = C_NULL; f_rows::Int64 = 0
    f_classes::Int64 = 0                  # f = SparseMultinomial / SparseMultiGLM (BZ_F_SPARSE_MULTINOMIAL, _MULTI_GLM): K, x is n / K rows of K
    g_lambda::Float64 = 0; g_p::Float64 = 0; g_group::Int64 = 0; g_u::Ptr{Cvoid} = C_NULL
    g_group_ptr::Ptr{Cvoid} = C_NULL; g_ngroups::Int64 = 0; g_l1::Float64 = 0   # g = GroupLasso (BZ_G_GROUP_LASSO) alone
    g_lo::Float64 = 0; g_hi::Float64 = 0
    g_l2::Float64 = 0; g_weights::Ptr{Cvoid} = C_NULL   # g = ElasticNet (BZ_G_ELASTIC_NET) alone
    g_lo_vec::Ptr{Cvoid} = C_NULL; g_hi_vec::Ptr{Cvoid} = C_NULL; g_lambda_vec::Ptr{Cvoid} = C_NULL
    c_A::Ptr{Cvoid} = C_NULL; c_b::Ptr{Cvoid} = C_NULL
    D_lo::Float64 = 0; D_hi::Float64 = 0; D_lo_vec::Ptr{Cvoid} = C_NULL; D_hi_vec::Ptr{Cvoid} = C_NULL
    # generic oracles (all four kinds BZ_*_CALLBACK): host callbacks, see lower_generic!
    cb_user::Ptr{Cvoid} = C_NULL; cb_f_gradient::Ptr{Cvoid} = C_NULL; cb_g_prox::Ptr{Cvoid} = C_NULL
    cb_c_eval::Ptr{Cvoid} = C_NULL; cb_c_jtprod::Ptr{Cvoid} = C_NULL; cb_D_proj::Ptr{Cvoid} = C_NULL
    # f = SparseQuadratic (BZ_F_SPARSE_QUADRATIC): symmetric Q in CSR, 0-based; q in f_b
    # f = SparseLeastSquares (BZ_F_SPARSE_LEAST_SQUARES): A (f_rows x n) in CSR, 0-based; b in f_b
    # f = SparseLogistic (BZ_F_SPARSE_LOGISTIC): A (f_rows x n) in CSR, 0-based; the labels in f_b
    f_sp_rowptr::Ptr{Cvoid} = C_NULL; f_sp_col::Ptr{Cvoid} = C_NULL; f_sp_val::Ptr{Cvoid} = C_NULL; f_sp_nnz::Int64 = 0
    # f = SparseGLM (BZ_F_SPARSE_GLM) alone: the row loss (BZ_LOSS_*), Huber's delta, the row weights w[f_rows] or C_NULL, the scale
    f_loss::Int32 = 0; f_loss_delta::Float64 = 0; f_w::Ptr{Cvoid} = C_NULL; f_scale::Float64 = 1
    # c = SparseAffine (BZ_C_SPARSE_AFFINE): A in CSR, 0-based
    c_sp_rowptr::Ptr{Cvoid} = C_NULL; c_sp_col::Ptr{Cvoid} = C_NULL; c_sp_val::Ptr{Cvoid} = C_NULL; c_sp_nnz::Int64 = 0
end
Base.@kwdef mutable struct PanocOpts
    tol::Float64 = 1e-8; maxit::Int64 = 1000; freq::Int32 = 10; verbose::Int32 = 0
    minimum_gamma::Float64 = 1e-7; alpha::Float64 = 0.95; beta::Float64 = 0.5
    max_backtracks::Int32 = 20; lbfgs_memory::Int32 = 5; fuse::Int32 = 1; persist::Int32 = 1
    lbfgs_compact::Int32 = 2; affine_refresh::Int32 = 16
    directions::Int32 = 0; reserved::Int32 = 0; broyden_theta_bar::Float64 = 0.2      # BZ_DIR_LBFGS / _ANDERSON (1) / _BROYDEN (2)
    gamma::Float64 = 0; Lf::Float64 = 0; adaptive::Int32 = -1; reserved2::Int32 = 0  # 0 = nothing; adaptive -1 = (gamma === nothing)
end
Base.@kwdef mutable struct PanocStats
    iters::Int64 = 0; f_z::Float64 = 0; g_z::Float64 = 0; al_z::Float64 = 0; gamma::Float64 = 0
    tau::Float64 = 0; stop_norm::Float64 = 0; n_grad::Int64 = 0; n_prox::Int64 = 0
    n_backtracks::Int64 = 0; n_gamma_halvings::Int64 = 0; n_fused_iters::Int64 = 0
    n_lbfgs_skips::Int64 = 0; elapsed_s::Float64 = 0; status::Int32 = 0; persist_fallbacks::Int32 = 0
    n_affine_images::Int64 = 0; n_gated_launches::Int64 = 0; n_gate_aborts::Int64 = 0; n_gate_fallbacks::Int64 = 0
    n_dense_onepass::Int64 = 0; n_dense_fallbacks::Int64 = 0; n_affine_blends::Int64 = 0
end

Base.@kwdef mutable struct AlpsOpts
    tol_prim::Float64 = 1e-6; tol_dual::Float64 = 1e-6; inner_tol::Float64 = cbrt(1e-6)
    maxit::Int64 = 100; theta_penalty::Float64 = 0.8; kappa_penalty::Float64 = 0.5; kappa_tol::Float64 = 0.1
    subsolver_maxit::Int64 = 1_000_000_000; verbose::Int32 = 0; warm_start::Int32 = 0
end
Base.@kwdef mutable struct AlpsStats
    tot_it::Int64 = 0; tot_inner_it::Int64 = 0; elapsed_s::Float64 = 0; status::Int32 = 0; reserved::Int32 = 0
    inner_tol::Float64 = 0; norm_res_prim::Float64 = 0; objective::Float64 = 0
end

function check(rc::Cint)
    rc == 0 && return
    msg = unsafe_string(ccall((:bz_last_error, lib), Cstring, ()))
    error(msg)                       # same ErrorException the reference throws (auglagfun.jl:33-34)
end
# library calls on a problem whose oracles are callbacks: an exception parked by a callback (BZ_ERR_CALLBACK) is rethrown
# as it was raised — the caller sees what the reference's own `gradient!` / `prox!` / `eval!` would have thrown
function check(rc::Cint, p)
    box = p.keep isa Tuple ? p.keep[end] : nothing
    if box !== nothing && box[].err !== nothing
        e = box[].err
        box[].err = nothing
        throw(e)
    end
    check(rc)
end

const _ctx = Ref{Ptr{Cvoid}}(C_NULL)
function context()
    if _ctx[] == C_NULL
        o = Ref(CtxOpts(0, 0, 1, 0, C_NULL))
        check(ccall((:bz_ctx_create, lib), Cint, (Ref{CtxOpts}, Ref{Ptr{Cvoid}}), o, _ctx))
    end
    _ctx[]
end

# ---- structured oracle types this build adds (SURVEY §8(b)) ------------------------------------
struct DiagQuadratic{T} <: Bazinga.ProximableFunction
    q::Vector{T}; b::Vector{T}            # f(x) = sum x_i (0.5 q_i x_i - b_i)
end

"f(x) = 0.5 x'A_h x - b'x, A_h the 5-point Laplacian (4,-1,-1,-1,-1) on an nx-by-ny grid, row-major, Dirichlet-0"
struct Stencil5ptQuadratic{T} <: Bazinga.ProximableFunction
    nx::Int; ny::Int; b::Vector{T}
end
"c(x) = A x - b with a dense A (demo/basispursuit.jl:38-49); `At` keeps A row-major for the device"
struct DenseAffine{T} <: Bazinga.SmoothFunction
    A::Matrix{T}; b::Vector{T}; At::Matrix{T}
    DenseAffine(A::Matrix{T}, b::Vector{T}) where {T} = new{T}(A, b, permutedims(A))
end
Bazinga.eval!(cx, c::DenseAffine, x) = (cx .= c.A * x .- c.b; nothing)
Bazinga.jtprod!(jtv, c::DenseAffine, x, v) = (jtv .= c.A' * v; nothing)

"""`SparseAffine(A::SparseMatrixCSC, b)`: c(x) = A x - b with a sparse A that is never densified (the shape of
demo/obstacle.jl:93-113).  The library takes CSR: the CSC arrays of `sparse(A')` ARE the CSR arrays of A, made 0-based here."""
struct SparseAffine{T} <: Bazinga.SmoothFunction
    A::SparseMatrixCSC{T,Int}; b::Vector{T}
    rowptr::Vector{Int64}; col::Vector{Int32}; val::Vector{T}
    function SparseAffine(A::SparseMatrixCSC{T}, b::Vector{T}) where {T}
        At = sparse(A')
        new{T}(A, b, Int64.(At.colptr .- 1), Int32.(At.rowval .- 1), Vector{T}(At.nzval))
    end
end
Bazinga.eval!(cx, c::SparseAffine, x) = (cx .= c.A * x .- c.b; nothing)
Bazinga.jtprod!(jtv, c::SparseAffine, x, v) = (jtv .= c.A' * v; nothing)

"""`SparseQuadratic(Q::SparseMatrixCSC, q)`: f(x) = 0.5 x'Qx + q'x with a sparse symmetric Q that is never densified
(ProximalOperators.Quadratic with a sparse Q).  Symmetry is the caller's contract: the CSC arrays of a symmetric Q ARE its
CSR arrays, made 0-based here."""
struct SparseQuadratic{T} <: Bazinga.ProximableFunction
    Q::SparseMatrixCSC{T,Int}; q::Vector{T}
    rowptr::Vector{Int64}; col::Vector{Int32}; val::Vector{T}
    SparseQuadratic(Q::SparseMatrixCSC{T}, q::Vector{T}) where {T} =
        new{T}(Q, q, Int64.(Q.colptr .- 1), Int32.(Q.rowval .- 1), Vector{T}(Q.nzval))
end
function Bazinga.gradient!(dfx, f::SparseQuadratic, x)
    dfx .= f.Q * x
    fx = sum(x .* dfx) / 2
    dfx .+= f.q
    return fx + sum(x .* f.q)
end

"""`SparseLeastSquares(A::SparseMatrixCSC, b)`: f(x) = 0.5||A x - b||^2 with a sparse A that is never densified and never
squared into A'A (ProximalOperators.LeastSquares, lambda = 1, with a sparse A).  The library takes CSR: the CSC arrays of
`sparse(A')` ARE the CSR arrays of A, made 0-based here."""
struct SparseLeastSquares{T} <: Bazinga.ProximableFunction
    A::SparseMatrixCSC{T,Int}; b::Vector{T}
    rowptr::Vector{Int64}; col::Vector{Int32}; val::Vector{T}
    function SparseLeastSquares(A::SparseMatrixCSC{T}, b::Vector{T}) where {T}
        At = sparse(A')
        new{T}(A, b, Int64.(At.colptr .- 1), Int32.(At.rowval .- 1), Vector{T}(At.nzval))
    end
end
function Bazinga.gradient!(dfx, f::SparseLeastSquares, x)
    r = f.A * x .- f.b
    dfx .= f.A' * r
    return sum(r .* r) / 2
end

"""`SparseGLM(A::SparseMatrixCSC, b, loss; delta = 0, weights = nothing, scale = 1)`: f(x) = sum_i scale w_i l(b_i, a_i'x) with
`loss` one of :least_squares, :logistic, :huber (delta > 0), :squared_hinge, :poisson (BZ_LOSS_* 0 .. 4); the formulas are those of
include/bazinga_hip.h.  Labels (+-1), counts (>= 0), delta, the weights (>= 0) and the scale (> 0) are checked here."""
struct SparseGLM{T} <: Bazinga.ProximableFunction
    A::SparseMatrixCSC{T,Int}; b::Vector{T}; loss::Int32; delta::Float64; w::Union{Nothing,Vector{T}}; scale::Float64
    rowptr::Vector{Int64}; col::Vector{Int32}; val::Vector{T}
    function SparseGLM(A::SparseMatrixCSC{T}, b::Vector{T}, loss::Symbol; delta = 0.0, weights = nothing, scale = 1.0) where {T}
        code = findfirst(==(loss), (:least_squares, :logistic, :huber, :squared_hinge, :poisson))
        code === nothing && throw(ArgumentError("unknown loss $loss"))
        length(b) == size(A, 1) || throw(ArgumentError("one b per row of A"))
        loss in (:logistic, :squared_hinge) && !all(v -> abs(v) == 1, b) && throw(ArgumentError("labels must be -1 or +1"))
        loss == :poisson && !all(v -> isfinite(v) && v >= 0, b) && throw(ArgumentError("counts must be finite and >= 0"))
        loss == :huber && !(isfinite(delta) && delta > 0) && throw(ArgumentError("the huber loss needs delta finite and > 0"))
        (isfinite(scale) && scale > 0) || throw(ArgumentError("scale must be finite and > 0"))
        weights === nothing || (length(weights) == length(b) && all(v -> isfinite(v) && v >= 0, weights)) ||
            throw(ArgumentError("weights must be finite and >= 0, one per row"))
        At = sparse(A')
        new{T}(A, b, Int32(code - 1), Float64(delta), weights === nothing ? nothing : Vector{T}(weights), Float64(scale),
               Int64.(At.colptr .- 1), Int32.(At.rowval .- 1), Vector{T}(At.nzval))
    end
end
# the losses l(b, t) and l'(b, t) of loss code `loss` (BZ_LOSS_*), element by element on arrays of one shape (least squares: v^2,
# halved on the sum): ordered compares and arithmetic alone
function glm_terms(::Type{T}, loss, delta, b, t) where {T}
    if loss == 0
        v = t .- b; l = v .* v; dl = v
    elseif loss == 1
        u = b .* t; e = exp.(.-abs.(u))
        l = ifelse.(u .< 0, .-u, zero(T)) .+ log1p.(e)
        dl = .-b .* ifelse.(u .>= 0, e ./ (one(T) .+ e), one(T) ./ (one(T) .+ e))
    elseif loss == 2
        v = t .- b; d = T(delta); a = ifelse.(v .< 0, .-v, v); inside = a .<= d
        l = ifelse.(inside, T(0.5) .* v .* v, d .* (a .- T(0.5) * d))
        dl = ifelse.(inside, v, ifelse.(v .> 0, d, ifelse.(v .< 0, -d, v)))
    elseif loss == 3
        h = one(T) .- b .* t; off = h .<= 0
        l = ifelse.(off, zero(T), T(0.5) .* h .* h); dl = ifelse.(off, zero(T), .-b .* h)
    else
        e = exp.(t); bt = ifelse.(b .== 0, zero(T), b .* t)
        l = ifelse.(e .< T(Inf), e .- bt, e); dl = e .- b
    end
    return l, dl
end
function Bazinga.gradient!(dfx, f::SparseGLM{T}, x) where {T}
    w = f.w === nothing ? T(f.scale) : T.(f.scale .* Float64.(f.w))
    l, dl = glm_terms(T, f.loss, f.delta, f.b, f.A * x)
    dfx .= f.A' * (w .* dl)
    return f.loss == 0 ? sum(w .* l) / 2 : sum(w .* l)
end

"""`SparseMultiGLM(A::SparseMatrixCSC, B::Matrix, loss; delta = 0, weights = nothing, scale = 1)`: K independent row losses of one
sparse design matrix, f(X) = sum_i scale w_i sum_k l(B_ik, t_ik), T = A X, with A (m x n_f) never densified and B m x K,
2 <= K <= 64 (a vector b is `SparseGLM`'s): multi-response regression with :least_squares (with `NormL21(lambda, K)` the multi-task
Lasso), multi-label classification with :logistic or :squared_hinge and B in {-1, +1}.  `loss`, `delta`, `weights` (one per ROW,
shared by its K responses) and `scale` are `SparseGLM`'s, checked here on every entry of B.  The variable is the flat vector x of
length n_f K holding X ROW-MAJOR (response fastest), as `SparseMultinomial` has it; `coef(f, x)` gives X back.  The library takes
B row-major too: `b` holds `vec(permutedims(B))`."""
struct SparseMultiGLM{T} <: Bazinga.ProximableFunction
    A::SparseMatrixCSC{T,Int}; B::Matrix{T}; b::Vector{T}; K::Int; loss::Int32; delta::Float64; w::Union{Nothing,Vector{T}}; scale::Float64
    rowptr::Vector{Int64}; col::Vector{Int32}; val::Vector{T}
    function SparseMultiGLM(A::SparseMatrixCSC{T}, B::Matrix{T}, loss::Symbol; delta = 0.0, weights = nothing, scale = 1.0) where {T}
        code = findfirst(==(loss), (:least_squares, :logistic, :huber, :squared_hinge, :poisson))
        code === nothing && throw(ArgumentError("unknown loss $loss"))
        K = size(B, 2)
        2 <= K <= 64 || throw(ArgumentError("B must have K in 2 .. 64 columns (K = 1 is SparseGLM)"))
        size(B, 1) == size(A, 1) || throw(ArgumentError("one row of B per row of A"))
        loss in (:logistic, :squared_hinge) && !all(v -> abs(v) == 1, B) && throw(ArgumentError("labels must be -1 or +1"))
        loss == :poisson && !all(v -> isfinite(v) && v >= 0, B) && throw(ArgumentError("counts must be finite and >= 0"))
        loss == :huber && !(isfinite(delta) && delta > 0) && throw(ArgumentError("the huber loss needs delta finite and > 0"))
        (isfinite(scale) && scale > 0) || throw(ArgumentError("scale must be finite and > 0"))
        weights === nothing || (length(weights) == size(B, 1) && all(v -> isfinite(v) && v >= 0, weights)) ||
            throw(ArgumentError("weights must be finite and >= 0, one per row"))
        At = sparse(A')
        new{T}(A, B, vec(permutedims(B)), K, Int32(code - 1), Float64(delta), weights === nothing ? nothing : Vector{T}(weights),
               Float64(scale), Int64.(At.colptr .- 1), Int32.(At.rowval .- 1), Vector{T}(At.nzval))
    end
end
coef(f::SparseMultiGLM, x) = permutedims(reshape(x, f.K, size(f.A, 2)))
function Bazinga.gradient!(dfx, f::SparseMultiGLM{T}, x) where {T}
    w = f.w === nothing ? T(f.scale) : T.(f.scale .* Float64.(f.w))       # (a vector broadcasts over the K columns of a row)
    l, dl = glm_terms(T, f.loss, f.delta, f.B, f.A * coef(f, x))
    dfx .= vec(permutedims(f.A' * (w .* dl)))
    return f.loss == 0 ? sum(w .* l) / 2 : sum(w .* l)
end

"""`SparseMultinomial(A::SparseMatrixCSC, labels, K; weights = nothing, scale = 1)`: multinomial (softmax) regression,
f(X) = sum_i scale w_i (logsumexp_k(t_ik) - t_{i,b_i}), T = A X, with a sparse A (m x n_f) that is never densified and labels
b in {0 .. K - 1} (0-based, as the library stores them), 2 <= K <= 64.  The variable is the flat vector x of length n_f K holding
X ROW-MAJOR (class fastest): x[(j - 1) K + k] = X[j, k], i.e. `vec(permutedims(X))`; `coef(f, x)` gives X back.  The formulas are
those of include/bazinga_hip.h.  Labels, the weights (>= 0) and the scale (> 0) are checked here."""
struct SparseMultinomial{T} <: Bazinga.ProximableFunction
    A::SparseMatrixCSC{T,Int}; b::Vector{T}; K::Int; w::Union{Nothing,Vector{T}}; scale::Float64
    rowptr::Vector{Int64}; col::Vector{Int32}; val::Vector{T}
    function SparseMultinomial(A::SparseMatrixCSC{T}, labels::Vector{T}, K::Integer; weights = nothing, scale = 1.0) where {T}
        2 <= K <= 64 || throw(ArgumentError("K must be in 2 .. 64"))
        length(labels) == size(A, 1) || throw(ArgumentError("one label per row of A"))
        all(v -> isfinite(v) && v == floor(v) && 0 <= v < K, labels) || throw(ArgumentError("labels must be integers in [0, K)"))
        (isfinite(scale) && scale > 0) || throw(ArgumentError("scale must be finite and > 0"))
        weights === nothing || (length(weights) == length(labels) && all(v -> isfinite(v) && v >= 0, weights)) ||
            throw(ArgumentError("weights must be finite and >= 0, one per row"))
        At = sparse(A')
        new{T}(A, labels, Int(K), weights === nothing ? nothing : Vector{T}(weights), Float64(scale),
               Int64.(At.colptr .- 1), Int32.(At.rowval .- 1), Vector{T}(At.nzval))
    end
end
coef(f::SparseMultinomial, x) = permutedims(reshape(x, f.K, size(f.A, 2)))
# per row: mx = max_k t_k ; e = exp(t - mx) ; S = sum e ; p = e / S ; loss = w ((mx - t_b) + log S) ; r = w (p - onehot(b))
function Bazinga.gradient!(dfx, f::SparseMultinomial{T}, x) where {T}
    X = coef(f, x)
    t = f.A * X
    w = f.w === nothing ? fill(T(f.scale), length(f.b)) : T.(f.scale .* Float64.(f.w))
    mx = maximum(t, dims = 2)
    e = exp.(t .- mx)
    S = sum(e, dims = 2)
    R = e ./ S
    loss = zero(T)
    for i in eachindex(f.b)
        k = Int(f.b[i]) + 1
        R[i, k] -= one(T)
        loss += w[i] * ((mx[i] - t[i, k]) + log(S[i]))
    end
    dfx .= vec(permutedims(f.A' * (w .* R)))
    return loss
end

"""`SparseLogistic(A::SparseMatrixCSC, labels)`: f(x) = sum_i log(1 + exp(-b_i a_i'x)), the logistic loss of a sparse design
matrix that is never densified, labels b in {-1, +1} (checked here).  The plain sum: no 1/2 and no 1/m.  The library takes CSR:
the CSC arrays of `sparse(A')` ARE the CSR arrays of A, made 0-based here."""
struct SparseLogistic{T} <: Bazinga.ProximableFunction
    A::SparseMatrixCSC{T,Int}; b::Vector{T}
    rowptr::Vector{Int64}; col::Vector{Int32}; val::Vector{T}
    function SparseLogistic(A::SparseMatrixCSC{T}, labels::Vector{T}) where {T}
        all(v -> abs(v) == 1, labels) || throw(ArgumentError("labels must be -1 or +1"))
        length(labels) == size(A, 1) || throw(ArgumentError("one label per row of A"))
        At = sparse(A')
        new{T}(A, labels, Int64.(At.colptr .- 1), Int32.(At.rowval .- 1), Vector{T}(At.nzval))
    end
end
# u = b .* (A x) ; loss = softplus(-u) = max(-u, 0) + log1p(exp(-|u|)) ; r = -b sigma(-u): ordered compares and arithmetic
# alone, so that a NaN in u reaches both
function Bazinga.gradient!(dfx, f::SparseLogistic{T}, x) where {T}
    u = f.b .* (f.A * x)
    e = exp.(.-abs.(u))
    loss = ifelse.(u .< 0, .-u, zero(T)) .+ log1p.(e)
    s = ifelse.(u .>= 0, e ./ (one(T) .+ e), one(T) ./ (one(T) .+ e))
    dfx .= f.A' * (.-f.b .* s)
    return sum(loss)
end

"""`NormL21(λ, group)`: the group Lasso g(x) = Σ_j λ_j ‖x[(j-1)K+1 : jK]‖₂ over the length(x) ÷ K contiguous groups of K = `group`
elements, 1 ≤ K ≤ 64 (BZ_G_NORM_L21) — with SparseMultinomial's class-fastest layout and K = n_classes, a feature's row of
coefficients.  λ is a number, or a vector with one entry per group in the problem's type (finite, ≥ 0; a zero leaves its group
unpenalised: an intercept row); the vector must stay alive until bz_problem_create returns."""
struct NormL21{L} <: Bazinga.ProximableFunction
    lambda::L; group::Int
    function NormL21(lambda::L, group::Integer) where {L<:Union{Real,AbstractVector{<:Real}}}
        1 <= group <= 64 || throw(ArgumentError("the group size must be in 1 .. 64"))
        all(v -> isfinite(v) && v >= 0, lambda) || throw(ArgumentError("λ must be finite and nonnegative"))
        new{L}(lambda, Int(group))
    end
end
# the definition of include/bazinga_hip.h, group by group (the host twin of k_fbstep_group, to rounding: the sum of squares here
# is Julia's, not the kernel's fixed fold)
function ProximalOperators.prox!(z, g::NormL21, x, gamma)
    K = g.group
    length(x) % K == 0 || throw(ArgumentError("length(x) must be a multiple of the group size"))
    T = eltype(x); gz = zero(T)
    for j in 1:(length(x) ÷ K)
        r = ((j - 1) * K + 1):(j * K)
        lam = T(g.lambda isa Real ? g.lambda : g.lambda[j])
        nrm = sqrt(sum(abs2, view(x, r))); gl = T(gamma) * lam
        if nrm <= gl
            z[r] .= zero(T)
        else
            scal = nrm > gl ? one(T) - gl / nrm : nrm - gl
            z[r] .= scal .* view(x, r)
            gz += lam * (scal * nrm)
        end
    end
    return gz
end

"""`GroupLasso(λ, sizes; l1 = 0)`: the group Lasso over groups of unequal size with an optional ℓ1 mix,
g(x) = l1 ‖x‖₁ + Σ_j λ_j ‖x[group j]‖₂, the groups contiguous and `sizes[j]` ≥ 1 long, Σ sizes = length(x) (BZ_G_GROUP_LASSO).  λ is a
number, or a vector with one entry per group in the problem's type (finite, ≥ 0; a zero leaves its group unpenalised: an
intercept); l1 is a number ≥ 0, fixed once the problem is created.  The object holds the 0-based Int64 group pointer the
library reads; it and a vector λ must stay alive until bz_problem_create returns."""
struct GroupLasso{L} <: Bazinga.ProximableFunction
    lambda::L; ptr::Vector{Int64}; l1::Float64
    function GroupLasso(lambda::L, sizes::AbstractVector{<:Integer}; l1::Real = 0) where {L<:Union{Real,AbstractVector{<:Real}}}
        !isempty(sizes) && all(>=(1), sizes) || throw(ArgumentError("every group must hold at least one element"))
        all(v -> isfinite(v) && v >= 0, lambda) || throw(ArgumentError("λ must be finite and nonnegative"))
        lambda isa Real || length(lambda) == length(sizes) || throw(ArgumentError("λ must have one entry per group"))
        isfinite(l1) && l1 >= 0 || throw(ArgumentError("l1 must be finite and nonnegative"))
        new{L}(lambda, Int64[0; cumsum(Int64.(sizes))], Float64(l1))
    end
end
# the definition of include/bazinga_hip.h, group by group (the host twin of k_fbstep_ragged, to rounding: the sums here are
# Julia's, not the kernel's 64 accumulators)
function ProximalOperators.prox!(z, g::GroupLasso, x, gamma)
    length(x) == g.ptr[end] || throw(ArgumentError("length(x) must be the sum of the group sizes"))
    T = eltype(x); gz = zero(T); t = T(gamma) * T(g.l1)
    soft(y) = g.l1 > 0 ? (y > t ? y - t : (y < -t ? y + t : (isnan(y) ? y : zero(T)))) : y
    for j in 1:(length(g.ptr) - 1)
        r = (g.ptr[j] + 1):g.ptr[j + 1]
        lam = T(g.lambda isa Real ? g.lambda : g.lambda[j])
        u = soft.(view(x, r))
        nrm = sqrt(sum(abs2, u)); gl = T(gamma) * lam
        if nrm <= gl
            z[r] .= zero(T)
        else
            scal = nrm > gl ? one(T) - gl / nrm : nrm - gl
            z[r] .= scal .* u
            gz += lam * (scal * nrm) + T(g.l1) * scal * sum(abs, u)
        end
    end
    return gz
end

"""`ElasticNet(l1, l2)` / `ElasticNet(l1, l2, weights)`: the elastic net with penalty factors,
g(x) = Σᵢ wᵢ (l1 |xᵢ| + l2/2 xᵢ²) (BZ_G_ELASTIC_NET; `ProximalOperators.ElasticNet(mu, lambda)` is the form without weights and
lowers to the same kind).  l1 and l2 are finite numbers ≥ 0; `weights` is a vector in the problem's type with one finite entry
≥ 0 per element (a zero leaves its element wholly unpenalised: an intercept), or `nothing`: every wᵢ = 1.  glmnet's penalty
λ Σ pfⱼ (α |βⱼ| + (1 − α)/2 βⱼ²) is `ElasticNet(λ α, λ (1 − α), pf)`.  A weight vector must stay alive until bz_problem_create
returns."""
struct ElasticNet{W<:Union{Nothing,AbstractVector{<:Real}}} <: Bazinga.ProximableFunction
    l1::Float64; l2::Float64; weights::W
    function ElasticNet(l1::Real, l2::Real, weights::W = nothing) where {W<:Union{Nothing,AbstractVector{<:Real}}}
        isfinite(l1) && l1 >= 0 || throw(ArgumentError("l1 must be finite and nonnegative"))
        isfinite(l2) && l2 >= 0 || throw(ArgumentError("l2 must be finite and nonnegative"))
        weights === nothing || all(v -> isfinite(v) && v >= 0, weights) || throw(ArgumentError("weights must be finite and nonnegative"))
        new{W}(Float64(l1), Float64(l2), weights)
    end
end
# the definition of include/bazinga_hip.h, operation for operation in the type of x (the host twin of prox_elem's arm)
function ProximalOperators.prox!(z, g::ElasticNet, x, gamma)
    T = eltype(x); l1 = T(g.l1); l2 = T(g.l2); h2 = T(0.5) * l2; gz = zero(T)
    for i in eachindex(x)
        t = g.weights === nothing ? T(gamma) : T(gamma) * T(g.weights[i])
        a = t * l1; d = one(T) + t * l2; y = x[i]
        s = y + (y <= -a ? a : (y >= a ? -a : -y))
        z[i] = s / d
        term = l1 * abs(z[i]) + h2 * (z[i] * z[i])
        gz += g.weights === nothing ? term : T(g.weights[i]) * term
    end
    return gz
end

"`LBFGS(M; compact = nothing)`: how the operator is evaluated (bz_panoc_opts.lbfgs_compact) — `false` the two-loop recursion in the reference's order, `true` the compact representation, `nothing` (default) compact where the one-pass kernel applies"
struct LBFGS
    memory::Int; compact::Union{Nothing,Bool}
    LBFGS(memory = 5; compact = nothing) = new(memory, compact)
end

# ---- lowering: pattern-match the oracle structs -> bz_problem_desc ----------------------------
dtype_code(::Type{Float64}) = Int32(0)
dtype_code(::Type{Float32}) = Int32(1)

# Every lower_*! returns the temporaries whose memory the descriptor points into (or `nothing`): the Problem
# constructor roots them with GC.@preserve until bz_problem_create has copied the data.
lower_f!(d, f::Bazinga.Zero) = (d.f_kind = 0; nothing)
lower_f!(d, f::ProximalOperators.Zero) = (d.f_kind = 0; nothing)
lower_f!(d, f::DiagQuadratic) = (d.f_kind = 1; d.f_q = pointer(f.q); d.f_b = pointer(f.b); nothing)
lower_f!(d, f::Stencil5ptQuadratic) = (d.f_kind = 2; d.f_grid_nx = f.nx; d.f_grid_ny = f.ny; d.f_b = pointer(f.b); nothing)
# dense f: Julia matrices are column-major, the library wants row-major -> pass the transpose's memory
function lower_f!(d, f::ProximalOperators.LeastSquares)
    At = permutedims(f.A)
    d.f_kind = 3; d.f_A = pointer(At); d.f_rows = size(f.A, 1); d.f_b = pointer(f.b)
    return At                                                          # kept alive by the caller
end
lower_f!(d, f::ProximalOperators.Quadratic) = (d.f_kind = 4; d.f_A = pointer(f.Q); d.f_rows = size(f.Q, 1);
                                               d.f_b = pointer(f.q); nothing)      # Q symmetric: layout-agnostic
lower_f!(d, f::SparseQuadratic) = (d.f_kind = 6; d.f_sp_rowptr = pointer(f.rowptr); d.f_sp_col = pointer(f.col);
                                   d.f_sp_val = pointer(f.val); d.f_sp_nnz = length(f.val); d.f_b = pointer(f.q); nothing)
lower_f!(d, f::SparseLeastSquares) = (d.f_kind = 7; d.f_rows = length(f.b); d.f_sp_rowptr = pointer(f.rowptr);
                                      d.f_sp_col = pointer(f.col); d.f_sp_val = pointer(f.val); d.f_sp_nnz = length(f.val);
                                      d.f_b = pointer(f.b); nothing)
lower_f!(d, f::SparseLogistic) = (d.f_kind = 8; d.f_rows = length(f.b); d.f_sp_rowptr = pointer(f.rowptr);
                                  d.f_sp_col = pointer(f.col); d.f_sp_val = pointer(f.val); d.f_sp_nnz = length(f.val);
                                  d.f_b = pointer(f.b); nothing)
function lower_f!(d, f::SparseGLM)
    d.f_kind = 9; d.f_rows = length(f.b); d.f_sp_rowptr = pointer(f.rowptr); d.f_sp_col = pointer(f.col)
    d.f_sp_val = pointer(f.val); d.f_sp_nnz = length(f.val); d.f_b = pointer(f.b)
    d.f_loss = f.loss; d.f_loss_delta = f.delta; d.f_scale = f.scale
    d.f_w = f.w === nothing ? C_NULL : pointer(f.w)
    return nothing
end
function lower_f!(d, f::SparseMultinomial)
    d.f_kind = 10; d.f_rows = length(f.b); d.f_classes = f.K; d.f_sp_rowptr = pointer(f.rowptr); d.f_sp_col = pointer(f.col)
    d.f_sp_val = pointer(f.val); d.f_sp_nnz = length(f.val); d.f_b = pointer(f.b)
    d.f_scale = f.scale
    d.f_w = f.w === nothing ? C_NULL : pointer(f.w)
    return nothing
end
function lower_f!(d, f::SparseMultiGLM)
    d.f_kind = 11; d.f_rows = size(f.B, 1); d.f_classes = f.K; d.f_sp_rowptr = pointer(f.rowptr); d.f_sp_col = pointer(f.col)
    d.f_sp_val = pointer(f.val); d.f_sp_nnz = length(f.val); d.f_b = pointer(f.b)        # (B row-major: f_rows * K values)
    d.f_loss = f.loss; d.f_loss_delta = f.delta; d.f_scale = f.scale
    d.f_w = f.w === nothing ? C_NULL : pointer(f.w)
    return nothing
end
lower_f!(d, f) = :generic

lower_g!(d, g::Bazinga.Zero) = (d.g_kind = 0)
lower_g!(d, g::ProximalOperators.Zero) = (d.g_kind = 0)
lower_g!(d, g::ProximalOperators.IndFree) = (d.g_kind = 0)
lower_g!(d, g::ProximalOperators.NormL1{<:Real}) = (d.g_kind = 1; d.g_lambda = g.lambda)
# (an array lambda: one weight per element, in the problem's type; the array must stay alive until bz_problem_create returns)
lower_g!(d, g::ProximalOperators.NormL1{<:AbstractVector}) = (d.g_kind = 1; d.g_lambda_vec = pointer(g.lambda))
lower_g!(d, g::Bazinga.NormL1Nonneg) = (d.g_kind = 2; d.g_lambda = g.lambda)
# (the group Lasso: one weight per GROUP with a vector; n % group and the slack form are checked by bz_problem_create)
lower_g!(d, g::NormL21{<:Real}) = (d.g_kind = 9; d.g_group = g.group; d.g_lambda = g.lambda)
lower_g!(d, g::NormL21{<:AbstractVector}) = (d.g_kind = 9; d.g_group = g.group; d.g_lambda_vec = pointer(g.lambda))
# (the group Lasso over a group pointer: the pointer is the object's own; ptr[end] == n and the slack form are checked by bz_problem_create)
lower_g!(d, g::GroupLasso{<:Real}) = (d.g_kind = 10; d.g_group_ptr = pointer(g.ptr); d.g_ngroups = length(g.ptr) - 1; d.g_l1 = g.l1; d.g_lambda = g.lambda)
lower_g!(d, g::GroupLasso{<:AbstractVector}) = (d.g_kind = 10; d.g_group_ptr = pointer(g.ptr); d.g_ngroups = length(g.ptr) - 1; d.g_l1 = g.l1; d.g_lambda_vec = pointer(g.lambda))
# the elastic net (BZ_G_ELASTIC_NET): ProximalOperators' type with numbers, or BazingaHIP.ElasticNet with optional penalty factors
lower_g!(d, g::ProximalOperators.ElasticNet{<:Real,<:Real}) = (d.g_kind = 11; d.g_lambda = g.mu; d.g_l2 = g.lambda)
lower_g!(d, g::ElasticNet{Nothing}) = (d.g_kind = 11; d.g_lambda = g.l1; d.g_l2 = g.l2)
# (penalty factors: one per element, in the problem's type; the array must stay alive until bz_problem_create returns)
lower_g!(d, g::ElasticNet{<:AbstractVector}) = (d.g_kind = 11; d.g_lambda = g.l1; d.g_l2 = g.l2; d.g_weights = pointer(g.weights))
lower_g!(d, g::Bazinga.NormL1Box) = (d.g_kind = 3; d.g_lambda = g.lambda; d.g_u = pointer(g.u))
lower_g!(d, g::ProximalOperators.IndBox{<:Real,<:Real}) = (d.g_kind = 4; d.g_lo = g.lb; d.g_hi = g.ub)
lower_g!(d, g::Bazinga.NormL0Box) = (d.g_kind = 5; d.g_lambda = g.lambda; d.g_u = pointer(g.u))
lower_g!(d, g::Bazinga.NormLpPowerNonneg) = (d.g_kind = 6; d.g_lambda = g.alpha; d.g_p = g.p)
lower_g!(d, g::Bazinga.NormLpPowerBox) = (d.g_kind = 7; d.g_lambda = g.alpha; d.g_p = g.p; d.g_u = pointer(g.u))
lower_g!(d, g) = :generic

# c: any SmoothFunction whose eval!/jtprod! are the identity (e.g. test/definitions/identityFunction.jl)
abstract type IdentityLike <: Bazinga.SmoothFunction end
lower_c!(d, c::IdentityLike) = (d.c_kind = 0)
lower_c!(d, c::DenseAffine) = (d.c_kind = 1; d.c_A = pointer(c.At); d.c_b = pointer(c.b))
lower_c!(d, c::SparseAffine) = (d.c_kind = 3; d.c_sp_rowptr = pointer(c.rowptr); d.c_sp_col = pointer(c.col);
                                d.c_sp_val = pointer(c.val); d.c_sp_nnz = length(c.val); d.c_b = pointer(c.b))
lower_c!(d, c) = :generic

lower_D!(d, D::Bazinga.ZeroSet) = (d.D_kind = 0)
lower_D!(d, D::Bazinga.FreeSet) = (d.D_kind = 1)
lower_D!(d, D::Bazinga.IndicatorSet{<:ProximalOperators.IndBox{<:Real,<:Real}}) =
    (d.D_kind = 2; d.D_lo = D.f.lb; d.D_hi = D.f.ub)
"""
    PairwiseSet(kind)   kind in (:vc, :cc, :eitheror, :xor)

The package's 2-element projections (`project_onto_VC_set!` etc.) applied to every adjacent pair
`(cx[2j-1], cx[2j])`, the way `demo/mpvca.jl:103-107` and `demo/eitheror.jl:121-131` define their sets.
"""
struct PairwiseSet <: Bazinga.ClosedSet
    kind::Symbol
end
function Bazinga.proj!(z, D::PairwiseSet, x)
    p! = D.kind === :vc ? Bazinga.project_onto_VC_set! : D.kind === :cc ? Bazinga.project_onto_CC_set! :
         D.kind === :eitheror ? Bazinga.project_onto_EITHEROR_set! : Bazinga.project_onto_XOR_set!
    for j in 1:2:length(x)
        p!(@view(z[j:j+1]), x[j:j+1])
    end
    return nothing
end
lower_D!(d, D::PairwiseSet) = (d.D_kind = Dict(:vc => 3, :cc => 4, :eitheror => 5, :xor => 6)[D.kind])
lower_D!(d, D) = :generic

# ---- generic oracles: host callbacks (BZ_*_CALLBACK) --------------------------------------------
# Whatever the structured types above do not cover — the closures of demo/rosenbrock.jl:39-80, any user type with
# the package's protocol (src/Bazinga.jl:11-16) — is handed to the library as @cfunction callbacks.  The host
# evaluates f / grad f, prox_g, c, J'v and proj_D; the L-BFGS and line-search vector work stays on the device.
# When one of the four is generic, all four travel as callbacks (the structured types have the protocol anyway).
mutable struct GenericOracles{F,G,C,DD,T}
    f::F; g::G; c::C; D::DD
    err::Any                     # an exception raised inside a callback, parked until the library call has returned
end
# A callback cannot unwind through the library's C frames: it parks the exception and asks the library to end the call
# in progress (bz_callback_abort -> BZ_ERR_CALLBACK); `check_generic` rethrows it on the Julia side.
function _cb_guard(body, o, default)
    o.err === nothing || (ccall((:bz_callback_abort, lib), Cvoid, ()); return default)
    try
        return body()
    catch e
        o.err = e
        ccall((:bz_callback_abort, lib), Cvoid, ())
        return default
    end
end
function _cb_f(u::Ptr{Cvoid}, x::Ptr{T}, dfx::Ptr{T}, n::Int64)::Float64 where {T}
    o = unsafe_pointer_to_objref(u)
    _cb_guard(o, NaN) do
        Float64(Bazinga.gradient!(unsafe_wrap(Array, dfx, n), o.f, unsafe_wrap(Array, x, n)))
    end
end
function _cb_g(u::Ptr{Cvoid}, x::Ptr{T}, gamma::Float64, z::Ptr{T}, n::Int64)::Float64 where {T}
    o = unsafe_pointer_to_objref(u)
    _cb_guard(o, NaN) do
        Float64(Bazinga.prox!(unsafe_wrap(Array, z, n), o.g, unsafe_wrap(Array, x, n), T(gamma)))
    end
end
function _cb_ceval(u::Ptr{Cvoid}, x::Ptr{T}, cx::Ptr{T}, n::Int64, ny::Int64)::Cvoid where {T}
    o = unsafe_pointer_to_objref(u)
    _cb_guard(o, nothing) do
        Bazinga.eval!(unsafe_wrap(Array, cx, ny), o.c, unsafe_wrap(Array, x, n)); nothing
    end
end
function _cb_cjt(u::Ptr{Cvoid}, x::Ptr{T}, v::Ptr{T}, jtv::Ptr{T}, n::Int64, ny::Int64)::Cvoid where {T}
    o = unsafe_pointer_to_objref(u)
    _cb_guard(o, nothing) do
        Bazinga.jtprod!(unsafe_wrap(Array, jtv, n), o.c, unsafe_wrap(Array, x, n), unsafe_wrap(Array, v, ny)); nothing
    end
end
function _cb_D(u::Ptr{Cvoid}, v::Ptr{T}, s::Ptr{T}, ny::Int64)::Cvoid where {T}
    o = unsafe_pointer_to_objref(u)
    _cb_guard(o, nothing) do
        Bazinga.proj!(unsafe_wrap(Array, s, ny), o.D, unsafe_wrap(Array, v, ny)); nothing
    end
end
function lower_generic!(d, f, g, c, D, ::Type{T}) where {T}
    box = Ref(GenericOracles{typeof(f),typeof(g),typeof(c),typeof(D),T}(f, g, c, D, nothing))     # rooted by the Problem
    d.f_kind = 5; d.g_kind = 8; d.c_kind = 2; d.D_kind = 7
    d.cb_user = pointer_from_objref(box[])
    d.cb_f_gradient = @cfunction(_cb_f, Float64, (Ptr{Cvoid}, Ptr{T}, Ptr{T}, Int64))
    d.cb_g_prox = @cfunction(_cb_g, Float64, (Ptr{Cvoid}, Ptr{T}, Float64, Ptr{T}, Int64))
    d.cb_c_eval = @cfunction(_cb_ceval, Cvoid, (Ptr{Cvoid}, Ptr{T}, Ptr{T}, Int64, Int64))
    d.cb_c_jtprod = @cfunction(_cb_cjt, Cvoid, (Ptr{Cvoid}, Ptr{T}, Ptr{T}, Ptr{T}, Int64, Int64))
    d.cb_D_proj = @cfunction(_cb_D, Cvoid, (Ptr{Cvoid}, Ptr{T}, Ptr{T}, Int64))
    return box
end

mutable struct Problem
    h::Ptr{Cvoid}
    keep::Any
    # slack = true: the ALS form on xs = [x; s] (auglagfunslack.jl).  The library takes it for c = identity with an
    # element-wise f (Zero, DiagQuadratic; ny == n) and for c = DenseAffine with f Zero, DiagQuadratic, LeastSquares or
    # Quadratic (ny arbitrary, n a whole number of 16-byte packs); a sparse c, the stencil f, pairwise D and generic
    # oracles are BZ_ERR_UNSUPPORTED there
    function Problem(f, g, c, D, n, ny, ::Type{T}; slack::Bool = false) where {T}
        d = ProblemDesc(dtype = dtype_code(T), n = n, ny = ny, slack = Int32(slack))
        tmp = (lower_f!(d, f), lower_g!(d, g), lower_c!(d, c), lower_D!(d, D))      # temporaries the descriptor points into
        keep = any(t -> t === :generic, tmp) ? lower_generic!(d, f, g, c, D, T) : nothing
        h = Ref{Ptr{Cvoid}}(C_NULL)
        GC.@preserve f g c D tmp keep check(ccall((:bz_problem_create, lib), Cint,
            (Ptr{Cvoid}, Ref{ProblemDesc}, Ref{Ptr{Cvoid}}), context(), Ref(d), h))
        p = new(h[], (f, g, c, D, keep))      # generic oracles: the callback box lives as long as the problem
        finalizer(p -> ccall((:bz_problem_destroy, lib), Cvoid, (Ptr{Cvoid},), p.h), p)
    end
end

# lambda of g (NormL1, NormL1Nonneg, NormL1Box, NormL0Box, NormL21, GroupLasso) between solves, on the live problem: a number for a problem
# lowered from a number, a vector (the problem's type, length n; NormL21: one entry per group) for one lowered from an array
set_g_lambda!(p::Problem, lambda::Real) = check(ccall((:bz_problem_set_g_lambda, lib), Cint,
    (Ptr{Cvoid}, Cdouble, Ptr{Cvoid}), p.h, lambda, C_NULL))
set_g_lambda!(p::Problem, lambda::AbstractVector) = GC.@preserve lambda check(ccall((:bz_problem_set_g_lambda, lib), Cint,
    (Ptr{Cvoid}, Cdouble, Ptr{Cvoid}), p.h, 0.0, pointer(lambda)))

# l1 and l2 of g = ElasticNet between solves, on the live problem (a glmnet path moves λ, hence both); the weights stay
set_g_elastic_net!(p::Problem, l1::Real, l2::Real) = check(ccall((:bz_problem_set_g_elastic_net, lib), Cint,
    (Ptr{Cvoid}, Cdouble, Cdouble), p.h, l1, l2))

# ---- the subsolver seam: drop-in for ProximalAlgorithms.PANOCplus -----------------------------
struct PANOCplusHIP
    opts::PanocOpts
end
"""`PANOCplus(; directions=LBFGS(5), maxit, tol, verbose, freq, minimum_gamma, ...)` — same keywords
as ProximalAlgorithms.PANOCplus as the reference configures it (demo/rosenbrock.jl:109-115)."""
function PANOCplus(; directions = nothing, maxit = 1000, tol = 1e-8, verbose = false, freq = 10,
                   minimum_gamma = 1e-7, alpha = 0.95, beta = 0.5, max_backtracks = 20,
                   Lf = nothing, gamma = Lf === nothing ? nothing : alpha / Lf, adaptive = gamma === nothing, kwargs...)
    M = directions === nothing ? 5 : directions.memory
    compact = !(directions isa LBFGS) || directions.compact === nothing ? 2 : Int(directions.compact)
    PANOCplusHIP(PanocOpts(tol = tol, maxit = min(maxit, typemax(Int64)), freq = min(freq, typemax(Int32)),
                           verbose = verbose, minimum_gamma = minimum_gamma, alpha = alpha, beta = beta,
                           max_backtracks = max_backtracks, lbfgs_memory = M, lbfgs_compact = compact,
                           affine_refresh = get(kwargs, :affine_refresh, 16),
                           gamma = gamma === nothing ? 0.0 : gamma, Lf = Lf === nothing ? 0.0 : Lf, adaptive = Int32(adaptive)))
end

# one device problem per live AugLagFun; the entry (and, through the finalizer, the device buffers) goes with the functor
const _problems = WeakKeyDict{Any,Problem}()

"`solver(f = alFun, g = gFun, x0 = x) -> (sol, it)`   (alps.jl:66; als.jl:72 with the slack functors).  Keyword arguments
take no part in dispatch: the one keyword method hands over to `_solve`, which dispatches on the functor types."
(s::PANOCplusHIP)(; f, g, x0) = _solve(s, f, g, x0)

function _solve(s::PANOCplusHIP, f::Bazinga.AugLagFun, g::Bazinga.NonsmoothCostFun, x0::AbstractVector{T}) where {T}
    p = get!(() -> Problem(f.f, g.g, f.c, f.D, length(x0), length(f.y), T), _problems, f)
    mu = convert(Vector{T}, f.mu); y = convert(Vector{T}, f.y)
    check(ccall((:bz_problem_set_multipliers, lib), Cint, (Ptr{Cvoid}, Ptr{T}, Ptr{T}), p.h, mu, y), p)
    x = similar(x0); st = Ref(PanocStats())
    check(ccall((:bz_panoc_solve, lib), Cint, (Ptr{Cvoid}, Ref{PanocOpts}, Ptr{T}, Ptr{T}, Ref{PanocStats}),
                p.h, Ref(s.opts), x0, x, st), p)
    f.fx = T(st[].f_z)          # side channels alps reads back (alps.jl:68)
    g.gz = T(st[].g_z)
    g.gamma = st[].gamma
    return x, Int(st[].iters)
end

# the slack functors of auglagfunslack.jl (als.jl:72)
function _solve(s::PANOCplusHIP, f::Bazinga.AugLagFunSlack, g::Bazinga.NonsmoothCostFunSlack, x0::AbstractVector{T}) where {T}
    p = get!(() -> Problem(f.f, g.g, f.c, g.D, f.nx, f.ny, T; slack = true), _problems, f)
    mu = convert(Vector{T}, f.mu); y = convert(Vector{T}, f.y)
    check(ccall((:bz_problem_set_multipliers, lib), Cint, (Ptr{Cvoid}, Ptr{T}, Ptr{T}), p.h, mu, y), p)
    xs = similar(x0); st = Ref(PanocStats())
    check(ccall((:bz_panoc_solve, lib), Cint, (Ptr{Cvoid}, Ref{PanocOpts}, Ptr{T}, Ptr{T}, Ref{PanocStats}),
                p.h, Ref(s.opts), x0, xs, st), p)
    g.gz = T(st[].g_z)          # als.jl:79 reads gSlack.gz and evaluates f(x) itself
    g.gamma = st[].gamma
    return xs, Int(st[].iters)
end

# ---- the whole outer loop with device-resident vectors (bz_alps_solve) --------------------------
const _status = (:first_order, :max_iter, :exception, :unknown)          # alps.jl:105-113

"""`alps(f, g, c, D, x0, y0; kw...)`: same keywords, defaults and 10-tuple as `Bazinga.alps` (alps.jl:14-25,115);
only scalars cross PCIe between subproblems.  `warm_start = true` (not a keyword of the reference; default `false` = alps.jl:64)
starts every subproblem after the first at the step size the previous one ended with."""
function alps(f, g, c, D, x0::AbstractVector{T}, y0::AbstractVector{T}; tol::Real = T(1e-6), tol_prim::Real = tol,
              tol_dual::Real = tol, inner_tol::Real = cbrt(tol_dual), maxit::Integer = 100,
              theta_penalty::Real = 0.8, kappa_penalty::Real = 0.5, kappa_tol::Real = 0.1, verbose::Bool = false,
              subsolver = PANOCplus, subsolver_maxit::Integer = 1_000_000_000, warm_start::Bool = false) where {T}
    p = Problem(f, g, c, D, length(x0), length(y0), T)
    ao = AlpsOpts(tol_prim = tol_prim, tol_dual = tol_dual, inner_tol = inner_tol, maxit = maxit,
                  theta_penalty = theta_penalty, kappa_penalty = kappa_penalty, kappa_tol = kappa_tol,
                  subsolver_maxit = subsolver_maxit, verbose = verbose, warm_start = Int32(warm_start))
    po = subsolver(tol = inner_tol, verbose = verbose).opts
    x = similar(x0); y = similar(y0); s = similar(y0); mu = similar(y0); st = Ref(AlpsStats())
    check(ccall((:bz_alps_solve, lib), Cint,
                (Ptr{Cvoid}, Ref{AlpsOpts}, Ref{PanocOpts}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ref{AlpsStats}),
                p.h, Ref(ao), Ref(po), x0, y0, x, y, s, mu, st), p)
    r = st[]
    return x, y, Int(r.tot_it), Int(r.tot_inner_it), r.elapsed_s, _status[r.status + 1], T(r.inner_tol),
           (r.tot_it == 0 ? nothing : T(r.norm_res_prim)), s, mu      # alps.jl:34,115: `nothing` before the first outer iteration
end

"""`als(f, g, c, D, x0, y0; kw...)`: same keywords, defaults and 10-tuple as `Bazinga.als` (als.jl:14-25,118), the whole
outer loop on the device (bz_als_solve).  Lowered for c = identity with f Zero / DiagQuadratic and for c = DenseAffine with
f Zero / DiagQuadratic / LeastSquares / Quadratic — the (f, g, c, D) of demo/portfolio.jl with its constraint written as
`DenseAffine([mu'; ones(1, n)], zeros(2))` and its set as `ClosedSet(IndBox([rho, 1], [Inf, 1]))`."""
function als(f, g, c, D, x0::AbstractVector{T}, y0::AbstractVector{T}; tol::Real = T(1e-6), tol_prim::Real = tol,
             tol_dual::Real = tol, inner_tol::Real = cbrt(tol_dual), maxit::Integer = 100,
             theta_penalty::Real = 0.8, kappa_penalty::Real = 0.5, kappa_tol::Real = 0.1, verbose::Bool = false,
             subsolver = PANOCplus, subsolver_maxit::Integer = 1_000_000_000, warm_start::Bool = false) where {T}
    p = Problem(f, g, c, D, length(x0), length(y0), T; slack = true)
    ao = AlpsOpts(tol_prim = tol_prim, tol_dual = tol_dual, inner_tol = inner_tol, maxit = maxit,
                  theta_penalty = theta_penalty, kappa_penalty = kappa_penalty, kappa_tol = kappa_tol,
                  subsolver_maxit = subsolver_maxit, verbose = verbose, warm_start = Int32(warm_start))
    po = subsolver(tol = inner_tol, verbose = verbose).opts
    x = similar(x0); y = similar(y0); s = similar(y0); mu = similar(y0); st = Ref(AlpsStats())
    check(ccall((:bz_als_solve, lib), Cint,
                (Ptr{Cvoid}, Ref{AlpsOpts}, Ref{PanocOpts}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ref{AlpsStats}),
                p.h, Ref(ao), Ref(po), x0, y0, x, y, s, mu, st), p)
    r = st[]
    return x, y, Int(r.tot_it), Int(r.tot_inner_it), r.elapsed_s, _status[r.status + 1], T(r.inner_tol),
           (r.tot_it == 0 ? nothing : T(r.norm_res_prim)), s, mu
end

end # module
