#-------------------------------------------------------------------------------
# HMCMTHip -- the reference-side binding of libhmcmt_hip.so (include/hmcmt.h).
#
# Drop this module next to the reference's HMCMT package.  It overrides exactly the hot path:
#   compDataGradient(mtMesh, mtData, invParam, hmcprior)   (HMCSampler/HMCSampler.jl:277-330)
#   the forward solve inside getHamiltonian                (HMCSampler/HMCSampler.jl:358-397)
#   proposeLeapfrog(hmcParamCurrent, mtMesh, ...)          (HMCSampler/HMCSampler.jl:206-269), optional:
#                                                          the whole trajectory on the GPU (hmcmt_leapfrog)
# and leaves every other reference function (readstartupFile, runHMCSampler, parallelHMCSampler, writers)
# untouched.  Select it with `linearsolver: hip` in the startup file.
#
# One process = one GPU: under `addprocs(n)` + parallelHMCSampler (parallelHMC.jl:23-40) worker p uses device
# (p - 2) mod ndevices (worker ids start at 2), the master process device 0; HMCMT_DEVICE overrides.
#
# NOTE: this file could not be executed in the build container (no julia binary; tests/test_abi.py checks its
# struct field lists and bound symbols against include/hmcmt.h mechanically).  It is a thin `ccall` layer: every
# call passes the reference's own arrays straight through -- Julia's Vector{Float64} / Vector{ComplexF64} /
# Vector{Int64} have exactly the memory layout the C ABI expects (interleaved re/im doubles, 1-based int64
# indices).  The same ABI is exercised from Python/ctypes by tests/test_gpu_parity*.py and from compiled C by
# tests/c_abi/abi_check.c.
#-------------------------------------------------------------------------------
module HMCMTHip

using LinearAlgebra            # diag
using SparseArrays
using Distributed              # myid
using HMCMT.HMCFileIO, HMCMT.HMCStruct, HMCMT.HMCUtility

export HipContext, hipContext, compDataGradient, compJacMat, compJacTMat, compJacMatVec, compJacTMatVec, compJacMatMat, compJacTMatMat, hipLinearize!, hipGNHessVec, hipGNHessMat, hipSensitivity, hipForward, setPrior!, set_mass_lowrank!, chain_adapt_lowrank!, chain_adapt_lowrank_info, chain_set_mass_lowrank!, chain_mass_lowrank, chain_sketch_begin!, chain_sketch_info, chain_sketch, chain_pca, HmcmtSketchInfo, proposeLeapfrog, proposeLeapfrogDevice!,
       hipWait, HmcmtChainRecord, chainBegin!, chainMomentum!, chainStep!, chainState, chainMoments, chainSetEnergy!, chainEnd!, chain_save, chain_restore!, chain_blob_info, HmcmtChainBlobHeader, chainHistBegin!, chainHist, chainQuantiles, chainDataMomentsBegin!, chainDataMoments, chain_hist!, chainAcovBegin!, chainAcov, chainEss, chain_ess!, chainCovBegin!, chainCov, chainCorr, chain_cov!, HmcmtAdaptOptions, HmcmtAdaptInfo, chainSetDt!, chainSetMassDiag!, chainMassDiag, chainAdaptBegin!, chainAdaptInfo, chainAdaptEnd!, chain_seed!, chain_rng_state, HmcmtMapOptions, HmcmtMapRecord, map_options, map_begin!, map_step!, map_run!, map_state, map_end!, find_map, chain_sample!, chain_run!, chain_nuts_sample!, chain_nuts_run!, HmcmtNutsRecord, run_chain!, hipStats, hipGuard, hipPersistInfo, hipPersistWidth, hipPersistEnvelope, hipPersistOrder, hipPersistPack, hipNextCuShare, destroy!, commId, SampleComm, allgatherSamples

const libhmcmt = get(ENV, "HMCMT_HIP_LIB", joinpath(@__DIR__, "..", "hmcmt2d_amd", "libhmcmt_hip.so"))

# field order and types of include/hmcmt.h (checked by tests/test_abi.py against the ctypes mirror)
struct HmcmtOptions
    precond::Int32
    maxit::Int32
    tol::Float64
    check_every::Int32
    verify::Int32
    warm_start::Int32
    fdm_precision::Int32
end

struct HmcmtStats
    iters_fwd_max::Int32
    iters_adj_max::Int32
    iters_fwd_sum::Int32
    iters_adj_sum::Int32
    err_est_max::Float64
    true_res_max::Float64
    status::Int32
    nsystems::Int32
    fallback_solves::Int32
    smoother_sweeps::Int32
end

# hmcmt_chain_record of include/hmcmt.h: what hmcmt_chain_step reports of one sample (tests/test_chain_host.py compares the fields
# with the ctypes mirror)
struct HmcmtChainRecord
    accepted::Int32
    nfevals::Int32
    K0::Float64
    K1::Float64
    D1::Float64
    M1::Float64
    D::Float64
    M::Float64
    hdif::Float64
    nsamples::Int64
    nmoments::Int64
end

# hmcmt_nuts_record of include/hmcmt.h: what hmcmt_chain_nuts_sample reports of one sample -- the chain record at the selected state,
# then the tree (tests/test_nuts_host.py compares the layout with the ctypes mirror)
struct HmcmtNutsRecord
    rec::HmcmtChainRecord
    depth::Int32
    nleaves::Int32
    stop::Int32
    dirs::UInt32
    selected::Int64
    alpha::Float64
end

# hmcmt_adapt_options and hmcmt_adapt_info of include/hmcmt.h: the warm-up hmcmt_chain_adapt_begin starts and where it stands
# (tests/test_adapt_host.py compares the fields with the ctypes mirrors)
struct HmcmtAdaptOptions
    nwarmup::Int64
    adapt_mass::Int32
    init_buffer::Int32
    term_buffer::Int32
    base_window::Int32
    delta::Float64
    gamma::Float64
    t0::Float64
    kappa::Float64
    dt_min::Float64
    dt_max::Float64
end

struct HmcmtAdaptInfo
    step::Int64
    nwarmup::Int64
    window_count::Int64
    next_window_end::Int64
    active::Int32
    windows_done::Int32
    dt::Float64
    dt_bar::Float64
    mu::Float64
    s_bar::Float64
    alpha_last::Float64
    alpha_sum::Float64
end

mutable struct HipContext
    ptr::Ptr{Cvoid}
    nAC::Int
    nData::Int
    device::Int
    realData::Bool          # DataType Rho_Pha: the reference's obsData / predData are real vectors
end

# component codes of include/hmcmt.h (the same table as hmcmt2d_amd/marshal.py COMPONENT_CODES; tests/test_abi.py compares them)
# (7 TZY, 8 RealTZY, 9 ImagTZY: the tipper T = Hz/Hy, listed after the other components)
const COMPONENT_CODES = Dict("ZXY" => 1, "ZYX" => 2, "RhoXY" => 3, "PhsXY" => 4, "RhoYX" => 5, "PhsYX" => 6,
                             "TZY" => 7, "RealTZY" => 8, "ImagTZY" => 9)

function compModes(dataComp, dataType::AbstractString)
    isimp = occursin("Impedance", dataType)
    (isimp || occursin("Rho_Pha", dataType) || occursin("Rho_Phs", dataType)) ||
        error("unsupported DataType $dataType (Impedance or Rho_Pha)")
    out = Int64[]
    for c in dataComp
        haskey(COMPONENT_CODES, c) || error("unsupported data component $c (log10Rho*: the reference's forward and sensitivity disagree on it)")
        code = COMPONENT_CODES[c]
        (code <= 2 || code == 7) == isimp || error("data component $c does not belong to DataType $dataType")
        (!isempty(out) && out[end] >= 7 && code < 7) &&
            error("data component $c is listed after a tipper component (the tipper components come last)")
        push!(out, code)
    end
    return out
end

function checkerr(ctx::Ptr{Cvoid}, rc::Cint)
    rc == 0 && return
    msg = unsafe_string(ccall((:hmcmt_last_error, libhmcmt), Cstring, (Ptr{Cvoid},), ctx))
    error("libhmcmt_hip error $rc: $msg")        # same behaviour as checkMUMPSerror (MUMPSfuncs.jl:59-73)
end

"""
    defaultDevice()

GPU of this Julia process: `HMCMT_DEVICE` if set, else worker id - 2 modulo `HMCMT_NDEVICES` (default 8) on a
worker started by `addprocs`, else 0.
"""
function defaultDevice()
    haskey(ENV, "HMCMT_DEVICE") && return parse(Int, ENV["HMCMT_DEVICE"])
    ndev = parse(Int, get(ENV, "HMCMT_NDEVICES", "8"))
    return myid() >= 2 ? mod(myid() - 2, ndev) : 0
end

"""
    hipContext(mtMesh, mtData, invParam; device=defaultDevice())

Builds the GPU context once per run (replaces the operator set-up the reference redoes on every
call: setupTensorMesh2D!, getBoundaryIndex, preSetRxFieldSens).
"""
function hipContext(mtMesh::TensorMesh2D, mtData::MTData, invParam::InvDataModel; device::Integer=defaultDevice())
    ny, nz = mtMesh.gridSize
    compMode = compModes(mtData.dataComp, mtData.dataType)
    realData = !occursin("Impedance", mtData.dataType)
    rxY = Vector{Float64}(mtData.rxLoc[:, 1]); rxZ = Vector{Float64}(mtData.rxLoc[:, 2])
    dataID = Vector{UInt8}(mtData.dataID)
    obs = Vector{ComplexF64}(invParam.obsData)
    dataW = Vector{Float64}(diag(invParam.dataW))
    activeIdx = Vector{Int64}(invParam.activeCell.rowval)        # 1-based cell id of each column
    ctxref = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:hmcmt_create, libhmcmt), Cint,
               (Ref{Ptr{Cvoid}}, Int32,
                Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                Int64, Ptr{Float64},
                Int64, Ptr{Float64}, Ptr{Float64},
                Int64, Ptr{Int64},
                Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64},
                Ptr{UInt8}, Ptr{ComplexF64}, Ptr{Float64},
                Int64, Ptr{Int64}, Ptr{Float64}, Ptr{HmcmtOptions}),
               ctxref, Int32(device),
               ny, nz, mtMesh.yLen, mtMesh.zLen, mtMesh.origin,
               length(mtData.freqs), mtData.freqs,
               length(rxY), rxY, rxZ,
               length(compMode), compMode,
               length(obs), mtData.freqID, mtData.rxID, mtData.dtID,
               dataID, obs, dataW,
               length(activeIdx), activeIdx, invParam.bgModel, C_NULL)
    checkerr(C_NULL, rc)
    ctx = HipContext(ctxref[], length(activeIdx), length(obs), Int(device), realData)
    finalizer(destroy!, ctx)
    return ctx
end

function destroy!(ctx::HipContext)
    if ctx.ptr != C_NULL
        ccall((:hmcmt_destroy, libhmcmt), Cint, (Ptr{Cvoid},), ctx.ptr)
        ctx.ptr = C_NULL
    end
end

# one context per InvDataModel of this process (WeakKeyDict: the context goes with its problem)
const contexts = WeakKeyDict{Any,HipContext}()
getctx(mtMesh, mtData, invParam) = get!(() -> hipContext(mtMesh, mtData, invParam), contexts, invParam)

"""
    compDataGradient(mtMesh, mtData, invParam, hmcprior) -> (predData, dataMisfit, dataGrad)

Same signature and return values as HMCSampler.compDataGradient (HMCSampler.jl:277-330).
"""
function compDataGradient(mtMesh::TensorMesh2D, mtData::MTData, invParam::InvDataModel, hmcprior::HMCPrior)
    ctx = getctx(mtMesh, mtData, invParam)
    m = invParam.strModel
    pred = Vector{ComplexF64}(undef, ctx.nData)
    grad = Vector{Float64}(undef, ctx.nAC)
    misfit = Ref{Float64}(0.0)
    rc = ccall((:hmcmt_grad, libhmcmt), Cint,
               (Ptr{Cvoid}, Ptr{Float64}, Ptr{ComplexF64}, Ref{Float64}, Ptr{Float64}),
               ctx.ptr, m, pred, misfit, grad)
    checkerr(ctx.ptr, rc)
    # keep mtMesh.sigma in the state the reference leaves it in (HMCSampler.jl:293-294)
    mtMesh.sigma = invParam.activeCell * exp.(m) + invParam.bgModel
    return (ctx.realData ? real.(pred) : pred), misfit[], grad
end

"""
    compJacMat(mtMesh, mtData, invParam; wrt=:sigma) -> J (nData x nAC)

The data Jacobian at invParam.strModel (MTSensitivity/compJacMat.jl): d data / d sigma of the active cells (wrt=:lnsigma:
d / d ln sigma).  ComplexF64 for DataType Impedance, Float64 for Rho_Pha.  hmcmt_jacobian fills J^T column by column (its
row-major [nData][nAC] is Julia's column-major [nAC, nData]).
"""
compJacMat(mtMesh::TensorMesh2D, mtData::MTData, invParam::InvDataModel; wrt::Symbol=:sigma) =
    permutedims(compJacTMat(mtMesh, mtData, invParam; wrt=wrt))

"""
    compJacTMat(mtMesh, mtData, invParam; wrt=:sigma) -> J^T (nAC x nData), as MTSensitivity/compJacTMat.jl orients it.
"""
function compJacTMat(mtMesh::TensorMesh2D, mtData::MTData, invParam::InvDataModel; wrt::Symbol=:sigma)
    ctx = getctx(mtMesh, mtData, invParam)
    JT = ctx.realData ? Matrix{Float64}(undef, ctx.nAC, ctx.nData) : Matrix{ComplexF64}(undef, ctx.nAC, ctx.nData)
    st = Ref{HmcmtStats}()
    rc = ccall((:hmcmt_jacobian, libhmcmt), Cint,
               (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Int32, Ptr{Cvoid}, Ref{HmcmtStats}),
               ctx.ptr, invParam.strModel, 0, ctx.nData, jacWrt(wrt), JT, st)
    checkerr(ctx.ptr, rc)
    return JT
end

"""
    hipSensitivity(mtMesh, mtData, invParam; wrt=:sigma) -> sens (nAC): sqrt(sum_k |dataW_k J_ka|^2), J not formed
"""
function hipSensitivity(mtMesh::TensorMesh2D, mtData::MTData, invParam::InvDataModel; wrt::Symbol=:sigma)
    ctx = getctx(mtMesh, mtData, invParam)
    sens = Vector{Float64}(undef, ctx.nAC)
    st = Ref{HmcmtStats}()
    rc = ccall((:hmcmt_sensitivity, libhmcmt), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int32, Ptr{Float64}, Ref{HmcmtStats}),
               ctx.ptr, invParam.strModel, jacWrt(wrt), sens, st)
    checkerr(ctx.ptr, rc)
    return sens
end
"""
    hipLinearize!(mtMesh, mtData, invParam)

Sets the linearisation point of the matrix-free Jacobian products at invParam.strModel (hmcmt_linearize): valid until the next
evaluating call on the context.
"""
function hipLinearize!(mtMesh::TensorMesh2D, mtData::MTData, invParam::InvDataModel)
    ctx = getctx(mtMesh, mtData, invParam)
    checkerr(ctx.ptr, ccall((:hmcmt_linearize, libhmcmt), Cint, (Ptr{Cvoid}, Ptr{Float64}), ctx.ptr, invParam.strModel))
    return ctx
end

"""
    compJacMatVec(mtMesh, mtData, invParam, v; wrt=:sigma) -> compJacMat(...) * v (nData) by the tangent-linear route: one solve, no J
"""
function compJacMatVec(mtMesh::TensorMesh2D, mtData::MTData, invParam::InvDataModel, v::Vector{Float64}; wrt::Symbol=:sigma)
    ctx = hipLinearize!(mtMesh, mtData, invParam)
    Jv = Vector{ComplexF64}(undef, ctx.nData)
    st = Ref{HmcmtStats}()
    rc = ccall((:hmcmt_jvp, libhmcmt), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int32, Ptr{Cvoid}, Ref{HmcmtStats}), ctx.ptr, v, jacWrt(wrt), Jv, st)
    checkerr(ctx.ptr, rc)
    return ctx.realData ? real.(Jv) : Jv
end

"""
    compJacTMatVec(mtMesh, mtData, invParam, datVec; wrt=:sigma) -> real(J^T conj(datVec)) (nAC)

The reference's real(compJacTMatVec(exTE, hxTM, datVec, ...)) (MTSensitivity/compJacTMatVec.jl:8) for a free data vector.
"""
function compJacTMatVec(mtMesh::TensorMesh2D, mtData::MTData, invParam::InvDataModel, datVec::AbstractVector; wrt::Symbol=:sigma)
    ctx = hipLinearize!(mtMesh, mtData, invParam)
    u = Vector{ComplexF64}(datVec)
    out = Vector{Float64}(undef, ctx.nAC)
    st = Ref{HmcmtStats}()
    rc = ccall((:hmcmt_jtvp, libhmcmt), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Float64}, Ref{HmcmtStats}), ctx.ptr, u, jacWrt(wrt), out, st)
    checkerr(ctx.ptr, rc)
    return out
end

"""
    hipGNHessVec(mtMesh, mtData, invParam, v; wrt=:sigma) -> Re(J^H W^2 J) v (nAC), W = dataW; no prior term (hmcmt_gn_hessvec)
"""
function hipGNHessVec(mtMesh::TensorMesh2D, mtData::MTData, invParam::InvDataModel, v::Vector{Float64}; wrt::Symbol=:sigma)
    ctx = hipLinearize!(mtMesh, mtData, invParam)
    out = Vector{Float64}(undef, ctx.nAC)
    st = Ref{HmcmtStats}()
    rc = ccall((:hmcmt_gn_hessvec, libhmcmt), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int32, Ptr{Float64}, Ref{HmcmtStats}), ctx.ptr, v, jacWrt(wrt), out, st)
    checkerr(ctx.ptr, rc)
    return out
end
"""
    compJacMatMat(mtMesh, mtData, invParam, V; wrt=:sigma) -> compJacMat(...) * V (nData x nvec)

The columns of V (nAC x nvec, nvec <= 32) in ONE solve of all systems and directions (hmcmt_jvp_block); column j is compJacMatVec(V[:, j]).
"""
function compJacMatMat(mtMesh::TensorMesh2D, mtData::MTData, invParam::InvDataModel, V::Matrix{Float64}; wrt::Symbol=:sigma)
    ctx = hipLinearize!(mtMesh, mtData, invParam)
    size(V, 1) == ctx.nAC || throw(ArgumentError("V: nAC rows"))
    JV = Matrix{ComplexF64}(undef, ctx.nData, size(V, 2))
    st = Ref{HmcmtStats}()
    rc = ccall((:hmcmt_jvp_block, libhmcmt), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int32, Int32, Ptr{Cvoid}, Ref{HmcmtStats}), ctx.ptr, V, Int32(size(V, 2)), jacWrt(wrt), JV, st)
    checkerr(ctx.ptr, rc)
    return ctx.realData ? real.(JV) : JV
end

"""
    compJacTMatMat(mtMesh, mtData, invParam, U; wrt=:sigma) -> real(J^T conj(U)) (nAC x nvec), one adjoint-type solve (hmcmt_jtvp_block)
"""
function compJacTMatMat(mtMesh::TensorMesh2D, mtData::MTData, invParam::InvDataModel, U::AbstractMatrix; wrt::Symbol=:sigma)
    ctx = hipLinearize!(mtMesh, mtData, invParam)
    size(U, 1) == ctx.nData || throw(ArgumentError("U: nData rows"))
    u = Matrix{ComplexF64}(U)
    out = Matrix{Float64}(undef, ctx.nAC, size(u, 2))
    st = Ref{HmcmtStats}()
    rc = ccall((:hmcmt_jtvp_block, libhmcmt), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int32, Ptr{Float64}, Ref{HmcmtStats}), ctx.ptr, u, Int32(size(u, 2)), jacWrt(wrt), out, st)
    checkerr(ctx.ptr, rc)
    return out
end

"""
    hipGNHessMat(mtMesh, mtData, invParam, V; wrt=:sigma) -> Re(J^H W^2 J) V (nAC x nvec): one solve of each type (hmcmt_gn_hessvec_block)
"""
function hipGNHessMat(mtMesh::TensorMesh2D, mtData::MTData, invParam::InvDataModel, V::Matrix{Float64}; wrt::Symbol=:sigma)
    ctx = hipLinearize!(mtMesh, mtData, invParam)
    size(V, 1) == ctx.nAC || throw(ArgumentError("V: nAC rows"))
    out = Matrix{Float64}(undef, ctx.nAC, size(V, 2))
    st = Ref{HmcmtStats}()
    rc = ccall((:hmcmt_gn_hessvec_block, libhmcmt), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int32, Int32, Ptr{Float64}, Ref{HmcmtStats}), ctx.ptr, V, Int32(size(V, 2)), jacWrt(wrt), out, st)
    checkerr(ctx.ptr, rc)
    return out
end

# the same on device memory of the context's GPU (raw pointers; the point set by hipLinearize!): complete on return
function hipJacMatMatDevice!(ctx, dV::Ptr{Cvoid}, nvec::Integer, dJV::Ptr{Cvoid}; wrt::Symbol=:sigma)
    st = Ref{HmcmtStats}()
    checkerr(ctx.ptr, ccall((:hmcmt_jvp_block_device, libhmcmt), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int32, Ptr{Cvoid}, Ref{HmcmtStats}), ctx.ptr, dV, Int32(nvec), jacWrt(wrt), dJV, st))
    return st[]
end
function hipJacTMatMatDevice!(ctx, dU::Ptr{Cvoid}, nvec::Integer, dJTU::Ptr{Cvoid}; wrt::Symbol=:sigma)
    st = Ref{HmcmtStats}()
    checkerr(ctx.ptr, ccall((:hmcmt_jtvp_block_device, libhmcmt), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int32, Ptr{Cvoid}, Ref{HmcmtStats}), ctx.ptr, dU, Int32(nvec), jacWrt(wrt), dJTU, st))
    return st[]
end
function hipGNHessMatDevice!(ctx, dV::Ptr{Cvoid}, nvec::Integer, dHV::Ptr{Cvoid}; wrt::Symbol=:sigma)
    st = Ref{HmcmtStats}()
    checkerr(ctx.ptr, ccall((:hmcmt_gn_hessvec_block_device, libhmcmt), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int32, Ptr{Cvoid}, Ref{HmcmtStats}), ctx.ptr, dV, Int32(nvec), jacWrt(wrt), dHV, st))
    return st[]
end
jacWrt(wrt::Symbol) = wrt === :sigma ? Int32(0) : wrt === :lnsigma ? Int32(1) : throw(ArgumentError("wrt: :sigma or :lnsigma"))

"""
    hipForward(mtMesh, mtData, invParam) -> (predData, dataMisfit)

Replaces `MT2DFwdSolver` + `compDataMisfit` in getHamiltonian (HMCSampler.jl:364,384).
"""
function hipForward(mtMesh::TensorMesh2D, mtData::MTData, invParam::InvDataModel)
    ctx = getctx(mtMesh, mtData, invParam)
    pred = Vector{ComplexF64}(undef, ctx.nData)
    misfit = Ref{Float64}(0.0)
    rc = ccall((:hmcmt_forward, libhmcmt), Cint,
               (Ptr{Cvoid}, Ptr{Float64}, Ptr{ComplexF64}, Ref{Float64}),
               ctx.ptr, invParam.strModel, pred, misfit)
    checkerr(ctx.ptr, rc)
    return (ctx.realData ? real.(pred) : pred), misfit[]
end

"""
    setPrior!(ctx, invParam, hmcParam)

Registers the prior (refModel, Wm) and the mass matrix for device-resident trajectories (hmcmt_set_prior,
hmcmt_set_mass).  Wm is symmetric, so its CSC arrays are its CSR arrays; they go over 0-based.  A diagonal invM goes
over as its diagonal; any other is the reference's non-diagonal mass M = Wm (setMassMatrix(invParam),
HMCSampler.jl:478-489, masstype: nondiagonal): the library factors Wm once (and keeps the factor while Wm stays the
same) and runs the trajectory with Wm^-1 p and chol(Wm).L on the device.
"""
const HMCMT_MASS_WM = Int32(1)
function setPrior!(ctx::HipContext, invParam::InvDataModel, hmcParam::HMCParameter)
    diagonal = hmcParam.invM isa Diagonal || isdiag(hmcParam.invM)
    Wm = invParam.Wm
    rowptr = Vector{Int64}(Wm.colptr .- 1)
    colind = Vector{Int64}(Wm.rowval .- 1)
    val = Vector{Float64}(Wm.nzval)
    invM = diagonal ? Vector{Float64}(diag(hmcParam.invM)) : ones(Float64, length(invParam.refModel))
    rc = ccall((:hmcmt_set_prior, libhmcmt), Cint,
               (Ptr{Cvoid}, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}),
               ctx.ptr, invParam.refModel, rowptr, colind, val, invM)
    checkerr(ctx.ptr, rc)
    if !diagonal
        rc = ccall((:hmcmt_set_mass, libhmcmt), Cint, (Ptr{Cvoid}, Int32), ctx.ptr, HMCMT_MASS_WM)
        checkerr(ctx.ptr, rc)
    end
    return ctx
end

"""
    set_mass_lowrank!(ctx, invM, U, lam)

The low-rank-plus-diagonal mass M^-1 = S (I + U (Λ - I) U') S, S = diag(sqrt.(invM)) (hmcmt_set_mass_lowrank, include/hmcmt.h): `invM`
the nAC scales squared, or `nothing` for the diagonal in force; `U` nAC × r with orthonormal columns -- Julia's column-major matrix is
the C layout, one direction after the other --, `lam` its r variances in units of the scales, 1 ≤ r ≤ HMCMT_MASS_RANK_MAX.  Call it
behind `setPrior!`; like it, it ends a running chain.
"""
const HMCMT_MASS_LOWRANK = Int32(2)
const HMCMT_MASS_RANK_MAX = 32
function set_mass_lowrank!(ctx::HipContext, invM::Union{Nothing,Vector{Float64}}, U::Matrix{Float64}, lam::Vector{Float64})
    size(U, 1) == ctx.nAC || error("set_mass_lowrank!: U must be nAC = $(ctx.nAC) × r")
    length(lam) == size(U, 2) || error("set_mass_lowrank!: lam must hold one entry per column of U")
    invM === nothing || length(invM) == ctx.nAC || error("set_mass_lowrank!: invM must hold nAC = $(ctx.nAC) entries")
    rc = ccall((:hmcmt_set_mass_lowrank, libhmcmt), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}),
               ctx.ptr, invM === nothing ? C_NULL : invM, Int32(size(U, 2)), U, lam)
    checkerr(ctx.ptr, rc)
    return ctx
end

"""
    proposeLeapfrog(hmcParamCurrent, mtMesh, mtData, invParam, hmcprior) -> (propModel, propMomentum)

Same signature and return values as HMCSampler.proposeLeapfrog (HMCSampler.jl:206-269); the L + 1 gradient
evaluations, the momentum / position updates, the step clamp and the bound reflection run on the GPU
(hmcmt_leapfrog).  The forward response at the proposal comes back with the trajectory: getHamiltonian's
`hipForward` at the same model is then answered from the library's memo without a solve.
"""
function proposeLeapfrog(hmcParamCurrent::HMCParameter, mtMesh::TensorMesh2D, mtData::MTData,
                         invParam::InvDataModel, hmcprior::HMCPrior)
    ctx = getctx(mtMesh, mtData, invParam)
    # every trajectory: runHMCSampler re-randomises invParam.refModel on each run (HMCSampler.jl:100-109) and the mass
    # matrix may change between runs; the upload is O(nnz(Wm)), nothing beside a trajectory
    setPrior!(ctx, invParam, hmcParamCurrent)
    intstep = rand(hmcprior.timestep[1]:hmcprior.timestep[2])          # unirandInteger (HMCUtility.jl)
    n = ctx.nAC
    m1 = Vector{Float64}(undef, n); p1 = Vector{Float64}(undef, n)
    pred = Vector{ComplexF64}(undef, ctx.nData)
    misfit = Ref{Float64}(0.0); mnorm = Ref{Float64}(0.0); nf = Ref{Int32}(0)
    rc = ccall((:hmcmt_leapfrog, libhmcmt), Cint,
               (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Float64, Int32, Float64, Float64, Float64,
                Ptr{Float64}, Ptr{Float64}, Ptr{ComplexF64}, Ref{Float64}, Ref{Float64}, Ref{Int32}),
               ctx.ptr, hmcParamCurrent.rhomodel, hmcParamCurrent.momentum, hmcprior.dt, Int32(intstep),
               hmcprior.regParam, log(hmcprior.sigBounds[1]), log(hmcprior.sigBounds[2]),
               m1, p1, pred, misfit, mnorm, nf)
    checkerr(ctx.ptr, rc)
    hmcprior.nfevals += nf[]
    invParam.strModel = copy(m1)
    mtMesh.sigma = invParam.activeCell * exp.(m1) + invParam.bgModel
    return m1, p1
end

"""
    proposeLeapfrogDevice!(ctx, d_m, d_p, dt, L, regParam, lnSigMin, lnSigMax; startGrad=0,
                           d_pred=C_NULL, d_misfit=C_NULL, d_mnorm=C_NULL) -> nfevals

hmcmt_leapfrog_device for callers that keep the chain state in GPU memory (e.g. AMDGPU.jl `ROCArray`s: pass
`pointer(a)`): d_m, d_p are updated in place, nothing crosses PCIe; complete with `hipWait(ctx)`.  `startGrad` as in
include/hmcmt.h (0 evaluate, 1 previous proposal accepted, 2 rejected).  Call `setPrior!` first.
"""
function proposeLeapfrogDevice!(ctx::HipContext, d_m::Ptr, d_p::Ptr, dt::Real, L::Integer, regParam::Real,
                                lnSigMin::Real, lnSigMax::Real; startGrad::Integer=0,
                                d_pred::Ptr=C_NULL, d_misfit::Ptr=C_NULL, d_mnorm::Ptr=C_NULL)
    nf = Ref{Int32}(0)
    rc = ccall((:hmcmt_leapfrog_device, libhmcmt), Cint,
               (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Int32, Float64, Float64, Float64, Int32,
                Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{Int32}),
               ctx.ptr, d_m, d_p, Float64(dt), Int32(L), Float64(regParam), Float64(lnSigMin), Float64(lnSigMax),
               Int32(startGrad), d_pred, d_misfit, d_mnorm, nf)
    checkerr(ctx.ptr, rc)
    return Int(nf[])
end

"""
    chainBegin!(ctx, mStart, dt, regParam, lnSigMin, lnSigMax; burnin=0) -> (D0, M0)
    chainMomentum!(ctx, z) -> K;  chainStep!(ctx, L, u; mOut=nothing, predOut=nothing) -> HmcmtChainRecord
    chainState(ctx) -> (m, p, pred);  chainMoments(ctx) -> (count, mean, m2);  chainEnd!(ctx)

The HMC chain on the device (hmcmt_chain_*, include/hmcmt.h): runHMCSampler's loop (HMCSampler.jl:132-186) with model, momentum,
predicted data and the streaming posterior moments in GPU memory.  Call `setPrior!` first.  The random numbers are the caller's:
`z` standard normals (clipped at +-2.5 by the library, getMomentumVector), `u` one uniform per sample.  `run_chain!` is the loop.
"""
function chainBegin!(ctx::HipContext, mStart::Vector{Float64}, dt::Real, regParam::Real, lnSigMin::Real, lnSigMax::Real;
                     burnin::Integer=0)
    D0 = Ref{Float64}(0.0); M0 = Ref{Float64}(0.0)
    rc = ccall((:hmcmt_chain_begin, libhmcmt), Cint,
               (Ptr{Cvoid}, Ptr{Float64}, Float64, Float64, Float64, Float64, Int64, Ref{Float64}, Ref{Float64}),
               ctx.ptr, mStart, Float64(dt), Float64(regParam), Float64(lnSigMin), Float64(lnSigMax), Int64(burnin), D0, M0)
    checkerr(ctx.ptr, rc)
    return D0[], M0[]
end

function chainMomentum!(ctx::HipContext, z::Vector{Float64})
    K = Ref{Float64}(0.0)
    rc = ccall((:hmcmt_chain_momentum, libhmcmt), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ref{Float64}), ctx.ptr, z, K)
    checkerr(ctx.ptr, rc)
    return K[]
end

# (the record travels as Ref{HmcmtChainRecord}: an isbits struct with the C layout)
function chainStep!(ctx::HipContext, L::Integer, u::Real; mOut::Union{Nothing,Vector{Float64}}=nothing,
                    predOut::Union{Nothing,Vector{ComplexF64}}=nothing)
    rec = Ref(HmcmtChainRecord(0, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0, 0))
    pm = mOut === nothing ? Ptr{Float64}(C_NULL) : pointer(mOut)
    pp = predOut === nothing ? Ptr{ComplexF64}(C_NULL) : pointer(predOut)
    rc = GC.@preserve mOut predOut @ccall libhmcmt.hmcmt_chain_step(ctx.ptr::Ptr{Cvoid}, Int32(L)::Int32, Float64(u)::Float64,
                                                                   rec::Ref{HmcmtChainRecord}, pm::Ptr{Float64}, pp::Ptr{ComplexF64})::Cint
    checkerr(ctx.ptr, rc)
    return rec[]
end

function chainState(ctx::HipContext)
    m = Vector{Float64}(undef, ctx.nAC); p = Vector{Float64}(undef, ctx.nAC)
    pred = Vector{ComplexF64}(undef, ctx.nData)
    rc = ccall((:hmcmt_chain_state, libhmcmt), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{ComplexF64}), ctx.ptr, m, p, pred)
    checkerr(ctx.ptr, rc)
    return m, p, (ctx.realData ? real.(pred) : pred)
end

function chainMoments(ctx::HipContext)
    count = Ref{Int64}(0)
    mean = Vector{Float64}(undef, ctx.nAC); m2 = Vector{Float64}(undef, ctx.nAC)
    rc = ccall((:hmcmt_chain_moments, libhmcmt), Cint, (Ptr{Cvoid}, Ref{Int64}, Ptr{Float64}, Ptr{Float64}, Int32),
               ctx.ptr, count, mean, m2, Int32(0))
    checkerr(ctx.ptr, rc)
    return Int(count[]), mean, m2
end

# replaces the D and M the chain holds for its current model (hmcmt_chain_set_energy): a restored chain, or the reference's start
chainSetEnergy!(ctx::HipContext, D::Real, M::Real) =
    checkerr(ctx.ptr, ccall((:hmcmt_chain_set_energy, libhmcmt), Cint, (Ptr{Cvoid}, Float64, Float64), ctx.ptr, Float64(D), Float64(M)))

chainEnd!(ctx::HipContext) = checkerr(ctx.ptr, ccall((:hmcmt_chain_end, libhmcmt), Cint, (Ptr{Cvoid},), ctx.ptr))

# field order and types of hmcmt_chain_blob_header (include/hmcmt.h; checked by tests/test_checkpoint_host.py against the ctypes mirror)
struct HmcmtChainBlobHeader
    version::UInt32
    nsections::UInt32
    total_bytes::UInt64
    nAC::Int64
    nData::Int64
    mass_kind::Int32
    seeded::UInt32
    nsamples::Int64
    nmoments::Int64
    tags::NTuple{16,UInt32}
    section_bytes::NTuple{16,UInt64}
end

"""
    chain_save(ctx) -> Vector{UInt8};  chain_restore!(ctx, blob);  chain_blob_info(blob) -> NamedTuple

Checkpoint and resume of the chain (hmcmt_chain_save, hmcmt_chain_restore, hmcmt_chain_blob_info; include/hmcmt.h has the blob's format
to the byte).  `chain_save` is a read-out: state, moments, generator, the mass in force, every accumulator that is on and an adaptation
that was begun, as one blob; the chain goes on as if it had not been called.  `chain_restore!` comes behind `setPrior!` (and the mass
call for M = Wm) IN PLACE OF `chainBegin!` and every accumulator's and adaptation's begin call; it evaluates nothing, and the first
sample behind it evaluates its start gradient (one evaluation more in its record).  A momentum is not restored: a host-fed chain calls
`chainMomentum!` again.  `chain_blob_info` validates a blob's container without a context or a GPU: the header's fields and
`sections`, the (tag, bytes) pairs in table order.
"""
function chain_save(ctx::HipContext)
    n = Ref{UInt64}(0)
    checkerr(ctx.ptr, @ccall libhmcmt.hmcmt_chain_save_size(ctx.ptr::Ptr{Cvoid}, n::Ref{UInt64})::Cint)
    blob = Vector{UInt8}(undef, n[])
    written = Ref{UInt64}(0)
    rc = GC.@preserve blob @ccall libhmcmt.hmcmt_chain_save(ctx.ptr::Ptr{Cvoid}, pointer(blob)::Ptr{UInt8}, UInt64(length(blob))::UInt64,
                                                            written::Ref{UInt64})::Cint
    checkerr(ctx.ptr, rc)
    return blob
end

function chain_restore!(ctx::HipContext, blob::Vector{UInt8})
    rc = GC.@preserve blob @ccall libhmcmt.hmcmt_chain_restore(ctx.ptr::Ptr{Cvoid}, pointer(blob)::Ptr{UInt8}, UInt64(length(blob))::UInt64)::Cint
    checkerr(ctx.ptr, rc)
end

function chain_blob_info(blob::Vector{UInt8})
    h = Ref(HmcmtChainBlobHeader(0, 0, 0, 0, 0, 0, 0, 0, 0, ntuple(_ -> UInt32(0), 16), ntuple(_ -> UInt64(0), 16)))
    rc = GC.@preserve blob @ccall libhmcmt.hmcmt_chain_blob_info(pointer(blob)::Ptr{UInt8}, UInt64(length(blob))::UInt64,
                                                                 h::Ref{HmcmtChainBlobHeader})::Cint
    rc == 0 || error("libhmcmt_hip error $rc: not an intact chain blob of version 1")
    v = h[]
    tag(t) = String(UInt8[(t >> s) & 0xff for s in (0, 8, 16, 24)])
    return (version=v.version, total_bytes=v.total_bytes, nAC=v.nAC, nData=v.nData, mass_kind=v.mass_kind, seeded=v.seeded != 0,
            nsamples=v.nsamples, nmoments=v.nmoments, sections=[(tag(v.tags[k]), v.section_bytes[k]) for k in 1:v.nsections])
end

"""
    chain_seed!(ctx, seed, stream=0);  chain_rng_state(ctx) -> (seed, stream, t)
    chain_sample!(ctx, Lmin, Lmax; mOut=nothing, predOut=nothing) -> HmcmtChainRecord
    chain_run!(ctx, nsamples, Lmin, Lmax; keepSamples=true) -> (recs, models[nAC, done], preds[nData, done])

The chain's own random numbers (hmcmt_chain_seed, hmcmt_chain_sample, hmcmt_chain_run, include/hmcmt.h): Philox4x32-10 by counter --
key = seed, counter = (cell or 0xFFFFFFFF, stream, t) -- with the momenta drawn on the GPU and L, u in the library, so that a chain is a
function of (seed, stream) and the problem alone: the same chain as hmcmt2d_amd/sampler.py's runHMCSampler(library_rng=(seed, stream)),
sample by sample.  `chain_seed!` comes behind `chainBegin!` (a begin forgets the seed); (seed, stream, t) is all a checkpoint of the
generator needs.  `chain_run!` is the whole loop in one C call: it stops at the first failing sample, and then throws after cutting
its results to the `done` valid ones.  `run_chain!(...; seed=(s, c))` runs the sampler this way.
"""
chain_seed!(ctx::HipContext, seed::Integer, stream::Integer=0) =
    checkerr(ctx.ptr, @ccall libhmcmt.hmcmt_chain_seed(ctx.ptr::Ptr{Cvoid}, UInt64(seed)::UInt64, UInt32(stream)::UInt32)::Cint)

function chain_rng_state(ctx::HipContext)
    seed = Ref{UInt64}(0); stream = Ref{UInt32}(0); t = Ref{UInt64}(0)
    checkerr(ctx.ptr, @ccall libhmcmt.hmcmt_chain_rng_state(ctx.ptr::Ptr{Cvoid}, seed::Ref{UInt64}, stream::Ref{UInt32}, t::Ref{UInt64})::Cint)
    return seed[], stream[], t[]
end

function chain_sample!(ctx::HipContext, Lmin::Integer, Lmax::Integer; mOut::Union{Nothing,Vector{Float64}}=nothing,
                       predOut::Union{Nothing,Vector{ComplexF64}}=nothing)
    rec = Ref(HmcmtChainRecord(0, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0, 0))
    pm = mOut === nothing ? Ptr{Float64}(C_NULL) : pointer(mOut)
    pp = predOut === nothing ? Ptr{ComplexF64}(C_NULL) : pointer(predOut)
    rc = GC.@preserve mOut predOut @ccall libhmcmt.hmcmt_chain_sample(ctx.ptr::Ptr{Cvoid}, Int32(Lmin)::Int32, Int32(Lmax)::Int32,
                                                                     rec::Ref{HmcmtChainRecord}, pm::Ptr{Float64}, pp::Ptr{ComplexF64})::Cint
    checkerr(ctx.ptr, rc)
    return rec[]
end

function chain_run!(ctx::HipContext, nsamples::Integer, Lmin::Integer, Lmax::Integer; keepSamples::Bool=true)
    recs = Vector{HmcmtChainRecord}(undef, nsamples)
    models = keepSamples ? Matrix{Float64}(undef, ctx.nAC, nsamples) : nothing
    preds = keepSamples ? Matrix{ComplexF64}(undef, ctx.nData, nsamples) : nothing
    pm = keepSamples ? pointer(models) : Ptr{Float64}(C_NULL)
    pp = keepSamples ? pointer(preds) : Ptr{ComplexF64}(C_NULL)
    done = Ref{Int64}(0)
    rc = GC.@preserve recs models preds @ccall libhmcmt.hmcmt_chain_run(ctx.ptr::Ptr{Cvoid}, Int64(nsamples)::Int64, Int32(Lmin)::Int32,
                                                                       Int32(Lmax)::Int32, pointer(recs)::Ptr{HmcmtChainRecord},
                                                                       pm::Ptr{Float64}, pp::Ptr{ComplexF64}, done::Ref{Int64})::Cint
    k = Int(done[])
    resize!(recs, k)
    if keepSamples
        models = models[:, 1:k]; preds = preds[:, 1:k]
    end
    checkerr(ctx.ptr, rc)
    return recs, models, preds
end

"""
    chain_nuts_sample!(ctx, maxDepth; mOut=nothing, predOut=nothing) -> HmcmtNutsRecord
    chain_nuts_run!(ctx, nsamples, maxDepth; keepSamples=true) -> (recs, models[nAC, done], preds[nData, done])

The No-U-turn sampler on a seeded chain (hmcmt_chain_nuts_sample, hmcmt_chain_nuts_run, include/hmcmt.h): every sample chooses its
trajectory length, a tree of at most `maxDepth` (1 .. 10) doublings; the record is the chain record at the selected state plus depth,
nleaves, stop, dirs, selected and alpha.  Diagonal and low-rank mass.  Same conventions as `chain_sample!` / `chain_run!`;
`run_chain!(...; seed=(s, c), nuts=maxDepth)` runs the sampler this way.
"""
function chain_nuts_sample!(ctx::HipContext, maxDepth::Integer; mOut::Union{Nothing,Vector{Float64}}=nothing,
                            predOut::Union{Nothing,Vector{ComplexF64}}=nothing)
    rec = Ref(HmcmtNutsRecord(HmcmtChainRecord(0, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0, 0), 0, 0, 0, 0, 0, 0.0))
    pm = mOut === nothing ? Ptr{Float64}(C_NULL) : pointer(mOut)
    pp = predOut === nothing ? Ptr{ComplexF64}(C_NULL) : pointer(predOut)
    rc = GC.@preserve mOut predOut @ccall libhmcmt.hmcmt_chain_nuts_sample(ctx.ptr::Ptr{Cvoid}, Int32(maxDepth)::Int32,
                                                                          rec::Ref{HmcmtNutsRecord}, pm::Ptr{Float64}, pp::Ptr{ComplexF64})::Cint
    checkerr(ctx.ptr, rc)
    return rec[]
end

function chain_nuts_run!(ctx::HipContext, nsamples::Integer, maxDepth::Integer; keepSamples::Bool=true)
    recs = Vector{HmcmtNutsRecord}(undef, nsamples)
    models = keepSamples ? Matrix{Float64}(undef, ctx.nAC, nsamples) : nothing
    preds = keepSamples ? Matrix{ComplexF64}(undef, ctx.nData, nsamples) : nothing
    pm = keepSamples ? pointer(models) : Ptr{Float64}(C_NULL)
    pp = keepSamples ? pointer(preds) : Ptr{ComplexF64}(C_NULL)
    done = Ref{Int64}(0)
    rc = GC.@preserve recs models preds @ccall libhmcmt.hmcmt_chain_nuts_run(ctx.ptr::Ptr{Cvoid}, Int64(nsamples)::Int64, Int32(maxDepth)::Int32,
                                                                            pointer(recs)::Ptr{HmcmtNutsRecord}, pm::Ptr{Float64},
                                                                            pp::Ptr{ComplexF64}, done::Ref{Int64})::Cint
    k = Int(done[])
    resize!(recs, k)
    if keepSamples
        models = models[:, 1:k]; preds = preds[:, 1:k]
    end
    checkerr(ctx.ptr, rc)
    return recs, models, preds
end

"""
    chainHistBegin!(ctx, targets, nbins, lo, hi);  chainHist(ctx, ntarget, nbins) -> (count, counts[nbins, ntarget])
    chainQuantiles(ctx, q, ntarget) -> values[ntarget, nq];  chainDataMomentsBegin!(ctx);  chainDataMoments(ctx) -> (count, mean, m2)
    chain_hist!(ctx, invParam, hmcprior; targets=all cells, nbins=300) -> (targets, nbins, lo, hi)

Marginal posteriors from the chain's commit (hmcmt_chain_hist_*, hmcmt_chain_data_moments*, include/hmcmt.h): per-cell histograms of
ln sigma over [lo, hi) -- values outside are clamped into the edge bins -- and the Welford moments of the predicted data, both fed by
the commits behind the burn-in from their begin call on.  `targets` are 1-based active-cell indices here (0-based in C).  The arrays
come back in C's row-major layout, i.e. with Julia's first index running over the bins / the targets.  Call the begin functions behind
`chainBegin!` (which ends both accumulators) and in front of the first `chainMomentum!`; `chain_hist!` does so with the reference's
sitePPD settings: 300 bins over the ln of hmcprior.sigBounds.
"""
function chainHistBegin!(ctx::HipContext, targets::Vector{<:Integer}, nbins::Integer, lo::Real, hi::Real)
    t0 = Int64.(targets) .- 1
    rc = @ccall libhmcmt.hmcmt_chain_hist_begin(ctx.ptr::Ptr{Cvoid}, Int64(length(t0))::Int64, t0::Ptr{Int64}, Int32(nbins)::Int32,
                                                Float64(lo)::Float64, Float64(hi)::Float64)::Cint
    checkerr(ctx.ptr, rc)
end

function chainHist(ctx::HipContext, ntarget::Integer, nbins::Integer)
    count = Ref{Int64}(0)
    counts = Matrix{UInt32}(undef, nbins, ntarget)
    rc = @ccall libhmcmt.hmcmt_chain_hist(ctx.ptr::Ptr{Cvoid}, count::Ref{Int64}, counts::Ptr{UInt32}, Int32(0)::Int32)::Cint
    checkerr(ctx.ptr, rc)
    return Int(count[]), counts
end

function chainQuantiles(ctx::HipContext, q::Vector{Float64}, ntarget::Integer)
    out = Matrix{Float64}(undef, ntarget, length(q))
    rc = @ccall libhmcmt.hmcmt_chain_hist_quantiles(ctx.ptr::Ptr{Cvoid}, Int32(length(q))::Int32, q::Ptr{Float64}, out::Ptr{Float64},
                                                    Int32(0)::Int32)::Cint
    checkerr(ctx.ptr, rc)
    return out
end

chainDataMomentsBegin!(ctx::HipContext) = checkerr(ctx.ptr, @ccall libhmcmt.hmcmt_chain_data_moments_begin(ctx.ptr::Ptr{Cvoid})::Cint)

function chainDataMoments(ctx::HipContext)
    count = Ref{Int64}(0)
    mean = Vector{ComplexF64}(undef, ctx.nData); m2 = Vector{ComplexF64}(undef, ctx.nData)
    pmean = Ptr{Float64}(pointer(mean)); pm2 = Ptr{Float64}(pointer(m2))
    rc = GC.@preserve mean m2 @ccall libhmcmt.hmcmt_chain_data_moments(ctx.ptr::Ptr{Cvoid}, count::Ref{Int64}, pmean::Ptr{Float64},
                                                                       pm2::Ptr{Float64}, Int32(0)::Int32)::Cint
    checkerr(ctx.ptr, rc)
    return Int(count[]), (ctx.realData ? real.(mean) : mean), (ctx.realData ? real.(m2) : m2)
end

function chain_hist!(ctx::HipContext, invParam::InvDataModel, hmcprior::HMCPrior; targets::Vector{<:Integer}=collect(1:ctx.nAC),
                     nbins::Integer=300)
    lo = log(hmcprior.sigBounds[1]); hi = log(hmcprior.sigBounds[2])
    chainHistBegin!(ctx, targets, nbins, lo, hi)
    return targets, nbins, lo, hi
end

"""
    chainAcovBegin!(ctx, targets, maxlag);  chainAcov(ctx, ntarget, maxlag) -> (count, mean[ntarget], acov[ntarget, maxlag + 1])
    chainEss(ctx, ntarget) -> (tau, ess, window);  chain_ess!(ctx; targets=all cells, maxlag=63) -> (targets, maxlag)

Effective sample size from the chain's commit (hmcmt_chain_acov_*, hmcmt_chain_ess, include/hmcmt.h): per-cell lagged autocovariances of
ln sigma for the lags 0 .. maxlag (at most 1023), fed by the commits behind the burn-in from the begin call on, and from them the
integrated autocorrelation time `tau`, the effective sample size `ess` and the `window` of Geyer's initial positive sequence, computed
on the GPU (window < 0: the lags ran out, tau is a lower bound).  `targets` are 1-based active-cell indices here (0-based in C); an
empty vector means every active cell.  `acov` comes back in C's lag-major layout, i.e. with Julia's first index running over the
targets.  Call the begin function behind `chainBegin!` (which ends the accumulator) and in front of the first `chainMomentum!`;
`chain_ess!` does so with the defaults of the Python sampler.
"""
function chainAcovBegin!(ctx::HipContext, targets::Vector{<:Integer}, maxlag::Integer)
    t0 = Int64.(targets) .- 1
    ptr = isempty(t0) ? Ptr{Int64}(C_NULL) : pointer(t0)
    rc = GC.@preserve t0 @ccall libhmcmt.hmcmt_chain_acov_begin(ctx.ptr::Ptr{Cvoid}, Int64(length(t0))::Int64, ptr::Ptr{Int64},
                                                                Int32(maxlag)::Int32)::Cint
    checkerr(ctx.ptr, rc)
end

function chainAcov(ctx::HipContext, ntarget::Integer, maxlag::Integer)
    count = Ref{Int64}(0)
    mean = Vector{Float64}(undef, ntarget)
    acov = Matrix{Float64}(undef, ntarget, maxlag + 1)
    rc = @ccall libhmcmt.hmcmt_chain_acov(ctx.ptr::Ptr{Cvoid}, count::Ref{Int64}, mean::Ptr{Float64}, acov::Ptr{Float64},
                                          Int32(0)::Int32)::Cint
    checkerr(ctx.ptr, rc)
    return Int(count[]), mean, acov
end

function chainEss(ctx::HipContext, ntarget::Integer)
    tau = Vector{Float64}(undef, ntarget); ess = Vector{Float64}(undef, ntarget); window = Vector{Int32}(undef, ntarget)
    rc = @ccall libhmcmt.hmcmt_chain_ess(ctx.ptr::Ptr{Cvoid}, tau::Ptr{Float64}, ess::Ptr{Float64}, window::Ptr{Int32},
                                         Int32(0)::Int32)::Cint
    checkerr(ctx.ptr, rc)
    return tau, ess, window
end

function chain_ess!(ctx::HipContext; targets::Vector{<:Integer}=Int[], maxlag::Integer=63)
    chainAcovBegin!(ctx, targets, maxlag)
    return (isempty(targets) ? collect(1:ctx.nAC) : targets), maxlag
end

"""
    chainCovBegin!(ctx, rows, batch);  chainCov(ctx, nrow) -> (count, mean[nAC], var[nAC], cov[nAC, nrow])
    chainCorr(ctx, nrow) -> corr[nAC, nrow];  chain_cov!(ctx; rows=all cells, batch=0) -> (rows, batch)

Posterior covariance and correlation from the chain's commit (hmcmt_chain_cov_*, hmcmt_chain_corr, include/hmcmt.h): the cross moments
of ln sigma between the cells `rows` and every active cell, fed by the commits behind the burn-in from the begin call on and folded in
by a kernel every `batch` commits (1 .. 16; 0: the default, 8; the results do not depend on it).  `rows` are 1-based active-cell
indices here (0-based in C); an empty vector means every active cell, the full matrix.  `cov` and `corr` come back in C's row-major
layout, i.e. with Julia's first index running over the cells: column r is the map of `rows[r]`.  Biased estimator (1/N).  Call the
begin function behind `chainBegin!` (which ends the accumulator) and in front of the first `chainMomentum!`; `chain_cov!` does so
with the defaults of the Python sampler, and `run_chain!(...; cov=(rows=..., batch=...))` does both ends.
"""
function chainCovBegin!(ctx::HipContext, rows::Vector{<:Integer}, batch::Integer)
    r0 = Int64.(rows) .- 1
    ptr = isempty(r0) ? Ptr{Int64}(C_NULL) : pointer(r0)
    rc = GC.@preserve r0 @ccall libhmcmt.hmcmt_chain_cov_begin(ctx.ptr::Ptr{Cvoid}, Int64(length(r0))::Int64, ptr::Ptr{Int64},
                                                               Int32(batch)::Int32)::Cint
    checkerr(ctx.ptr, rc)
end

function chainCov(ctx::HipContext, nrow::Integer)
    count = Ref{Int64}(0)
    mean = Vector{Float64}(undef, ctx.nAC); var = Vector{Float64}(undef, ctx.nAC)
    cov = Matrix{Float64}(undef, ctx.nAC, nrow)
    rc = @ccall libhmcmt.hmcmt_chain_cov(ctx.ptr::Ptr{Cvoid}, count::Ref{Int64}, mean::Ptr{Float64}, var::Ptr{Float64}, cov::Ptr{Float64},
                                         Int32(0)::Int32)::Cint
    checkerr(ctx.ptr, rc)
    return Int(count[]), mean, var, cov
end

function chainCorr(ctx::HipContext, nrow::Integer)
    corr = Matrix{Float64}(undef, ctx.nAC, nrow)
    rc = @ccall libhmcmt.hmcmt_chain_corr(ctx.ptr::Ptr{Cvoid}, corr::Ptr{Float64}, Int32(0)::Int32)::Cint
    checkerr(ctx.ptr, rc)
    return corr
end

function chain_cov!(ctx::HipContext; rows::Vector{<:Integer}=Int[], batch::Integer=0)
    chainCovBegin!(ctx, rows, batch)
    return (isempty(rows) ? collect(1:ctx.nAC) : rows), batch
end

"""
    chain_sketch_begin!(ctx; ell=32, pivot=nothing);  chain_sketch(ctx) -> (info, mean[nAC], var[nAC], rows[nAC, fill])
    chain_pca(ctx, rank) -> (lam[kept], U[nAC, kept], err)

Posterior principal components from the chain's commit by a frequent-directions row sketch (hmcmt_chain_sketch_*, hmcmt_chain_pca,
include/hmcmt.h): 2 ell rows of nAC doubles stand for the counted commits' differences from the pivot (`pivot` = nAC values, or
`nothing`: the first counted model), shrunk to ell rows whenever the buffer is full -- one wait per ell counted commits.  `info` is the
HmcmtSketchInfo (count, ell, fill, shrinks, Delta, pivot_given); `rows` and `U` come back in C's row-major layout, i.e. with Julia's
first index running over the cells: column k is row k.  Every lam[k] lies within err = Delta / count of the k-th eigenvalue of the exact
(biased) covariance of the counted commits.  Call the begin function behind `chainBegin!` (which ends the sketch) and in front of the
first `chainMomentum!`; `run_chain!(...; sketch=(; ell=32, rank=8))` does both ends.
"""
struct HmcmtSketchInfo
    count::Int64
    ell::Int32
    fill::Int32
    shrinks::Int64
    Delta::Float64
    pivot_given::Int32
    reserved_::Int32
end

function chain_sketch_begin!(ctx::HipContext; ell::Integer=32, pivot::Union{Nothing,Vector{Float64}}=nothing)
    pivot === nothing || length(pivot) == ctx.nAC || error("chain_sketch_begin!: pivot needs $(ctx.nAC) entries")
    ptr = pivot === nothing ? Ptr{Float64}(C_NULL) : pointer(pivot)
    rc = GC.@preserve pivot @ccall libhmcmt.hmcmt_chain_sketch_begin(ctx.ptr::Ptr{Cvoid}, Int32(ell)::Int32, ptr::Ptr{Float64})::Cint
    checkerr(ctx.ptr, rc)
    return Int(ell)
end

function chain_sketch_info(ctx::HipContext)
    info = Ref(HmcmtSketchInfo(0, 0, 0, 0, 0.0, 0, 0))
    rc = @ccall libhmcmt.hmcmt_chain_sketch(ctx.ptr::Ptr{Cvoid}, info::Ref{HmcmtSketchInfo}, C_NULL::Ptr{Float64}, C_NULL::Ptr{Float64},
                                            C_NULL::Ptr{Float64}, Int32(0)::Int32)::Cint
    checkerr(ctx.ptr, rc)
    return info[]
end

function chain_sketch(ctx::HipContext)
    fill = Int(chain_sketch_info(ctx).fill)
    info = Ref(HmcmtSketchInfo(0, 0, 0, 0, 0.0, 0, 0))
    mean = Vector{Float64}(undef, ctx.nAC); var = Vector{Float64}(undef, ctx.nAC)
    rows = Matrix{Float64}(undef, ctx.nAC, fill)
    rc = @ccall libhmcmt.hmcmt_chain_sketch(ctx.ptr::Ptr{Cvoid}, info::Ref{HmcmtSketchInfo}, mean::Ptr{Float64}, var::Ptr{Float64},
                                            rows::Ptr{Float64}, Int32(0)::Int32)::Cint
    checkerr(ctx.ptr, rc)
    return info[], mean, var, rows
end

function chain_pca(ctx::HipContext, rank::Integer)
    kept = Ref{Int32}(0); err = Ref{Float64}(0.0)
    lam = Vector{Float64}(undef, rank); U = Matrix{Float64}(undef, ctx.nAC, rank)
    rc = @ccall libhmcmt.hmcmt_chain_pca(ctx.ptr::Ptr{Cvoid}, Int32(rank)::Int32, kept::Ref{Int32}, lam::Ptr{Float64}, U::Ptr{Float64},
                                         err::Ref{Float64}, Int32(0)::Int32)::Cint
    checkerr(ctx.ptr, rc)
    k = Int(kept[])
    return lam[1:k], U[:, 1:k], err[]
end

"""
    chainSetDt!(ctx, dt);  chainSetMassDiag!(ctx, invM);  chainMassDiag(ctx) -> invM[nAC]
    chainAdaptBegin!(ctx, nwarmup; adaptMass=true, initBuffer=75, termBuffer=50, baseWindow=25, delta=0.8, gamma=0.05, t0=10.0,
                     kappa=0.75, dtMin=0.0, dtMax=0.0);  chainAdaptInfo(ctx) -> HmcmtAdaptInfo;  chainAdaptEnd!(ctx)

The chain's step size and diagonal mass between two steps, and their warm-up (hmcmt_chain_set_dt, hmcmt_chain_set_mass_diag,
hmcmt_chain_mass_diag, hmcmt_chain_adapt_*, include/hmcmt.h): dual averaging of dt towards the acceptance `delta` and, with
`adaptMass`, Stan's windowed estimate of the diagonal of M^-1 from the chain's own samples, on the GPU.  `chainSetMassDiag!` drops a
momentum drawn before it: draw a new one before the next step.  Call `chainAdaptBegin!` behind `chainBegin!` (which ends an
adaptation); `run_chain!(...; adapt=(nwarmup=..., ...))` does so with the keywords above.
"""
chainSetDt!(ctx::HipContext, dt::Real) = checkerr(ctx.ptr, @ccall libhmcmt.hmcmt_chain_set_dt(ctx.ptr::Ptr{Cvoid}, Float64(dt)::Float64)::Cint)

function chainSetMassDiag!(ctx::HipContext, invM::Vector{Float64})
    length(invM) == ctx.nAC || error("chainSetMassDiag!: invM must hold nAC = $(ctx.nAC) entries")
    checkerr(ctx.ptr, @ccall libhmcmt.hmcmt_chain_set_mass_diag(ctx.ptr::Ptr{Cvoid}, invM::Ptr{Float64})::Cint)
end

function chainMassDiag(ctx::HipContext)
    invM = Vector{Float64}(undef, ctx.nAC)
    checkerr(ctx.ptr, @ccall libhmcmt.hmcmt_chain_mass_diag(ctx.ptr::Ptr{Cvoid}, invM::Ptr{Float64}, Int32(0)::Int32)::Cint)
    return invM
end

function chainAdaptBegin!(ctx::HipContext, nwarmup::Integer; adaptMass::Bool=true, initBuffer::Integer=75, termBuffer::Integer=50,
                          baseWindow::Integer=25, delta::Real=0.8, gamma::Real=0.05, t0::Real=10.0, kappa::Real=0.75,
                          dtMin::Real=0.0, dtMax::Real=0.0)
    o = Ref(HmcmtAdaptOptions(Int64(nwarmup), Int32(adaptMass), Int32(initBuffer), Int32(termBuffer), Int32(baseWindow),
                              Float64(delta), Float64(gamma), Float64(t0), Float64(kappa), Float64(dtMin), Float64(dtMax)))
    checkerr(ctx.ptr, @ccall libhmcmt.hmcmt_chain_adapt_begin(ctx.ptr::Ptr{Cvoid}, o::Ref{HmcmtAdaptOptions})::Cint)
end

function chainAdaptInfo(ctx::HipContext)
    info = Ref(HmcmtAdaptInfo(0, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0))
    checkerr(ctx.ptr, @ccall libhmcmt.hmcmt_chain_adapt_info(ctx.ptr::Ptr{Cvoid}, info::Ref{HmcmtAdaptInfo})::Cint)
    return info[]
end

chainAdaptEnd!(ctx::HipContext) = checkerr(ctx.ptr, @ccall libhmcmt.hmcmt_chain_adapt_end(ctx.ptr::Ptr{Cvoid})::Cint)

# hmcmt_adapt_lowrank_options and hmcmt_adapt_lowrank_info of include/hmcmt.h, field for field
struct HmcmtAdaptLowrankOptions
    rank::Int32
    max_samples::Int32
    cutoff::Float64
    gamma::Float64
end
struct HmcmtAdaptLowrankInfo
    windows::Int32
    stored::Int32
    skipped::Int32
    dims::Int32
    rank::Int32
    fallback::Int32
    stride::Int64
    theta_min::Float64
    theta_max::Float64
    defect::Float64
    host_ms::Float64
end

"""
    chain_adapt_lowrank!(ctx; rank=8, maxSamples=64, cutoff=2.0, gamma=1e-5)
    chain_adapt_lowrank_info(ctx) -> HmcmtAdaptLowrankInfo
    chain_set_mass_lowrank!(ctx, invM, U, lam)          # U nAC × r; r = 0 with invM: back to the diagonal
    chain_mass_lowrank(ctx) -> (invM, U, lam)           # U nAC × r, r = 0 under the diagonal mass

The low-rank mass of a live chain (hmcmt_chain_adapt_lowrank, hmcmt_chain_set_mass_lowrank, hmcmt_chain_mass_lowrank, include/hmcmt.h):
`chain_adapt_lowrank!` right behind `chainAdaptBegin!(...; adaptMass=true)` makes every window end estimate the directions and
factors from the window's draws and gradients; `run_chain!(...; adapt=(nwarmup=..., lowrank=(rank=4,)))` does so.
"""
function chain_adapt_lowrank!(ctx::HipContext; rank::Integer=8, maxSamples::Integer=64, cutoff::Real=2.0, gamma::Real=1e-5)
    o = Ref(HmcmtAdaptLowrankOptions(Int32(rank), Int32(maxSamples), Float64(cutoff), Float64(gamma)))
    checkerr(ctx.ptr, @ccall libhmcmt.hmcmt_chain_adapt_lowrank(ctx.ptr::Ptr{Cvoid}, o::Ref{HmcmtAdaptLowrankOptions})::Cint)
end

function chain_adapt_lowrank_info(ctx::HipContext)
    info = Ref(HmcmtAdaptLowrankInfo(0, 0, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0))
    checkerr(ctx.ptr, @ccall libhmcmt.hmcmt_chain_adapt_lowrank_info(ctx.ptr::Ptr{Cvoid}, info::Ref{HmcmtAdaptLowrankInfo})::Cint)
    return info[]
end

function chain_set_mass_lowrank!(ctx::HipContext, invM::Union{Nothing,Vector{Float64}}, U::Matrix{Float64}, lam::Vector{Float64})
    size(U, 2) == 0 || size(U, 1) == ctx.nAC || error("chain_set_mass_lowrank!: U must be nAC = $(ctx.nAC) × r")
    length(lam) == size(U, 2) || error("chain_set_mass_lowrank!: lam must hold one entry per column of U")
    invM === nothing || length(invM) == ctx.nAC || error("chain_set_mass_lowrank!: invM must hold nAC = $(ctx.nAC) entries")
    checkerr(ctx.ptr, @ccall libhmcmt.hmcmt_chain_set_mass_lowrank(ctx.ptr::Ptr{Cvoid}, (invM === nothing ? C_NULL : invM)::Ptr{Float64},
                                                                 Int32(size(U, 2))::Int32, U::Ptr{Float64}, lam::Ptr{Float64})::Cint)
end

function chain_mass_lowrank(ctx::HipContext)
    rank = Ref{Int32}(0)
    invM = Vector{Float64}(undef, ctx.nAC); U = Matrix{Float64}(undef, ctx.nAC, HMCMT_MASS_RANK_MAX); lam = Vector{Float64}(undef, HMCMT_MASS_RANK_MAX)
    checkerr(ctx.ptr, @ccall libhmcmt.hmcmt_chain_mass_lowrank(ctx.ptr::Ptr{Cvoid}, rank::Ref{Int32}, invM::Ptr{Float64}, U::Ptr{Float64},
                                                             lam::Ptr{Float64}, Int32(0)::Int32)::Cint)
    r = Int(rank[])
    return invM, U[:, 1:r], lam[1:r]
end

"""
    run_chain!(ctx, invParam, hmcprior, hmcParam; keepSamples=true, rhoref=nothing, seed=nothing, nuts=nothing, cov=nothing, sketch=nothing, adapt=nothing) -> (hmcmodel, hmcstats, hmcdata, moments[, cov][, sketch][, adapt][, nuts])

runHMCSampler (HMCSampler.jl:72-196) through the chain API, step for step what hmcmt2d_amd/sampler.py's device chain does, the
reference's start included: the chain's state starts at the file's model invParam.strModel (:88), while start and reference model
become the homogeneous one of `rhoref` Ωm (drawn as :100-104 draws it when `nothing`) and the first Hamiltonian is taken there
(:112-115) -- one `chainBegin!` at the homogeneous model for D, M and the first data column, one at the file's model, and
`chainSetEnergy!` with the first one's D and M.  The mass is hmcParam's (`setPrior!`).  Draw order: the first momentum's normals,
rhoref; per sample L, u, the next momentum's normals.  `keepSamples=false`: no sample leaves the GPU (hmcmodel has no column,
hmcdata its first only); `moments` = (count, mean, m2) of the samples behind hmcprior.burninsamples either way.
`cov=(rows=Int[], batch=0)` (both optional; see `chainCovBegin!`) streams the posterior covariance beside the moments and appends a fifth
result, the named tuple (count, rows, mean, var, cov, corr) -- `nothing` for the arrays of a chain that ends inside its burn-in.
`sketch=(; ell=32, rank=8)` (both optional, and `pivot`; see `chain_sketch_begin!`) streams the row sketch beside the moments and appends
the named tuple (info, mean, var, rows, lam, U, err) -- `nothing` for the arrays of a chain that counted fewer than two samples.
`adapt=(nwarmup=hmcprior.burninsamples, ...)` (the keywords of `chainAdaptBegin!`, all optional) warms the chain up over its first
`nwarmup <= hmcprior.burninsamples` samples and appends a last result, the named tuple (nwarmup, dt, alpha, dtFinal, invM): the step
size each sample's trajectory used, each sample's acceptance probability, the adapted step size and the diagonal of M^-1 in force
at the end.  hmcprior.dt is the start and is not modified.
`seed=(s, c)`: the chain draws its own numbers in the library (`chain_seed!(ctx, s, c)`) and runs through `chain_run!` -- single
samples with `adapt`, whose trace watches every step.  Julia's generator then draws `rhoref` alone, and the chain is sample by sample
the one runHMCSampler(device_chain=True, library_rng=(s, c)) gives for the same rhoref.  Column it + 1 of hmstats takes its K from
sample it + 1's record; the last column's K is NaN (that momentum is never drawn).
`nuts=maxDepth` (with `seed`): the samples are NUTS samples (`chain_nuts_run!`, `chain_nuts_sample!`), hmcprior.timestep is not
used, the warm-up's alpha is the tree's, and a last result is appended: the vector of the samples' HmcmtNutsRecord.
"""
function run_chain!(ctx::HipContext, invParam::InvDataModel, hmcprior::HMCPrior, hmcParam::HMCParameter; keepSamples::Bool=true,
                    rhoref::Union{Nothing,Real}=nothing, seed::Union{Nothing,Tuple{<:Integer,<:Integer}}=nothing,
                    nuts::Union{Nothing,Integer}=nothing, cov::Union{Nothing,NamedTuple}=nothing, sketch::Union{Nothing,NamedTuple}=nothing,
                    adapt::Union{Nothing,NamedTuple}=nothing)
    (nuts === nothing || seed !== nothing) || error("run_chain!: nuts needs seed=(s, c): the tree's draws are the library's")
    n, nd = ctx.nAC, ctx.nData
    nsamples = hmcprior.totalsamples
    fileModel = Vector{Float64}(invParam.strModel)
    z = randn(n)
    rho0 = 1.0 / exp(invParam.strModel[1])
    if rhoref === nothing
        rhoref = round(rho0 * 0.5 + (rho0 * 1.5 - rho0 * 0.5) * rand())
    end
    println("Homogeneous starting model with a resistivity of $(rhoref) Ωm is used.")
    strModel = log.(ones(n) ./ rhoref)
    invParam.strModel = copy(strModel)
    invParam.refModel = copy(strModel)
    setPrior!(ctx, invParam, hmcParam)
    lo, hi = log(hmcprior.sigBounds[1]), log(hmcprior.sigBounds[2])
    D, M = chainBegin!(ctx, strModel, hmcprior.dt, hmcprior.regParam, lo, hi; burnin=hmcprior.burninsamples)
    predStart = chainState(ctx)[3]
    if fileModel != strModel
        chainBegin!(ctx, fileModel, hmcprior.dt, hmcprior.regParam, lo, hi; burnin=hmcprior.burninsamples)
        chainSetEnergy!(ctx, D, M)
    end
    covRows = cov === nothing ? Int[] : first(chain_cov!(ctx; rows=Vector{Int}(get(cov, :rows, Int[])), batch=get(cov, :batch, 0)))
    sketch === nothing || chain_sketch_begin!(ctx; ell=get(sketch, :ell, 32), pivot=get(sketch, :pivot, nothing))
    if adapt !== nothing
        nwarmup = get(adapt, :nwarmup, hmcprior.burninsamples)
        nwarmup <= hmcprior.burninsamples || error("run_chain!: adapt nwarmup = $(nwarmup) exceeds hmcprior.burninsamples: the moments would mix in warm-up samples")
        chainAdaptBegin!(ctx, nwarmup; Base.structdiff(adapt, NamedTuple{(:nwarmup, :lowrank)})...)
        lowrank = get(adapt, :lowrank, nothing)
        lowrank === nothing || lowrank === false || chain_adapt_lowrank!(ctx; (lowrank === true ? (;) : lowrank)...)
        adaptDt = fill(NaN, nsamples); adaptAlpha = zeros(nsamples)
    end
    ncols = keepSamples ? nsamples : 0
    hmcmodel = zeros(Float64, n, ncols)
    hmcdata = zeros(ComplexF64, nd, ncols + 1)
    hmcdata[:, 1] = predStart
    hmcstats = initHMCStatus(nsamples)
    if seed === nothing
        K = chainMomentum!(ctx, z)
        hmcstats.hmstats[:, 1] = [D, M, K, D + M + K]
    else
        chain_seed!(ctx, seed[1], seed[2])                   # (behind the begins: a begin forgets the seed; z is not used)
    end
    mOut = keepSamples ? Vector{Float64}(undef, n) : nothing
    predOut = keepSamples ? Vector{ComplexF64}(undef, nd) : nothing
    Lmin, Lmax = hmcprior.timestep[1], hmcprior.timestep[2]
    # the library's numbers: the whole run in one call, or sample by sample where the warm-up's trace watches every step
    seededRecs = (seed === nothing || adapt !== nothing) ? nothing :
                 (nuts === nothing ? chain_run!(ctx, nsamples, Lmin, Lmax; keepSamples=keepSamples) :
                                     chain_nuts_run!(ctx, nsamples, nuts; keepSamples=keepSamples))
    nutsRecs = HmcmtNutsRecord[]
    for it = 1:nsamples
        adapt === nothing || (adaptDt[it] = chainAdaptInfo(ctx).dt)
        if seed === nothing
            L = rand(Lmin:Lmax)
            u = rand()
            rec = chainStep!(ctx, L, u; mOut=mOut, predOut=predOut)
        elseif seededRecs === nothing
            rec = nuts === nothing ? chain_sample!(ctx, Lmin, Lmax; mOut=mOut, predOut=predOut) :
                                     chain_nuts_sample!(ctx, nuts; mOut=mOut, predOut=predOut)
        else
            rec = seededRecs[1][it]
            if keepSamples
                mOut = seededRecs[2][:, it]; predOut = seededRecs[3][:, it]
            end
        end
        if nuts !== nothing                                  # (the tree's record wraps the chain record: unwrapped before any field is read)
            push!(nutsRecs, rec)
            alphaOf = rec.alpha
            rec = rec.rec
        else
            alphaOf = rec.hdif > 0 ? 1.0 : exp(rec.hdif)
        end
        adapt === nothing || (adaptAlpha[it] = alphaOf)
        hmcprior.nfevals += rec.nfevals
        if rec.accepted == 1
            hmcstats.nAccept += 1
            hmcstats.acceptstats[it] = true
        else
            hmcstats.nReject += 1
        end
        if seed === nothing
            K = chainMomentum!(ctx, randn(n))
            hmcstats.hmstats[:, it + 1] = [rec.D, rec.M, K, rec.D + rec.M + K]
        else
            hmcstats.hmstats[3:4, it] = [rec.K0, hmcstats.hmstats[1, it] + hmcstats.hmstats[2, it] + rec.K0]
            hmcstats.hmstats[:, it + 1] = [rec.D, rec.M, NaN, NaN]
            it == 1 && (hmcstats.hmstats[:, 1] = [D, M, rec.K0, D + M + rec.K0])
        end
        if keepSamples
            hmcmodel[:, it] = mOut
            hmcdata[:, it + 1] = rec.accepted == 1 ? predOut : hmcdata[:, it]      # (:164-168: a rejection repeats the column)
        end
    end
    adaptStats = adapt === nothing ? () : ((nwarmup=nwarmup, dt=adaptDt, alpha=adaptAlpha, dtFinal=chainAdaptInfo(ctx).dt, invM=chainMassDiag(ctx)),)
    nutsStats = nuts === nothing ? () : (nutsRecs,)
    sketchStats = ()
    if sketch !== nothing
        if nsamples > hmcprior.burninsamples + 1
            sinfo, smean, svar, srows = chain_sketch(ctx)
            slam, sU, serr = chain_pca(ctx, get(sketch, :rank, 8))
            sketchStats = ((info=sinfo, mean=smean, var=svar, rows=srows, lam=slam, U=sU, err=serr),)
        else
            sketchStats = ((info=chain_sketch_info(ctx), mean=nothing, var=nothing, rows=nothing, lam=nothing, U=nothing, err=nothing),)
        end
    end
    cov === nothing && return (hmcmodel, hmcstats, hmcdata, chainMoments(ctx), sketchStats..., adaptStats..., nutsStats...)
    if nsamples > hmcprior.burninsamples
        count, cmean, cvar, cmat = chainCov(ctx, length(covRows))
        covStats = (count=count, rows=covRows, mean=cmean, var=cvar, cov=cmat, corr=chainCorr(ctx, length(covRows)))
    else
        covStats = (count=0, rows=covRows, mean=nothing, var=nothing, cov=nothing, corr=nothing)
    end
    return (hmcmodel, hmcstats, hmcdata, chainMoments(ctx), covStats, sketchStats..., adaptStats..., nutsStats...)
end

hipWait(ctx::HipContext) = checkerr(ctx.ptr, ccall((:hmcmt_wait, libhmcmt), Cint, (Ptr{Cvoid},), ctx.ptr))

"""
    commId() -> Vector{UInt8}(128);  SampleComm(device, nranks, rank, id);  allgatherSamples(comm, block) -> Matrix

The RCCL all-gather of the chains' sample blocks (hmcmt_comm_id / hmcmt_comm_create / hmcmt_allgather_samples): what
replaces `remotecall_fetch` of every worker's samples in parallelHMCSampler (parallelHMC.jl:23-45) when each worker
process owns a GPU.  The master obtains the id once and ships it to the workers (e.g. `remotecall_fetch(() -> commId(), 2)`
on rank 0, then as an argument of the workers' calls); every worker then holds every chain's block.
"""
commId() = (id = Vector{UInt8}(undef, 128);
            checkerr(C_NULL, ccall((:hmcmt_comm_id, libhmcmt), Cint, (Ptr{UInt8},), id)); id)

mutable struct SampleComm
    ptr::Ptr{Cvoid}
    nranks::Int
    function SampleComm(device::Integer, nranks::Integer, rank::Integer, id::Vector{UInt8})
        ref = Ref{Ptr{Cvoid}}(C_NULL)
        rc = ccall((:hmcmt_comm_create, libhmcmt), Cint, (Ref{Ptr{Cvoid}}, Int32, Int32, Int32, Ptr{UInt8}),
                   ref, Int32(device), Int32(nranks), Int32(rank), id)
        rc == 0 || error("libhmcmt_hip error $rc: " *
                         unsafe_string(ccall((:hmcmt_comm_last_error, libhmcmt), Cstring, (Ptr{Cvoid},), C_NULL)))
        c = new(ref[], Int(nranks))
        finalizer(x -> (x.ptr != C_NULL && ccall((:hmcmt_comm_destroy, libhmcmt), Cint, (Ptr{Cvoid},), x.ptr); x.ptr = C_NULL), c)
        return c
    end
end

function allgatherSamples(comm::SampleComm, block::Vector{Float64})
    recv = Matrix{Float64}(undef, length(block), comm.nranks)          # column r+1 = rank r's block
    rc = ccall((:hmcmt_allgather_samples, libhmcmt), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Int32),
               comm.ptr, block, recv, length(block), Int32(0))
    rc == 0 || error("libhmcmt_hip error $rc: " *
                     unsafe_string(ccall((:hmcmt_comm_last_error, libhmcmt), Cstring, (Ptr{Cvoid},), comm.ptr)))
    return recv
end

"""
    hipStats(ctx) -> HmcmtStats   (iteration counts, error estimate, fallback counter of the last call)
"""
function hipStats(ctx::HipContext)
    st = Ref{HmcmtStats}()
    rc = ccall((:hmcmt_get_stats, libhmcmt), Cint, (Ptr{Cvoid}, Ref{HmcmtStats}), ctx.ptr, st)
    checkerr(ctx.ptr, rc)
    return st[]
end

"""
    hipGuard(ctx) -> (checks, worst, last, trips)

The production guard of the iterative solves (`hmcmt_guard`, DESIGN 4.3): true residuals of both solves, formed every
`HMCMT_GUARD_EVERY`-th evaluation; `trips` counts the checks above `HMCMT_GUARD_LIMIT`.  A sampler loop reads it once per
output interval next to `hmcstats` and stops the chain on a trip.
"""
function hipGuard(ctx::HipContext)
    out = zeros(Float64, 4)
    rc = ccall((:hmcmt_guard, libhmcmt), Cint, (Ptr{Cvoid}, Ptr{Float64}), ctx.ptr, out)
    checkerr(ctx.ptr, rc)
    return (checks = Int(out[1]), worst = out[2], last = out[3], trips = Int(out[4]))
end

"""
    hipPersistInfo(ctx) -> NamedTuple

Shape and use of the one-launch-per-solve kernel (`hmcmt_persist_info`, include/hmcmt.h; DESIGN 5.0): `threads_half == 0` --
the mesh is outside its envelope; `usable_now == 0` -- this context is not alone on its share of the device (all solves then run
the launch-per-phase loop: same results, slower); `timeouts` / `placement_fallbacks` > 0 -- the device is shared with something
this library cannot see.
"""
function hipPersistInfo(ctx::HipContext)
    out = zeros(Int64, 14)
    rc = ccall((:hmcmt_persist_info, libhmcmt), Cint, (Ptr{Cvoid}, Ptr{Int64}, Int32), ctx.ptr, out, Int32(length(out)))
    checkerr(ctx.ptr, rc)
    return (threads_half = out[1], workgroups_per_system = out[2], slots_per_xcd = out[3], enabled = out[4], solves = out[5],
            placement_fallbacks = out[6], usable_now = out[7], slab_modes = out[8], column_parts = out[9], timeouts = out[10],
            cu_share_index = out[11], cu_share_count = out[12], strips = out[13], why_off = out[14])
end

"""
    hipPersistWidth(ctx) -> Int

Row width (padded nodes: 112 / 208 / 416) of the width-specialised persistent kernel the context launches (`hmcmt_persist_width`);
0: the generic kernel.
"""
function hipPersistWidth(ctx::HipContext)
    w = Ref{Int32}(0)
    rc = ccall((:hmcmt_persist_width, libhmcmt), Cint, (Ptr{Cvoid}, Ptr{Int32}), ctx.ptr, w)
    rc == 0 || error("hmcmt_persist_width failed")
    return Int(w[])
end

"""
    hipPersistOrder(ctx, kind = 0) -> (order, rebalanced)

The order (0-based system indices; position queue + queues * round) in which the persistent kernel's queues take the systems of a
forward (`kind = 0`) or adjoint (`1`) solve, and how often the context has re-balanced it from the iteration counts of the
previous solve (`hmcmt_persist_order`; meshes whose systems take turns on the chip).
"""
function hipPersistOrder(ctx::HipContext, kind::Integer = 0)
    dims = zeros(Int32, 7)
    ccall((:hmcmt_dims, libhmcmt), Cint, (Ptr{Cvoid}, Ptr{Int32}), ctx.ptr, dims) == 0 || error("hmcmt_dims failed")
    order = zeros(Int32, dims[3])          # (systems = 2 x frequencies)
    n = Ref{Int64}(0)
    rc = ccall((:hmcmt_persist_order, libhmcmt), Cint, (Ptr{Cvoid}, Int32, Ptr{Int32}, Ptr{Int64}), ctx.ptr, Int32(kind), order, n)
    rc == 0 || error("hmcmt_persist_order failed")
    return order, Int(n[])
end

"""
    hipPersistPack(cost, queues) -> (order, makespan)

The packing behind `hipPersistOrder` on the caller's costs (`hmcmt_persist_pack`; no device needed): systems onto `queues`
queues that take turns, longest first into the least loaded queue that has room; `order` holds 0-based system indices by
position queue + queues * round, `makespan` the largest queue sum.
"""
function hipPersistPack(cost::AbstractVector{<:Real}, queues::Integer)
    c = Vector{Float64}(cost)
    order = zeros(Int32, length(c))
    m = Ref{Float64}(0.0)
    rc = ccall((:hmcmt_persist_pack, libhmcmt), Cint, (Ptr{Float64}, Int32, Int32, Ptr{Int32}, Ptr{Float64}), c, Int32(length(c)), Int32(queues), order, m)
    rc == 0 || error("hmcmt_persist_pack failed")
    return order, m[]
end

"""
    hipPersistEnvelope(ny, nz; cus_per_xcd = 32, nsystems = 32) -> NamedTuple

Would a mesh of ny x nz cells (nz including the air layers) run the one-launch-per-solve kernel, and in which shape
(`hmcmt_persist_envelope`; pure arithmetic, no device needed)?  `column_parts == 0`: outside its envelope.
"""
function hipPersistEnvelope(ny::Integer, nz::Integer; cus_per_xcd::Integer = 32, nsystems::Integer = 32)
    out = zeros(Int64, 6)
    rc = ccall((:hmcmt_persist_envelope, libhmcmt), Cint, (Int64, Int64, Int32, Int64, Ptr{Int64}), ny, nz, Int32(cus_per_xcd), nsystems, out)
    rc == 0 || error("hmcmt_persist_envelope: invalid sizes")
    return (column_parts = out[1], threads_half = out[2], workgroups_per_system = out[3], slab_modes = out[4], lds_bytes = out[5], slots_per_xcd = out[6])
end

# hmcmt_map_options and hmcmt_map_record of include/hmcmt.h: the options of a MAP run and what hmcmt_map_begin / hmcmt_map_step report
# of the state they return (tests/test_map_host.py compares the fields with the ctypes mirrors)
struct HmcmtMapOptions
    history::Int32
    max_backtracks::Int32
    c1::Float64
    shrink::Float64
    curv_eps::Float64
    gtol::Float64
end

struct HmcmtMapRecord
    iter::Int32
    status::Int32
    nfevals::Int32
    backtracks::Int32
    resets::Int32
    npairs::Int32
    pair_stored::Int32
    nbound::Int32
    alpha::Float64
    gamma::Float64
    phi::Float64
    D::Float64
    M::Float64
    pg_inf::Float64
    pg_2::Float64
    gTd::Float64
    sTy::Float64
    phi_trial::NTuple{16,Float64}
end
const MAP_RUNNING = Int32(0); const MAP_CONVERGED = Int32(1); const MAP_STALLED = Int32(2)
blankMapRecord() = HmcmtMapRecord(0, 0, 0, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, ntuple(_ -> NaN, 16))

"""
    map_options(; history=8, max_backtracks=10, c1=1e-4, shrink=0.5, curv_eps=1e-10, gtol=1e-5) -> HmcmtMapOptions
    map_begin!(ctx, mStart, regParam, lnSigMin, lnSigMax; options...) -> HmcmtMapRecord
    map_step!(ctx) -> HmcmtMapRecord;  map_run!(ctx, maxiter) -> Vector{HmcmtMapRecord}
    map_state(ctx) -> (m, grad, pred);  map_end!(ctx)
    find_map(ctx, invParam, hmcprior; m0=nothing, maxiter=50, options...) -> (model, records)

The MAP model on the device (hmcmt_map_*, include/hmcmt.h): projected L-BFGS over the library's gradient of D + M, model, gradient and
history in GPU memory, one wait per trial evaluation.  Call `setPrior!` first.  A run ends CONVERGED, STALLED (no step lowers the
objective: the reference's gradient is not everywhere the derivative of its misfit) or at `maxiter`.  `find_map` starts from
`invParam.strModel`, takes regParam and the bounds from `hmcprior`, and returns the model with the records; to start a chain there,
write the model into `invParam.strModel`, from which `runHMCSampler` runs its first trajectory.
"""
function map_options(; kw...)
    o = Ref(HmcmtMapOptions(0, 0, 0.0, 0.0, 0.0, 0.0))
    @ccall libhmcmt.hmcmt_map_default_options(o::Ref{HmcmtMapOptions})::Cvoid
    d = o[]
    get_(k, v) = haskey(kw, k) ? kw[k] : v
    return HmcmtMapOptions(Int32(get_(:history, d.history)), Int32(get_(:max_backtracks, d.max_backtracks)), Float64(get_(:c1, d.c1)),
                           Float64(get_(:shrink, d.shrink)), Float64(get_(:curv_eps, d.curv_eps)), Float64(get_(:gtol, d.gtol)))
end

function map_begin!(ctx::HipContext, mStart::Vector{Float64}, regParam::Real, lnSigMin::Real, lnSigMax::Real; kw...)
    o = Ref(map_options(; kw...))
    rec = Ref(blankMapRecord())
    rc = GC.@preserve mStart @ccall libhmcmt.hmcmt_map_begin(ctx.ptr::Ptr{Cvoid}, pointer(mStart)::Ptr{Float64}, Float64(regParam)::Float64,
                                                            Float64(lnSigMin)::Float64, Float64(lnSigMax)::Float64,
                                                            o::Ref{HmcmtMapOptions}, rec::Ref{HmcmtMapRecord})::Cint
    checkerr(ctx.ptr, rc)
    return rec[]
end

function map_step!(ctx::HipContext)
    rec = Ref(blankMapRecord())
    checkerr(ctx.ptr, @ccall libhmcmt.hmcmt_map_step(ctx.ptr::Ptr{Cvoid}, rec::Ref{HmcmtMapRecord})::Cint)
    return rec[]
end

function map_run!(ctx::HipContext, maxiter::Integer)
    recs = Vector{HmcmtMapRecord}(undef, max(maxiter, 1))
    done = Ref{Int32}(0)
    rc = GC.@preserve recs @ccall libhmcmt.hmcmt_map_run(ctx.ptr::Ptr{Cvoid}, Int32(maxiter)::Int32, pointer(recs)::Ptr{HmcmtMapRecord},
                                                        done::Ref{Int32})::Cint
    resize!(recs, Int(done[]))
    checkerr(ctx.ptr, rc)
    return recs
end

function map_state(ctx::HipContext)
    m = Vector{Float64}(undef, ctx.nAC); g = Vector{Float64}(undef, ctx.nAC)
    pred = Vector{ComplexF64}(undef, ctx.nData)
    rc = GC.@preserve m g pred @ccall libhmcmt.hmcmt_map_state(ctx.ptr::Ptr{Cvoid}, pointer(m)::Ptr{Float64}, pointer(g)::Ptr{Float64},
                                                              pointer(pred)::Ptr{ComplexF64}, Int32(0)::Int32)::Cint
    checkerr(ctx.ptr, rc)
    return m, g, pred
end

map_end!(ctx::HipContext) = checkerr(ctx.ptr, @ccall libhmcmt.hmcmt_map_end(ctx.ptr::Ptr{Cvoid})::Cint)

function find_map(ctx::HipContext, invParam, hmcprior; m0::Union{Nothing,Vector{Float64}}=nothing, maxiter::Integer=50, kw...)
    mStart = m0 === nothing ? Vector{Float64}(invParam.strModel) : m0
    rec0 = map_begin!(ctx, mStart, hmcprior.regParam, log(hmcprior.sigBounds[1]), log(hmcprior.sigBounds[2]); kw...)
    recs = vcat([rec0], rec0.status == MAP_RUNNING ? map_run!(ctx, maxiter) : HmcmtMapRecord[])
    m, _, _ = map_state(ctx)
    map_end!(ctx)
    return m, recs
end

"""
    hipNextCuShare(index, count)

The calling task's NEXT `HipContext(...)` is confined to share `index` (0-based) of `count` = 1, 2 or 4 equal shares of the CUs of
every XCD (`hmcmt_next_cu_share`): what `parallelHMCSampler` calls before it builds the contexts of `count` chains that are to
run concurrently on one GPU (parallelHMC.jl:23-45 with more chains than devices).  Julia tasks may migrate between threads:
call it and the constructor without a yield in between (or pin the task).
"""
function hipNextCuShare(index::Integer, count::Integer)
    rc = ccall((:hmcmt_next_cu_share, libhmcmt), Cint, (Int32, Int32), Int32(index), Int32(count))
    rc == 0 || error("hmcmt_next_cu_share($index, $count): (index, count) with count 1, 2 or 4")
    return nothing
end

end # module
