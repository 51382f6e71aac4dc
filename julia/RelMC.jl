# RelMC.jl — Julia host layer over the C ABI of include/relmc.h (north-star: "host code in Julia
# calling HIP through a thin C-ABI/ccall layer").  Keeps the reference's call surface:
#   mc_sampling(U, n, Ng, Nl)                     (Montecarlo_nsq_single/mc_sampling.m:2)
#   mc_simulation(state, TestSystem, mpopt, Ng, Nl) (mc_simulation.m:1)
#   nsqMain(; ...)                                (nsqMain.m:208-406)
# NOTE: Julia is not installed in the build image nor on the GPU box, so this file is NOT executed
# by the repository's tests; the Python mirror (powersystemsreliabilityassessment_amd/api.py) is.
module RelMC

const LIB = joinpath(@__DIR__, "..", "powersystemsreliabilityassessment_amd", "csrc", "librelmc.so")
const MAX_BUS = 128
const MAX_COMP = 256

struct CaseDesc
    base_mva::Cdouble
    nb::Int32; ng::Int32; nl::Int32; nd::Int32; ref_bus::Int32
    bus_pd::Ptr{Cdouble}
    inj_bus::Ptr{Int32}
    inj_pmin::Ptr{Cdouble}; inj_pmax::Ptr{Cdouble}; inj_cost::Ptr{Cdouble}
    br_from::Ptr{Int32}; br_to::Ptr{Int32}
    br_b::Ptr{Cdouble}; br_rate::Ptr{Cdouble}
    unavail::Ptr{Cdouble}
    always_up::Ptr{UInt8}
    total_load::Cdouble
end

mutable struct SolverOpts
    singular_policy::Int32; max_it::Int32
    feastol::Cdouble; gradtol::Cdouble; comptol::Cdouble; costtol::Cdouble
    xi::Cdouble; sigma::Cdouble; z0::Cdouble; alpha_min::Cdouble; max_stepsize::Cdouble
    screen::Int32; reserved::Int32            # screen = 1: zero-curtailment pre-screen (relmc.h), relmc_acc.n_screened counts the skipped units
    SolverOpts() = new()
end

mutable struct Acc
    n::Int64; n_fail::Int64; n_singular::Int64; n_infeasible::Int64; n_nonconverged::Int64; sum_iters::Int64
    comp_fail::NTuple{MAX_COMP,Int64}
    n_screened::Int64
    sum_dns::Cdouble; sum_dns2::Cdouble
    sum_nodal::NTuple{MAX_BUS,Cdouble}
    Acc() = new()
end

mutable struct Indices
    n::Int64
    edns::Cdouble; lole::Cdouble; plc::Cdouble; beta::Cdouble; eens::Cdouble; mean_iters::Cdouble
    nodal_eens::NTuple{MAX_BUS,Cdouble}
    comp_importance::NTuple{MAX_COMP,Cdouble}
    Indices() = new()
end

"isbits image of relmc_solver_opts, for embedding in NsqOpts"
struct SolverOptsC
    singular_policy::Int32; max_it::Int32
    feastol::Cdouble; gradtol::Cdouble; comptol::Cdouble; costtol::Cdouble
    xi::Cdouble; sigma::Cdouble; z0::Cdouble; alpha_min::Cdouble; max_stepsize::Cdouble
    screen::Int32; reserved::Int32
end
SolverOptsC(o::SolverOpts) = SolverOptsC(o.singular_policy, o.max_it, o.feastol, o.gradtol, o.comptol, o.costtol, o.xi, o.sigma, o.z0,
                                         o.alpha_min, o.max_stepsize, o.screen, o.reserved)

"relmc_nsq_opts (include/relmc.h): the options of the whole nsqMain loop"
struct NsqOpts
    beta_limit::Cdouble; max_samples::Int64; batch::Int64; seed::UInt64; hours_per_year::Cdouble
    solver::SolverOptsC
    history_cap::Int64
    beta_history::Ptr{Cdouble}; edns_history::Ptr{Cdouble}; lole_history::Ptr{Cdouble}; plc_history::Ptr{Cdouble}
    distinct_states::Int32
end

# relmc_nsq_result is read out of a byte buffer at these offsets (Acc and Indices are mutable mirrors and cannot be embedded)
const NSQ_RESULT_BYTES = 8 * (7 + MAX_COMP + 2 + MAX_BUS) + 8 * (7 + MAX_BUS + MAX_COMP) + 40
const NSQ_RESULT_IDX = 8 * (7 + MAX_COMP + 2 + MAX_BUS)
const NSQ_RESULT_TAIL = NSQ_RESULT_IDX + 8 * (7 + MAX_BUS + MAX_COMP)     # checkpoints, converged, wall_seconds, kernel_seconds, batches

"TestSystem after the load model of nsqMain.m:121-153 (0-based indices inside)."
struct TestSystem
    base_mva::Float64; nb::Int; ng::Int; nl::Int; nd::Int; ref_bus::Int
    bus_pd::Vector{Float64}
    inj_bus::Vector{Int32}; inj_pmin::Vector{Float64}; inj_pmax::Vector{Float64}; inj_cost::Vector{Float64}
    br_from::Vector{Int32}; br_to::Vector{Int32}; br_b::Vector{Float64}; br_rate::Vector{Float64}
    unavail::Vector{Float64}; always_up::Vector{UInt8}
    load::Float64                     # TestSystem.load, nsqMain.m:125
end

mutable struct Engine
    h::Ptr{Cvoid}
    sys::TestSystem
end

check(rc, h, what) = rc == 0 || error("$what failed ($rc): " * unsafe_string(ccall((:relmc_last_error, LIB), Cstring, (Ptr{Cvoid},), h)))

# The primary elimination orders this package ships for the two IEEE test systems (0-based bus numbers, reference bus last; tuned offline with
# relmc_tune_order, identical to case24.RTS24_ELIM_ORDER / case96.RTS96_ELIM_ORDER of the Python host, so that every host runs the same pass
# program -- an order changes the rounding of the factorisation: iteration counts of single states may move by one, DESIGN.md 3.2).
# Pass them as `Engine(sys; elim_order=RTS24_ELIM_ORDER)`; without a hint the library's rule decides.
const RTS24_ELIM_ORDER = Int32[4, 21, 18, 5, 19, 17, 3, 6, 22, 23, 1, 20, 2, 11, 13, 16, 10, 0, 14, 15, 7, 8, 9, 12]
const RTS96_ELIM_ORDER = Int32[69, 41, 27, 3, 61, 2, 67, 42, 4, 17, 47, 60, 11, 53, 66, 18, 36, 54, 43, 5, 52, 71, 24, 51, 59, 64, 30, 44, 21, 6, 62, 29, 37, 14, 58, 48, 35, 55, 7, 49, 28, 68, 1, 34, 13, 25, 19, 31, 45, 40, 23, 56, 16, 38, 72, 65, 0, 57, 10, 33, 32, 39, 63, 15, 50, 9, 8, 70, 26, 22, 20, 46, 12]

# `elim_order`: optional primary elimination order of the device solver's static schedule (0-based bus numbers, the reference bus last),
# e.g. one found by `tune_order` below; `nothing` = the library's rule (relmc_case_order_hint).
function Engine(sys::TestSystem; device::Integer=0, elim_order::Union{Nothing,Vector{Int32}}=nothing)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:relmc_ctx_create, LIB), Int32, (Int32, Ref{Ptr{Cvoid}}), device, h)
    rc == 0 || error("relmc_ctx_create failed ($rc): no usable HIP device (there is no CPU fallback)")
    eng = Engine(h[], sys)
    GC.@preserve sys begin
        d = CaseDesc(sys.base_mva, sys.nb, sys.ng, sys.nl, sys.nd, sys.ref_bus, pointer(sys.bus_pd),
                     pointer(sys.inj_bus), pointer(sys.inj_pmin), pointer(sys.inj_pmax), pointer(sys.inj_cost),
                     pointer(sys.br_from), pointer(sys.br_to), pointer(sys.br_b), pointer(sys.br_rate),
                     pointer(sys.unavail), pointer(sys.always_up), sys.load)
        if elim_order !== nothing
            check(ccall((:relmc_case_order_hint, LIB), Int32, (Ptr{Cvoid}, Ptr{Int32}, Int32), eng.h, elim_order, length(elim_order)), eng.h, "relmc_case_order_hint")
        end
        check(ccall((:relmc_case_load, LIB), Int32, (Ptr{Cvoid}, Ref{CaseDesc}), eng.h, Ref(d)), eng.h, "relmc_case_load")
    end
    finalizer(e -> ccall((:relmc_ctx_destroy, LIB), Cvoid, (Ptr{Cvoid},), e.h), eng)
    return eng
end

"mpoption('PF_DC',1,...,'OPF_ALG_DC',200,'OPF_FLOW_LIM',1) of nsqMain.m:185-186 = MIPS defaults.  screen = 1: the zero-curtailment pre-screen
(relmc.h: states with a proven LP optimum of 0 are counted, not solved; Acc.n_screened counts them; every other output unchanged)."
function mpoption(; singular_policy::Integer=0, screen::Integer=0)
    o = SolverOpts()
    ccall((:relmc_solver_opts_default, LIB), Cvoid, (Ref{SolverOpts},), o)
    o.singular_policy = singular_policy
    o.screen = screen
    return o
end

"eqstatus = mc_sampling(failure_probabilities, num_samples, numGenerators, numLines): n x (Ng+Nl), 1 = failed."
function mc_sampling(eng::Engine, failure_probabilities, num_samples::Integer, numGenerators::Integer, numLines::Integer;
                     seed::Integer=1, first_index::Integer=0)
    @assert numGenerators == eng.sys.ng && numLines == eng.sys.nl
    @assert failure_probabilities === nothing || failure_probabilities == eng.sys.unavail
    ncomp = numGenerators + numLines
    out = Matrix{UInt8}(undef, ncomp, num_samples)          # column-major: one scenario per column = row-major n x ncomp
    check(ccall((:relmc_mc_sampling, LIB), Int32, (Ptr{Cvoid}, UInt64, UInt64, Int64, Ptr{UInt8}),
                eng.h, seed, first_index, num_samples, out), eng.h, "relmc_mc_sampling")
    return permutedims(out)
end

"[dns, nodal_dns] = mc_simulation(component_states, TestSystem, mpopt, numGenerators, numLines); states: n x (Ng+Nl)."
function mc_simulation(eng::Engine, component_states::AbstractMatrix, mpopt::SolverOpts=mpoption(),
                       numGenerators::Integer=eng.sys.ng, numLines::Integer=eng.sys.nl)
    n = size(component_states, 1)
    st = Matrix{UInt8}(permutedims(component_states .!= 0))
    dns = Vector{Float64}(undef, n); nodal = Matrix{Float64}(undef, eng.sys.nb, n)
    status = Vector{Int32}(undef, n); iters = Vector{Int32}(undef, n)
    check(ccall((:relmc_mc_simulation, LIB), Int32,
                (Ptr{Cvoid}, Ptr{UInt8}, Int64, Ref{SolverOpts}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}, Ptr{Int32}),
                eng.h, st, n, mpopt, dns, nodal, status, iters), eng.h, "relmc_mc_simulation")
    return dns, permutedims(nodal), status, iters
end

"One pass of the nsqMain loop body over global scenarios [first_index, first_index+n): additive accumulators."
function nsq_accumulate(eng::Engine, seed::Integer, first_index::Integer, n::Integer, mpopt::SolverOpts=mpoption())
    acc = Acc()
    check(ccall((:relmc_nsq_accumulate, LIB), Int32, (Ptr{Cvoid}, UInt64, UInt64, Int64, Ref{SolverOpts}, Ref{Acc}),
                eng.h, seed, first_index, n, mpopt, acc), eng.h, "relmc_nsq_accumulate")
    return acc
end

"The reference's unique-state database (nsqMain.m:220-245) per range: every distinct state solved once, weighted by its count."
function nsq_accumulate_distinct(eng::Engine, seed::Integer, first_index::Integer, n::Integer, mpopt::SolverOpts=mpoption())
    acc = Acc(); nd = Ref{Int64}(0)
    check(ccall((:relmc_nsq_accumulate_distinct, LIB), Int32, (Ptr{Cvoid}, UInt64, UInt64, Int64, Ref{SolverOpts}, Ref{Acc}, Ref{Int64}),
                eng.h, seed, first_index, n, mpopt, acc, nd), eng.h, "relmc_nsq_accumulate_distinct")
    return acc, nd[]
end

function indices(eng::Engine, acc::Acc; hours_per_year=8760.0)
    out = Indices()
    ccall((:relmc_nsq_indices, LIB), Cvoid, (Ref{Acc}, Int32, Int32, Cdouble, Ref{Indices}),
          acc, eng.sys.nb, eng.sys.ng + eng.sys.nl, hours_per_year, out)
    return out
end

# ---- the reference's persistent unique-state database (nsqMain.m:91-99, 220-278) on the device -------------------------

struct DbStats
    rows::Int64; samples::Int64; new_rows::Int64; batch_distinct::Int64
end

db_reset(eng::Engine) = check(ccall((:relmc_db_reset, LIB), Int32, (Ptr{Cvoid},), eng.h), eng.h, "relmc_db_reset")
"(units evaluated a second time under the alternate elimination order, how many of them then converged) since the case was loaded"
function retry_stats(eng::Engine)
    u = Ref{Int64}(0); c = Ref{Int64}(0)
    check(ccall((:relmc_retry_stats, LIB), Int32, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}), eng.h, u, c), eng.h, "relmc_retry_stats")
    return (u[], c[])
end
"units that did not fit the kernel's list of non-converged units and kept their first-attempt results (relmc_retry_overflow)"
function retry_overflow(eng::Engine)
    u = Ref{Int64}(0)
    check(ccall((:relmc_retry_overflow, LIB), Int32, (Ptr{Cvoid}, Ref{Int64}), eng.h, u), eng.h, "relmc_retry_overflow")
    return u[]
end
"(primary static elimination order 0/1/2, failures of each probed order among the 8192 calibration states; -1 = not probed)"
function case_order(eng::Engine)
    p = Ref{Int32}(0); f = zeros(Int32, 3)
    check(ccall((:relmc_case_order, LIB), Int32, (Ptr{Cvoid}, Ref{Int32}, Ptr{Int32}), eng.h, p, f), eng.h, "relmc_case_order")
    return (Int(p[]), f)
end
"""
    tune_order(sys; evaluations=20000, seed=1, start=nothing) -> (order, (lds_before, passes_before, lds_after, passes_after))

relmc_tune_order: host-only search of the primary elimination order against the library's own scheduler (no GPU needed); pass the result to
`Engine(sys; elim_order=order)`.
"""
function tune_order(sys::TestSystem; evaluations::Integer=20000, seed::Integer=1, start::Union{Nothing,Vector{Int32}}=nothing)
    order = zeros(Int32, sys.nb); st = zeros(Int32, 4)
    GC.@preserve sys begin
        d = CaseDesc(sys.base_mva, sys.nb, sys.ng, sys.nl, sys.nd, sys.ref_bus, pointer(sys.bus_pd),
                     pointer(sys.inj_bus), pointer(sys.inj_pmin), pointer(sys.inj_pmax), pointer(sys.inj_cost),
                     pointer(sys.br_from), pointer(sys.br_to), pointer(sys.br_b), pointer(sys.br_rate),
                     pointer(sys.unavail), pointer(sys.always_up), sys.load)
        rc = ccall((:relmc_tune_order, LIB), Int32, (Ref{CaseDesc}, Int32, UInt64, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}),
                   Ref(d), evaluations, seed, start === nothing ? C_NULL : start, order, st)
        rc == 0 || error("relmc_tune_order failed ($rc)")
    end
    return order, Tuple(Int.(st))
end
"(rows, samples) of the state database"
function db_size(eng::Engine)
    rows = Ref{Int64}(0); samples = Ref{Int64}(0)
    check(ccall((:relmc_db_size, LIB), Int32, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}), eng.h, rows, samples), eng.h, "relmc_db_size")
    return (rows[], samples[])
end

"One pass of the loop body (dedupe, count bumps of known states, evaluation of the new ones, indices from ALL rows): (Acc of the whole database, DbStats)."
function nsq_db_batch(eng::Engine, seed::Integer, first_index::Integer, n::Integer, mpopt::SolverOpts=mpoption())
    acc = Acc(); st = Ref(DbStats(0, 0, 0, 0))
    check(ccall((:relmc_nsq_db_batch, LIB), Int32, (Ptr{Cvoid}, UInt64, UInt64, Int64, Ref{SolverOpts}, Ref{Acc}, Ref{DbStats}),
                eng.h, seed, first_index, n, mpopt, acc, st), eng.h, "relmc_nsq_db_batch")
    return acc, st[]
end

"state_database rows [first_row, first_row + n_rows) in the reference's column layout (nsqMain.m:91-99)."
function db_export(eng::Engine, first_row::Integer, n_rows::Integer)
    ncomp = eng.sys.ng + eng.sys.nl; nb = eng.sys.nb
    states = Matrix{UInt8}(undef, ncomp, n_rows); count = Vector{Int64}(undef, n_rows); dns = Vector{Float64}(undef, n_rows)
    flag = Vector{Int32}(undef, n_rows); nodal = Matrix{Float64}(undef, nb, n_rows)
    check(ccall((:relmc_db_export, LIB), Int32,
                (Ptr{Cvoid}, Int64, Int64, Ptr{UInt8}, Ptr{Int64}, Ptr{Cdouble}, Ptr{Int32}, Ptr{Cdouble}, Ptr{Int32}, Ptr{Int32}, Ptr{UInt8}),
                eng.h, first_row, n_rows, states, count, dns, flag, nodal, C_NULL, C_NULL, C_NULL), eng.h, "relmc_db_export")
    return hcat(Float64.(permutedims(states)), Float64.(count), dns, Float64.(flag), permutedims(nodal))     # the reference's matrix
end

"Resume: a state_database matrix in the reference's column layout (as db_export returns it) back into the EMPTY database.
One row per state and counts >= 1: otherwise the call fails naming the first offending row and the database stays empty."
function db_import(eng::Engine, db::AbstractMatrix{Float64}; mpopt::SolverOpts = mpoption())
    ncomp = eng.sys.ng + eng.sys.nl; nb = eng.sys.nb; n = size(db, 1)
    states = Matrix{UInt8}(permutedims(db[:, 1:ncomp] .!= 0)); count = Vector{Int64}(round.(Int64, db[:, ncomp + 1]))
    dns = Vector{Float64}(db[:, ncomp + 2]); nodal = Matrix{Float64}(permutedims(db[:, ncomp + 4:ncomp + 3 + nb]))
    check(ccall((:relmc_db_import, LIB), Int32,
                (Ptr{Cvoid}, Ref{SolverOpts}, Int64, Ptr{UInt8}, Ptr{Int64}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}, Ptr{Int32}, Ptr{UInt8}),
                eng.h, mpopt, n, states, count, dns, nodal, C_NULL, C_NULL, C_NULL), eng.h, "relmc_db_import")
end

# ---- multi-GPU: one process per GPU (Distributed / MPI.jl), ONE RCCL all-reduce of the accumulators per convergence check ---
const COMM_ID_BYTES = 128
function comm_unique_id()
    id = Vector{UInt8}(undef, COMM_ID_BYTES)
    rc = ccall((:relmc_comm_unique_id, LIB), Int32, (Ptr{UInt8},), id)
    rc == 0 || error("relmc_comm_unique_id failed ($rc)")
    return id                          # rank 0 broadcasts these 128 bytes by its own means (Distributed.remotecall, MPI.Bcast!, a file)
end
comm_init(eng::Engine, nranks::Integer, rank::Integer, id::Vector{UInt8}) =
    check(ccall((:relmc_comm_init, LIB), Int32, (Ptr{Cvoid}, Int32, Int32, Ptr{UInt8}), eng.h, nranks, rank, id), eng.h, "relmc_comm_init")
function comm_allreduce!(eng::Engine, acc::Acc)
    check(ccall((:relmc_comm_allreduce_acc, LIB), Int32, (Ptr{Cvoid}, Ref{Acc}), eng.h, acc), eng.h, "relmc_comm_allreduce_acc")
    return acc
end
comm_destroy(eng::Engine) = ccall((:relmc_comm_destroy, LIB), Int32, (Ptr{Cvoid},), eng.h)
"The host's own transport instead of RCCL: `fn = @cfunction(f, Int32, (Ptr{Cvoid}, Ptr{Acc}))` must leave the sum over all ranks in the
accumulators it is handed (0 = ok), e.g. MPI.Allreduce! on the two halves of the struct (relmc_comm_set_host_allreduce)."
comm_set_host_allreduce(eng::Engine, nranks::Integer, rank::Integer, fn::Ptr{Cvoid}, user::Ptr{Cvoid}=C_NULL) =
    check(ccall((:relmc_comm_set_host_allreduce, LIB), Int32, (Ptr{Cvoid}, Int32, Int32, Ptr{Cvoid}, Ptr{Cvoid}), eng.h, nranks, rank, fn, user),
          eng.h, "relmc_comm_set_host_allreduce")
"Vector transport of the host collective: `fn = @cfunction(f, Int32, (Ptr{Cvoid}, Ptr{Cdouble}, Int64))` leaves the sum over all ranks of `count` doubles
in the buffer (e.g. MPI.Allreduce!); the library's vector all-reduces (annual indices, per-checkpoint sums) are then one callback each
(relmc_comm_set_host_allreduce_f64)."
comm_set_host_allreduce_f64(eng::Engine, fn::Ptr{Cvoid}, user::Ptr{Cvoid}=C_NULL) =
    check(ccall((:relmc_comm_set_host_allreduce_f64, LIB), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), eng.h, fn, user), eng.h, "relmc_comm_set_host_allreduce_f64")
"(kind 0 none / 1 RCCL / 2 host, ranks, this rank, all-reduces issued, seconds in them) as the communicator itself reports (relmc_comm_info)"
function comm_info(eng::Engine)
    kind = Ref{Int32}(0); n = Ref{Int32}(0); r = Ref{Int32}(0); calls = Ref{Int64}(0); sec = Ref{Cdouble}(0.0)
    check(ccall((:relmc_comm_info, LIB), Int32, (Ptr{Cvoid}, Ref{Int32}, Ref{Int32}, Ref{Int32}, Ref{Int64}, Ref{Cdouble}), eng.h, kind, n, r, calls, sec),
          eng.h, "relmc_comm_info")
    return (kind=kind[], nranks=n[], rank=r[], allreduces=calls[], seconds=sec[])
end

"nsqMain: `while beta > beta_limit && n < max_iterations` (nsqMain.m:208-318) + post-processing (:345-393).
distinct_states: false = every sample solved; true = distinct states of each batch solved once; :database = the reference's
persistent unique-state database across batches.  More than one rank: give the engine a communicator first (comm_init = RCCL, or
comm_set_host_allreduce = the host's own transport) and call nsqMain on EVERY rank -- the library splits every batch over the
ranks, all-reduces once per batch and hands every rank the same result (relmc_nsq_run); there is no loop on the Julia side.
verbose: the reference's console output."
function nsqMain(eng::Engine; beta_limit=0.0017, max_iterations=100_000, samples_per_batch=100, seed=1, mpopt=mpoption(),
                 distinct_states=false, verbose=false)
    total = Acc(); ccall((:relmc_acc_zero, LIB), Cvoid, (Ref{Acc},), total)
    idx = Indices(); rows = 0
    t0 = time()
    # the loop runs inside the library (relmc_nsq_run), which also evaluates small batches such as the reference's 100 many checkpoints
    # per launch (DESIGN.md 6.8) and shards the batches over the ranks of the engine's communicator
    ncp = cld(max_iterations, samples_per_batch)
    beta_history = zeros(ncp); edns_history = zeros(ncp); lole_history = zeros(ncp); plc_history = zeros(ncp)
    mode = distinct_states === :database ? 2 : (distinct_states === true ? 1 : 0)
    buf = zeros(UInt8, NSQ_RESULT_BYTES)
    k = 0
    GC.@preserve beta_history edns_history lole_history plc_history buf total idx begin
        o = NsqOpts(beta_limit, max_iterations, samples_per_batch, seed, 8760.0, SolverOptsC(mpopt), ncp, pointer(beta_history),
                    pointer(edns_history), pointer(lole_history), pointer(plc_history), mode)
        check(ccall((:relmc_nsq_run, LIB), Int32, (Ptr{Cvoid}, Ref{NsqOpts}, Ptr{UInt8}), eng.h, Ref(o), buf), eng.h, "relmc_nsq_run")
        unsafe_copyto!(Ptr{UInt8}(pointer_from_objref(total)), pointer(buf), NSQ_RESULT_IDX)
        unsafe_copyto!(Ptr{UInt8}(pointer_from_objref(idx)), pointer(buf) + NSQ_RESULT_IDX, NSQ_RESULT_TAIL - NSQ_RESULT_IDX)
        k = unsafe_load(Ptr{Int64}(pointer(buf) + NSQ_RESULT_TAIL))
    end
    resize!(beta_history, k); resize!(edns_history, k); resize!(lole_history, k); resize!(plc_history, k)
    done = idx.n; beta = idx.beta
    mode == 2 && (rows = db_size(eng)[1])
    if verbose
        for c in 1:k
            n_c = min(c * samples_per_batch, done)
            n_c % 1000 == 0 && println("Iteration ", lpad(n_c, 6), ": Beta = ", round(beta_history[c], digits=6), ", EDNS = ",
                                       round(edns_history[c], digits=4), " MW, LOLE = ", round(lole_history[c], digits=4), " hr/yr")
        end
    end
    nb = eng.sys.nb; nc = eng.sys.ng + eng.sys.nl
    nodal = collect(idx.nodal_eens[1:nb]); imp = collect(idx.comp_importance[1:nc])
    if verbose                                                                                    # nsqMain.m:325-393
        println("Total simulation time: ", round(time() - t0, digits=2), " seconds\nTotal iterations: ", done)
        distinct_states === :database && println("Unique states evaluated: ", rows)
        println("Convergence achieved: ", beta <= beta_limit ? "YES" : "NO")
        println("EDNS (Expected Demand Not Supplied): ", round(idx.edns, digits=4), " MW\nLOLE (Loss of Load Expectation): ",
                round(idx.lole, digits=4), " hours/year\nPLC (Probability of Load Curtailment): ", round(idx.plc, digits=6),
                "\nBeta (Coefficient of Variation): ", round(idx.beta, digits=6), "\nTop 5 Buses by EENS (MWh/yr):")
        for k in sortperm(nodal, rev=true)[1:min(5, nb)]
            nodal[k] > 0 && println("  Bus ", lpad(k, 2), ": ", round(nodal[k] * 8760, digits=4), " MWh/yr")
        end
        if total.n_fail > 0
            println("Top 5 Critical Components (Prob. Down given System Failure):")
            for c in sortperm(imp, rev=true)[1:min(5, nc)]
                println("  ", c <= eng.sys.ng ? "Gen " * lpad(c, 2) : "Line " * lpad(c - eng.sys.ng, 2), ": ", round(imp[c] * 100, digits=2), "%")
            end
        else
            println("No failure events recorded to analyze weak points.")
        end
    end
    return (accumulated_edns=idx.edns, accumulated_lole=idx.lole, plc=idx.plc, current_beta=idx.beta,
            current_iteration=done, nodal_eens=nodal, comp_importance=imp, beta_history=beta_history, edns_history=edns_history,
            lole_history=lole_history, plc_history=plc_history, database_row_count=rows)
end

# ---- sequential track (Montecarlo_seq/) and HL1 copper sheet (GeneratingAdequacy/PowerSystemAdequacy.jl) ----------------

struct SeqYear
    ens::Cdouble; dlc::Cdouble; nlc::Cdouble; n_contingency::Int64
end

"relmc_seq_load: `reliability_data` = seqmeantime() [(Ng+Nl) x 2] = [MTTF MTTR]; `load_scale_factors` = anloducurve(hours)[3]."
function seq_load(eng::Engine, reliability_data::AbstractMatrix, load_scale_factors::Vector{Float64})
    mttf = Vector{Float64}(reliability_data[:, 1]); mttr = Vector{Float64}(reliability_data[:, 2])
    check(ccall((:relmc_seq_load, LIB), Int32, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Ptr{Cdouble}),
                eng.h, mttf, mttr, length(load_scale_factors), load_scale_factors), eng.h, "relmc_seq_load")
end

"state_duration_matrix = seq_mcsampling(reliability_data, Ng, Nl, num_years, hours_per_year): (Ng+Nl) x (years*hours), 1 = down."
function seq_mcsampling(eng::Engine, num_years::Integer, hours_per_year::Integer; seed::Integer=1, first_year::Integer=0)
    ncomp = eng.sys.ng + eng.sys.nl
    out = Matrix{UInt8}(undef, ncomp, num_years * hours_per_year)
    check(ccall((:relmc_seq_mcsampling, LIB), Int32, (Ptr{Cvoid}, UInt64, UInt64, Int32, Ptr{UInt8}),
                eng.h, seed, first_year, num_years, out), eng.h, "relmc_seq_mcsampling")
    return out
end

"[curtailment_mw, nodal] = seq_mcsimulation(component_status, load_scale_factor, ...), batched: states n x (Ng+Nl), scales n."
function seq_mcsimulation(eng::Engine, component_status::AbstractMatrix, load_scale_factor::Vector{Float64}, mpopt::SolverOpts=mpoption())
    n = size(component_status, 1)
    st = Matrix{UInt8}(permutedims(component_status .!= 0))
    dns = Vector{Float64}(undef, n); nodal = Matrix{Float64}(undef, eng.sys.nb, n)
    check(ccall((:relmc_seq_mcsimulation, LIB), Int32,
                (Ptr{Cvoid}, Ptr{UInt8}, Ptr{Cdouble}, Int64, Ref{SolverOpts}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}, Ptr{Int32}),
                eng.h, st, load_scale_factor, n, mpopt, dns, nodal, C_NULL, C_NULL), eng.h, "relmc_seq_mcsimulation")
    return dns, permutedims(nodal)
end

"Body of the `for iYear` loop (seqMain.m:85-176) for years [first_year, first_year + n_years), fused on the GPU."
function seq_years(eng::Engine, seed::Integer, first_year::Integer, n_years::Integer, mpopt::SolverOpts=mpoption(); curtail_threshold=0.01)
    yrs = Vector{SeqYear}(undef, n_years); acc = Acc()
    check(ccall((:relmc_seq_years, LIB), Int32, (Ptr{Cvoid}, UInt64, UInt64, Int32, Ref{SolverOpts}, Cdouble, Ptr{SeqYear}, Ref{Acc}),
                eng.h, seed, first_year, n_years, mpopt, curtail_threshold, yrs, acc), eng.h, "relmc_seq_years")
    return yrs, acc
end

"relmc_seq_event / relmc_seq_event_acc (include/relmc.h); tests/test_seq_events_host.py compares the fields with the C compiler's layout"
struct SeqEvent
    year::Int32; start_hour::Int32; duration::Int32; censored::Int32
    energy_mwh::Cdouble; peak_mw::Cdouble
    onset::NTuple{8,UInt32}; involved::NTuple{8,UInt32}
end
mutable struct SeqEventAcc
    years::Int64; events::Int64; censored::Int64; load_onset_events::Int64; sum_dur::Int64; sum_dur2::Int64; max_dur::Int64
    sum_energy::Cdouble; sum_energy2::Cdouble; max_energy::Cdouble; max_peak::Cdouble
    onset_events::NTuple{256,Int64}; involved_events::NTuple{256,Int64}
    onset_energy::NTuple{256,Cdouble}; involved_energy::NTuple{256,Cdouble}
    SeqEventAcc() = new()
end

"""
Loss events of `seq_years`' years (same arguments, same years byte for byte): a maximal run of consecutive hours with system curtailment
above the threshold inside one simulated year, with its duration, energy, peak and the outages that set it off (relmc_seq_events).
Returns the years, both accumulators, the duration histogram (`duration_bins` bins, the last one counts that many hours or more) and the
first `max_events` events in (year, start_hour) order.
"""
function seq_events(eng::Engine, seed::Integer, first_year::Integer, n_years::Integer, mpopt::SolverOpts=mpoption(); curtail_threshold=0.01,
                    duration_bins::Integer=168, max_events::Integer=0)
    (1 <= duration_bins <= 4096 && max_events >= 0 && n_years >= 0) ||
        throw(ArgumentError("duration_bins must lie in 1:4096, max_events and n_years must not be negative"))
    yrs = Vector{SeqYear}(undef, n_years); acc = Acc(); ev_acc = SeqEventAcc()
    hist = zeros(Int64, duration_bins); evs = Vector{SeqEvent}(undef, max_events)
    check(ccall((:relmc_seq_events, LIB), Int32,
                (Ptr{Cvoid}, UInt64, UInt64, Int32, Ref{SolverOpts}, Cdouble, Ptr{SeqYear}, Ref{Acc}, Ref{SeqEventAcc}, Int32, Ptr{Int64}, Int64, Ptr{SeqEvent}),
                eng.h, seed, first_year, n_years, mpopt, curtail_threshold, yrs, acc, ev_acc, duration_bins, hist, max_events, evs), eng.h, "relmc_seq_events")
    n = ev_acc.events
    return (years=yrs, acc=acc, ev_acc=ev_acc, lolf_occ_yr=n_years > 0 ? n / n_years : NaN, mean_duration_hours=n > 0 ? ev_acc.sum_dur / n : NaN,
            mean_energy_mwh=n > 0 ? ev_acc.sum_energy / n : NaN, duration_hist=hist, events=evs[1:min(n, max_events)])
end

"relmc_seq_opts (include/relmc.h): the options of the whole seqMain loop"
struct SeqOpts
    cov_threshold::Cdouble; max_years::Int32; batch_years::Int32; seed::UInt64; curtail_threshold::Cdouble
    solver::SolverOptsC
    years_cap::Int64
    results_year::Ptr{SeqYear}; cum_eens::Ptr{Cdouble}; cum_cov::Ptr{Cdouble}
end

# relmc_seq_result is read out of a byte buffer at these offsets (like relmc_nsq_result)
const SEQ_RESULT_ACC = 56                                                   # final_year, converged, eens, cov, lole, lolf, plc, n_contingency
const SEQ_RESULT_NODAL = SEQ_RESULT_ACC + 8 * (7 + MAX_COMP + 2 + MAX_BUS)
const SEQ_RESULT_IMP = SEQ_RESULT_NODAL + 8 * MAX_BUS
const SEQ_RESULT_TAIL = SEQ_RESULT_IMP + 8 * MAX_COMP                       # wall_seconds, kernel_seconds
const SEQ_RESULT_BYTES = SEQ_RESULT_TAIL + 16

"""
seqMain (seqMain.m:85-262): annual indices until CoV(EENS) < cov_threshold, then LOLE / LOLF, nodal EENS (:218) and component importance
(:233).  The loop, its stopping rule and the post-processing run below the C ABI (relmc_seq_run); with a communicator in the engine's
context the same call on every rank is the multi-rank run.
"""
function seqMain(eng::Engine; max_sim_years=4000, cov_threshold=0.05, curtail_threshold=0.01, seed=1, mpopt=mpoption(), batch_years=0)
    yrs = Vector{SeqYear}(undef, max_sim_years); cum_eens = zeros(Float64, max_sim_years); cum_cov = zeros(Float64, max_sim_years)
    buf = zeros(UInt8, SEQ_RESULT_BYTES)
    acc = Acc()
    GC.@preserve yrs cum_eens cum_cov buf acc begin
        o = SeqOpts(cov_threshold, max_sim_years, batch_years, seed, curtail_threshold, SolverOptsC(mpopt), max_sim_years,
                    pointer(yrs), pointer(cum_eens), pointer(cum_cov))
        check(ccall((:relmc_seq_run, LIB), Int32, (Ptr{Cvoid}, Ref{SeqOpts}, Ptr{UInt8}), eng.h, Ref(o), buf), eng.h, "relmc_seq_run")
        unsafe_copyto!(Ptr{UInt8}(pointer_from_objref(acc)), pointer(buf) + SEQ_RESULT_ACC, SEQ_RESULT_NODAL - SEQ_RESULT_ACC)
    end
    rd(T, off) = GC.@preserve buf unsafe_load(Ptr{T}(pointer(buf) + off))
    k = Int(rd(Int32, 0)); nb = eng.sys.nb; nc = eng.sys.ng + eng.sys.nl
    resize!(yrs, k); resize!(cum_eens, k); resize!(cum_cov, k)
    return (final_year=k, converged=rd(Int32, 4) != 0, eens=rd(Cdouble, 8), cov=rd(Cdouble, 16), lole=rd(Cdouble, 24), lolf=rd(Cdouble, 32),
            results_year=(ens=[y.ens for y in yrs], dlc=[y.dlc for y in yrs], nlc=[y.nlc for y in yrs]), results_cum=(eens=cum_eens, cov=cum_cov),
            nodal_eens_avg=[rd(Cdouble, SEQ_RESULT_NODAL + 8 * (i - 1)) for i in 1:nb],
            comp_importance=[rd(Cdouble, SEQ_RESULT_IMP + 8 * (i - 1)) for i in 1:nc],
            total_loss_hours=acc.n_fail, n_lp=acc.n, elapsed_time=rd(Cdouble, SEQ_RESULT_TAIL), kernel_seconds=rd(Cdouble, SEQ_RESULT_TAIL + 8))
end

mutable struct Hl1Acc
    n::Int64; sum_lole::Cdouble; sum_eue::Cdouble; sum_lole2::Cdouble; sum_eue2::Cdouble
    Hl1Acc() = new()
end

"run_non_sequential_mc (PowerSystemAdequacy.jl:169-208): one fleet state per iteration swept over the hourly load curve."
function run_non_sequential_mc(eng::Engine, capacity::Vector{Float64}, for_rate::Vector{Float64}, hourly_load::Vector{Float64},
                               n_iterations::Integer; seed::Integer=1)
    check(ccall((:relmc_hl1_load, LIB), Int32, (Ptr{Cvoid}, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Ptr{Cdouble}),
                eng.h, length(capacity), capacity, for_rate, length(hourly_load), hourly_load), eng.h, "relmc_hl1_load")
    acc = Hl1Acc()
    check(ccall((:relmc_hl1_nsq, LIB), Int32, (Ptr{Cvoid}, UInt64, UInt64, Int64, Ref{Hl1Acc}, Ptr{Cdouble}, Ptr{Cdouble}),
                eng.h, seed, 0, n_iterations, acc, C_NULL, C_NULL), eng.h, "relmc_hl1_nsq")
    return (lole_hours_yr=acc.sum_lole / acc.n, eue_mwh_yr=acc.sum_eue / acc.n)
end

"relmc_hl1_seq_year / relmc_hl1_seq_acc (include/relmc.h)"
struct Hl1SeqYear
    lole::Cdouble; eue::Cdouble; lolf::Cdouble
end
mutable struct Hl1SeqAcc
    years::Int64; sum_lole::Cdouble; sum_eue::Cdouble; sum_lolf::Cdouble; sum_lole2::Cdouble; sum_eue2::Cdouble; sum_lolf2::Cdouble
    Hl1SeqAcc() = new()
end
const HL1_START = Dict(:all_up => Int32(0), :stationary => Int32(1))      # RELMC_HL1_START_*

"""
run_sequential_mc (PowerSystemAdequacy.jl:214-268): `chains` chronological chains of years ÷ chains consecutive years each on the GPU.
The defaults are the reference's shape (one chain, every unit UP at the start); start=:stationary makes short parallel chains unbiased.
Returns LOLE, EUE, LOLF (events per year), LOLD (hours per event) and the per-year indices in chain-major order.
"""
function run_sequential_mc(eng::Engine, capacity::Vector{Float64}, mttf::Vector{Float64}, mttr::Vector{Float64},
                           hourly_load::Vector{Float64}, years::Integer; seed::Integer=1, chains::Integer=1, start::Symbol=:all_up)
    (years >= 1 && chains >= 1 && years % chains == 0) || throw(ArgumentError("years must be a positive multiple of chains"))
    check(ccall((:relmc_hl1_seq_load, LIB), Int32, (Ptr{Cvoid}, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Ptr{Cdouble}),
                eng.h, length(capacity), capacity, mttf, mttr, length(hourly_load), hourly_load), eng.h, "relmc_hl1_seq_load")
    acc = Hl1SeqAcc(); yrs = Vector{Hl1SeqYear}(undef, years)
    check(ccall((:relmc_hl1_seq, LIB), Int32, (Ptr{Cvoid}, UInt64, UInt64, Int64, Int32, Int32, Ref{Hl1SeqAcc}, Ptr{Hl1SeqYear}),
                eng.h, seed, 0, chains, years ÷ chains, HL1_START[start], acc, yrs), eng.h, "relmc_hl1_seq")
    lole = acc.sum_lole / years; lolf = acc.sum_lolf / years
    year_lole = [y.lole for y in yrs]; cum = cumsum(year_lole)
    return (lole_hours_yr=lole, eue_mwh_yr=acc.sum_eue / years, lolf_occ_yr=lolf, lold_hours=lolf > 0 ? lole / lolf : NaN,
            year_lole=year_lole, year_eue=[y.eue for y in yrs], year_lolf=[y.lolf for y in yrs],
            convergence_history=[cum[k] / k for k in 10:10:years])                  # :263-265
end

"relmc_hl1_event / relmc_hl1_event_acc (include/relmc.h); tests/test_hl1_events_host.py compares the fields with the C compiler's layout"
struct Hl1Event
    chain::Int64; start_step::Int64; duration::Int64; energy_mwh::Cdouble; peak_mw::Cdouble
end
mutable struct Hl1EventAcc
    years::Int64; events::Int64; censored::Int64; sum_dur::Int64; sum_dur2::Int64; max_dur::Int64
    sum_energy::Cdouble; sum_energy2::Cdouble; max_energy::Cdouble; max_peak::Cdouble
    Hl1EventAcc() = new()
end

"""
run_sequential_events: the loss events (maximal runs of consecutive loss hours) of run_sequential_mc's chronology, same arguments and
same chains under one seed.  Returns LOLF, LOLD (sum of the durations / events), the mean / maximum energy, the maximum duration and
peak, the censored count, the duration histogram (duration_bins bins, the last one counts that many hours or more) and the first
max_events events in (chain, start_step) order.
"""
function run_sequential_events(eng::Engine, capacity::Vector{Float64}, mttf::Vector{Float64}, mttr::Vector{Float64},
                               hourly_load::Vector{Float64}, years::Integer; seed::Integer=1, chains::Integer=1, start::Symbol=:all_up,
                               duration_bins::Integer=168, max_events::Integer=0)
    (years >= 1 && chains >= 1 && years % chains == 0) || throw(ArgumentError("years must be a positive multiple of chains"))
    (1 <= duration_bins <= 4096 && max_events >= 0) || throw(ArgumentError("duration_bins must lie in 1:4096, max_events must not be negative"))
    check(ccall((:relmc_hl1_seq_load, LIB), Int32, (Ptr{Cvoid}, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Ptr{Cdouble}),
                eng.h, length(capacity), capacity, mttf, mttr, length(hourly_load), hourly_load), eng.h, "relmc_hl1_seq_load")
    acc = Hl1EventAcc(); hist = zeros(Int64, duration_bins); evs = Vector{Hl1Event}(undef, max_events)
    check(ccall((:relmc_hl1_seq_events, LIB), Int32,
                (Ptr{Cvoid}, UInt64, UInt64, Int64, Int32, Int32, Ref{Hl1EventAcc}, Int32, Ptr{Int64}, Int64, Ptr{Hl1Event}),
                eng.h, seed, 0, chains, years ÷ chains, HL1_START[start], acc, duration_bins, hist, max_events, evs), eng.h, "relmc_hl1_seq_events")
    n = acc.events
    return (lolf_occ_yr=n / years, lold_hours=n > 0 ? acc.sum_dur / n : NaN, mean_energy_mwh=n > 0 ? acc.sum_energy / n : NaN,
            lole_hours_yr=acc.sum_dur / years, eue_mwh_yr=acc.sum_energy / years,
            max_duration=acc.max_dur, max_energy_mwh=acc.max_energy, max_peak_mw=acc.max_peak, censored=acc.censored,
            n_events=n, duration_hist=hist, events=evs[1:min(n, max_events)])
end

"relmc_hl1_sweep_level (include/relmc.h): one load level of relmc_hl1_seq_sweep; fleet 0 = every unit, 1 = without the withheld units"
struct Hl1SweepLevel
    scale::Cdouble; shift::Cdouble; fleet::Int32; reserved::Int32
end
const HL1_SWEEP_MAX_LEVELS = 16                                            # RELMC_HL1_SWEEP_MAX_LEVELS

"""
run_load_sweep (an extension beyond the reference): run_sequential_mc's chronology, same arguments and same chains under one seed,
against up to 16 load levels in one walk of the chains.  `levels` holds (scale, shift, withheld) triples: the level sees the load
scale * hourly_load + shift and, if withheld, the fleet without the units `withheld_units` (1-based indices).  Returns per level LOLE,
EUE, LOLF and the per-year indices (n_levels x years).
"""
function run_load_sweep(eng::Engine, capacity::Vector{Float64}, mttf::Vector{Float64}, mttr::Vector{Float64},
                        hourly_load::Vector{Float64}, years::Integer, levels::Vector{<:Tuple{Real,Real,Bool}};
                        withheld_units::Vector{<:Integer}=Int[], seed::Integer=1, chains::Integer=1, start::Symbol=:all_up)
    (years >= 1 && chains >= 1 && years % chains == 0) || throw(ArgumentError("years must be a positive multiple of chains"))
    n = length(levels)
    1 <= n <= HL1_SWEEP_MAX_LEVELS || throw(ArgumentError("between 1 and $HL1_SWEEP_MAX_LEVELS levels"))
    all(1 <= k <= length(capacity) for k in withheld_units) || throw(ArgumentError("withheld_units must be unit indices"))
    (isempty(withheld_units) && any(l[3] for l in levels)) && throw(ArgumentError("a withheld level needs withheld_units"))
    check(ccall((:relmc_hl1_seq_load, LIB), Int32, (Ptr{Cvoid}, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Ptr{Cdouble}),
                eng.h, length(capacity), capacity, mttf, mttr, length(hourly_load), hourly_load), eng.h, "relmc_hl1_seq_load")
    lv = [Hl1SweepLevel(Float64(l[1]), Float64(l[2]), l[3] ? Int32(1) : Int32(0), Int32(0)) for l in levels]
    mask = zeros(UInt32, 4)
    for k in withheld_units
        mask[((k - 1) >> 5) + 1] |= UInt32(1) << ((k - 1) & 31)
    end
    yrs = Vector{Hl1SeqYear}(undef, n * years)
    raw = zeros(UInt8, 56 * n)                                              # relmc_hl1_seq_acc[n], contiguous (Hl1SeqAcc is mutable: a Vector of it holds references)
    check(ccall((:relmc_hl1_seq_sweep, LIB), Int32,
                (Ptr{Cvoid}, UInt64, UInt64, Int64, Int32, Int32, Int32, Ptr{Hl1SweepLevel}, Ptr{UInt32}, Ptr{UInt8}, Ptr{Hl1SeqYear}),
                eng.h, seed, 0, chains, years ÷ chains, HL1_START[start], n, lv, isempty(withheld_units) ? C_NULL : mask, raw, yrs),
          eng.h, "relmc_hl1_seq_sweep")
    sums = reshape(reinterpret(Float64, raw), 7, n)                         # rows 2 .. 4: sum_lole, sum_eue, sum_lolf (row 1 is the Int64 years)
    Y = reshape(yrs, years, n)
    return (lole_hours_yr=[sums[2, j] / years for j in 1:n], eue_mwh_yr=[sums[3, j] / years for j in 1:n],
            lolf_occ_yr=[sums[4, j] / years for j in 1:n],
            year_lole=[Y[y, j].lole for j in 1:n, y in 1:years], year_eue=[Y[y, j].eue for j in 1:n, y in 1:years],
            year_lolf=[Y[y, j].lolf for j in 1:n, y in 1:years])
end

# Layout of the sweep level, kept apart from LAYOUT (tests/test_hl1_sweep_host.py compares it with the C compiler's and with ctypes)
const LAYOUT_HL1_SWEEP = [
    ("relmc_hl1_sweep_level", 24, [("scale", 0), ("shift", 8), ("fleet", 16), ("reserved", 20)]),
]

"relmc_hl1_maint_window (include/relmc.h, 16 bytes): unit `unit` (0-based) of schedule `schedule` is on maintenance in hours start_hour .. start_hour + hours - 1 of the year, modulo the year"
struct Hl1MaintWindow
    schedule::Int32; unit::Int32; start_hour::Int32; hours::Int32
end
const HL1_MAINT_MAX_SCHEDULES = 8                                          # RELMC_HL1_MAINT_MAX_SCHEDULES

"""
run_maintenance_schedules (an extension beyond the reference): run_sequential_mc's chronology, same arguments and same chains under one
seed, under up to 8 planned-maintenance schedules in one walk of the chains, at the load scale * hourly_load + shift.  `schedules` holds
one vector of (unit, start_hour, hours) triples per schedule: unit (1-based) is on maintenance in hours start_hour .. start_hour + hours - 1
of every year (0-based, modulo the year) and adds nothing to those hours' capacity; its failures and repairs run on.  Every schedule sees
the same fleet history, so two schedules may be differenced year by year.  Returns per schedule LOLE, EUE, LOLF and the per-year indices
(n_schedules x years).
"""
function run_maintenance_schedules(eng::Engine, capacity::Vector{Float64}, mttf::Vector{Float64}, mttr::Vector{Float64},
                                   hourly_load::Vector{Float64}, years::Integer, schedules::Vector{<:Vector{<:Tuple{Integer,Integer,Integer}}};
                                   seed::Integer=1, chains::Integer=1, start::Symbol=:all_up, scale::Real=1.0, shift::Real=0.0)
    (years >= 1 && chains >= 1 && years % chains == 0) || throw(ArgumentError("years must be a positive multiple of chains"))
    n = length(schedules)
    1 <= n <= HL1_MAINT_MAX_SCHEDULES || throw(ArgumentError("between 1 and $HL1_MAINT_MAX_SCHEDULES schedules"))
    H = length(hourly_load)
    for s in schedules, w in s
        (1 <= w[1] <= length(capacity) && 0 <= w[2] < H && 1 <= w[3] <= H) || throw(ArgumentError("window $w: unit, start_hour or hours out of range"))
    end
    check(ccall((:relmc_hl1_seq_load, LIB), Int32, (Ptr{Cvoid}, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Ptr{Cdouble}),
                eng.h, length(capacity), capacity, mttf, mttr, H, hourly_load), eng.h, "relmc_hl1_seq_load")
    win = [Hl1MaintWindow(Int32(j - 1), Int32(w[1] - 1), Int32(w[2]), Int32(w[3])) for j in 1:n for w in schedules[j]]
    check(ccall((:relmc_hl1_maint_load, LIB), Int32, (Ptr{Cvoid}, Int32, Int64, Ptr{Hl1MaintWindow}),
                eng.h, n, length(win), isempty(win) ? C_NULL : win), eng.h, "relmc_hl1_maint_load")
    yrs = Vector{Hl1SeqYear}(undef, n * years)
    raw = zeros(UInt8, 56 * n)                                              # relmc_hl1_seq_acc[n], contiguous
    check(ccall((:relmc_hl1_maint_seq, LIB), Int32,
                (Ptr{Cvoid}, UInt64, UInt64, Int64, Int32, Int32, Cdouble, Cdouble, Ptr{UInt8}, Ptr{Hl1SeqYear}),
                eng.h, seed, 0, chains, years ÷ chains, HL1_START[start], Float64(scale), Float64(shift), raw, yrs),
          eng.h, "relmc_hl1_maint_seq")
    sums = reshape(reinterpret(Float64, raw), 7, n)                         # rows 2 .. 4: sum_lole, sum_eue, sum_lolf (row 1 is the Int64 years)
    Y = reshape(yrs, years, n)
    return (lole_hours_yr=[sums[2, j] / years for j in 1:n], eue_mwh_yr=[sums[3, j] / years for j in 1:n],
            lolf_occ_yr=[sums[4, j] / years for j in 1:n],
            year_lole=[Y[y, j].lole for j in 1:n, y in 1:years], year_eue=[Y[y, j].eue for j in 1:n, y in 1:years],
            year_lolf=[Y[y, j].lolf for j in 1:n, y in 1:years])
end

# Layout of the maintenance window, kept apart from LAYOUT (tests/test_hl1_maint_host.py compares it with the C compiler's and with ctypes)
const LAYOUT_HL1_MAINT = [
    ("relmc_hl1_maint_window", 16, [("schedule", 0), ("unit", 4), ("start_hour", 8), ("hours", 12)]),
]

"relmc_hl1_attr_unit (include/relmc.h, 32 bytes): one chain's loss steps with the unit DOWN: their number, their deficit, those the unit, UP, would have prevented, and the deficit it would have served"
struct Hl1AttrUnit
    down_hours::Cdouble; down_mwh::Cdouble; critical_hours::Cdouble; relief_mwh::Cdouble
end
"relmc_hl1_attr_acc (64 bytes): sums of x and x * x over the chains of a call, x = a chain's Hl1AttrUnit in field order"
struct Hl1AttrAcc
    sum::NTuple{4,Cdouble}; sum2::NTuple{4,Cdouble}
end

"""
run_sequential_attribution (the reference's comp_importance, seqMain.m:144-158, 233, on the HL1 chronology): run_sequential_mc's chronology,
same arguments and same chains under one seed, at the load scale * hourly_load + shift, with every loss step charged to the units that
are DOWN in it.  Returns the indices and, per unit, importance = down_hours / loss hours, energy_importance = down_mwh / EUE, and the
exact counterfactuals on the same fleet history lole_if_perfect = LOLE - critical_hours / years and eue_if_perfect = EUE - relief_mwh /
years, with the chains' unit records (units x chains).
"""
function run_sequential_attribution(eng::Engine, capacity::Vector{Float64}, mttf::Vector{Float64}, mttr::Vector{Float64},
                                    hourly_load::Vector{Float64}, years::Integer;
                                    seed::Integer=1, chains::Integer=1, start::Symbol=:all_up, scale::Real=1.0, shift::Real=0.0)
    (years >= 1 && chains >= 1 && years % chains == 0) || throw(ArgumentError("years must be a positive multiple of chains"))
    K = length(capacity)
    check(ccall((:relmc_hl1_seq_load, LIB), Int32, (Ptr{Cvoid}, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Ptr{Cdouble}),
                eng.h, K, capacity, mttf, mttr, length(hourly_load), hourly_load), eng.h, "relmc_hl1_seq_load")
    acc = Hl1SeqAcc(); yrs = Vector{Hl1SeqYear}(undef, years)
    uacc = Vector{Hl1AttrAcc}(undef, K); rec = Vector{Hl1AttrUnit}(undef, K * chains)
    check(ccall((:relmc_hl1_attr_seq, LIB), Int32,
                (Ptr{Cvoid}, UInt64, UInt64, Int64, Int32, Int32, Cdouble, Cdouble, Ref{Hl1SeqAcc}, Ptr{Hl1SeqYear}, Ptr{Hl1AttrAcc}, Ptr{Hl1AttrUnit}),
                eng.h, seed, 0, chains, years ÷ chains, HL1_START[start], Float64(scale), Float64(shift), acc, yrs, uacc, rec),
          eng.h, "relmc_hl1_attr_seq")
    lole, eue = acc.sum_lole / years, acc.sum_eue / years
    return (lole_hours_yr=lole, eue_mwh_yr=eue, lolf_occ_yr=acc.sum_lolf / years,
            importance=[uacc[k].sum[1] / acc.sum_lole for k in 1:K], energy_importance=[uacc[k].sum[2] / acc.sum_eue for k in 1:K],
            lole_if_perfect=[lole - uacc[k].sum[3] / years for k in 1:K], eue_if_perfect=[eue - uacc[k].sum[4] / years for k in 1:K],
            year_lole=[y.lole for y in yrs], year_eue=[y.eue for y in yrs], year_lolf=[y.lolf for y in yrs],
            unit_records=reshape(rec, K, chains))
end

# Layout of the attribution records, kept apart from LAYOUT (tests/test_hl1_attr_host.py compares it with the C compiler's and with ctypes)
const LAYOUT_HL1_ATTR = [
    ("relmc_hl1_attr_unit", 32, [("down_hours", 0), ("down_mwh", 8), ("critical_hours", 16), ("relief_mwh", 24)]),
    ("relmc_hl1_attr_acc", 64, [("sum", 0), ("sum2", 32)]),
]

"relmc_hl1_storage (include/relmc.h, 48 bytes): one energy storage of relmc_hl1_seq_storage; powers in MW, energies in MWh, efficiencies in (0, 1]"
struct Hl1Storage
    charge_mw::Cdouble; discharge_mw::Cdouble; energy_mwh::Cdouble; eta_charge::Cdouble; eta_discharge::Cdouble; soc0_mwh::Cdouble
end
"relmc_hl1_storage_year: short hours fully served by the storages, MWh delivered and MWh of surplus taken in one simulated year"
struct Hl1StorageYear
    served_hours::Cdouble; discharged_mwh::Cdouble; charged_mwh::Cdouble
end
mutable struct Hl1StorageAcc
    years::Int64; sum_lole::Cdouble; sum_eue::Cdouble; sum_lolf::Cdouble; sum_lole2::Cdouble; sum_eue2::Cdouble; sum_lolf2::Cdouble
    sum_served::Cdouble; sum_discharged::Cdouble; sum_charged::Cdouble; sum_served2::Cdouble; sum_discharged2::Cdouble; sum_charged2::Cdouble
    Hl1StorageAcc() = new()
end
const HL1_MAX_STORAGE = 8                                                  # RELMC_HL1_MAX_STORAGE

"""
run_sequential_storage (an extension beyond the reference): run_sequential_mc's chronology, same arguments and same chains under one
seed, at the load scale * hourly_load + shift with up to 8 energy storages.  A storage discharges into a shortfall of the fleet and
charges from its surplus only; its state of charge carries from hour to hour and from year to year inside a chain.  Returns LOLE, EUE and
LOLF of the hours left after storage, the hours served and the MWh cycled per year, and the per-year records.
"""
function run_sequential_storage(eng::Engine, capacity::Vector{Float64}, mttf::Vector{Float64}, mttr::Vector{Float64},
                                hourly_load::Vector{Float64}, storages::Vector{Hl1Storage}, years::Integer;
                                scale::Real=1.0, shift::Real=0.0, seed::Integer=1, chains::Integer=1, start::Symbol=:all_up)
    (years >= 1 && chains >= 1 && years % chains == 0) || throw(ArgumentError("years must be a positive multiple of chains"))
    length(storages) <= HL1_MAX_STORAGE || throw(ArgumentError("at most $HL1_MAX_STORAGE storages"))
    check(ccall((:relmc_hl1_seq_load, LIB), Int32, (Ptr{Cvoid}, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Ptr{Cdouble}),
                eng.h, length(capacity), capacity, mttf, mttr, length(hourly_load), hourly_load), eng.h, "relmc_hl1_seq_load")
    acc = Hl1StorageAcc()
    yrs = Vector{Hl1SeqYear}(undef, years); sty = Vector{Hl1StorageYear}(undef, years)
    check(ccall((:relmc_hl1_seq_storage, LIB), Int32,
                (Ptr{Cvoid}, UInt64, UInt64, Int64, Int32, Int32, Cdouble, Cdouble, Int32, Ptr{Hl1Storage}, Ref{Hl1StorageAcc}, Ptr{Hl1SeqYear},
                 Ptr{Hl1StorageYear}),
                eng.h, seed, 0, chains, years ÷ chains, HL1_START[start], Float64(scale), Float64(shift), length(storages),
                isempty(storages) ? C_NULL : storages, acc, yrs, sty), eng.h, "relmc_hl1_seq_storage")
    return (lole_hours_yr=acc.sum_lole / years, eue_mwh_yr=acc.sum_eue / years, lolf_occ_yr=acc.sum_lolf / years,
            served_hours_yr=acc.sum_served / years, discharged_mwh_yr=acc.sum_discharged / years, charged_mwh_yr=acc.sum_charged / years,
            years=yrs, storage_years=sty)
end

"relmc_hl1_var_opts (include/relmc.h, 88 bytes): the options of relmc_hl1_var_seq; resource_scale finite and >= 0 (0 beyond the library's resources), pick = HL1_VAR_PICK[...], reserved = 0"
struct Hl1VarOpts
    resource_scale::NTuple{8,Cdouble}; scale::Cdouble; shift::Cdouble; pick::Int32; reserved::Int32
end
const HL1_VAR_MAX_RESOURCES = 8                                            # RELMC_HL1_VAR_MAX_RESOURCES
const HL1_VAR_MAX_WEATHER = 256                                            # RELMC_HL1_VAR_MAX_WEATHER
const HL1_VAR_PICK = Dict(:random => Int32(0), :cycle => Int32(1))         # RELMC_HL1_VAR_PICK_*

# Layout of the options, kept apart from LAYOUT (tests/test_hl1_variable_host.py compares it with the C compiler's and with ctypes)
const LAYOUT_HL1_VAR = [
    ("relmc_hl1_var_opts", 88, [("resource_scale", 0), ("scale", 64), ("shift", 72), ("pick", 80), ("reserved", 84)]),
]

"""
run_sequential_variable (an extension beyond the reference): run_sequential_mc's chronology, same arguments and same chains under one
seed, with weather-driven resources and up to 8 energy storages.  output_mw[hour, resource, weather year] (column-major: the C ABI's
[n_weather][n_resources][nhours]) holds the hourly output of every resource in every weather year, weather_load[hour, weather year]
optionally each weather year's own load curve.  Every chain year draws a weather year (pick = :random or :cycle); a step's capacity is
the fleet's plus resource_scale[r] * output, its load scale * base + shift; the storages charge from the surplus, the resources' output
included.  Returns run_sequential_storage's fields and the weather year (0-based) of every simulated year.
"""
function run_sequential_variable(eng::Engine, capacity::Vector{Float64}, mttf::Vector{Float64}, mttr::Vector{Float64},
                                 hourly_load::Vector{Float64}, output_mw::Array{Float64,3}, years::Integer;
                                 weather_load::Union{Nothing,Matrix{Float64}}=nothing, storages::Vector{Hl1Storage}=Hl1Storage[],
                                 resource_scale::Vector{Float64}=ones(size(output_mw, 2)), scale::Real=1.0, shift::Real=0.0,
                                 pick::Symbol=:random, seed::Integer=1, chains::Integer=1, start::Symbol=:all_up)
    (years >= 1 && chains >= 1 && years % chains == 0) || throw(ArgumentError("years must be a positive multiple of chains"))
    nh, nres, nw = size(output_mw)
    nh == length(hourly_load) || throw(ArgumentError("output_mw has $nh hours, the load curve $(length(hourly_load))"))
    nres <= HL1_VAR_MAX_RESOURCES || throw(ArgumentError("at most $HL1_VAR_MAX_RESOURCES resources"))
    1 <= nw <= HL1_VAR_MAX_WEATHER || throw(ArgumentError("1 to $HL1_VAR_MAX_WEATHER weather years"))
    length(resource_scale) == nres || throw(ArgumentError("one resource_scale per resource"))
    weather_load === nothing || size(weather_load) == (nh, nw) || throw(ArgumentError("weather_load must be [hours, weather years]"))
    length(storages) <= HL1_MAX_STORAGE || throw(ArgumentError("at most $HL1_MAX_STORAGE storages"))
    check(ccall((:relmc_hl1_seq_load, LIB), Int32, (Ptr{Cvoid}, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Ptr{Cdouble}),
                eng.h, length(capacity), capacity, mttf, mttr, length(hourly_load), hourly_load), eng.h, "relmc_hl1_seq_load")
    check(ccall((:relmc_hl1_var_load, LIB), Int32, (Ptr{Cvoid}, Int32, Int32, Int32, Ptr{Cdouble}, Ptr{Cdouble}),
                eng.h, nw, nres, nh, nres == 0 ? C_NULL : output_mw, weather_load === nothing ? C_NULL : weather_load), eng.h, "relmc_hl1_var_load")
    opts = Ref(Hl1VarOpts(ntuple(r -> r <= nres ? resource_scale[r] : 0.0, 8), Float64(scale), Float64(shift), HL1_VAR_PICK[pick], Int32(0)))
    acc = Hl1StorageAcc()
    yrs = Vector{Hl1SeqYear}(undef, years); sty = Vector{Hl1StorageYear}(undef, years); wy = Vector{Int32}(undef, years)
    check(ccall((:relmc_hl1_var_seq, LIB), Int32,
                (Ptr{Cvoid}, UInt64, UInt64, Int64, Int32, Int32, Ref{Hl1VarOpts}, Int32, Ptr{Hl1Storage}, Ref{Hl1StorageAcc}, Ptr{Hl1SeqYear},
                 Ptr{Hl1StorageYear}, Ptr{Int32}),
                eng.h, seed, 0, chains, years ÷ chains, HL1_START[start], opts, length(storages),
                isempty(storages) ? C_NULL : storages, acc, yrs, sty, wy), eng.h, "relmc_hl1_var_seq")
    return (lole_hours_yr=acc.sum_lole / years, eue_mwh_yr=acc.sum_eue / years, lolf_occ_yr=acc.sum_lolf / years,
            served_hours_yr=acc.sum_served / years, discharged_mwh_yr=acc.sum_discharged / years, charged_mwh_yr=acc.sum_charged / years,
            years=yrs, storage_years=sty, year_weather=wy)
end

"The weather year (0-based) of chain year `year` (0-based) of chain `chain` (relmc_hl1_var_weather_year: host only, no engine needed)"
weather_year(seed::Integer, chain::Integer, year::Integer, years_per_chain::Integer, n_weather::Integer; pick::Symbol=:random) =
    ccall((:relmc_hl1_var_weather_year, LIB), Int32, (UInt64, UInt64, Int32, Int32, Int32, Int32), seed, chain, year, years_per_chain, n_weather,
          HL1_VAR_PICK[pick])

const HL1_STRESS_MAX_CLASSES = 8                                           # RELMC_HL1_STRESS_MAX_CLASSES

"""
run_sequential_stress (an extension beyond the reference): run_sequential_variable's chronology, same arguments, in which a UP unit of
outage class c fails with the hazard fail_mult / mttf of the hour.  fail_mult[hour, class, weather year] (column-major: the C ABI's
[n_weather][n_classes][nhours]) is finite and >= 0; unit_class[unit] is 0-based, -1 for a unit that ignores the weather.  Repairs are
unchanged.  With every unit in class -1 the records are run_sequential_variable's bit for bit.  Returns that function's fields.
"""
function run_sequential_stress(eng::Engine, capacity::Vector{Float64}, mttf::Vector{Float64}, mttr::Vector{Float64},
                               hourly_load::Vector{Float64}, output_mw::Array{Float64,3}, fail_mult::Array{Float64,3},
                               unit_class::Vector{Int32}, years::Integer;
                               weather_load::Union{Nothing,Matrix{Float64}}=nothing, storages::Vector{Hl1Storage}=Hl1Storage[],
                               resource_scale::Vector{Float64}=ones(size(output_mw, 2)), scale::Real=1.0, shift::Real=0.0,
                               pick::Symbol=:random, seed::Integer=1, chains::Integer=1, start::Symbol=:all_up)
    (years >= 1 && chains >= 1 && years % chains == 0) || throw(ArgumentError("years must be a positive multiple of chains"))
    nh, nres, nw = size(output_mw)
    nh == length(hourly_load) || throw(ArgumentError("output_mw has $nh hours, the load curve $(length(hourly_load))"))
    nres <= HL1_VAR_MAX_RESOURCES || throw(ArgumentError("at most $HL1_VAR_MAX_RESOURCES resources"))
    1 <= nw <= HL1_VAR_MAX_WEATHER || throw(ArgumentError("1 to $HL1_VAR_MAX_WEATHER weather years"))
    length(resource_scale) == nres || throw(ArgumentError("one resource_scale per resource"))
    weather_load === nothing || size(weather_load) == (nh, nw) || throw(ArgumentError("weather_load must be [hours, weather years]"))
    length(storages) <= HL1_MAX_STORAGE || throw(ArgumentError("at most $HL1_MAX_STORAGE storages"))
    ncls = size(fail_mult, 2)
    (size(fail_mult, 1) == nh && size(fail_mult, 3) == nw) || throw(ArgumentError("fail_mult must be [hours, classes, weather years] of the weather library"))
    1 <= ncls <= HL1_STRESS_MAX_CLASSES || throw(ArgumentError("1 to $HL1_STRESS_MAX_CLASSES outage classes"))
    (length(unit_class) == length(capacity) && all(-1 <= c < ncls for c in unit_class)) || throw(ArgumentError("one 0-based class, or -1, per unit"))
    check(ccall((:relmc_hl1_seq_load, LIB), Int32, (Ptr{Cvoid}, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Ptr{Cdouble}),
                eng.h, length(capacity), capacity, mttf, mttr, length(hourly_load), hourly_load), eng.h, "relmc_hl1_seq_load")
    check(ccall((:relmc_hl1_var_load, LIB), Int32, (Ptr{Cvoid}, Int32, Int32, Int32, Ptr{Cdouble}, Ptr{Cdouble}),
                eng.h, nw, nres, nh, nres == 0 ? C_NULL : output_mw, weather_load === nothing ? C_NULL : weather_load), eng.h, "relmc_hl1_var_load")
    check(ccall((:relmc_hl1_stress_load, LIB), Int32, (Ptr{Cvoid}, Int32, Int32, Int32, Ptr{Cdouble}, Int32, Ptr{Int32}),
                eng.h, nw, ncls, nh, fail_mult, length(unit_class), unit_class), eng.h, "relmc_hl1_stress_load")
    opts = Ref(Hl1VarOpts(ntuple(r -> r <= nres ? resource_scale[r] : 0.0, 8), Float64(scale), Float64(shift), HL1_VAR_PICK[pick], Int32(0)))
    acc = Hl1StorageAcc()
    yrs = Vector{Hl1SeqYear}(undef, years); sty = Vector{Hl1StorageYear}(undef, years); wy = Vector{Int32}(undef, years)
    check(ccall((:relmc_hl1_stress_seq, LIB), Int32,
                (Ptr{Cvoid}, UInt64, UInt64, Int64, Int32, Int32, Ref{Hl1VarOpts}, Int32, Ptr{Hl1Storage}, Ref{Hl1StorageAcc}, Ptr{Hl1SeqYear},
                 Ptr{Hl1StorageYear}, Ptr{Int32}),
                eng.h, seed, 0, chains, years ÷ chains, HL1_START[start], opts, length(storages),
                isempty(storages) ? C_NULL : storages, acc, yrs, sty, wy), eng.h, "relmc_hl1_stress_seq")
    return (lole_hours_yr=acc.sum_lole / years, eue_mwh_yr=acc.sum_eue / years, lolf_occ_yr=acc.sum_lolf / years,
            served_hours_yr=acc.sum_served / years, discharged_mwh_yr=acc.sum_discharged / years, charged_mwh_yr=acc.sum_charged / years,
            years=yrs, storage_years=sty, year_weather=wy)
end

"G[1 .. nhours + 1], the cumulative table of one row of failure-rate multipliers (relmc_hl1_stress_cumulative: host only, no engine needed)"
function stress_cumulative(fail_mult_row::Vector{Float64})
    cum = Vector{Float64}(undef, length(fail_mult_row) + 1)
    rc = ccall((:relmc_hl1_stress_cumulative, LIB), Int32, (Int32, Ptr{Cdouble}, Ptr{Cdouble}), length(fail_mult_row), fail_mult_row, cum)
    rc == 0 || throw(ArgumentError("the multipliers must be finite and not negative"))
    return cum
end

"""
The chain time at which a unit of a stressed class fails that became UP at chain time `t` with the draw `e` = -mttf * ln U
(relmc_hl1_stress_failure_time: host only, no engine needed).  weather[year] is the 0-based weather year of every chain year,
cum[hour + 1, weather year] the cumulative tables of the unit's class.  years * nhours + 1: not within the chain.
"""
stress_failure_time(t::Real, e::Real, weather::Vector{Int32}, cum::Matrix{Float64}) =
    ccall((:relmc_hl1_stress_failure_time, LIB), Cdouble, (Cdouble, Cdouble, Int32, Int32, Ptr{Int32}, Ptr{Cdouble}),
          t, e, size(cum, 1) - 1, length(weather), weather, cum)

"relmc_hl1_ms_unit (include/relmc.h, 64 bytes): a three-state unit, UP / DERATED / DOWN: capacities in MW, per state the mean holding time in hours and the probability of the first-listed destination (from UP: DOWN, DERATED; from DERATED: UP, DOWN; from DOWN: UP, DERATED)"
struct Hl1MsUnit
    capacity_mw::Cdouble; derated_mw::Cdouble; mean_h::NTuple{3,Cdouble}; first_p::NTuple{3,Cdouble}
end
"relmc_hl1_ms_year: unit-hours of one simulated year spent DERATED and DOWN, over the fleet"
struct Hl1MsYear
    derated_unit_h::Cdouble; down_unit_h::Cdouble
end
mutable struct Hl1MsAcc
    years::Int64; sum_lole::Cdouble; sum_eue::Cdouble; sum_lolf::Cdouble; sum_lole2::Cdouble; sum_eue2::Cdouble; sum_lolf2::Cdouble
    sum_derated::Cdouble; sum_down::Cdouble; sum_derated2::Cdouble; sum_down2::Cdouble
    Hl1MsAcc() = new()
end
"A two-state unit as a three-state one: mttf / mttr verbatim as the means of UP and DOWN, DERATED never reached"
two_state_unit(capacity::Real, mttf::Real, mttr::Real) =
    Hl1MsUnit(Float64(capacity), 0.0, (Float64(mttf), 1.0, Float64(mttr)), (1.0, 1.0, 1.0))

"""
run_sequential_multistate (an extension beyond the reference): run_sequential_mc's chronology with units that have a derated state.
Units whose first_p are (1, any, 1) are two-state, and a fleet of them gives run_sequential_mc's year records bit for bit.  Returns LOLE,
EUE and LOLF, the unit-hours per year spent DERATED and DOWN, and the per-year records.
"""
function run_sequential_multistate(eng::Engine, units::Vector{Hl1MsUnit}, hourly_load::Vector{Float64}, years::Integer;
                                   seed::Integer=1, chains::Integer=1, start::Symbol=:all_up)
    (years >= 1 && chains >= 1 && years % chains == 0) || throw(ArgumentError("years must be a positive multiple of chains"))
    check(ccall((:relmc_hl1_ms_load, LIB), Int32, (Ptr{Cvoid}, Int32, Ptr{Hl1MsUnit}, Int32, Ptr{Cdouble}),
                eng.h, length(units), units, length(hourly_load), hourly_load), eng.h, "relmc_hl1_ms_load")
    acc = Hl1MsAcc()
    yrs = Vector{Hl1SeqYear}(undef, years); sty = Vector{Hl1MsYear}(undef, years)
    check(ccall((:relmc_hl1_ms_seq, LIB), Int32,
                (Ptr{Cvoid}, UInt64, UInt64, Int64, Int32, Int32, Ref{Hl1MsAcc}, Ptr{Hl1SeqYear}, Ptr{Hl1MsYear}),
                eng.h, seed, 0, chains, years ÷ chains, HL1_START[start], acc, yrs, sty), eng.h, "relmc_hl1_ms_seq")
    return (lole_hours_yr=acc.sum_lole / years, eue_mwh_yr=acc.sum_eue / years, lolf_occ_yr=acc.sum_lolf / years,
            derated_unit_h_yr=acc.sum_derated / years, down_unit_h_yr=acc.sum_down / years, years=yrs, state_years=sty)
end

# Layout of the HL1 sequential structs, kept apart from LAYOUT (tests/test_hl1_seq_host.py compares it with the C compiler's)
const LAYOUT_HL1_SEQ = [
    ("relmc_hl1_seq_year", 24, [("lole", 0), ("eue", 8), ("lolf", 16)]),
    ("relmc_hl1_seq_acc", 56, [("years", 0), ("sum_lole", 8), ("sum_eue", 16), ("sum_lolf", 24), ("sum_lole2", 32), ("sum_eue2", 40), ("sum_lolf2", 48)]),
]

"""
run_monte_carlo_simulation (generating_adequancy_comparative.jl:15-120, tail_risk.jl:12-91): the HL1 planning model's Monte Carlo on the
GPU.  `outage_start` are 1-based maintenance start weeks (0 = none), `energy_limit` MWh per year (Inf = not energy-limited, at most 8
ELUs), `lfu_sigma_mw` the LFU standard deviation.  Returns LOLE, EUE, LOLF, the per-year indices, the hourly loss probability and the
MWh used per ELU per year (n_years x n_elu).
"""
function run_planning_mc(eng::Engine, capacity::Vector{Float64}, for_rate::Vector{Float64}, outage_start::Vector{Int32},
                         outage_weeks::Vector{Int32}, energy_limit::Vector{Float64}, hourly_load::Vector{Float64}, lfu_sigma_mw::Float64,
                         n_years::Integer; seed::Integer=1)
    n_years >= 1 || throw(ArgumentError("n_years must be positive"))
    check(ccall((:relmc_hl1_plan_load, LIB), Int32, (Ptr{Cvoid}, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}, Ptr{Int32}, Ptr{Cdouble},
                                                     Int32, Ptr{Cdouble}, Cdouble),
                eng.h, length(capacity), capacity, for_rate, outage_start, outage_weeks, energy_limit, length(hourly_load), hourly_load,
                lfu_sigma_mw), eng.h, "relmc_hl1_plan_load")
    n_elu = count(isfinite, energy_limit)
    acc = Hl1SeqAcc(); yrs = Vector{Hl1SeqYear}(undef, n_years); hours = zeros(Int64, length(hourly_load))
    elu = zeros(Float64, n_elu, n_years)                                   # column-major: column y = the C record [y][n_elu]
    check(ccall((:relmc_hl1_plan, LIB), Int32, (Ptr{Cvoid}, UInt64, UInt64, Int64, Ref{Hl1SeqAcc}, Ptr{Hl1SeqYear}, Ptr{Int64}, Ptr{Cdouble}),
                eng.h, seed, 0, n_years, acc, yrs, hours, n_elu > 0 ? elu : C_NULL), eng.h, "relmc_hl1_plan")
    year_lole = [y.lole for y in yrs]; cum = cumsum(year_lole)
    return (lole_hours_yr=acc.sum_lole / n_years, eue_mwh_yr=acc.sum_eue / n_years, lolf_occ_yr=acc.sum_lolf / n_years,
            year_lole=year_lole, year_eue=[y.eue for y in yrs], year_lolf=[y.lolf for y in yrs],
            hourly_loss_prob=hours ./ n_years, elu_energy=permutedims(elu),
            lole_history=[cum[k] / k for k in 100:100:n_years])                 # comparative.jl:114-116
end

const AREA_MAX = 8                                                            # RELMC_AREA_MAX
const HL1_AREA_POLICY = Dict(:isolated => Int32(0), :interconnected => Int32(1))   # RELMC_HL1_AREA_ISOLATED / _INTERCONNECTED
const HL1_AREA_FLOW = Dict(:reference => Int32(0), :max_flow => Int32(1))         # RELMC_HL1_AREA_FLOW_*
const HL1_TIE_MAX = 32                                                        # RELMC_HL1_TIE_MAX
const HL1_TIE_DRAW_BASE = 128                                                 # RELMC_HL1_TIE_DRAW_BASE

"""
run_fast_sequential_simulation (AdequacyAssessmentII.jl:185-250): the multi-area chronology on the GPU.  `units_per_area` counts the
units of each area; `capacity`, `mttf`, `mttr` are area-major; `hourly_load` is n_areas x nhours; ties are 1-based (from, to, capacity)
as the reference's TieLine.  policy :isolated or :interconnected, flow :reference (the reference's loop) or :max_flow.  Returns per-area
LOLE, EUE, LOLF, the system row (a loss hour in any area) and the per-year indices (years x (n_areas + 1) x 3, chain-major).
`tie_mttf` / `tie_mttr` (hours, one per tie; an extension, the reference's ties never fail): ties with a finite MTTF fail and repair like
units (relmc_hl1_area_tie_outages), `Inf` = never; without them no tie fails.
"""
function run_fast_sequential_simulation(eng::Engine, units_per_area::Vector{Int32}, capacity::Vector{Float64}, mttf::Vector{Float64},
                                        mttr::Vector{Float64}, hourly_load::Matrix{Float64}, tie_from::Vector{Int32}, tie_to::Vector{Int32},
                                        tie_capacity::Vector{Float64}, policy::Symbol, n_years::Integer; seed::Integer=1, chains::Integer=1,
                                        start::Symbol=:all_up, flow::Symbol=:reference,
                                        tie_mttf::Union{Nothing,Vector{Float64}}=nothing, tie_mttr::Union{Nothing,Vector{Float64}}=nothing)
    (n_years >= 1 && chains >= 1 && n_years % chains == 0) || throw(ArgumentError("n_years must be a positive multiple of chains"))
    (tie_mttf === nothing) == (tie_mttr === nothing) || throw(ArgumentError("tie_mttf and tie_mttr go together"))
    tie_mttf === nothing || (length(tie_mttf) == length(tie_mttr) == length(tie_from) <= HL1_TIE_MAX) ||
        throw(ArgumentError("one tie_mttf / tie_mttr per tie, $HL1_TIE_MAX ties at most"))
    n = length(units_per_area)
    (1 <= n <= AREA_MAX && size(hourly_load, 1) == n) || throw(ArgumentError("1..$AREA_MAX areas, one load row per area"))
    load = Matrix(permutedims(hourly_load))                                  # column-major n x H -> the C layout [n_areas][nhours]
    check(ccall((:relmc_hl1_area_load, LIB), Int32, (Ptr{Cvoid}, Int32, Ptr{Int32}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int32,
                                                     Ptr{Cdouble}, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Cdouble}),
                eng.h, n, units_per_area, capacity, mttf, mttr, size(hourly_load, 2), load, length(tie_from), tie_from .- Int32(1),
                tie_to .- Int32(1), tie_capacity), eng.h, "relmc_hl1_area_load")
    if tie_mttf !== nothing && any(isfinite, tie_mttf)                        # the load has removed any earlier outage data
        check(ccall((:relmc_hl1_area_tie_outages, LIB), Int32, (Ptr{Cvoid}, Int32, Ptr{Cdouble}, Ptr{Cdouble}),
                    eng.h, length(tie_mttf), tie_mttf, tie_mttr), eng.h, "relmc_hl1_area_tie_outages")
    end
    acc = zeros(Float64, 7, n + 1)           # relmc_hl1_seq_acc[n + 1]: column r = one 56-byte record (row 1 holds the Int64 count)
    yrs = Vector{Hl1SeqYear}(undef, n_years * (n + 1))
    check(ccall((:relmc_hl1_area, LIB), Int32, (Ptr{Cvoid}, UInt64, UInt64, Int64, Int32, Int32, Int32, Int32, Ptr{Cdouble},
                                                Ptr{Hl1SeqYear}),
                eng.h, seed, 0, chains, n_years ÷ chains, HL1_START[start], HL1_AREA_POLICY[policy], HL1_AREA_FLOW[flow], acc, yrs),
          eng.h, "relmc_hl1_area")
    sums = permutedims(acc[2:4, :])                                          # [row, (sum_lole, sum_eue, sum_lolf)]
    y = reshape(yrs, n + 1, n_years)
    return (lole=sums[1:n, 1] ./ n_years, eue=sums[1:n, 2] ./ n_years, lolf=sums[1:n, 3] ./ n_years,
            system_lole=sums[n + 1, 1] / n_years, system_eue=sums[n + 1, 2] / n_years, system_lolf=sums[n + 1, 3] / n_years,
            year_indices=[getfield(y[r, t], f) for t in 1:n_years, r in 1:n + 1, f in (:lole, :eue, :lolf)])
end

"relmc_hl1_area_level (include/relmc.h): one level of relmc_hl1_area_sweep; fleet 0 = every unit, 1 = without the withheld units"
struct Hl1AreaLevel
    load_scale::NTuple{8,Cdouble}; load_shift::NTuple{8,Cdouble}; tie_scale::Cdouble; fleet::Int32; reserved::Int32
end
const HL1_AREA_SWEEP_MAX_LEVELS = 8                                           # RELMC_HL1_AREA_SWEEP_MAX_LEVELS

"""
run_area_sweep (an extension beyond the reference): the INTERCONNECTED chronology of the model that run_fast_sequential_simulation loaded
last on this engine (tie outages included), same chains under one seed, against up to 8 levels in one walk of the chains.  `levels`
holds (load_scale, load_shift, tie_scale, withheld) with one scale and one shift per area: area a sees load_scale[a] * load + load_shift[a],
every scaled tie tie_scale times its capacity and, if withheld, the fleet without the units `withheld_units` (1-based global indices).
`scaled_ties` (1-based) are the ties tie_scale applies to (default: all).  Returns LOLE, EUE and LOLF as n_levels x (n_areas + 1) (the last
column is the system) and the per-year indices (n_levels x years x (n_areas + 1) x 3).  Only the system row under :max_flow is monotone in
load and tie capacity.
"""
function run_area_sweep(eng::Engine, n_areas::Integer, n_ties::Integer, n_years::Integer,
                        levels::Vector{<:Tuple{Vector{Float64},Vector{Float64},Real,Bool}};
                        withheld_units::Vector{<:Integer}=Int[], scaled_ties::Union{Nothing,Vector{<:Integer}}=nothing, seed::Integer=1,
                        chains::Integer=1, start::Symbol=:all_up, flow::Symbol=:max_flow)
    (n_years >= 1 && chains >= 1 && n_years % chains == 0) || throw(ArgumentError("n_years must be a positive multiple of chains"))
    nl = length(levels)
    1 <= nl <= HL1_AREA_SWEEP_MAX_LEVELS || throw(ArgumentError("between 1 and $HL1_AREA_SWEEP_MAX_LEVELS levels"))
    1 <= n_areas <= AREA_MAX || throw(ArgumentError("1..$AREA_MAX areas"))
    all(length(l[1]) == n_areas && length(l[2]) == n_areas for l in levels) || throw(ArgumentError("one load scale and shift per area"))
    all(1 <= k <= 128 for k in withheld_units) || throw(ArgumentError("withheld_units must be unit indices"))
    (isempty(withheld_units) && any(l[4] for l in levels)) && throw(ArgumentError("a withheld level needs withheld_units"))
    pad(v) = ntuple(i -> i <= n_areas ? Float64(v[i]) : 0.0, 8)
    lv = [Hl1AreaLevel(pad(l[1]), pad(l[2]), Float64(l[3]), l[4] ? Int32(1) : Int32(0), Int32(0)) for l in levels]
    mask = zeros(UInt32, 4)
    for k in withheld_units
        mask[((k - 1) >> 5) + 1] |= UInt32(1) << ((k - 1) & 31)
    end
    tmask = zeros(UInt8, max(n_ties, 1))
    if scaled_ties !== nothing
        all(1 <= t <= n_ties for t in scaled_ties) || throw(ArgumentError("scaled_ties must be tie indices"))
        tmask[scaled_ties] .= 0x01
    end
    rows = n_areas + 1
    yrs = Vector{Hl1SeqYear}(undef, nl * n_years * rows)
    raw = zeros(UInt8, 56 * nl * rows)                                        # relmc_hl1_seq_acc[nl][rows], contiguous
    check(ccall((:relmc_hl1_area_sweep, LIB), Int32,
                (Ptr{Cvoid}, UInt64, UInt64, Int64, Int32, Int32, Int32, Int32, Ptr{Hl1AreaLevel}, Ptr{UInt32}, Ptr{UInt8}, Ptr{UInt8},
                 Ptr{Hl1SeqYear}),
                eng.h, seed, 0, chains, n_years ÷ chains, HL1_START[start], HL1_AREA_FLOW[flow], nl, lv,
                isempty(withheld_units) ? C_NULL : mask, scaled_ties === nothing ? C_NULL : tmask, raw, yrs),
          eng.h, "relmc_hl1_area_sweep")
    sums = reshape(reinterpret(Float64, raw), 7, rows, nl)                    # rows 2 .. 4: sum_lole, sum_eue, sum_lolf
    Y = reshape(yrs, rows, n_years, nl)
    return (lole=[sums[2, r, j] / n_years for j in 1:nl, r in 1:rows], eue=[sums[3, r, j] / n_years for j in 1:nl, r in 1:rows],
            lolf=[sums[4, r, j] / n_years for j in 1:nl, r in 1:rows],
            year_indices=[getfield(Y[r, t, j], f) for j in 1:nl, t in 1:n_years, r in 1:rows, f in (:lole, :eue, :lolf)])
end

# Layout of the multi-area sweep level, kept apart from LAYOUT (tests/test_hl1_area_sweep_host.py compares it with the C compiler's and
# with ctypes)
const LAYOUT_HL1_AREA_SWEEP = [
    ("relmc_hl1_area_level", 144, [("load_scale", 0), ("load_shift", 64), ("tie_scale", 128), ("fleet", 136), ("reserved", 140)]),
]

"relmc_hl1_area_var_opts (include/relmc.h, 208 bytes): the options of relmc_hl1_area_var; resource_scale finite and >= 0 (0 beyond the library's resources), load_scale / load_shift per area (1 / 0 beyond the model's areas), policy = HL1_AREA_POLICY[...], flow = HL1_AREA_FLOW[...], pick = HL1_VAR_PICK[...], reserved = 0"
struct Hl1AreaVarOpts
    resource_scale::NTuple{8,Cdouble}; load_scale::NTuple{8,Cdouble}; load_shift::NTuple{8,Cdouble}; policy::Int32; flow::Int32; pick::Int32; reserved::Int32
end
"relmc_hl1_area_storage (include/relmc.h, 56 bytes): the storage `s` in the 0-based area `area`; reserved = 0"
struct Hl1AreaStorage
    s::Hl1Storage; area::Int32; reserved::Int32
end

# Layout of the two structs, kept apart from LAYOUT (tests/test_hl1_area_variable_host.py compares it with the C compiler's and with ctypes)
const LAYOUT_HL1_AREA_VAR = [
    ("relmc_hl1_area_var_opts", 208, [("resource_scale", 0), ("load_scale", 64), ("load_shift", 128), ("policy", 192), ("flow", 196), ("pick", 200), ("reserved", 204)]),
    ("relmc_hl1_area_storage", 56, [("s", 0), ("area", 48), ("reserved", 52)]),
]

"""
run_area_variable (an extension beyond the reference): the chronology of the model that run_fast_sequential_simulation loaded last on
this engine (tie outages included), same chains under one seed, with weather-year resources and storages in the areas.
output_mw[hour, resource, weather year] (column-major: the C ABI's [n_weather][n_resources][nhours]) holds the hourly output of every
resource, resource_area[r] its 1-based area, weather_load[hour, area, weather year] optionally every area's load curve of every weather
year; storages are (1-based area, Hl1Storage) pairs, those of one area acting in the order given.  Per step the areas help each other
over the ties first; each area's storages then serve what is left of its deficit or charge from what is left of its surplus.  Returns
per row (areas, then the system) LOLE, EUE, LOLF, served hours and MWh discharged / charged per year, the per-year records
(years x (n_areas + 1) x 3, twice) and the weather year (0-based) of every simulated year.
"""
function run_area_variable(eng::Engine, n_areas::Integer, policy::Symbol, output_mw::Array{Float64,3}, resource_area::Vector{<:Integer},
                           n_years::Integer; weather_load::Union{Nothing,Array{Float64,3}}=nothing,
                           storages::Vector{<:Tuple{Integer,Hl1Storage}}=Tuple{Int,Hl1Storage}[],
                           resource_scale::Vector{Float64}=ones(size(output_mw, 2)), load_scale::Vector{Float64}=ones(n_areas),
                           load_shift::Vector{Float64}=zeros(n_areas), pick::Symbol=:random, flow::Symbol=:reference, seed::Integer=1,
                           chains::Integer=1, start::Symbol=:all_up)
    (n_years >= 1 && chains >= 1 && n_years % chains == 0) || throw(ArgumentError("n_years must be a positive multiple of chains"))
    1 <= n_areas <= AREA_MAX || throw(ArgumentError("1..$AREA_MAX areas"))
    nh, nres, nw = size(output_mw)
    nres <= HL1_VAR_MAX_RESOURCES || throw(ArgumentError("at most $HL1_VAR_MAX_RESOURCES resources"))
    1 <= nw <= HL1_VAR_MAX_WEATHER || throw(ArgumentError("1 to $HL1_VAR_MAX_WEATHER weather years"))
    (length(resource_area) == nres && all(1 <= a <= n_areas for a in resource_area)) || throw(ArgumentError("one 1-based area per resource"))
    length(resource_scale) == nres || throw(ArgumentError("one resource_scale per resource"))
    (length(load_scale) == n_areas && length(load_shift) == n_areas) || throw(ArgumentError("one load scale and shift per area"))
    weather_load === nothing || size(weather_load) == (nh, n_areas, nw) || throw(ArgumentError("weather_load must be [hours, areas, weather years]"))
    length(storages) <= HL1_MAX_STORAGE || throw(ArgumentError("at most $HL1_MAX_STORAGE storages"))
    all(1 <= s[1] <= n_areas for s in storages) || throw(ArgumentError("a storage's area must be one of 1..$n_areas"))
    check(ccall((:relmc_hl1_area_var_load, LIB), Int32, (Ptr{Cvoid}, Int32, Int32, Int32, Ptr{Int32}, Int32, Ptr{Cdouble}, Ptr{Cdouble}),
                eng.h, n_areas, nw, nres, nres == 0 ? C_NULL : Int32.(resource_area .- 1), nh, nres == 0 ? C_NULL : output_mw,
                weather_load === nothing ? C_NULL : weather_load), eng.h, "relmc_hl1_area_var_load")
    opts = Ref(Hl1AreaVarOpts(ntuple(r -> r <= nres ? resource_scale[r] : 0.0, 8), ntuple(a -> a <= n_areas ? load_scale[a] : 1.0, 8),
                              ntuple(a -> a <= n_areas ? load_shift[a] : 0.0, 8), HL1_AREA_POLICY[policy], HL1_AREA_FLOW[flow],
                              HL1_VAR_PICK[pick], Int32(0)))
    st = [Hl1AreaStorage(s[2], Int32(s[1] - 1), Int32(0)) for s in storages]
    rows = n_areas + 1
    raw = zeros(UInt8, 104 * rows)                                            # relmc_hl1_storage_acc[rows], contiguous
    yrs = Vector{Hl1SeqYear}(undef, n_years * rows); sty = Vector{Hl1StorageYear}(undef, n_years * rows); wy = Vector{Int32}(undef, n_years)
    check(ccall((:relmc_hl1_area_var, LIB), Int32,
                (Ptr{Cvoid}, UInt64, UInt64, Int64, Int32, Int32, Ref{Hl1AreaVarOpts}, Int32, Ptr{Hl1AreaStorage}, Ptr{UInt8}, Ptr{Hl1SeqYear},
                 Ptr{Hl1StorageYear}, Ptr{Int32}),
                eng.h, seed, 0, chains, n_years ÷ chains, HL1_START[start], opts, length(st), isempty(st) ? C_NULL : st, raw, yrs, sty, wy),
          eng.h, "relmc_hl1_area_var")
    sums = reshape(reinterpret(Float64, raw), 13, rows)                       # rows 2 .. 4: sum_lole, sum_eue, sum_lolf; 8 .. 10: served, discharged, charged
    Y = reshape(yrs, rows, n_years); S = reshape(sty, rows, n_years)
    return (lole=sums[2, :] ./ n_years, eue=sums[3, :] ./ n_years, lolf=sums[4, :] ./ n_years,
            served_hours=sums[8, :] ./ n_years, discharged_mwh=sums[9, :] ./ n_years, charged_mwh=sums[10, :] ./ n_years,
            year_indices=[getfield(Y[r, t], f) for t in 1:n_years, r in 1:rows, f in (:lole, :eue, :lolf)],
            year_storage=[getfield(S[r, t], f) for t in 1:n_years, r in 1:rows, f in (:served_hours, :discharged_mwh, :charged_mwh)],
            year_weather=wy)
end

# Structs the HL1 planning wrappers pass (the planning calls reuse the sequential model's records; no struct of their own), checked
# against the C compiler by tests/test_hl1_plan_host.py
const LAYOUT_HL1_PLAN = [
    ("relmc_hl1_seq_year", 24, [("lole", 0), ("eue", 8), ("lolf", 16)]),
    ("relmc_hl1_seq_acc", 56, [("years", 0), ("sum_lole", 8), ("sum_eue", 16), ("sum_lolf", 24), ("sum_lole2", 32), ("sum_eue2", 40), ("sum_lolf2", 48)]),
]

# ---- importance sampling for the non-sequential track (include/relmc.h: cross-entropy tilt of the unavailabilities) ----------------

const IS_TUNE_MAX_PASSES = 32                                                 # RELMC_IS_TUNE_MAX_PASSES

"relmc_is_acc (include/relmc.h): the weighted accumulators of a tilted sample range"
mutable struct IsAcc
    n::Int64; n_fail::Int64; n_singular::Int64; n_infeasible::Int64; n_nonconverged::Int64; sum_iters::Int64
    sum_w::Cdouble; sum_w2::Cdouble; sum_wfail::Cdouble; sum_w2fail::Cdouble; sum_wdns::Cdouble; sum_w2dns2::Cdouble
    comp_wfail::NTuple{MAX_COMP,Cdouble}
    comp_wdns::NTuple{MAX_COMP,Cdouble}
    sum_wnodal::NTuple{MAX_BUS,Cdouble}
    IsAcc() = new()
end

"relmc_is_indices (include/relmc.h)"
mutable struct IsIndices
    n::Int64
    edns::Cdouble; lole::Cdouble; plc::Cdouble; beta::Cdouble; eens::Cdouble; mean_iters::Cdouble
    beta_plc::Cdouble; mean_w::Cdouble; ess::Cdouble
    nodal_eens::NTuple{MAX_BUS,Cdouble}
    comp_importance::NTuple{MAX_COMP,Cdouble}
    IsIndices() = new()
end

"relmc_is_tune_opts (include/relmc.h): the options of the cross-entropy tuner"
struct IsTuneOpts
    seed::UInt64; n_pilot::Int64; max_iters::Int32; final_iters::Int32; min_elite::Int64; rho::Cdouble
    objective::Int32; reserved::Int32; alpha::Cdouble; q_max::Cdouble
    solver::SolverOptsC
end

"relmc_is_tune_report (include/relmc.h)"
mutable struct IsTuneReport
    passes::Int32; final_passes::Int32
    n_fail::NTuple{IS_TUNE_MAX_PASSES,Int64}; n_elite::NTuple{IS_TUNE_MAX_PASSES,Int64}
    sum_e::NTuple{IS_TUNE_MAX_PASSES,Cdouble}; level::NTuple{IS_TUNE_MAX_PASSES,Cdouble}
    kernel_seconds::Cdouble; wall_seconds::Cdouble
    IsTuneReport() = new()
end

"relmc_is_run_opts (include/relmc.h)"
struct IsRunOpts
    beta_limit::Cdouble; max_samples::Int64; batch::Int64; seed::UInt64; hours_per_year::Cdouble
    solver::SolverOptsC
    unavail_is::Ptr{Cdouble}
    history_cap::Int64
    beta_history::Ptr{Cdouble}; edns_history::Ptr{Cdouble}; plc_history::Ptr{Cdouble}
end

# relmc_is_run_result is read out of a byte buffer at these offsets (IsAcc and IsIndices are mutable mirrors and cannot be embedded)
const IS_ACC_BYTES = 8 * (12 + 2 * MAX_COMP + MAX_BUS)
const IS_INDICES_BYTES = 8 * (10 + MAX_BUS + MAX_COMP)
const IS_RUN_TAIL = IS_ACC_BYTES + IS_INDICES_BYTES                           # checkpoints, batches, converged, reserved, wall_seconds, kernel_seconds
const IS_RUN_BYTES = IS_RUN_TAIL + 40

tilt_ptr(eng::Engine, unavail_is) = unavail_is === nothing ? Ptr{Cdouble}(C_NULL) :
    (length(unavail_is) == eng.sys.ng + eng.sys.nl ? pointer(unavail_is) : throw(ArgumentError("unavail_is must have Ng+Nl entries")))

"(eqstatus n x (Ng+Nl), W): relmc_mc_sampling's draws against the tilted unavailabilities (`nothing` = the case's own) and their likelihood ratios."
function is_sampling(eng::Engine, seed::Integer, first_index::Integer, n::Integer; unavail_is::Union{Nothing,Vector{Float64}}=nothing)
    ncomp = eng.sys.ng + eng.sys.nl
    out = Matrix{UInt8}(undef, ncomp, n); w = Vector{Float64}(undef, n)
    GC.@preserve unavail_is check(ccall((:relmc_is_sampling, LIB), Int32, (Ptr{Cvoid}, UInt64, UInt64, Int64, Ptr{Cdouble}, Ptr{UInt8}, Ptr{Cdouble}),
                                        eng.h, seed, first_index, n, tilt_ptr(eng, unavail_is), out, w), eng.h, "relmc_is_sampling")
    return permutedims(out), w
end

"Tilted samples [first_index, first_index+n), evaluated and reduced with their weights (relmc_nsq_is_accumulate)."
function nsq_is_accumulate(eng::Engine, seed::Integer, first_index::Integer, n::Integer; unavail_is::Union{Nothing,Vector{Float64}}=nothing,
                           mpopt::SolverOpts=mpoption())
    acc = IsAcc()
    GC.@preserve unavail_is check(ccall((:relmc_nsq_is_accumulate, LIB), Int32,
                                        (Ptr{Cvoid}, UInt64, UInt64, Int64, Ref{SolverOpts}, Ptr{Cdouble}, Ref{IsAcc}),
                                        eng.h, seed, first_index, n, mpopt, tilt_ptr(eng, unavail_is), acc), eng.h, "relmc_nsq_is_accumulate")
    return acc
end

function is_indices(eng::Engine, acc::IsAcc; hours_per_year=8760.0)
    out = IsIndices()
    ccall((:relmc_nsq_is_indices, LIB), Cvoid, (Ref{IsAcc}, Int32, Int32, Cdouble, Ref{IsIndices}),
          acc, eng.sys.nb, eng.sys.ng + eng.sys.nl, hours_per_year, out)
    return out
end

"The cross-entropy tuner (relmc_nsq_is_tune): (unavail_is, IsTuneReport).  objective :plc or :edns."
function is_tune(eng::Engine; objective::Symbol=:edns, seed::Integer=1, n_pilot::Integer=20000, max_iters::Integer=5, final_iters::Integer=2,
                 min_elite::Integer=100, rho::Real=0.1, alpha::Real=1.0, q_max::Real=0.5, mpopt::SolverOpts=mpoption())
    o = IsTuneOpts(seed, n_pilot, max_iters, final_iters, min_elite, rho, objective == :plc ? Int32(0) : Int32(1), Int32(0), alpha, q_max,
                   SolverOptsC(mpopt))
    q = zeros(Float64, eng.sys.ng + eng.sys.nl); rep = IsTuneReport()
    check(ccall((:relmc_nsq_is_tune, LIB), Int32, (Ptr{Cvoid}, Ref{IsTuneOpts}, Ptr{Cdouble}, Ref{IsTuneReport}), eng.h, Ref(o), q, rep),
          eng.h, "relmc_nsq_is_tune")
    return q, rep
end

"Batches under the tilt until beta <= beta_limit or max_samples (relmc_nsq_is_run); tunes first when no tilt is given."
function nsq_is_run(eng::Engine; unavail_is::Union{Nothing,Vector{Float64}}=nothing, beta_limit::Real=0.0017, max_samples::Integer=100000,
                    batch::Integer=1000, seed::Integer=1, mpopt::SolverOpts=mpoption(), hours_per_year::Real=8760.0)
    q = unavail_is === nothing ? is_tune(eng; seed=seed + 1, mpopt=mpopt)[1] : unavail_is
    ncp = cld(max_samples, batch)
    hb = zeros(ncp); he = zeros(ncp); hp = zeros(ncp)
    raw = zeros(UInt8, IS_RUN_BYTES)
    GC.@preserve q hb he hp begin
        o = IsRunOpts(beta_limit, max_samples, batch, seed, hours_per_year, SolverOptsC(mpopt), tilt_ptr(eng, q), ncp, pointer(hb), pointer(he), pointer(hp))
        check(ccall((:relmc_nsq_is_run, LIB), Int32, (Ptr{Cvoid}, Ref{IsRunOpts}, Ptr{UInt8}), eng.h, Ref(o), raw), eng.h, "relmc_nsq_is_run")
    end
    f64(off) = reinterpret(Float64, raw[off + 1:off + 8])[1]; i64(off) = reinterpret(Int64, raw[off + 1:off + 8])[1]
    k = i64(IS_RUN_TAIL)
    return (n=i64(IS_ACC_BYTES), edns=f64(IS_ACC_BYTES + 8), lole=f64(IS_ACC_BYTES + 16), plc=f64(IS_ACC_BYTES + 24), beta=f64(IS_ACC_BYTES + 32),
            beta_plc=f64(IS_ACC_BYTES + 56), mean_w=f64(IS_ACC_BYTES + 64), ess=f64(IS_ACC_BYTES + 72),
            converged=reinterpret(Int32, raw[IS_RUN_TAIL + 17:IS_RUN_TAIL + 20])[1] != 0, wall_seconds=f64(IS_RUN_TAIL + 24),
            kernel_seconds=f64(IS_RUN_TAIL + 32), beta_history=hb[1:k], edns_history=he[1:k], plc_history=hp[1:k], unavail_is=q)
end

# Layout of the importance-sampling structs, kept apart from LAYOUT (tests/test_importance_host.py compares it with the C compiler's and with ctypes)
const LAYOUT_IS = [
    ("relmc_is_acc", IS_ACC_BYTES, [("n", 0), ("sum_iters", 40), ("sum_w", 48), ("sum_w2dns2", 88), ("comp_wfail", 96), ("comp_wdns", 96 + 8 * MAX_COMP), ("sum_wnodal", 96 + 16 * MAX_COMP)]),
    ("relmc_is_indices", IS_INDICES_BYTES, [("n", 0), ("edns", 8), ("mean_iters", 48), ("beta_plc", 56), ("mean_w", 64), ("ess", 72), ("nodal_eens", 80), ("comp_importance", 80 + 8 * MAX_BUS)]),
    ("relmc_is_tune_opts", 152, [("seed", 0), ("n_pilot", 8), ("max_iters", 16), ("final_iters", 20), ("min_elite", 24), ("rho", 32), ("objective", 40), ("reserved", 44), ("alpha", 48), ("q_max", 56), ("solver", 64)]),
    ("relmc_is_tune_report", 16 + 32 * IS_TUNE_MAX_PASSES + 8, [("passes", 0), ("final_passes", 4), ("n_fail", 8), ("n_elite", 8 + 8 * IS_TUNE_MAX_PASSES), ("sum_e", 8 + 16 * IS_TUNE_MAX_PASSES), ("level", 8 + 24 * IS_TUNE_MAX_PASSES), ("kernel_seconds", 8 + 32 * IS_TUNE_MAX_PASSES), ("wall_seconds", 16 + 32 * IS_TUNE_MAX_PASSES)]),
    ("relmc_is_run_opts", 168, [("beta_limit", 0), ("max_samples", 8), ("batch", 16), ("seed", 24), ("hours_per_year", 32), ("solver", 40), ("unavail_is", 128), ("history_cap", 136), ("beta_history", 144), ("edns_history", 152), ("plc_history", 160)]),
    ("relmc_is_run_result", IS_RUN_BYTES, [("acc", 0), ("idx", IS_ACC_BYTES), ("checkpoints", IS_RUN_TAIL), ("batches", IS_RUN_TAIL + 8), ("converged", IS_RUN_TAIL + 16), ("reserved", IS_RUN_TAIL + 20), ("wall_seconds", IS_RUN_TAIL + 24), ("kernel_seconds", IS_RUN_TAIL + 32)]),
]

# Layout table of the plain-C structs this file mirrors: tests/test_c_abi.py compiles a C program printing sizeof / offsetof of
# include/relmc.h's structs and compares with these numbers and with the ctypes mirror, so drift in either mirror is caught
# without a Julia installation.  (name, sizeof, [(field, offset) ...])
const LAYOUT = [
    ("relmc_case_desc", 128, [("base_mva", 0), ("nb", 8), ("ref_bus", 24), ("bus_pd", 32), ("always_up", 112), ("total_load", 120)]),
    ("relmc_solver_opts", 88, [("singular_policy", 0), ("max_it", 4), ("feastol", 8), ("max_stepsize", 72), ("screen", 80)]),
    ("relmc_acc", 8 * (7 + MAX_COMP + 2 + MAX_BUS), [("n", 0), ("comp_fail", 48), ("n_screened", 48 + 8 * MAX_COMP), ("sum_dns", 56 + 8 * MAX_COMP), ("sum_nodal", 72 + 8 * MAX_COMP)]),
    ("relmc_indices", 8 * (7 + MAX_BUS + MAX_COMP), [("n", 0), ("edns", 8), ("nodal_eens", 56), ("comp_importance", 56 + 8 * MAX_BUS)]),
    ("relmc_db_stats", 32, [("rows", 0), ("samples", 8), ("new_rows", 16), ("batch_distinct", 24)]),
    ("relmc_seq_year", 32, [("ens", 0), ("dlc", 8), ("nlc", 16), ("n_contingency", 24)]),
    ("relmc_hl1_acc", 40, [("n", 0), ("sum_lole", 8), ("sum_eue2", 32)]),
    ("relmc_nsq_opts", 176, [("beta_limit", 0), ("max_samples", 8), ("batch", 16), ("seed", 24), ("hours_per_year", 32), ("solver", 40), ("history_cap", 128), ("beta_history", 136), ("plc_history", 160), ("distinct_states", 168)]),
    ("relmc_seq_opts", 152, [("cov_threshold", 0), ("max_years", 8), ("batch_years", 12), ("seed", 16), ("curtail_threshold", 24), ("solver", 32), ("years_cap", 120), ("results_year", 128), ("cum_cov", 144)]),
    ("relmc_seq_result", SEQ_RESULT_BYTES, [("final_year", 0), ("converged", 4), ("eens", 8), ("plc", 40), ("n_contingency", 48), ("acc", SEQ_RESULT_ACC), ("nodal_eens_avg", SEQ_RESULT_NODAL), ("comp_importance", SEQ_RESULT_IMP), ("wall_seconds", SEQ_RESULT_TAIL), ("kernel_seconds", SEQ_RESULT_TAIL + 8)]),
    ("relmc_nsq_result", NSQ_RESULT_BYTES, [("acc", 0), ("idx", NSQ_RESULT_IDX), ("checkpoints", NSQ_RESULT_TAIL), ("converged", NSQ_RESULT_TAIL + 8), ("wall_seconds", NSQ_RESULT_TAIL + 16), ("kernel_seconds", NSQ_RESULT_TAIL + 24), ("batches", NSQ_RESULT_TAIL + 32)]),
]

end # module
