"""
    FlightBatch

Julia-side binding of `libflightbatch` (include/flightbatch.h): the drop-in for the hot path of
`Model(SimpleWorld(Cessna172Sv0()))` — `f_ode!` / `f_step!` / `f_periodic!` / `init!` / `step!` — executed for N
independent aircraft on one MI355X. It follows the only in-tree FFI precedent of Flight.jl, the plain
`ccall((:sym, lib), Ret, (ArgTypes...), args...)` pattern of `lib/FlightCore/src/joysticks.jl:45-53`.

NOT EXECUTED in this repository's CI (no Julia toolchain in the build environment); the Python package
`flightbatch` is the executed mirror of exactly these calls. Array convention of the C ABI: column-major
`[N x Nfield]`, aircraft index fastest — i.e. a Julia `Matrix{Float64}(undef, N, Nfield)` passes as is.

Usage (what a Flight.jl maintainer would write):

    using Flight, FlightBatch
    world  = FlightBatch.BatchedWorld(1_048_576)              # ≙ Model(SimpleWorld(Cessna172Sv0())) x N
    sim    = FlightBatch.BatchedSimulation(world; dt = 0.01)   # ≙ Simulation(world; dt = 0.01)
    FlightBatch.init!(sim, C172.TrimParameters())               # ≙ init!(sim, C172.TrimParameters())
    FlightBatch.step!(sim, 10.0, true)                          # ≙ step!(sim, 10.0, true)
    x = FlightBatch.state(world)                                # N x 27, same component order as world.x
"""
module FlightBatch

using Flight.FlightCore.Modeling: ModelDefinition
import Flight.FlightCore.Modeling: f_init!, f_ode!, f_step!, f_periodic!
using Flight: FlightPhysics
using Flight.FlightApps: C172
using Flight.FlightPhysics: Propellers, Piston, Control
using Flight.FlightPhysics.Kinematics: WA, ECEF, NED                   # kinematic descriptors (exported at FP/kinematics.jl:11)
using Flight.FlightApps.C172.C172S.C172Sv0: Cessna172Sv0               # FA/c172/c172s/c172s0.jl:9,14-18
using Flight.FlightApps.C172.C172X.C172Xv2: Cessna172Xv2               # FA/c172/c172x/c172x2.jl:12,54-59
import Flight.FlightPhysics.Linearization: linearize                   # FP/linearization.jl:8

const lib = get(ENV, "FLIGHTBATCH_LIB", "libflightbatch")

# layout constants of include/flightbatch.h
const NX, NS, NU, NY, NTP, NTS = 27, 2, 16, 174, 18, 7
const TABLE_EGM96, TABLE_PROPELLER, TABLE_PISTON, TABLE_AERO = Cint(0), Cint(1), Cint(2), Cint(3)

struct Params   # fb_params
    dt::Cdouble; periodic_n::Cint; surface::Cint; T_sl::Cdouble; p_sl::Cdouble
    wind_ned::NTuple{3,Cdouble}; h_terrain::Cdouble
end

check(rc::Integer) = rc == 0 || error(unsafe_string(ccall((:fb_last_error, lib), Cstring, ())))

const MODEL_C172S0, MODEL_C172X2, MODEL_ROBOT2D = Cint(0), Cint(1), Cint(2)
const KIN = Dict(WA => Cint(0), ECEF => Cint(1), NED => Cint(2))        # FB_KIN_*: the vehicle's kinematic descriptor
const TABLE_CTL_GAINS = Cint(5)
const NCU, NCS = 28, 66                                                 # FB_NCU, FB_NCS (Cessna172Xv2 control laws)

"N instances of SimpleWorld(aircraft) resident on one GPU (the batched counterpart of a root Model).
`aircraft` is `Cessna172Sv0(kin)` or `Cessna172Xv2(kin)` (kin = WA(), ECEF() or NED()); its type picks the model id."
mutable struct BatchedWorld <: ModelDefinition
    handle::Ptr{Cvoid}
    n::Int
    nx::Int
    function BatchedWorld(n::Integer, aircraft = Cessna172Sv0(); device::Integer = 0)
        model = aircraft isa Cessna172Xv2 ? MODEL_C172X2 : MODEL_C172S0
        kin = KIN[typeof(aircraft.vehicle.kinematics)]
        h = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:fb_create, lib), Cint, (Cint, Cint, Cint, Int64, Cint, Ptr{Ptr{Cvoid}}), model, kin, 0, n, device, h))
        nx = Ref{Cint}(0)
        check(ccall((:fb_dims, lib), Cint, (Ptr{Cvoid}, Ptr{Cint}, Ptr{Cint}, Ptr{Cint}, Ptr{Cint}), h[], nx, C_NULL, C_NULL, C_NULL))
        w = new(h[], n, nx[])      # 27 (WA) / 26 (ECEF) / 24 (NED), Xv2 seven more: length(Model(aircraft).x)
        finalizer(w -> ccall((:fb_destroy, lib), Cint, (Ptr{Cvoid},), w.handle), w)
        upload_tables!(w)
        # Xv2: the ten gain lookups of c172x/control/data packed as include/flightbatch.h documents (flightbatch/ctl_gains.py)
        aircraft isa Cessna172Xv2 && set_table!(w, TABLE_CTL_GAINS, pack_ctl_gains(aircraft.avionics.ctl))
        return w
    end
end

# ---- FB_TABLE_CTL_GAINS: the ten gain-scheduling lookups of ControlLawsLon / ControlLawsLat (c172x_ctl.jl:203-213, 814-819), each a
# PIDData / LQRData of `extrapolate(scale(interpolate(points, BSpline(Linear())), EAS_range, h_range), Flat())` objects
# (FP/control.jl:950-972). Blob layout (include/flightbatch.h; executed twin: flightbatch/ctl_gains.py `_pack`): per lookup a 6-double
# header [nE, nH, EAS_lo, EAS_hi, h_lo, h_hi], then for every grid point — h slowest, EAS next — one record:
#   LQR: vec(K_fbk) (column-major NU x NX), vec(K_fwd), vec(K_int), x_trim, u_trim, z_trim      PID: k_p, k_i, k_d, τ_f
scaled_coefs(e) = e.itp.itp.coefs            # Extrapolation -> ScaledInterpolation -> BSplineInterpolation (Linear(): coefs == the data array)
scaled_ranges(e) = e.itp.ranges
function pack_lookup(fields::Vector)
    rE, rH = scaled_ranges(fields[1])
    nE, nH = length(rE), length(rH)
    blob = Float64[nE, nH, first(rE), last(rE), first(rH), last(rH)]
    for j in 1:nH, i in 1:nE, f in fields
        @assert scaled_ranges(f) == (rE, rH)
        append!(blob, vec(collect(Float64, scaled_coefs(f)[i, j])))      # SMatrix / SVector: column-major; scalar: one value
    end
    return blob
end
pack_lookup(l::Control.LQRData) = pack_lookup(Any[l.K_fbk, l.K_fwd, l.K_int, l.x_trim, l.u_trim, l.z_trim])
pack_lookup(l::Control.PIDData) = pack_lookup(Any[l.k_p, l.k_i, l.k_d, l.τ_f])
"blob order of include/flightbatch.h: te2te, tv2te, vh2te, q2e, c2θ, v2t (lon), ar2ar, φβ2ar, p2φ, χ2φ (lat)"
function pack_ctl_gains(ctl)::Vector{Float64}
    (; lon, lat) = ctl
    vcat(map(pack_lookup, (lon.te2te_lookup, lon.tv2te_lookup, lon.vh2te_lookup, lon.q2e_lookup, lon.c2θ_lookup, lon.v2t_lookup,
                           lat.ar2ar_lookup, lat.φβ2ar_lookup, lat.p2φ_lookup, lat.χ2φ_lookup))...)
end

# avionics.ctl.u / avionics.gdc.u and the control laws' record, as N x NCU / N x NCS matrices (columns = FB_CU_* / FB_CS_*)
ctl_inputs(w::BatchedWorld) = (cu = Matrix{Float64}(undef, w.n, NCU);
    check(ccall((:fb_get_ctl_inputs, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), w.handle, cu)); cu)
ctl_inputs!(w::BatchedWorld, cu::Matrix{Float64}) = check(ccall((:fb_set_ctl_inputs, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), w.handle, cu))
ctl_record(w::BatchedWorld) = (cs = Matrix{Float64}(undef, w.n, NCS);
    check(ccall((:fb_get_ctl_state, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), w.handle, cs)); cs)

function set_table!(w::BatchedWorld, kind::Cint, data::Array)
    dims = Int64[size(data)...]
    check(ccall((:fb_set_table, lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Int64}, Cint), w.handle, kind, data, dims, length(dims)))
end

"Hand the library the very tables Flight.jl builds at construction time (SURVEY.md Appendix B)."
function upload_tables!(w::BatchedWorld)
    # EGM96: the Float32 721 x 1441 grid behind Geodesy.egm96_interp (geodesy.jl:186-198)
    egm = Matrix{Float32}(undef, 721, 1441)
    # the file Geodesy itself reads: joinpath(dirname(@__FILE__), "data", "ww15mgh_le.bin") in FP/geodesy.jl:166, i.e. next to the
    # package's entry file (pathof works on the package module FlightPhysics, not on its submodule Geodesy)
    read!(joinpath(dirname(pathof(FlightPhysics)), "data", "ww15mgh_le.bin"), egm)
    set_table!(w, TABLE_EGM96, egm)
    # propeller: Lookup(2, Blade()).data, six 21 x 21 x 1 arrays (propellers.jl:235-250) -> [21, 21, 6]
    lookup = Propellers.Lookup(2, Propellers.Blade())
    d = lookup.data
    prop = cat((dropdims(getfield(d, f); dims = 3) for f in (:C_Fx, :C_Mx, :C_Fz_α, :C_Mz_α, :C_P, :η_p))...; dims = 3)
    set_table!(w, TABLE_PROPELLER, prop)
    # piston and aero blobs are packed in the csrc/tables.h layout by the helpers below
    set_table!(w, TABLE_PISTON, pack_piston(Piston.PistonEngineLookup(300 / 2700, 3100 / 2700)))
    set_table!(w, TABLE_AERO, pack_aero(C172.aero_lookup))
end

# The two packers read the interpolation objects' knots / coefs and lay them out as csrc/tables.h documents (AT_* / PT_* offsets,
# 0-based, in doubles; 2-D tables column-major like the Julia arrays); flightbatch/tables.py (`piston_blob`, `aero_blob`) is the
# executed twin and tests/test_host_and_abi.py checks it against the oracle's builders.
#   linear_interpolation(knots, data, extrapolation_bc = ...) == extrapolate(interpolate(knots, data, Gridded(Linear())), ...):
#       .itp.knots :: Tuple of knot vectors, .itp.coefs :: the data array
#   extrapolate(scale(interpolate(A, BSpline(Linear())), ranges...), Line()): .itp.ranges, .itp.itp.coefs (see scaled_coefs above)
gridded_knots(e) = e.itp.knots
gridded_coefs(e) = e.itp.coefs
put_at!(b::Vector{Float64}, off0::Integer, a) = (v = vec(collect(Float64, a)); b[off0 + 1 : off0 + length(v)] .= v; b)

# csrc/tables.h PT_* offsets
const PT_DELTA_WOT_V, PT_MU_WOT_V, PT_PISTD_N_K, PT_PISTD_MU_K, PT_PISTD_V, PT_PIWOT_N_K, PT_PIWOT_D_K, PT_PIWOT_V = 0, 18, 36, 49, 52, 91, 96, 99
const PT_F_K, PT_PI_RATIO_V, PT_SFC_RATIO_V, PT_SFC_N_K, PT_SFC_PI_K, PT_SFC_POW_V, PT_SIZE = 114, 125, 136, 147, 152, 160, 200
"PistonEngineLookup (FP/piston.jl:60-195) -> the FB_TABLE_PISTON blob"
function pack_piston(l)::Vector{Float64}
    b = zeros(PT_SIZE)
    # δ_wot(n, μ), μ_wot(n, δ): scaled B-splines on fixed ranges the kernels know (piston.jl:78-79, 92-93); only the 2 x 9 samples travel
    @assert scaled_ranges(l.δ_wot) == (range(0.667, 1, length = 2), range(0.401, 0.936, length = 9))
    @assert scaled_ranges(l.μ_wot) == (range(0.667, 1, length = 2), range(0.441, 1, length = 9))
    put_at!(b, PT_DELTA_WOT_V, scaled_coefs(l.δ_wot)); put_at!(b, PT_MU_WOT_V, scaled_coefs(l.μ_wot))
    n13, μ3 = gridded_knots(l.π_std)                       # π_std(n, μ): 13 x 3, Flat (piston.jl:110-133)
    put_at!(b, PT_PISTD_N_K, n13); put_at!(b, PT_PISTD_MU_K, μ3); put_at!(b, PT_PISTD_V, gridded_coefs(l.π_std))
    n5, δ3 = gridded_knots(l.π_wot)                        # π_wot(n, δ): 5 x 3 (piston.jl:140-149)
    put_at!(b, PT_PIWOT_N_K, n5); put_at!(b, PT_PIWOT_D_K, δ3); put_at!(b, PT_PIWOT_V, gridded_coefs(l.π_wot))
    (f11,) = gridded_knots(l.π_ratio)                      # π_ratio(f), sfc_ratio(f): 11 knots shared (piston.jl:157-172)
    @assert gridded_knots(l.sfc_ratio)[1] == f11
    put_at!(b, PT_F_K, f11); put_at!(b, PT_PI_RATIO_V, gridded_coefs(l.π_ratio)); put_at!(b, PT_SFC_RATIO_V, gridded_coefs(l.sfc_ratio))
    nsfc, πsfc = gridded_knots(l.sfc_pow)                  # sfc_pow(n, π): 5 x 8, Line (piston.jl:179-189)
    put_at!(b, PT_SFC_N_K, nsfc); put_at!(b, PT_SFC_PI_K, πsfc); put_at!(b, PT_SFC_POW_V, gridded_coefs(l.sfc_pow))
    return b
end

# csrc/tables.h AT_* offsets
const AT_GE_K, AT_CD_GE_V, AT_CL_GE_V, AT_DF4_K, AT_CD_DF_V, AT_CL_DF_V, AT_CM_DF_V, AT_UNIT3_K, AT_CD_DE_V, AT_CD_BETA_V = 0, 13, 26, 39, 43, 47, 51, 55, 58, 61
const AT_CD_ALPHA_K, AT_CD_ALPHA_DF_V, AT_CY_BETA_K, AT_DF2_K, AT_CY_BETA_DF_V, AT_ALPHA2_K, AT_CY_P_V, AT_CY_R_V, AT_CL_R_V = 64, 90, 194, 197, 199, 205, 207, 211, 215
const AT_CL_ALPHA_K, AT_CL_ALPHA_V, AT_SCALARS, AT_SIZE = 219, 236, 270, 291
"C172.aero_lookup (FA/c172/c172.jl:51-205: NamedTuple of scalars and Gridded(Linear()) / Flat() interpolations) -> the FB_TABLE_AERO blob"
function pack_aero(l)::Vector{Float64}
    (; C_D, C_Y, C_L, C_l, C_m, C_n) = l
    b = zeros(AT_SIZE)
    k1(e) = gridded_knots(e)[1]
    @assert k1(C_D.ge) == k1(C_L.ge)                        # ground-effect tables share their 13 knots (c172.jl:67, 117)
    put_at!(b, AT_GE_K, k1(C_D.ge)); put_at!(b, AT_CD_GE_V, gridded_coefs(C_D.ge)); put_at!(b, AT_CL_GE_V, gridded_coefs(C_L.ge))
    @assert k1(C_D.δf) == k1(C_L.δf) == k1(C_m.δf) == gridded_knots(C_D.α_δf)[2]
    put_at!(b, AT_DF4_K, k1(C_D.δf)); put_at!(b, AT_CD_DF_V, gridded_coefs(C_D.δf)); put_at!(b, AT_CL_DF_V, gridded_coefs(C_L.δf)); put_at!(b, AT_CM_DF_V, gridded_coefs(C_m.δf))
    @assert k1(C_D.δe) == k1(C_D.β)
    put_at!(b, AT_UNIT3_K, k1(C_D.δe)); put_at!(b, AT_CD_DE_V, gridded_coefs(C_D.δe)); put_at!(b, AT_CD_BETA_V, gridded_coefs(C_D.β))
    put_at!(b, AT_CD_ALPHA_K, gridded_knots(C_D.α_δf)[1]); put_at!(b, AT_CD_ALPHA_DF_V, gridded_coefs(C_D.α_δf))       # 26 x 4
    put_at!(b, AT_CY_BETA_K, gridded_knots(C_Y.β_δf)[1]); put_at!(b, AT_DF2_K, gridded_knots(C_Y.β_δf)[2]); put_at!(b, AT_CY_BETA_DF_V, gridded_coefs(C_Y.β_δf))   # 3 x 2
    @assert gridded_knots(C_Y.p) == gridded_knots(C_Y.r) == gridded_knots(C_l.r) && gridded_knots(C_Y.p)[2] == gridded_knots(C_Y.β_δf)[2]
    put_at!(b, AT_ALPHA2_K, gridded_knots(C_Y.p)[1]); put_at!(b, AT_CY_P_V, gridded_coefs(C_Y.p)); put_at!(b, AT_CY_R_V, gridded_coefs(C_Y.r)); put_at!(b, AT_CL_R_V, gridded_coefs(C_l.r))
    put_at!(b, AT_CL_ALPHA_K, gridded_knots(C_L.α)[1]); put_at!(b, AT_CL_ALPHA_V, gridded_coefs(C_L.α))                 # 17 x 2 (stall 0 / 1)
    put_at!(b, AT_SCALARS, Float64[C_D.z, C_Y.δr, C_Y.δa, C_L.δe, C_L.q, C_L.α_dot, C_l.δa, C_l.δr, C_l.β, C_l.p,          # AS_* order of csrc/tables.h
                                C_m.z, C_m.δe, C_m.α, C_m.q, C_m.α_dot, C_n.δr, C_n.δa, C_n.β, C_n.p, C_n.r])
    return b
end

# ---- the verbs --------------------------------------------------------------------------------------------
state(w::BatchedWorld) = (x = Matrix{Float64}(undef, w.n, w.nx); s = Matrix{Int32}(undef, w.n, NS);
    check(ccall((:fb_get_state, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Int32}), w.handle, x, s)); x)
outputs(w::BatchedWorld) = (y = Matrix{Float64}(undef, w.n, NY);
    check(ccall((:fb_get_outputs, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), w.handle, y)); y)

"`outputs(world, mask)`: only the blocks of mdl.y named by the FB_YF_* bits (KIN = 1, AIR = 2, AERO = 4, LDG = 8, PWP = 16, FUEL = 32, DYN = 64)"
function outputs(w::BatchedWorld, mask::Integer)
    first = (0, 40, 62, 78, 111, 133, 134, NY)
    rows = sum(first[i + 1] - first[i] for i in 1:7 if mask & (1 << (i - 1)) != 0)
    y = Matrix{Float64}(undef, w.n, rows)
    check(ccall((:fb_get_output_fields, lib), Cint, (Ptr{Cvoid}, UInt32, Ptr{Cdouble}), w.handle, mask, y)); y
end

"f_init!(world, C172.TrimParameters()) — one trim per aircraft, on the device."
function f_init!(w::BatchedWorld, trim::C172.TrimParameters)
    tp = Matrix{Float64}(undef, w.n, NTP)
    tp[:, 1:3] .= trim.Ob.loc[:]'; tp[:, 4] .= Float64(trim.Ob.h); tp[:, 5] .= trim.ψ_nb; tp[:, 6] .= trim.EAS
    tp[:, 7] .= trim.γ_wb_n; tp[:, 8] .= trim.ψ_wb_dot; tp[:, 9] .= trim.θ_wb_dot; tp[:, 10] .= trim.β_a
    tp[:, 11] .= Float64(trim.fuel_load); tp[:, 12] .= Float64(trim.mixture); tp[:, 13] .= Float64(trim.flaps)
    p = trim.payload
    tp[:, 14:18] .= Float64[Float64(p.m_pilot) Float64(p.m_copilot) Float64(p.m_lpass) Float64(p.m_rpass) Float64(p.m_baggage)]
    ts = repeat(collect(C172.TrimState())', w.n)          # initial guess, c172.jl:796-804
    ok = Vector{Int32}(undef, w.n); cost = Vector{Float64}(undef, w.n)
    check(ccall((:fb_trim, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}, Ptr{Cdouble}), w.handle, tp, ts, ok, cost))
    all(==(1), ok) || @warn("Trimming failed for $(count(!=(1), ok)) aircraft")    # c172.jl:936-938
    return nothing
end
"""linearize(world, C172.TrimParameters(); scheme = 0) — `linearize(aircraft, trim_params)` (FP/aircraftbase.jl:292-334) for every aircraft at
once: still-air trim, then ẋ0, x0, u0, y0 and the four matrices a, b, c, d (forward differences, FiniteDiff's steps, with scheme = 0 = FB_LIN_FORWARD). The
matrices come back as [N, rows, cols] arrays; wrap one aircraft's slices in `LinearizedSS` (FP/linearization.jl:39-48) for labelled axes."""
function linearize(w::BatchedWorld, trim::C172.TrimParameters; scheme::Integer = 0)
    tp = Matrix{Float64}(undef, w.n, NTP)
    tp[:, 1:3] .= trim.Ob.loc[:]'; tp[:, 4] .= Float64(trim.Ob.h); tp[:, 5] .= trim.ψ_nb; tp[:, 6] .= trim.EAS
    tp[:, 7] .= trim.γ_wb_n; tp[:, 8] .= trim.ψ_wb_dot; tp[:, 9] .= trim.θ_wb_dot; tp[:, 10] .= trim.β_a
    tp[:, 11] .= Float64(trim.fuel_load); tp[:, 12] .= Float64(trim.mixture); tp[:, 13] .= Float64(trim.flaps)
    p = trim.payload
    tp[:, 14:18] .= Float64[Float64(p.m_pilot) Float64(p.m_copilot) Float64(p.m_lpass) Float64(p.m_rpass) Float64(p.m_baggage)]
    ts = repeat(collect(C172.TrimState())', w.n)
    ok = Vector{Int32}(undef, w.n); cost = Vector{Float64}(undef, w.n)
    nx, nu, ny = Ref{Cint}(0), Ref{Cint}(0), Ref{Cint}(0)
    check(ccall((:fb_linearize_dims, lib), Cint, (Ptr{Cvoid}, Ptr{Cint}, Ptr{Cint}, Ptr{Cint}), w.handle, nx, nu, ny))
    nx, nu, ny = nx[], nu[], ny[]
    xdot0 = Matrix{Float64}(undef, w.n, nx); x0 = similar(xdot0); u0 = Matrix{Float64}(undef, w.n, nu); y0 = Matrix{Float64}(undef, w.n, ny)
    a = Array{Float64}(undef, w.n, nx, nx); b = Array{Float64}(undef, w.n, nx, nu)
    c = Array{Float64}(undef, w.n, ny, nx); d = Array{Float64}(undef, w.n, ny, nu)
    status = Vector{Int32}(undef, w.n)
    check(ccall((:fb_linearize, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble},
                Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}),
                w.handle, tp, ts, ok, cost, scheme, xdot0, x0, u0, y0, a, b, c, d, status))
    all(==(1), ok) || @warn("Trimming failed for $(count(!=(1), ok)) aircraft")
    return (; xdot0, x0, u0, y0, a, b, c, d, status, success = ok .== 1, cost)   # a, b, c, d: A, B, C, D
end
f_ode!(w::BatchedWorld) = (check(ccall((:fb_f_ode, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), w.handle, C_NULL)); nothing)
f_step!(w::BatchedWorld) = (check(ccall((:fb_f_step, lib), Cint, (Ptr{Cvoid},), w.handle)); nothing)
f_periodic!(w::BatchedWorld) = (check(ccall((:fb_f_periodic, lib), Cint, (Ptr{Cvoid},), w.handle)); nothing)

# ---- Model(lss) on the device (FB_MODEL_LSS; FP/linearization.jl:157-192): N linear models of one (nx, nu, ny), each with its own matrices
"N instances of `Model(lss::LinearizedSS)` resident on one GPU. Built from the named tuple `linearize(world, trim)` returns
(`LinearWorld(lin)`), or device to device from the world that was linearised (`linear_world(world; ix, iu, iy)`, the reference's `subsystem`)."
mutable struct LinearWorld <: ModelDefinition
    handle::Ptr{Cvoid}
    n::Int
    nx::Int
    nu::Int
    ny::Int
    function LinearWorld(handle::Ptr{Cvoid})
        nx, nu, ny = Ref{Cint}(0), Ref{Cint}(0), Ref{Cint}(0)
        check(ccall((:fb_dims, lib), Cint, (Ptr{Cvoid}, Ptr{Cint}, Ptr{Cint}, Ptr{Cint}, Ptr{Cint}), handle, nx, C_NULL, nu, ny))
        w = new(handle, ccall((:fb_size, lib), Int64, (Ptr{Cvoid},), handle), nx[], nu[], ny[])
        finalizer(w -> ccall((:fb_destroy, lib), Cint, (Ptr{Cvoid},), w.handle), w)
        return w
    end
end
function LinearWorld(lin; device::Integer = 0)
    n, nx = size(lin.x0); nu = size(lin.u0, 2); ny = size(lin.y0, 2)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:fb_lss_create, lib), Cint, (Cint, Cint, Cint, Int64, Cint, Ptr{Ptr{Cvoid}}), nx, nu, ny, n, device, h))
    w = LinearWorld(h[])
    check(ccall((:fb_lss_set_model, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                Ptr{Cdouble}, Ptr{Cdouble}), w.handle, lin.xdot0, lin.x0, lin.u0, lin.y0, lin.a, lin.b, lin.c, lin.d))
    return w
end
"`Model(subsystem(lss; x, u, y))` from the result of the last `linearize(world, trim)`, which is still on the device: ix, iu, iy are 1-based
index vectors into the state-space vectors (`nothing`: every index)."
function linear_world(w::BatchedWorld; ix = nothing, iu = nothing, iy = nothing)
    zero_based(v) = v === nothing ? Cint[] : Cint.(v .- 1)
    jx, ju, jy = zero_based(ix), zero_based(iu), zero_based(iy)
    arg(v, j) = v === nothing ? C_NULL : j      # (ccall converts and roots a Vector{Cint} itself)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:fb_lss_from_linearization, lib), Cint, (Ptr{Cvoid}, Ptr{Cint}, Cint, Ptr{Cint}, Cint, Ptr{Cint}, Cint, Ptr{Ptr{Cvoid}}),
                w.handle, arg(ix, jx), length(jx), arg(iu, ju), length(ju), arg(iy, jy), length(jy), h))
    return LinearWorld(h[])
end
"`lqr(P, Q, R)` (FA design/c172/c172x_design.jl:181) for every system of `w`, on its device: Q (nx x nx) and R (nu x nu) are the batch's,
symmetric, R positive definite. Returns k (N x nu x nx), x (N x nx x nx), resid, iters, status (0, or FB_LQR_NOT_CONVERGED = 1 |
FB_LQR_SINGULAR = 2: K, X and resid are NaN there)."
function lqr(w::LinearWorld, q::Matrix{Float64}, r::Matrix{Float64})
    size(q) == (w.nx, w.nx) || throw(DimensionMismatch("Q must be nx x nx"))
    size(r) == (w.nu, w.nu) || throw(DimensionMismatch("R must be nu x nu"))
    k = Array{Float64}(undef, w.n, w.nu, w.nx); x = Array{Float64}(undef, w.n, w.nx, w.nx)
    resid = Vector{Float64}(undef, w.n); iters = Vector{Int32}(undef, w.n); status = Vector{Int32}(undef, w.n)
    check(ccall((:fb_lqr, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}, Ptr{Int32}),
                w.handle, q, r, k, x, resid, iters, status))
    return (; k, x, resid, iters, status)
end
"The poles of every system of `w`, on its device (`dampreport(P)`, FA design/robot2d/robot2d_design.ipynb): the nx eigenvalues of A by balancing,
Hessenberg reduction and double-shift QR. Returns re, im (N x nx; within a system ascending by |pole|, then Re, then Im; a pair is exact
conjugates), iters (QR sweeps) and status (0, or FB_POLES_NOT_CONVERGED = 1 | FB_POLES_NOT_FINITE = 2: the poles are NaN there)."
function poles(w::LinearWorld)
    re = Matrix{Float64}(undef, w.n, w.nx); im = Matrix{Float64}(undef, w.n, w.nx)
    iters = Vector{Int32}(undef, w.n); status = Vector{Int32}(undef, w.n)
    check(ccall((:fb_lss_poles, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}, Ptr{Int32}), w.handle, re, im, iters, status))
    return (; re, im, iters, status)
end
"`stepinfo(step(P[:y, :u], t_sim))` (FA design/robot2d/robot2d_design.ipynb) of the channels `channels` = [(iu, iy), ...] (1-based) of every system of
`w`, on its device: the unit step response from rest by the classical RK4 at the caller's `dt`, sampled at k dt. Returns y0, yf, stepsize, peak,
peaktime, overshoot, undershoot, settlingtime, risetime (each N x m) and status (0, or FB_STEPINFO_DIVERGED = 1: every field NaN,
FB_STEPINFO_FLAT = 2: the ratios and times NaN). `y0`, `yf`: N x m matrices whose NaN entries mean the first / last sample, or `nothing`."
function stepinfo(w::LinearWorld, channels, t_sim::Real; dt::Real, y0=nothing, yf=nothing, settling_th::Real=0.02, risetime_th=(0.1, 0.9))
    m = length(channels)
    iu = Int32[c[1] - 1 for c in channels]; iy = Int32[c[2] - 1 for c in channels]
    opts = Float64[settling_th, risetime_th[1], risetime_th[2]]
    info = Array{Float64}(undef, w.n, m, 9); status = Matrix{Int32}(undef, w.n, m)
    p0 = y0 === nothing ? Ptr{Cdouble}(C_NULL) : pointer(y0); pf = yf === nothing ? Ptr{Cdouble}(C_NULL) : pointer(yf)
    Base.GC.@preserve y0 yf check(ccall((:fb_lss_stepinfo, lib), Cint,
          (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}, Int32, Cdouble, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}),
          w.handle, iu, iy, m, t_sim, dt, opts, p0, pf, 1, Ptr{Cdouble}(C_NULL), info, status))
    f = k -> info[:, :, k]
    return (; y0 = f(1), yf = f(2), stepsize = f(3), peak = f(4), peaktime = f(5), overshoot = f(6), undershoot = f(7), settlingtime = f(8),
            risetime = f(9), status)
end
"P(jω) = c inv(jωI - A) b + d of channel (iu, iy) (1-based) of every system of `w` on the grid `freqs` (rad/s, positive), on its device: the
plant of `sensitivity(plant, pid)` (FA design/pidopt.jl:39). Returns (re, im), each N x length(freqs)."
function freqresp(w::LinearWorld, iu::Integer, iy::Integer, freqs::Vector{Float64})
    re = Matrix{Float64}(undef, w.n, length(freqs)); im = Matrix{Float64}(undef, w.n, length(freqs))
    check(ccall((:fb_lss_freqresp, lib), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}),
                w.handle, iu - 1, iy - 1, freqs, length(freqs), re, im))
    return (; re, im)
end
"`Metrics(plant, build_PID(point), settings)` and `cost` (FA design/pidopt.jl:36-70) for every system of `w` and each of its m candidates, on
its device: pid is N x m x 4 (k_p, k_i, k_d, τ_f), the plant channel (iu, iy) (1-based) of each system, weights a 5-vector (`nothing`: ones).
The step response is RK4 with the caller's dt over round(t_sim / dt) steps, Ms the peak of the sensitivity over `freqs`. Returns metrics
(N x m x 5: Ms, ∫e, ef, ∫u, up), cost and status (N x m; 0, FB_PID_DIVERGED = 1 or FB_PID_SINGULAR = 2: cost is infinite there)."
function pid_metrics(w::LinearWorld, iu::Integer, iy::Integer, freqs::Vector{Float64}, t_sim::Real, dt::Real, pid::Array{Float64, 3};
                     weights::Union{Vector{Float64}, Nothing} = nothing)
    size(pid, 1) == w.n && size(pid, 3) == 4 || throw(DimensionMismatch("pid must be N x m x 4"))
    m = size(pid, 2)
    metrics = Array{Float64}(undef, w.n, m, 5); cost = Matrix{Float64}(undef, w.n, m); status = Matrix{Int32}(undef, w.n, m)
    check(ccall((:fb_pid_metrics, lib), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Cint, Cdouble, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Cint,
                                               Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}),
                w.handle, iu - 1, iy - 1, freqs, length(freqs), t_sim, dt, weights === nothing ? C_NULL : weights, pid, m, metrics, cost, status))
    return (; metrics, cost, status)
end
"A (N x nx x nx) and B (N x nx x nu) of the handle's own copy of the model: the matrices the device steps and designs on"
function model(w::LinearWorld)
    a = Array{Float64}(undef, w.n, w.nx, w.nx); b = Array{Float64}(undef, w.n, w.nx, w.nu)
    check(ccall((:fb_lss_get_model, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}), w.handle, a, b))
    return (; a, b)
end
"C (N x ny x nx) and D (N x ny x nu) of the handle's own copy of the model: the companion of `model`"
function model_cd(w::LinearWorld)
    c = Array{Float64}(undef, w.n, w.ny, w.nx); d = Array{Float64}(undef, w.n, w.ny, w.nu)
    check(ccall((:fb_lss_get_cd, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}), w.handle, c, d))
    return (; c, d)
end
"`connect` / `series` / `feedback` (FA design/c172/c172x_design.jl:199-216, 226-227, 244-263) on the device: with v = [u_p; u_c] and z = [y_p; y_c]
the interconnection v = feedback z[reads] + inputs w closed around `p` and `c` (`nothing`: no compensator). `feedback` is nv x nf for the batch or
N x nv x nf per system, `inputs` nv x nw or N x nv x nw; `reads`, `outputs`: 1-based rows of z (`outputs = nothing`: every row). Returns the new
`LinearWorld` (states [x_p; x_c], inputs w, outputs z[outputs], at rest) and status (0, FB_CONNECT_ILL_POSED = 1 or FB_CONNECT_NOT_FINITE = 2:
that system's matrices are NaN)."
function connect(p::LinearWorld, c::Union{LinearWorld, Nothing} = nothing; feedback::Array{Float64}, inputs::Array{Float64}, reads, outputs = nothing)
    jz = Int32.(reads .- 1); iz = outputs === nothing ? Int32[] : Int32.(outputs .- 1)
    nw = size(inputs, ndims(inputs))
    status = Vector{Int32}(undef, p.n)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:fb_lss_connect, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int32}, Int32, Ptr{Cdouble}, Int32, Ptr{Cdouble}, Int32, Int32, Ptr{Int32},
                                               Int32, Ptr{Int32}, Ptr{Ptr{Cvoid}}),
                p.handle, c === nothing ? C_NULL : c.handle, jz, length(jz), feedback, ndims(feedback) == 3 ? 1 : 0, inputs, ndims(inputs) == 3 ? 1 : 0, nw,
                outputs === nothing ? C_NULL : iz, length(iz), status, h))
    return (; world = LinearWorld(h[]), status)
end
"`get_design_model!` / `subsystem` / `delete_vars` (FA design/c172/c172x_design.jl:23-82) on the device: the change of state variables x' = y[rows]
(T = C[rows, :]: T A inv(T), T B, C inv(T), D; x0' = y0[rows], xdot0' = T xdot0 with the 1-based entries `xdot_zero` exactly 0), then the
subsystem `ix`, `iu`, `iy` (1-based, `nothing`: every index) of the result. `rows = nothing`: T = I, the entries are copied bit for bit. Returns
the new `LinearWorld`, status (0, FB_SURGERY_SINGULAR = 1 or FB_SURGERY_NOT_FINITE = 2: that system's matrices are NaN) and rpiv (the
smallest pivot magnitude of T over the largest)."
function transform(w::LinearWorld, rows = nothing; xdot_zero = Int[], ix = nothing, iu = nothing, iy = nothing)
    zero_based(v) = v === nothing ? Int32[] : Int32.(v .- 1)
    jr, jx, ju, jy = zero_based(rows), zero_based(ix), zero_based(iu), zero_based(iy)
    arg(v, j) = v === nothing ? C_NULL : j
    mask = zeros(Int32, w.nx); mask[xdot_zero] .= 1
    status = Vector{Int32}(undef, w.n); rpiv = Vector{Float64}(undef, w.n)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:fb_lss_transform, lib), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Int32, Ptr{Int32}, Int32, Ptr{Int32}, Int32,
                                                 Ptr{Int32}, Ptr{Cdouble}, Ptr{Ptr{Cvoid}}),
                w.handle, arg(rows, jr), mask, arg(ix, jx), length(jx), arg(iu, ju), length(ju), arg(iy, jy), length(jy), status, rpiv, h))
    return (; world = LinearWorld(h[]), status, rpiv)
end
"M = inv([A B; C[z, :] D[z, :]]) and K_fwd = M22 + K M12 (FA design/c172/c172x_design.jl:184-188) on the device: `z` are nu 1-based output
rows, `k` is nu x nx for the batch, N x nu x nx per system (`lqr`'s) or `nothing`. Returns x = M12 (N x nx x nu), u = M22 (N x nu x nu), k_fwd
(`nothing` without k), status (as `transform`'s, for L) and rpiv."
function steady_state(w::LinearWorld, z; k::Union{Array{Float64}, Nothing} = nothing)
    iz = Int32.(z .- 1)
    nz = length(iz)
    x = Array{Float64}(undef, w.n, w.nx, nz); u = Array{Float64}(undef, w.n, w.nu, nz)
    k_fwd = k === nothing ? nothing : Array{Float64}(undef, w.n, w.nu, nz)
    status = Vector{Int32}(undef, w.n); rpiv = Vector{Float64}(undef, w.n)
    check(ccall((:fb_lss_steady, lib), Cint, (Ptr{Cvoid}, Ptr{Int32}, Int32, Ptr{Cdouble}, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                                              Ptr{Cdouble}, Ptr{Int32}),
                w.handle, iz, nz, k === nothing ? C_NULL : k, k !== nothing && ndims(k) == 3 ? 1 : 0, x, u, k === nothing ? C_NULL : k_fwd, rpiv, status))
    return (; x, u, k_fwd, status, rpiv)
end
"`c2d(sys, Ts)` on the device: the zero-order-hold sampled model of every system of a continuous `LinearWorld` (Phi = e^(A Ts) in A's place,
Gamma in B's, delta in xdot0's; x+ = x0 + Phi (x - x0) + Gamma (u - u0) + delta), a new `LinearWorld` whose step is the map and whose dt is
Ts. Returns the world, status (0, FB_C2D_NOT_FINITE = 1 or FB_C2D_RANGE = 2: that system's Phi, Gamma and delta are NaN) and the squarings
of each system's scaling and squaring. The continuous-time design verbs refuse a sampled world; `sample_time(w)` is its Ts (0 for a
continuous one)."
function c2d(w::LinearWorld, ts::Real)
    status = Vector{Int32}(undef, w.n); squarings = Vector{Int32}(undef, w.n)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:fb_lss_c2d, lib), Cint, (Ptr{Cvoid}, Cdouble, Ptr{Int32}, Ptr{Int32}, Ptr{Ptr{Cvoid}}), w.handle, Float64(ts), squarings, status, h))
    return (; world = LinearWorld(h[]), status, squarings)
end
function sample_time(w::LinearWorld)
    ts = Ref{Cdouble}(0.0)
    check(ccall((:fb_lss_sample_time, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), w.handle, ts))
    return ts[]
end
"`lqr(Discrete, Phi, Gamma, Q, R)` for every system of a sampled `LinearWorld` (`c2d(w, Ts).world`), on its device: the stabilising solution
of the discrete Riccati equation by the doubling algorithm and K = inv(R + Gamma' X Gamma) Gamma' X Phi. Q (nx x nx) and R (nu x nu) are
the batch's, symmetric, R positive definite. Returns k (N x nu x nx), x (N x nx x nx), resid, iters (doublings), status (0, or
FB_DLQR_NOT_CONVERGED = 1 | FB_DLQR_SINGULAR = 2: K, X and resid are NaN there) and, with `closed = true`, world: the designed loop as a
sampled `LinearWorld` of its own (Phi - Gamma K in A's place, C - D K in C's), else `nothing`. A continuous world is refused."
function dlqr(w::LinearWorld, q::Matrix{Float64}, r::Matrix{Float64}; closed::Bool = false)
    size(q) == (w.nx, w.nx) || throw(DimensionMismatch("Q must be nx x nx"))
    size(r) == (w.nu, w.nu) || throw(DimensionMismatch("R must be nu x nu"))
    k = Array{Float64}(undef, w.n, w.nu, w.nx); x = Array{Float64}(undef, w.n, w.nx, w.nx)
    resid = Vector{Float64}(undef, w.n); iters = Vector{Int32}(undef, w.n); status = Vector{Int32}(undef, w.n)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:fb_lss_dlqr, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}, Ptr{Int32},
                                            Ptr{Ptr{Cvoid}}), w.handle, q, r, k, x, resid, iters, status, closed ? h : C_NULL))
    world = closed ? LinearWorld(h[]) : nothing
    return (; k, x, resid, iters, status, world)
end
"`marginplot`'s numbers on the device: gain and phase margins of L = gain (c inv(jωI - A) b + d) of channel (iu, iy) (1-based) of every system
of a continuous `LinearWorld` under negative unity feedback, from the brackets of the grid `freqs` (rad/s, positive, strictly increasing),
each refined by bisection. `gain`: `nothing` (ones), a number for the batch or a vector of N. Returns gm (a factor; +Inf without a phase
crossing), wpc, pm (degrees; +Inf without a gain crossing), wgc, ms and wms (the peak of 1 / |1 + L| over the grid and its frequency), npc,
ngc, status (0 or FB_MARGINS_NOT_FINITE = 1, FB_MARGINS_SINGULAR = 2: that system's numbers are NaN; FB_MARGINS_TRUNCATED = 4: more than
8 crossings of a kind), sel (N x 10, the rows of `fb_lss_margins`) and, with `all = true`, every kept crossing as an N x 8 x 6 array
(ω*, Re L*, Im L* of the phase crossings, then of the gain crossings). Margins say nothing about closed-loop stability: `poles` of the
closed loop does."
function margins(w::LinearWorld, iu::Integer, iy::Integer, freqs::Vector{Float64}; gain = nothing, all::Bool = false)
    g = gain === nothing ? nothing : (gain isa Real ? fill(Float64(gain), w.n) : Vector{Float64}(gain))
    g === nothing || length(g) == w.n || throw(DimensionMismatch("margins: gain has $(length(g)) entries for $(w.n) systems"))
    sel = Matrix{Float64}(undef, w.n, 10); counts = Matrix{Int32}(undef, w.n, 2); status = Vector{Int32}(undef, w.n)
    every = all ? Array{Float64}(undef, w.n, 8, 6) : nothing
    check(ccall((:fb_lss_margins, lib), Cint,
                (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}, Ptr{Cdouble}, Ptr{Int32}),
                w.handle, iu - 1, iy - 1, freqs, length(freqs), g === nothing ? C_NULL : g, sel, counts, every === nothing ? C_NULL : every, status))
    return (; gm = sel[:, 1], wpc = sel[:, 2], pm = sel[:, 3], wgc = sel[:, 4], ms = 1.0 ./ sel[:, 9], wms = sel[:, 10],
            npc = counts[:, 1], ngc = counts[:, 2], status, sel, all = every)
end
"Marks a continuous `LinearWorld` that has a model as sampled with sample time `ts`: A's place is read as Phi, B's as Gamma, xdot0's as delta
(`fb_lss_set_sampled`). The way in for a model given as (Phi, Gamma), such as a loop with a sample of delay (an eigenvalue of Phi at 0)."
set_sampled!(w::LinearWorld, ts::Real) = (check(ccall((:fb_lss_set_sampled, lib), Cint, (Ptr{Cvoid}, Cdouble), w.handle, Float64(ts))); w)
"`freqresp(sysd, w)` on the device: P(e^(jωTs)) = c inv(zI - Phi) gamma + d of channel (iu, iy) (1-based) of every system of a sampled
`LinearWorld` on `freqs` (rad/s, at most π/Ts). Returns a complex N x nw matrix (NaN where a pivot was zero or not finite)."
function dfreqresp(w::LinearWorld, iu::Integer, iy::Integer, freqs::Vector{Float64})
    re = Matrix{Float64}(undef, w.n, length(freqs)); im = Matrix{Float64}(undef, w.n, length(freqs))
    check(ccall((:fb_lss_dfreqresp, lib), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}),
                w.handle, iu - 1, iy - 1, freqs, length(freqs), re, im))
    return complex.(re, im)
end
"`margins` for a sampled `LinearWorld`: L = gain (c inv(zI - Phi) gamma + d) on z = e^(jωTs), the same arguments and the same named tuple;
`freqs` in rad/s, strictly increasing, at most π/Ts. The brackets are refined by bisecting the arc of the unit circle. A phase crossing at
the Nyquist frequency itself is not bracketed. `dpoles` of the closed loop says whether it is stable."
function dmargins(w::LinearWorld, iu::Integer, iy::Integer, freqs::Vector{Float64}; gain = nothing, all::Bool = false)
    g = gain === nothing ? nothing : (gain isa Real ? fill(Float64(gain), w.n) : Vector{Float64}(gain))
    g === nothing || length(g) == w.n || throw(DimensionMismatch("dmargins: gain has $(length(g)) entries for $(w.n) systems"))
    sel = Matrix{Float64}(undef, w.n, 10); counts = Matrix{Int32}(undef, w.n, 2); status = Vector{Int32}(undef, w.n)
    every = all ? Array{Float64}(undef, w.n, 8, 6) : nothing
    check(ccall((:fb_lss_dmargins, lib), Cint,
                (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}, Ptr{Cdouble}, Ptr{Int32}),
                w.handle, iu - 1, iy - 1, freqs, length(freqs), g === nothing ? C_NULL : g, sel, counts, every === nothing ? C_NULL : every, status))
    return (; gm = sel[:, 1], wpc = sel[:, 2], pm = sel[:, 3], wgc = sel[:, 4], ms = 1.0 ./ sel[:, 9], wms = sel[:, 10],
            npc = counts[:, 1], ngc = counts[:, 2], status, sel, all = every)
end
"`poles(sysd)` on the device: the eigenvalues z of Phi of every system of a sampled `LinearWorld`, with `poles`' outputs, order (ascending
|z|) and status. `damp`'s reading is s = log(z) / Ts, wn = |s|, zeta = -cos(arg s); stable where every |z| < 1."
function dpoles(w::LinearWorld)
    re = Matrix{Float64}(undef, w.n, w.nx); im = Matrix{Float64}(undef, w.n, w.nx)
    iters = Vector{Int32}(undef, w.n); status = Vector{Int32}(undef, w.n)
    check(ccall((:fb_lss_dpoles, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}, Ptr{Int32}), w.handle, re, im, iters, status))
    return (; re, im, iters, status)
end
"`connect` on sampled `LinearWorld`s with the same Ts, with unit delays (`fb_lss_dconnect`): `delays` are 1-based rows of z = [y_p; y_c] that are also
kept one sample, q_k(t) = z[delays_k](t - 1); `reads` and `outputs` are 1-based rows of the extended vector [z; q] (`outputs = nothing`: every
row), so a read or an output takes a signal now or one sample late. `feedback`, `inputs` and the status are `connect`'s. Returns the new sampled
`LinearWorld` (states [x_p; x_c; q], inputs w, outputs [z; q][outputs], the plant's Ts, at rest) and status. A longer delay is a chain of calls."
function dconnect(p::LinearWorld, c::Union{LinearWorld, Nothing} = nothing; feedback::Array{Float64}, inputs::Array{Float64}, reads, outputs = nothing,
                  delays = Int[])
    dz = Int32.(delays .- 1); jz = Int32.(reads .- 1); iz = outputs === nothing ? Int32[] : Int32.(outputs .- 1)
    nw = size(inputs, ndims(inputs))
    status = Vector{Int32}(undef, p.n)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:fb_lss_dconnect, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int32}, Int32, Ptr{Int32}, Int32, Ptr{Cdouble}, Int32, Ptr{Cdouble}, Int32,
                                                Int32, Ptr{Int32}, Int32, Ptr{Int32}, Ptr{Ptr{Cvoid}}),
                p.handle, c === nothing ? C_NULL : c.handle, isempty(dz) ? C_NULL : dz, length(dz), jz, length(jz), feedback,
                ndims(feedback) == 3 ? 1 : 0, inputs, ndims(inputs) == 3 ? 1 : 0, nw, outputs === nothing ? C_NULL : iz, length(iz), status, h))
    return (; world = LinearWorld(h[]), status)
end
"`optimize_PID`'s metrics under the sampled PID law (`f_periodic!` of `PID` every Ts: backward-Euler integrator and filtered derivative,
output clamp, integrator halted while clamped) for every (system, candidate) pair of a sampled `LinearWorld`, channel (iu, iy) (1-based).
`pid` is N x m x 4 (k_p, k_i, k_d, τ_f >= 0); `bounds` is `nothing` or N x m x 2 (lo, hi; either may be infinite; a finite bound needs d = 0);
`freqs` in rad/s, at most π/Ts. Returns metrics (N x m x 5: Ms, ie, ef, iu, up; Ms is the linear law's, on the grid), cost, status (0, or
FB_DPID_DIVERGED = 1, FB_DPID_SINGULAR = 2, FB_DPID_DIRECT = 4) and counts (N x m x 2: ticks clamped, ticks with the integrator halted)."
function dpid_metrics(w::LinearWorld, iu::Integer, iy::Integer, freqs::Vector{Float64}, t_sim::Real, pid::Array{Float64, 3};
                      weights::Union{Vector{Float64}, Nothing} = nothing, bounds::Union{Array{Float64, 3}, Nothing} = nothing)
    size(pid, 1) == w.n && size(pid, 3) == 4 || throw(DimensionMismatch("pid must be N x m x 4"))
    m = size(pid, 2)
    bounds === nothing || size(bounds) == (w.n, m, 2) || throw(DimensionMismatch("bounds must be N x m x 2"))
    metrics = Array{Float64}(undef, w.n, m, 5); cost = Matrix{Float64}(undef, w.n, m)
    counts = Array{Int32}(undef, w.n, m, 2); status = Matrix{Int32}(undef, w.n, m)
    check(ccall((:fb_lss_dpid_metrics, lib), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Cint, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint,
                                                    Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}, Ptr{Int32}),
                w.handle, iu - 1, iy - 1, freqs, length(freqs), t_sim, weights === nothing ? C_NULL : weights, pid,
                bounds === nothing ? C_NULL : bounds, m, metrics, cost, counts, status))
    return (; metrics, cost, status, counts)
end
"The sampled LQR tracker law (`f_periodic!` of `LQR`, FP/control.jl:708-743) on every (system, candidate) pair of a sampled `LinearWorld`:
the step response to `zref` (nz numbers, the batch's) of the command variables `z` (1-based output rows) from rest over round(t_sim / Ts)
ticks. Gains: `k_fbk` N x m x nu x nx, `k_fwd` and `k_int` N x m x nu x nz; `bounds` N x m x nu x 2 (lo, hi on the deviation of u) or nothing.
Returns zmet N x m x nz x 3 (ie, ef, zp), umet N x m x nu x 2 (iu, up), counts N x m x nu x 2 (clamped, halted ticks), the samples
zs N x m x nz x ns and us N x m x nu x ns (every `stride`-th and the last) and status N x m (0, FB_DTRACK_DIVERGED = 1, FB_DTRACK_NOT_FINITE = 2)."
function dtracker_metrics(w::LinearWorld, z, k_fbk::Array{Float64, 4}, k_fwd::Array{Float64, 4}, k_int::Array{Float64, 4}, zref::Vector{Float64},
                          t_sim::Real; bounds::Union{Array{Float64, 4}, Nothing} = nothing, stride::Integer = 1)
    iz = Int32.(z .- 1)
    nz = length(iz); m = size(k_fbk, 2)
    size(k_fbk) == (w.n, m, w.nu, w.nx) || throw(DimensionMismatch("k_fbk must be N x m x nu x nx"))
    size(k_fwd) == (w.n, m, w.nu, nz) && size(k_int) == (w.n, m, w.nu, nz) || throw(DimensionMismatch("k_fwd and k_int must be N x m x nu x nz"))
    bounds === nothing || size(bounds) == (w.n, m, w.nu, 2) || throw(DimensionMismatch("bounds must be N x m x nu x 2"))
    length(zref) == nz || throw(DimensionMismatch("zref must have nz entries"))
    nt = round(Int, t_sim / sample_time(w))
    ns = Int(ccall((:fb_lss_stepinfo_samples, lib), Cint, (Cint, Cint), nt, stride))
    ns > 0 || throw(DimensionMismatch("t_sim / Ts and stride must both be at least 1"))
    zmet = Array{Float64}(undef, w.n, m, nz, 3); umet = Array{Float64}(undef, w.n, m, w.nu, 2); counts = Array{Int32}(undef, w.n, m, w.nu, 2)
    zs = Array{Float64}(undef, w.n, m, nz, ns); us = Array{Float64}(undef, w.n, m, w.nu, ns); status = Matrix{Int32}(undef, w.n, m)
    check(ccall((:fb_lss_dtracker_metrics, lib), Cint, (Ptr{Cvoid}, Ptr{Int32}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint,
                                                        Ptr{Cdouble}, Cdouble, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}),
                w.handle, iz, nz, k_fbk, k_fwd, k_int, bounds === nothing ? C_NULL : bounds, m, zref, t_sim, stride, zmet, umet, counts, zs, us, status))
    return (; zmet, umet, counts, zs, us, status)
end
"`steady_state` for a sampled `LinearWorld`: [X; U] = the last nz columns of inv([Phi - I, Gamma; C[z, :], D[z, :]]), k_fbk = k - Ts k_xi C_z
(k_xi given; else k) and k_fwd = U + k_fbk X. k (nu x nx) and k_xi (nu x nz): both for the batch, or both N x nu x . per system. status: 0,
FB_SURGERY_SINGULAR = 1, FB_SURGERY_NOT_FINITE = 2, FB_DSTEADY_DIRECT = 4 (k_xi on a system with D_z != 0: k_fbk and k_fwd NaN)."
function dsteady_state(w::LinearWorld, z; k::Union{Array{Float64}, Nothing} = nothing, k_xi::Union{Array{Float64}, Nothing} = nothing)
    iz = Int32.(z .- 1)
    nz = length(iz)
    x = Array{Float64}(undef, w.n, w.nx, nz); u = Array{Float64}(undef, w.n, w.nu, nz)
    k_fbk = k === nothing ? nothing : Array{Float64}(undef, w.n, w.nu, w.nx)
    k_fwd = k === nothing ? nothing : Array{Float64}(undef, w.n, w.nu, nz)
    status = Vector{Int32}(undef, w.n); rpiv = Vector{Float64}(undef, w.n)
    check(ccall((:fb_lss_dsteady, lib), Cint, (Ptr{Cvoid}, Ptr{Int32}, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                                               Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}),
                w.handle, iz, nz, k === nothing ? C_NULL : k, k_xi === nothing ? C_NULL : k_xi, k !== nothing && ndims(k) == 3 ? 1 : 0, x, u,
                k === nothing ? C_NULL : k_fbk, k === nothing ? C_NULL : k_fwd, rpiv, status))
    return (; x, u, k_fbk, k_fwd, status, rpiv)
end
"`:panel` or `:shfl`: how the stepper's lanes exchange stage values (FLIGHTBATCH_LSS_EXCHANGE when the handle was created)"
function exchange(w::LinearWorld)
    xch = Ref{Int32}(-1)
    check(ccall((:fb_lss_exchange, lib), Cint, (Ptr{Cvoid}, Ptr{Int32}), w.handle, xch))
    return xch[] == 0 ? :panel : :shfl
end
f_ode!(w::LinearWorld) = (check(ccall((:fb_f_ode, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), w.handle, C_NULL)); nothing)
f_step!(w::LinearWorld) = nothing        # @no_step LinearizedSS
f_periodic!(w::LinearWorld) = nothing    # @no_periodic LinearizedSS
state(w::LinearWorld) = (x = Matrix{Float64}(undef, w.n, w.nx);
    check(ccall((:fb_get_state, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Int32}), w.handle, x, C_NULL)); x)
outputs(w::LinearWorld) = (y = Matrix{Float64}(undef, w.n, w.ny);
    check(ccall((:fb_get_outputs, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), w.handle, y)); y)
inputs!(w::LinearWorld, u::Matrix{Float64}) = (size(u) == (w.n, w.nu) || throw(DimensionMismatch("u must be N x nu"));
    check(ccall((:fb_set_inputs, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Int32}), w.handle, u, C_NULL)); nothing)
"nsteps of RK4 at dt with u held, `steps_per_launch` steps fused per kernel launch"
function step!(w::LinearWorld, nsteps::Integer; dt::Real = 0.02, steps_per_launch::Integer = 50)
    p = Ref{Params}()
    check(ccall((:fb_get_params, lib), Cint, (Ptr{Cvoid}, Ptr{Params}), w.handle, p))
    q = p[]
    p[] = Params(dt, q.periodic_n, q.surface, q.T_sl, q.p_sl, q.wind_ned, q.h_terrain)
    check(ccall((:fb_set_params, lib), Cint, (Ptr{Cvoid}, Ptr{Params}), w.handle, p))
    check(ccall((:fb_set_steps_per_launch, lib), Cint, (Ptr{Cvoid}, Cint), w.handle, steps_per_launch))
    check(ccall((:fb_step, lib), Cint, (Ptr{Cvoid}, Int64), w.handle, nsteps))
    check(ccall((:fb_sync, lib), Cint, (Ptr{Cvoid},), w.handle))
    return nothing
end

"Simulation(world; dt, Δt) for the batch: fixed-step RK4 + Flight.jl's callback order, fused on the GPU."
mutable struct BatchedSimulation
    mdl::BatchedWorld
    dt::Float64
    Δt::Float64
    nstep::Int
    function BatchedSimulation(mdl::BatchedWorld; dt::Real = 0.02, Δt::Real = dt, steps_per_launch::Integer = 50)
        p = Ref{Params}()
        check(ccall((:fb_get_params, lib), Cint, (Ptr{Cvoid}, Ptr{Params}), mdl.handle, p))
        q = p[]
        p[] = Params(dt, round(Cint, Δt / dt), q.surface, q.T_sl, q.p_sl, q.wind_ned, q.h_terrain)
        check(ccall((:fb_set_params, lib), Cint, (Ptr{Cvoid}, Ptr{Params}), mdl.handle, p))
        check(ccall((:fb_set_steps_per_launch, lib), Cint, (Ptr{Cvoid}, Cint), mdl.handle, steps_per_launch))
        new(mdl, dt, Δt, 0)
    end
end
"""Each simulation's own environment: env [N x 6], columns wind N / E / D (`world.atmosphere.wind.u`, FlightPhysics/src/atmosphere.jl:156-165),
sea-level T / p (`world.atmosphere.sl.u`, :75-84), terrain elevation (FlightPhysics/src/terrain.jl:34-36). `nothing` returns to the batch-wide block."""
function set_env!(w::BatchedWorld, env::Union{Matrix{Float64}, Nothing})
    # the C ABI takes no length: a matrix of another size would be read out of bounds, a transposed 6 x N one silently misread
    env === nothing || size(env) == (w.n, 6) || throw(DimensionMismatch("set_env!: env must be $(w.n) x 6 (aircraft x wind N / E / D, T_sl, p_sl, h_terrain), got $(size(env))"))
    check(ccall((:fb_set_env, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), w.handle, env === nothing ? C_NULL : env))
    nothing
end
"f_init!(world) for a Cessna172Xv2 batch whose state and inputs the host has set (C172.Init-style initial condition): the avionics half of f_init!."
function f_init!(w::BatchedWorld)
    check(ccall((:fb_f_init, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Cint), w.handle, C_NULL, 0))
    nothing
end
init!(sim::BatchedSimulation, args...) = (f_init!(sim.mdl, args...); sim.nstep = 0; nothing)
function step!(sim::BatchedSimulation, Δt_total::Real = sim.dt, stop_at_tdt::Bool = true)
    n = round(Int, Δt_total / sim.dt)
    check(ccall((:fb_step, lib), Cint, (Ptr{Cvoid}, Int64), sim.mdl.handle, n))
    check(ccall((:fb_sync, lib), Cint, (Ptr{Cvoid},), sim.mdl.handle))
    sim.nstep += n
    return nothing
end
Base.getproperty(sim::BatchedSimulation, s::Symbol) = s === :t ? getfield(sim, :nstep) * getfield(sim, :dt) : getfield(sim, s)

# ---- scripted scenarios: `user_callback!` as a table on the device (include/flightbatch.h, FB_TABLE_SCENARIO) ------------------------
# Simulation(mdl; user_callback!) calls a closure after every step (FC/sim.jl:185, 334-336); for a batch the closures of the demos
# (FlightApps/demos/c172_demos.jl:423-486, 525-642: a phase symbol, per phase "set these inputs; if <condition> set those, next phase") are
# a table of phases, rules and actions that a kernel interprets between the stepping launches. `blob` is the packed table (the layout is in
# the header; flightbatch/scenario.py builds it on the Python side), `par` the per-aircraft parameter rows [N x n_par].
# The callback is model-agnostic in the reference (FC/sim.jl:279), and so are these verbs: a Cessna172Xv2 world takes every source and
# destination; a Cessna172Sv0 world (fp64, any mechanisation) takes tables that write the vehicle's inputs and records — the nlsim_q / nlsim_θ
# elevator step, c172_demos.jl:108-206 — and the library refuses control-law rows (sources CS / CU, destination CU) on it, with the reason.
const TABLE_SCENARIO = Cint(6)
# the world's kinds of a blob (FB_SCN_SRC_ENV, FB_SCN_SRC_Y, FB_SCN_DST_ENV): the aircraft's own environment rows — a world whose rows are set
# (fb_set_env) only; a table writes the three wind rows — and any row of mdl.y at the state behind the step
const SCN_SRC_ENV = Cint(18)
const SCN_SRC_Y = Cint(19)
const SCN_DST_ENV = Cint(4)
function set_scenario!(w::BatchedWorld, blob::Vector{Float64}, par::Union{Matrix{Float64}, Nothing} = nothing; every::Integer = 1)
    len = Ref{Int64}(length(blob))
    check(ccall((:fb_set_table, lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Int64}, Cint), w.handle, TABLE_SCENARIO, blob, len, 1))
    check(ccall((:fb_scenario_configure, lib), Cint, (Ptr{Cvoid}, Cint), w.handle, every))
    n_par = round(Int, blob[5])
    if n_par > 0
        par !== nothing && size(par) == (w.n, n_par) || throw(DimensionMismatch("set_scenario!: par must be $(w.n) x $(n_par)"))
        check(ccall((:fb_scenario_set_params, lib), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), w.handle, par))
    end
    nothing
end
clear_scenario!(w::BatchedWorld) = (check(ccall((:fb_scenario_configure, lib), Cint, (Ptr{Cvoid}, Cint), w.handle, 0)); nothing)
"every aircraft's phase, the step at which it entered it, and its record rows [N x n_rec]"
function scenario_state(w::BatchedWorld, n_rec::Integer)
    phase = Vector{Int32}(undef, w.n); since = Vector{Int64}(undef, w.n); rec = Matrix{Float64}(undef, w.n, max(n_rec, 1))
    check(ccall((:fb_scenario_get_state, lib), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int64}, Ptr{Cdouble}), w.handle, phase, since, rec))
    return phase, since, rec[:, 1:n_rec]
end

# ---- multi-GPU trajectory collection: one process per GPU, one RCCL all-gather of the state panels (include/flightbatch.h) -------
"rank 0: `id = comm_unique_id()`, hand the 128 bytes to the other ranks (file, MPI, sockets); every rank: `comm_init(world_handle, nranks, rank, id)`"
comm_unique_id() = (id = Vector{UInt8}(undef, 128); check(ccall((:fb_comm_unique_id, lib), Cint, (Ptr{UInt8},), id)); id)
function comm_init(w::BatchedWorld, nranks::Integer, rank::Integer, id::Vector{UInt8})
    comm = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:fb_comm_init, lib), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{UInt8}, Ptr{Ptr{Cvoid}}), w.handle, nranks, rank, id, comm))
    return comm[]
end
"shard sizes of all ranks, exchanged by `comm_init`: `(n_of, n_max)`"
function comm_shard_sizes(comm::Ptr{Cvoid}, nranks::Integer)
    n_of = Vector{Int64}(undef, nranks); n_max = Ref{Int64}(0)
    check(ccall((:fb_comm_shard_sizes, lib), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}), comm, n_of, n_max))
    return n_of, n_max[]
end
"all-gather of the device-layout state into `recv_dev` (device pointer to nranks x Nx x n_max doubles; equal shards: n_max = N), asynchronous on the world's stream"
gather_state!(w::BatchedWorld, comm::Ptr{Cvoid}, recv_dev::Ptr{Cvoid}) =
    check(ccall((:fb_gather_state, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), w.handle, comm, recv_dev))

# ---- saving: the SavingCallback / TimeSeries(sim) of FC/sim.jl:210-217,644-704, kept on the device -------------------
const LOG_X0 = Cint(1000)   # FB_LOG_X0: rows >= LOG_X0 select state rows, rows < LOG_X0 rows of the output record y
"Log `rows` (0-based, see include/flightbatch.h FB_Y_*) every `saveat` seconds into a device buffer of `capacity` samples."
function save_on!(sim::BatchedSimulation, rows::Vector{Cint}; saveat::Real = sim.dt, capacity::Integer = 1024)
    check(ccall((:fb_log_configure, lib), Cint, (Ptr{Cvoid}, Int64, Int64, Ptr{Cint}, Cint),
                sim.mdl.handle, round(Int64, saveat / sim.dt), capacity, rows, length(rows)))
    check(ccall((:fb_log_record, lib), Cint, (Ptr{Cvoid},), sim.mdl.handle))   # y(t0), like reinit! does
end
"TimeSeries(sim) for the batch: (t, data) with data[aircraft, row, sample]."
function timeseries(sim::BatchedSimulation, nrows::Integer)
    cnt = Ref{Int64}(0)
    check(ccall((:fb_log_count, lib), Cint, (Ptr{Cvoid}, Ptr{Int64}), sim.mdl.handle, cnt))
    t = Vector{Float64}(undef, cnt[])
    data = Array{Float64, 3}(undef, sim.mdl.n, nrows, cnt[])
    check(ccall((:fb_log_read, lib), Cint, (Ptr{Cvoid}, Int64, Int64, Ptr{Cdouble}, Ptr{Cdouble}), sim.mdl.handle, 0, cnt[], t, data))
    return t, data
end

end # module
