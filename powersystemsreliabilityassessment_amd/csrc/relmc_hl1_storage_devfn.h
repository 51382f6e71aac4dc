// relmc_hl1_storage_devfn.h — device-only helpers of the storage and weather-year contracts (include/relmc.h), shared by
// the three tracks of relmc_hl1_storage_track_kernel (relmc_hl1_storage_kernels.h) and the weather-year instantiations of relmc_hl1_area_kernel
// (relmc_area_kernels.h).  Inline functions only, as relmc_hl1_chrono.h:
// no kernel is defined here, so every unit may include it.  The functions are force-inlined leaves; every kernel that uses them compiles
// to the instructions it had with a copy of its own.
#pragma once
#include <utility>
#include "../../include/relmc.h"
#include "relmc_devfn.h"

namespace relmc {

// f(integral_constant<int, i>) for i = 0 .. RELMC_HL1_MAX_STORAGE - 1, written out at compile time (as hl1_rows): a storage's
// state of charge is a register named by a constant, never a run-time index into a per-thread array (scratch)
template <class F, int... I>
DEVFI void hl1_storage_each_(F&& f, std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }
template <class F>
DEVFI void hl1_storage_each(F&& f) { hl1_storage_each_(f, std::make_integer_sequence<int, RELMC_HL1_MAX_STORAGE>{}); }

// L = scale * base + shift with the product and the sum each rounded (hl1_sweep_load's rule, stated to the compiler the same way)
DEVFI double hl1_storage_load(double scale, double ld, double shift)
{
#pragma clang fp contract(off)
    const double p = scale * ld;
    return p + shift;
}

// cap + s * v with the product and the sum each rounded
DEVFI double hl1_var_add(double cap, double s, double v)
{
#pragma clang fp contract(off)
    const double p = s * v;
    return cap + p;
}

// The weather year of chain year y of `chain` (the contract's two rules; relmc_hl1_var_weather_year is the host's copy)
DEVFI int hl1_var_weather(uint64_t seed, uint64_t chain, int y, int years, int n_weather, int pick)
{
    if (pick == RELMC_HL1_VAR_PICK_CYCLE) return (int)((chain * (uint64_t)years + (uint64_t)y) % (uint64_t)n_weather);
    uint32_t w[4];
    philox4x32_10((uint32_t)chain, (uint32_t)(chain >> 32), RELMC_HL1_VAR_TAG, (uint32_t)y, (uint32_t)seed, (uint32_t)(seed >> 32), w);
    return (int)(((uint64_t)w[0] * (uint64_t)n_weather) >> 32);
}

DEVFI double hl1_storage_readlane(double v, int src)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), src), __builtin_amdgcn_readlane(__double2loint(v), src));
}

// What storage i can still do at the state of charge s, as two wave-uniform bits: bit i = it can discharge (s > 0 and discharge_mw > 0),
// bit 8 + i = it is not settled (s < energy_mwh and charge_mw > 0).  With the bit clear the contract's step leaves the storage, the
// need / surplus and the sums as they are (avail or y is 0), so such a storage is passed over.
DEVFI uint32_t hl1_storage_bits(const relmc_hl1_storage& p, double s, int i)
{
    return ((s > 0.0 && p.discharge_mw > 0.0) ? 1u << i : 0u) | ((s < p.energy_mwh && p.charge_mw > 0.0) ? 256u << i : 0u);
}

// The contract's short step.  A: a kernel's argument struct with the storages in st[] (Hl1StorageArgs, Hl1VarArgs, Hl1StressArgs).
// soc: storage i's state of charge in lane i (read and written through the lane; one register pair instead of eight); bits:
// hl1_storage_bits of every storage; z: a zero the compiler cannot see through, so that a storage's data is read from the kernel argument
// segment here, where it is used, and is not 96 scalar registers live across the whole chain.
// need -> what is left of it, xs = the sum of the x; every operation rounded once.
template <class Args>
DEVFI void hl1_storage_discharge(const Args& A, int ns, int z, int lane, double& soc, uint32_t& bits, double& need, double& xs)
{
    hl1_storage_each([&](auto ic) {
#pragma clang fp contract(off)
        constexpr int i = decltype(ic)::value;
        if (i < ns && need > 0.0 && ((bits >> i) & 1u)) {    // wave-uniform
            const relmc_hl1_storage& p = A.st[i + z];
            const double eta = p.eta_discharge, s = hl1_storage_readlane(soc, i);
            const double avail = __builtin_fmin(p.discharge_mw, s * eta);
            const double x = __builtin_fmin(avail, need);
            const double t = __builtin_fmax(0.0, s - x / eta);
            need = need - x;
            xs = xs + x;
            soc = lane == i ? t : soc;
            bits = (bits & ~(0x101u << i)) | hl1_storage_bits(p, t, i);
        }
    });
}

// The contract's long step: ys = the sum of the y
template <class Args>
DEVFI void hl1_storage_charge(const Args& A, int ns, int z, int lane, double& soc, uint32_t& bits, double surplus, double& ys)
{
    hl1_storage_each([&](auto ic) {
#pragma clang fp contract(off)
        constexpr int i = decltype(ic)::value;
        if (i < ns && surplus > 0.0 && ((bits >> (8 + i)) & 1u)) {      // wave-uniform
            const relmc_hl1_storage& p = A.st[i + z];
            const double eta = p.eta_charge, cap = p.energy_mwh, s = hl1_storage_readlane(soc, i);
            const double room = (cap - s) / eta;
            const double y = __builtin_fmin(__builtin_fmin(p.charge_mw, room), surplus);
            const double t = __builtin_fmin(cap, s + y * eta);
            surplus = surplus - y;
            ys = ys + y;
            soc = lane == i ? t : soc;
            bits = (bits & ~(0x101u << i)) | hl1_storage_bits(p, t, i);
        }
    });
}

// This lane's partials of the open year.  Loss hours, loss events and served hours are counts (exact in any order); the three energies are
// fp64 sums over the lane's steps of the year in ascending order, as relmc_hl1_seq_kernel's EUE partial.
struct Hl1StoragePartials { uint32_t lole, lolf, served; double eue, dis, chg; };

// The wave's open year: relmc_hl1_seq_kernel's fixed-order butterfly (hl1_seq_close_year) over the lanes' partials of both records;
// lane 0 stores (lole, eue, lolf) and (served_hours, discharged_mwh, charged_mwh); the partials restart at zero
DEVFI void hl1_storage_close_year(Hl1StoragePartials& a, double* __restrict__ out0, double* __restrict__ out1)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a.lole += (uint32_t)__shfl_xor((int)a.lole, off); a.lolf += (uint32_t)__shfl_xor((int)a.lolf, off); a.served += (uint32_t)__shfl_xor((int)a.served, off);
        a.eue += __shfl_xor(a.eue, off); a.dis += __shfl_xor(a.dis, off); a.chg += __shfl_xor(a.chg, off);
    }
    if ((threadIdx.x & 63) == 0) {
        out0[0] = (double)a.lole; out0[1] = a.eue; out0[2] = (double)a.lolf;
        out1[0] = (double)a.served; out1[1] = a.dis; out1[2] = a.chg;
    }
    a.lole = a.lolf = a.served = 0u;
    a.eue = a.dis = a.chg = 0.0;
}

}  // namespace relmc
