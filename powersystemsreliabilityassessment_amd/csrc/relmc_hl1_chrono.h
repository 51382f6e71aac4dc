// relmc_hl1_chrono.h — device-only helpers of the HL1 chronology contract (include/relmc.h), shared by the kernels of every HL1
// chronology track (relmc_hl1_chain_kernels.h, relmc_area_kernels.h and the others).  Inline functions only: no kernel is defined here,
// so every unit may include it.
#pragma once
#include "relmc_devfn.h"

namespace relmc {

// U of draw e of unit k in chain c (the 0x40000000 tag keeps the stream apart from the HL2 chronology and the HL1 non-sequential draws)
DEVFI double hl1_seq_u(uint64_t chain, int k, int e, uint64_t seed)
{
    uint32_t w[4];
    philox4x32_10((uint32_t)chain, (uint32_t)(chain >> 32), (uint32_t)k | 0x40000000u, (uint32_t)e >> 2, (uint32_t)seed, (uint32_t)(seed >> 32), w);
    const uint32_t x = (e & 2) ? ((e & 1) ? w[3] : w[2]) : ((e & 1) ? w[1] : w[0]);      // selects, not a dynamic index into w (scratch)
    return ((double)x + 0.5) * 2.3283064365386963e-10;
}

// Orders one lane's LDS accesses against the other lanes' of the same wavefront (no workgroup barrier: the four waves run four chains)
DEVFI void hl1_seq_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Load of a sweep level at one hour, L = scale * load + shift with the product and the sum each rounded, as numpy's scale * load + shift
// (the contract's __dmul_rn / __dadd_rn: those two are plain operators in the HIP headers and were fused into one v_fma_f64, so the rule
// is stated to the compiler).  For relmc_hl1_seq_sweep and, per area, relmc_hl1_area_sweep.
DEVFI double hl1_sweep_load(double scale, double ld, double shift)
{
#pragma clang fp contract(off)
    const double p = scale * ld;
    return p + shift;
}

// An event record without events (relmc_hl1_seq_events: a chain's record before its first event, a reduction slice before its first record)
DEVFI void hl1_event_rec_zero(Hl1EventRec& r)
{
    r.events = r.sum_dur = r.sum_dur2 = r.max_dur = r.censored = 0;
    r.sum_energy = r.sum_energy2 = r.max_energy = r.max_peak = 0.0;
}

}  // namespace relmc
